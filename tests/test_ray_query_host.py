"""Ray queries, the host side (no GPU): rt_camera_ray against the oracle's camera ray bit for bit, and the argument checks of the
rt_query_* entry points — every error returns non-zero with its message before a device is looked for, and n = 0 returns 0."""
import ctypes as C

import numpy as np
import pytest

from raytracinginrust_amd import render as R
from raytracinginrust_amd import scenes
from raytracinginrust_amd.api import Camera

W, H = 33, 17


def _cameras():
    """Cornell's (aperture 0.05), the random scene's (aperture 0.1: the lens disk's rejection loop matters), one with time0 != time1."""
    cornell = Camera((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, W / H, 0.05, 10.0, 0.0, 1.0)
    random_ = Camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, W / H, 0.1, 10.0, 0.0, 1.0)
    shutter = Camera((3.0, 4.0, -7.0), (0.5, 1.0, 0.25), (0.1, 1.0, 0.0), 55.0, W / H, 0.3, 6.5, 0.25, 1.75)
    return {"cornell": cornell, "random": random_, "shutter": shutter}


def _pixels():
    rs = np.random.RandomState(7)
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    px += [(int(rs.randint(0, W)), int(rs.randint(0, H))) for _ in range(20)]
    return px


@pytest.mark.parametrize("which", ["cornell", "random", "shutter"])
def test_camera_ray_equals_the_oracles_bit_for_bit(pbe, obe, which):
    cam = _cameras()[which]
    n = 0
    for seed in (0x5EED, 12345678901234567):
        for (i, j) in _pixels():
            for sample in range(8):
                got = R.camera_ray(cam, W, H, i, j, seed, sample)
                ref = (C.c_double * 7)()
                obe.lib.orc_camera_ray(C.byref(cam), W, H, i, j, seed, sample, ref)
                ref = np.array(ref, dtype=np.float64)
                assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (which, seed, i, j, sample, got.tolist(), ref.tolist())
                n += 1
    assert n == 2 * 24 * 8
    if which == "shutter":                      # the time draw is used: not every ray carries time0
        t = {float(R.camera_ray(cam, W, H, 3, 4, 1, s)[6]) for s in range(8)}
        assert len(t) == 8 and all(0.25 <= x < 1.75 for x in t)


def test_camera_ray_is_the_cornell_scene_functions_camera(pbe):
    """(the camera above is the one scenes.cornell_box returns for this aspect ratio: the GPU tests use that one)"""
    _, cam, _ = scenes.cornell_box(pbe, aspect_ratio=W / H)
    a = R.camera_ray(cam, W, H, 5, 6, 9, 2)
    b = R.camera_ray(_cameras()["cornell"], W, H, 5, 6, 9, 2)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _msg(lib):
    return lib.rt_last_error().decode()


def test_camera_ray_argument_checks(pbe):
    lib = pbe.lib
    cam = _cameras()["cornell"]
    out = (C.c_double * 7)()
    assert lib.rt_camera_ray(None, W, H, 0, 0, 0, 0, out) != 0 and "null argument" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), W, H, 0, 0, 0, 0, None) != 0 and "null argument" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), 1, H, 0, 0, 0, 0, out) != 0 and "W and H must be >= 2" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), W, 1, 0, 0, 0, 0, out) != 0 and "W and H must be >= 2" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), 65536, 32768, 0, 0, 0, 0, out) != 0 and "2^31 - 1" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), W, H, W, 0, 0, 0, out) != 0 and "outside" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), W, H, 0, H, 0, 0, out) != 0 and "outside" in _msg(lib)
    assert lib.rt_camera_ray(C.byref(cam), W, H, W - 1, H - 1, 0, 0, out) == 0


def test_query_argument_checks(pbe):
    """Every error of the query entry points comes with its message and before a device is looked for (so it can be seen here), in the
    order null arguments, frame size, flags, buffer size; n = 0 returns 0 and writes nothing."""
    lib = pbe.lib
    b, cam, _ = scenes.cornell_box(pbe)
    rays = np.zeros((4, 7)); rays[:, 5] = 1.0
    hits = np.full((4, 16), 7.0)
    rp, hp = rays.ctypes.data, hits.ctypes.data
    stream = None
    # null arguments
    assert lib.rt_query_hits(None, 4, rp, 1e-5, 0, 0, hp) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_hits(b.h, 4, None, 1e-5, 0, 0, hp) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_hits(b.h, 4, rp, 1e-5, 0, 0, None) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_hits_device(None, 4, rp, 1e-5, 0, 0, hp, hits.nbytes, stream) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_hits_device(b.h, 4, None, 1e-5, 0, 0, hp, hits.nbytes, stream) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_hits_device(b.h, 4, rp, 1e-5, 0, 0, None, hits.nbytes, stream) != 0 and "null argument" in _msg(lib)
    frame = np.zeros((17 * 33, 16))
    fp = frame.ctypes.data
    assert lib.rt_query_camera(None, C.byref(cam), 33, 17, 0, 0, 0, None, fp) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_camera(b.h, None, 33, 17, 0, 0, 0, None, fp) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_camera(b.h, C.byref(cam), 33, 17, 0, 0, 0, None, None) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_camera_device(None, C.byref(cam), 33, 17, 0, 0, 0, None, fp, frame.nbytes, stream) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_camera_device(b.h, None, 33, 17, 0, 0, 0, None, fp, frame.nbytes, stream) != 0 and "null argument" in _msg(lib)
    assert lib.rt_query_camera_device(b.h, C.byref(cam), 33, 17, 0, 0, 0, None, None, frame.nbytes, stream) != 0 and "null argument" in _msg(lib)
    ms = C.c_float()
    assert lib.rt_last_query_ms(None, C.byref(ms)) != 0 and "null argument" in _msg(lib)
    assert lib.rt_last_query_ms(b.h, None) != 0 and "null argument" in _msg(lib)
    assert lib.rt_last_query_ms(b.h, C.byref(ms)) != 0 and "no ray query" in _msg(lib)
    # flags: f64 and the reference's order only
    for flags in (R.RT_F32, R.RT_NEAR_FIRST_BVH, R.RT_PERSISTENT_BVH, R.RT_STOP_ON_ZERO, 1 << 20):
        assert lib.rt_query_hits(b.h, 4, rp, 1e-5, 0, flags, hp) != 0 and "flags = 0" in _msg(lib)
        assert lib.rt_query_hits_device(b.h, 4, rp, 1e-5, 0, flags, hp, hits.nbytes, stream) != 0 and "flags = 0" in _msg(lib)
        assert lib.rt_query_camera(b.h, C.byref(cam), 33, 17, 0, 0, flags, None, fp) != 0 and "flags = 0" in _msg(lib)
        assert lib.rt_query_camera_device(b.h, C.byref(cam), 33, 17, 0, 0, flags, None, fp, frame.nbytes, stream) != 0 and "flags = 0" in _msg(lib)
    # frame size
    for (w, h, text) in ((1, 17, "W and H must be >= 2"), (33, 1, "W and H must be >= 2"), (0, 0, "W and H must be >= 2"),
                         (65536, 32768, "2^31 - 1"), (0xFFFFFFFF, 0xFFFFFFFF, "2^31 - 1")):
        assert lib.rt_query_camera(b.h, C.byref(cam), w, h, 0, 0, 0, None, fp) != 0 and text in _msg(lib)
        assert lib.rt_query_camera_device(b.h, C.byref(cam), w, h, 0, 0, 0, None, fp, frame.nbytes, stream) != 0 and text in _msg(lib)
    # the record buffer of the device forms
    assert lib.rt_query_hits_device(b.h, 4, rp, 1e-5, 0, 0, hp, 4 * 128 - 1, stream) != 0 and "hit buffer too small" in _msg(lib)
    assert lib.rt_query_camera_device(b.h, C.byref(cam), 33, 17, 0, 0, 0, None, fp, 33 * 17 * 128 - 1, stream) != 0 and "hit buffer too small" in _msg(lib)
    assert lib.rt_query_hits_device(b.h, 4, rp + 8, 1e-5, 0, 0, hp, hits.nbytes, stream) != 0 and "16-byte aligned" in _msg(lib)
    # n = 0: nothing to do, nothing touched, no device needed
    assert lib.rt_query_hits(b.h, 0, rp, 1e-5, 0, 0, hp) == 0
    assert lib.rt_query_hits_device(b.h, 0, rp, 1e-5, 0, 0, hp, 0, stream) == 0
    assert np.all(hits == 7.0)
    assert R.query_hits(b, np.zeros((0, 7))).shape == (0, 16)
    with pytest.raises(ValueError):
        R.query_hits(b, np.zeros((3, 6)))


def test_queries_without_gpu_fail_loudly(pbe):
    if R.device_count() > 0:
        pytest.skip("a GPU is present")
    b, cam, _ = scenes.cornell_box(pbe)
    rays = np.zeros((4, 7)); rays[:, 5] = 1.0
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.query_hits(b, rays)
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.query_camera(b, cam, 33, 17)
    hits = np.zeros((33 * 17, 16))
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.query_hits_device(b, 4, rays.ctypes.data, hits.ctypes.data, d_hits_bytes=hits.nbytes)
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.query_camera_device(b, cam, 33, 17, hits.ctypes.data, d_hits_bytes=hits.nbytes)
    with pytest.raises(R.RenderError, match="no ray query"):
        R.last_query_ms(b)


def test_hit_fields_name_the_whole_record_and_set_scene_keeps_the_world(pbe):
    covered = sorted(k for s in R.HIT_FIELDS.values() for k in range(s.start, s.stop))
    assert covered == list(range(15)) and R.HIT_DOUBLES == 16 and R.RAY_DOUBLES == 7
    b, _, _ = scenes.cornell_box(pbe)
    assert b.world.kind == "hittable" and b.world.id >= 0


def test_aov_image_mappings():
    hits = np.zeros((2, 2, 16))
    hits[0, 0, :] = [1, 2.0, 0, 0, 0, 0.0, 1.0, -1.0, 1, 0, 0, 3, 0, 0, 0, 0]
    hits[0, 1, :] = [1, 6.0, 0, 0, 0, 1.0, 0.0, 0.0, 1, 0, 0, 260, 1, 1, 0, 0]
    hits[1, 0, :] = [1, 4.0, 0, 0, 0, 0.0, 0.0, 1.0, 0, 0, 0, -1, 2, -1, -1, 0]
    hits[1, 1, 11:15] = -1.0
    n = R.aov_image(hits, "normal")
    assert n[0, 0].tolist() == [127, 255, 0] and n[0, 1].tolist() == [255, 127, 127] and n[1, 1].tolist() == [127, 127, 127]
    d = R.aov_image(hits, "depth")
    assert d[0, 0].tolist() == [255] * 3 and d[0, 1].tolist() == [0] * 3 and d[1, 0].tolist() == [127] * 3 and d[1, 1].tolist() == [0] * 3
    m = R.aov_image(hits, "material")
    assert m[0, 0, 0] == 3 and m[0, 1, 0] == 4 and m[1, 0, 0] == 255 and m[1, 1, 0] == 255

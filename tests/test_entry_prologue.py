"""What the frame-taking entry points of librt_amd.so check before they touch the device, and in which order (csrc/rt_host.cpp: the frame
arguments, then — rt_render_device* only — the tile decomposition and the sample range, then a HIP device, then the flattened scene), and
on the GPU that a refused call leaves the scene as it was and that rt_scene_prepare and a first render set a device up the same way."""
import ctypes as C

import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from raytracinginrust_amd.api import Camera, SceneBuilder

DEPTH, SEED = 5, 1


def _render(lib, sc, cam, bg, W, H, spp, out):
    return lib.rt_render(sc, cam, bg, W, H, spp, DEPTH, SEED, 0, out)


def _render_samples(lib, sc, cam, bg, W, H, spp, out):
    return lib.rt_render_samples(sc, cam, bg, W, H, spp, DEPTH, SEED, 0, out, None)


def _render_device(lib, sc, cam, bg, W, H, spp, out):
    return lib.rt_render_device(sc, cam, bg, W, H, spp, DEPTH, SEED, 0, 64, 0, 1, None, 0, None)


def _render_device_pass(lib, sc, cam, bg, W, H, spp, out):
    return lib.rt_render_device_pass(sc, cam, bg, W, H, spp, DEPTH, SEED, 0, 0, 1, 64, 0, 1, None, 0, None)


def _calibrate(lib, sc, cam, bg, W, H, spp, out):
    return lib.rt_scene_calibrate(sc, cam, bg, W, H, spp, DEPTH, SEED, 0)


def _progressive_create(lib, sc, cam, bg, W, H, spp, out):
    frame = lib.rt_progressive_create(sc, cam, bg, W, H, DEPTH, SEED, 0)
    if frame:
        lib.rt_progressive_destroy(frame)
    return 0 if frame else -1


# (call, takes a sample count)
ENTRY_POINTS = {
    "rt_render": (_render, True),
    "rt_render_samples": (_render_samples, True),
    "rt_render_device": (_render_device, True),
    "rt_render_device_pass": (_render_device_pass, True),
    "rt_scene_calibrate": (_calibrate, True),
    "rt_progressive_create": (_progressive_create, False),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_first_message_of_every_frame_taking_entry_point(pbe, name):
    """The first thing each entry point says about a bad call: null argument, frame size, sample count, frame too large — and, on a machine
    without a device, "no HIP device" for a valid call, also for a scene whose world is not set (the device is looked for before the scene
    is flattened)."""
    lib = pbe.lib
    call, takes_spp = ENTRY_POINTS[name]
    b, cam, bg = scenes.cornell_box(pbe)
    bgc = (C.c_double * 3)(*bg)
    out = np.zeros(8 * 8 * 3, np.float64).ctypes.data

    def first_message(sc, W, H, spp):
        assert call(lib, sc, C.byref(cam), bgc, W, H, spp, out) != 0
        return lib.rt_last_error().decode()

    assert "null argument" in first_message(None, 8, 8, 2)
    assert "W and H must be >= 2" in first_message(b.h, 1, 8, 2)
    if takes_spp:
        assert "samples_per_pixel must be >= 1" in first_message(b.h, 8, 8, 0)
    assert "frame too large" in first_message(b.h, 65536, 65536, 2)
    if R.device_count() > 0:          # the no-device messages can only be seen on a machine without one
        return
    assert "no HIP device" in first_message(b.h, 8, 8, 2)
    empty = SceneBuilder(pbe)         # no world set: flattening it fails with "world not set", which is not reached
    assert "no HIP device" in first_message(empty.h, 8, 8, 2)


def test_prepare_looks_for_a_device_first(pbe):
    if R.device_count() > 0:
        return
    b, _, _ = scenes.cornell_box(pbe)
    for builder in (b, SceneBuilder(pbe)):
        with pytest.raises(R.RenderError, match="no HIP device"):
            R.prepare(builder)


# ---------------------------------------------------------------- GPU
W, H, SPP = 8, 8, 2


def _three_spheres(pbe):
    """A world that is one BVH of three spheres: a BVH kernel, where the Cornell box runs the list kernel."""
    b = SceneBuilder(pbe)
    world = [b.Sphere((0.0, -100.5, -1.0), 100.0, b.Lambertian(b.ConstantTexture((0.8, 0.8, 0.0)))),
             b.Sphere((-0.6, 0.0, -1.0), 0.5, b.Metal((0.8, 0.6, 0.2), 0.3)),
             b.Sphere((0.6, 0.0, -1.0), 0.5, b.Dielectric(1.5))]
    b.set_scene(b.BVH(world, 0.0, 1.0), [])
    return b, Camera((0.0, 0.5, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 3.0, 0.0, 1.0), (0.7, 0.8, 1.0)


SCENES = {"cornell": scenes.cornell_box, "bvh": _three_spheres}
_fresh = {}


def _fresh_render(pbe, scene):
    """Sums, per-sample radiance (as bit patterns) and launch geometry of a freshly built scene's first render; computed once per scene."""
    if scene not in _fresh:
        b, cam, bg = SCENES[scene](pbe)
        out, samples = R.render(b, cam, bg, W, H, SPP, DEPTH, want_samples=True)
        assert R.last_kernel_ms(b) > 0.0
        assert R.kernel_time_total(b)[1] == 1
        _fresh[scene] = (out.view(np.uint64), samples.view(np.uint64), R.last_launch_info(b), R.last_loop_info(b)["shape"])
    return _fresh[scene]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_a_refused_call_leaves_the_scene_as_it_was(pbe, scene):
    """rt_render_device refused by the host's own checks (an output buffer one byte short, a tile size of 0) launches nothing, and the
    render that follows on the same scene gives the samples of a freshly built one, bit for bit."""
    import torch
    lib = pbe.lib
    ref_out, ref_samples, ref_info, shape = _fresh_render(pbe, scene)
    assert shape == ("list" if scene == "cornell" else "lock-step")
    b, cam, bg = SCENES[scene](pbe)
    bgc = (C.c_double * 3)(*bg)
    d_out = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
    n_bytes = W * H * 3 * 8

    def render_device(tile_px, d_out_bytes):
        rc = lib.rt_render_device(b.h, C.byref(cam), bgc, W, H, SPP, DEPTH, 0x5EED, 0, tile_px, 0, 1, C.c_void_p(d_out.data_ptr()), d_out_bytes, None)
        return rc, lib.rt_last_error().decode()

    rc, msg = render_device(W * H, n_bytes - 1)
    assert rc != 0 and "output buffer too small" in msg
    rc, msg = render_device(0, n_bytes)
    assert rc != 0 and "bad tile decomposition" in msg
    assert R.kernel_time_total(b) == (0.0, 0)                # nothing was launched
    out, samples = R.render(b, cam, bg, W, H, SPP, DEPTH, want_samples=True)
    assert np.array_equal(samples.view(np.uint64), ref_samples) and np.array_equal(out.view(np.uint64), ref_out)
    assert R.last_launch_info(b) == ref_info
    assert R.last_kernel_ms(b) > 0.0
    assert R.kernel_time_total(b)[1] == 1                    # exactly the one launch that was made


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_prepare_then_render_equals_a_first_render(pbe, scene):
    """rt_scene_prepare (upload, launch slots, code object; no launch) followed by a render: the launch geometry and every sample of a
    fresh scene's first render, which does that work itself."""
    ref_out, ref_samples, ref_info, _ = _fresh_render(pbe, scene)
    b, cam, bg = SCENES[scene](pbe)
    R.prepare(b)
    assert R.kernel_time_total(b) == (0.0, 0)                # prepare launches nothing
    out, samples = R.render(b, cam, bg, W, H, SPP, DEPTH, want_samples=True)
    assert R.last_launch_info(b) == ref_info
    assert np.array_equal(samples.view(np.uint64), ref_samples) and np.array_equal(out.view(np.uint64), ref_out)
    assert R.last_kernel_ms(b) > 0.0
    out2 = R.render(b, cam, bg, W, H, SPP, DEPTH)
    assert np.array_equal(out2.view(np.uint64), ref_out)
    assert R.kernel_time_total(b)[1] == 2                    # counts exactly the launches made

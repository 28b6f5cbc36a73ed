"""Temporal accumulation on the GPU (rt_reproject, rt_reproject_device, rt_temporal_blend_device, csrc/rt_reproject.hip; progressive frames
with rt_progressive_set_view) against the specification of csrc/rt_reproject.h.

The reference for every comparison is the NumPy restatement of tests/reproject_cases.py (held to the host twin by
tests/test_reproject_host.py) on inputs made by kernels this feature does not touch: rt_query_camera / rt_query_camera_guide records of two
views and a 4-spp `render`.  What is required: 0 differing 64-bit words and equal counts, a NaN matching any NaN, on cornell (list), random
(one BVH, lens, moving spheres) and final (media), at 23 x 11 pixels (253: three whole waves and one of 61 lanes), with hostile sums and
counts written into the frame.  Neither kernel loops: a lane takes one pixel, or one pair of doubles, so there is no later trip to test."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import build_scene
from raytracinginrust_amd import _lib, render as R, scenes

import reproject_cases as RC

pytestmark = pytest.mark.gpu

GW, GH, DEPTH = 23, 11, 12
SEEDS = (0x5EED + 21, 0x5EED + 22, 0x5EED + 23)
SCENES = ("cornell", "random", "final")
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(scene, background, the scene's own camera and two more on a circle around its lookat, 3 and 6 degrees on)"""
    pbe = _lib.load()
    pb, cam, bg = build_scene(name, pbe, scenes.load_earthmap() if name == "final" else None)
    cams = [cam]
    for degrees in (3.0, 6.0):
        c = type(cam).from_buffer_copy(cam)
        c.lookfrom[:] = RC._orbit(tuple(cam.lookfrom), tuple(cam.lookat), degrees)
        cams.append(c)
    return pb, tuple(float(x) for x in bg), tuple(cams)


@functools.lru_cache(maxsize=None)
def _records(name, view, guide_samples=1):
    pb, _, cams = _scene(name)
    if guide_samples == 1:
        out = R.query_camera(pb, cams[view], GW, GH, 0, SEEDS[view])
    else:
        out = R.query_camera_guide(pb, cams[view], GW, GH, 0, guide_samples, SEEDS[view])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _frame(name):
    """A 4-spp frame of view 0 and per-pixel counts, with hostile entries written into both."""
    pb, bg, cams = _scene(name)
    s = R.render(pb, cams[0], bg, GW, GH, 4, DEPTH, SEEDS[0]).copy()
    n = np.full((GH, GW), 4, np.uint32)
    fs, fn = s.reshape(-1, 3), n.reshape(-1)
    fs[3::41, 0] = np.nan; fs[5::43, 1] = INF; fs[7::47, 2] = -INF; fs[11::53] = -0.0
    fn[13::37] = 0; fn[17::31] = 1; fn[19::29] = 2 ** 32 - 1; fn[2::7] = 9
    s.setflags(write=False); n.setflags(write=False)
    return s, n


def _agree(got, want, what=""):
    assert RC.differing_words(got[0], want[0]) == 0 and (got[1] == want[1]).all(), what


# ---------------------------------------------------------------- 1. the kernel is the specification, per scene class
@pytest.mark.parametrize("guide_samples", (1, 5))
@pytest.mark.parametrize("name", SCENES)
def test_reproject_equals_the_numpy_restatement(name, guide_samples):
    _, _, cams = _scene(name)
    s, n = _frame(name)
    g0, g1 = _records(name, 0, guide_samples), _records(name, 1, guide_samples)
    some = False
    for counts, samples, cap, sigma in ((n, 0, RC.CAP, RC.SIGMA), (None, 4, RC.CAP, RC.SIGMA), (n, 0, 3, (0.0, INF)), (None, 2 ** 40, 2 ** 31 - 1, (1.0, 1e-3)), (n, 0, 0, RC.SIGMA)):
        want = RC.numpy_reproject(s, counts, samples, g0, cams[0], g1, cap, sigma)
        _agree(R.reproject(s, g0, cams[0], g1, counts, samples, cap, sigma), want, (counts is None, cap, sigma))
        _agree(R.reproject_host(s, g0, cams[0], g1, counts, samples, cap, sigma), want, "host twin")
        some = some or (want[1] > 0).any()
    hit = g1[..., 0] != 0.0
    has = RC.numpy_reproject(s, n, 0, g0, cams[0], g1, RC.CAP, RC.SIGMA)[1] > 0
    print(f"{name} guide_samples={guide_samples}: {int(hit.sum())} hitting pixels, {int(has.sum())} with history")
    # a condition on the inputs, not a measurement: the comparison above covers pixels that get history and pixels that are refused it.  (How
    # many get it at 11 rows says nothing about a real frame: a pixel here is 2 to 4 degrees wide, and with 5 samples most pixels of the
    # final scene's boxes mix objects.)
    assert some and has.sum() >= 10 and (hit & ~has).sum() >= 10


# ---------------------------------------------------------------- 2. the _device forms
@pytest.mark.parametrize("name", ("cornell", "random"))
def test_device_forms_on_a_stream_of_the_callers(name):
    """Torch tensors on a stream of the caller's: word for word the restatement; nothing behind the last pixel is touched; the blend in both
    of its forms (16-byte aligned sums, and sums one double off) and in place."""
    import torch
    _, _, cams = _scene(name)
    s, n = _frame(name)
    g0, g1 = _records(name, 0), _records(name, 1)
    px = GW * GH
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678

    def up(a, dtype=None):
        return torch.from_numpy((a if dtype is None else a.view(dtype)).copy()).to(dev)
    with torch.cuda.stream(stream):
        d_s, d_n, d_g0, d_g1 = up(s), up(n, np.int32), up(g0), up(g1)
        d_hs = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        d_hn = torch.full((px + 1,), 77, dtype=torch.int32, device=dev)
        R.reproject_device(d_s, d_g0, cams[0], d_g1, GW, GH, d_hs, d_hn, d_prev_counts=d_n, max_history=RC.CAP, sigma=RC.SIGMA, stream=stream.cuda_stream)
        d_hs2 = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        d_hn2 = torch.full((px + 1,), 77, dtype=torch.int32, device=dev)
        R.reproject_device(d_s, d_g0, cams[0], d_g1, GW, GH, d_hs2, d_hn2, prev_samples=4, max_history=RC.CAP, sigma=RC.SIGMA, stream=stream.cuda_stream)
        # the blend of the frame with that history: out of place from aligned buffers, out of place from buffers one double off, in place
        d_bs = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        d_bn = torch.full((px + 1,), 77, dtype=torch.int32, device=dev)
        R.temporal_blend_device(d_s, d_hs, d_hn, GW, GH, d_bs, d_bn, d_counts=d_n, stream=stream.cuda_stream)
        flat = torch.full((3 * px + 2,), canary, dtype=torch.float64, device=dev)
        flat[1:3 * px + 1] = d_s.reshape(-1)
        d_bn2 = torch.full((px + 1,), 77, dtype=torch.int32, device=dev)
        R.temporal_blend_device(flat[1:], d_hs, d_hn, GW, GH, None, d_bn2, samples=4, stream=stream.cuda_stream)          # sums in place, one double off 16
        d_s3, d_n3 = d_s.clone(), d_n.clone()
        R.temporal_blend_device(d_s3, d_hs, d_hn, GW, GH, d_counts=d_n3, stream=stream.cuda_stream)                       # everything in place
    stream.synchronize()
    want = RC.numpy_reproject(s, n, 0, g0, cams[0], g1, RC.CAP, RC.SIGMA)
    want2 = RC.numpy_reproject(s, None, 4, g0, cams[0], g1, RC.CAP, RC.SIGMA)
    hs, hn = d_hs.cpu().numpy(), d_hn.cpu().numpy().view(np.uint32)
    _agree((hs[:px].reshape(GH, GW, 3), hn[:px].reshape(GH, GW)), want)
    _agree((d_hs2.cpu().numpy()[:px].reshape(GH, GW, 3), d_hn2.cpu().numpy().view(np.uint32)[:px].reshape(GH, GW)), want2)
    assert (hs[px] == canary).all() and hn[px] == 77 and (d_hs2.cpu().numpy()[px] == canary).all() and d_hn2.cpu().numpy()[px] == 77
    bs, bn = RC.numpy_blend(s, n, 0, want[0], want[1])
    _agree((d_bs.cpu().numpy()[:px].reshape(GH, GW, 3), d_bn.cpu().numpy().view(np.uint32)[:px].reshape(GH, GW)), (bs, bn))
    assert (d_bs.cpu().numpy()[px] == canary).all() and d_bn.cpu().numpy()[px] == 77
    _agree((d_s3.cpu().numpy(), d_n3.cpu().numpy().view(np.uint32)), (bs, bn))
    bs2, bn2 = RC.numpy_blend(s, None, 4, want[0], want[1])
    f = flat.cpu().numpy()
    _agree((f[1:3 * px + 1].reshape(GH, GW, 3), d_bn2.cpu().numpy().view(np.uint32)[:px].reshape(GH, GW)), (bs2, bn2))
    assert f[0] == canary and f[3 * px + 1] == canary and d_bn2.cpu().numpy()[px] == 77
    assert (bn == 2 ** 32 - 1).any() and (bn2 > 4).any()                                        # a count held at 2^32 - 1, and history that counts


def test_device_form_arguments(pbe):
    """What the device forms refuse before anything is launched."""
    lib = pbe.lib
    _, _, cams = _scene("cornell")
    sg = (C.c_double * 2)(*RC.SIGMA)
    d = C.c_void_p(0x1000)

    def err():
        return lib.rt_last_error().decode()
    assert lib.rt_reproject_device(d, None, 4, C.c_void_p(0x1008), C.byref(cams[0]), d, GW, GH, 8, sg, 0, d, d, None) != 0 and "16-byte aligned" in err()
    assert lib.rt_reproject_device(C.c_void_p(0x1004), None, 4, d, C.byref(cams[0]), d, GW, GH, 8, sg, 0, d, d, None) != 0 and "8-byte aligned" in err()
    assert lib.rt_reproject_device(d, C.c_void_p(0x1002), 4, d, C.byref(cams[0]), d, GW, GH, 8, sg, 0, d, d, None) != 0 and "4-byte aligned" in err()
    assert lib.rt_reproject_device(d, None, 0, d, C.byref(cams[0]), d, GW, GH, 8, sg, 0, d, d, None) != 0 and "prev_samples" in err()
    assert lib.rt_reproject_device(d, None, 4, d, C.byref(cams[0]), d, GW, GH, 8, sg, 0, None, d, None) != 0 and "null argument" in err()
    assert lib.rt_temporal_blend_device(d, None, 4, d, d, GW, 1, d, d, None) != 0 and "W and H" in err()
    assert lib.rt_temporal_blend_device(d, None, 4, C.c_void_p(0x1004), d, GW, GH, d, d, None) != 0 and "8-byte aligned" in err()
    assert lib.rt_temporal_blend_device(d, None, 4, d, None, GW, GH, d, d, None) != 0 and "null argument" in err()


# ---------------------------------------------------------------- 3. progressive frames
U = 2.0 ** -53


def _resolve(s, n):
    return R.adaptive_resolve_rgb8_host(s, n)[0]


@pytest.mark.parametrize("name,guide_samples", (("cornell", 1), ("cornell", 5), ("random", 1)))
def test_progressive_set_view_chains_the_history(name, guide_samples):
    pb, bg, cams = _scene(name)
    cap, sigma = 24, RC.SIGMA
    zeros = np.zeros((GH, GW, 3))
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0], guide_samples=guide_samples) as fr:
        assert fr.history_info() == {"views": 0, "pixels": 0} and not fr.history()[1].any()
        with pytest.raises(R.RenderError, match="0 samples and no history"):
            fr.rgb8_temporal()
        fr.add(4)
        s1 = fr.sum()
        image_before = fr.rgb8()[0]
        assert (fr.rgb8_temporal() == image_before).all()          # without a history the blend is the frame
        # the first move
        fr.set_view(cams[1], SEEDS[1], cap, sigma)
        h1 = fr.history()
        want1 = R.reproject_host(s1, _records(name, 0, guide_samples), cams[0], _records(name, 1, guide_samples), None, 4, cap, sigma)
        _agree(h1, want1, "the first history")
        _agree(want1, RC.numpy_reproject(s1, None, 4, _records(name, 0, guide_samples), cams[0], _records(name, 1, guide_samples), cap, sigma))
        assert fr.history_info() == {"views": 1, "pixels": int((want1[1] > 0).sum())} and (want1[1] > 0).sum() > 50 and (want1[1] <= 4).all()
        assert fr.samples == 0
        with pytest.raises(R.RenderError):
            fr.rgb8()                                               # every call that existed before ignores the history
        # the preview in the instant after the move: 0 samples of the new view
        b0 = R.temporal_blend_host(zeros, h1[0], h1[1], None, 0)
        assert (fr.rgb8_temporal() == _resolve(*b0)).all()
        # the frame is a fresh frame of the new view and seed
        smp = fr.add(4, want_samples=True)
        s2 = fr.sum()
        with R.Progressive(pb, cams[1], bg, GW, GH, DEPTH, SEEDS[1]) as fresh:
            fresh_smp = fresh.add(4, want_samples=True)
            fresh_sum = fresh.sum()
        assert RC.differing_words(smp, fresh_smp) == 0 and fr.samples == 4
        finite = np.isfinite(smp).all(axis=(2, 3))
        bound = 2.0 * (3 * U / (1.0 - 3 * U)) * np.abs(np.where(np.isfinite(smp), smp, 0.0)).sum(axis=2)
        assert (np.abs(np.where(finite[..., None], s2 - fresh_sum, 0.0)) <= bound).all()
        image, changed = fr.rgb8()
        assert (image == _resolve(s2, np.full((GH, GW), 4, np.uint32))).all() and changed == GW * GH
        _agree(fr.history(), h1, "a pass leaves the history alone")
        # the temporal resolves
        b1 = R.temporal_blend_host(s2, h1[0], h1[1], None, 4)
        assert (fr.rgb8_temporal() == _resolve(*b1)).all()
        assert (_resolve(*b1) != image).any()                       # ... which is not the plain resolve
        guide = _records(name, 1, guide_samples)
        for flags in (0, R.RT_DENOISE_SAME_MATERIAL):
            den = R.denoise_frame_host(b1[0], guide, counts=b1[1], iterations=2, sigma=R.DENOISE_SIGMA, flags=flags)
            assert (fr.rgb8_temporal(2, R.DENOISE_SIGMA, flags) == _resolve(den, b1[1])).all(), flags
        assert RC.differing_words(fr.sum(), s2) == 0 and (fr.rgb8_copy()[0] == image).all()
        # the second move: the history chains
        fr.set_view(cams[2], SEEDS[2], cap, sigma)
        want2 = R.reproject_host(b1[0], guide, cams[1], _records(name, 2, guide_samples), b1[1], 0, cap, sigma)
        _agree(fr.history(), want2, "the chained history")
        assert fr.history_info() == {"views": 2, "pixels": int((want2[1] > 0).sum())} and (want2[1] > 4).any() and (want2[1] <= 8).all()
        # max_history = 0 is a plain change of view; reset drops the history
        fr.add(2)
        fr.set_view(cams[0], SEEDS[0], 0, sigma)
        assert not fr.history()[1].any() and not fr.history()[0].any() and fr.history_info() == {"views": 3, "pixels": 0} and fr.samples == 0
        fr.add(2)
        fr.set_view(cams[1], SEEDS[1], cap, sigma)
        assert fr.history_info()["pixels"] > 50
        fr.reset()
        assert not fr.history()[1].any() and fr.history_info() == {"views": 4, "pixels": 0}
        with pytest.raises(R.RenderError, match="0 samples and no history"):
            fr.rgb8_temporal()


def test_set_view_arguments(pbe):
    pb, bg, cams = _scene("cornell")
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0], adaptive=True) as fr:
        fr.add(2)
        with pytest.raises(R.RenderError, match="adaptive frame"):
            fr.set_view(cams[1], SEEDS[1])
        with pytest.raises(R.RenderError, match="adaptive frame"):
            fr.rgb8_temporal()
        assert fr.samples == 2
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0]) as fr:
        fr.add(2)
        before = fr.sum()
        for kw, word in (({"max_history": 2 ** 31}, "max_history"), ({"sigma": (1.5, 0.01)}, "normal_min"), ({"sigma": (0.9, 0.0)}, "sigma_p")):
            with pytest.raises(R.RenderError, match=word):
                fr.set_view(cams[1], SEEDS[1], **kw)
        with pytest.raises(R.RenderError, match="iterations"):
            fr.rgb8_temporal(9)
        assert fr.samples == 2 and RC.differing_words(fr.sum(), before) == 0 and fr.history_info() == {"views": 0, "pixels": 0}

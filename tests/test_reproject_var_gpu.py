"""Temporal variance on the GPU (rt_reproject_variance, rt_reproject_variance_device, rt_temporal_blend_variance_device,
csrc/rt_reproject_var.hip; progressive frames with moments through rt_progressive_set_view, rt_progressive_read_history_variance and
rt_progressive_resolve_temporal_variance_rgb8) against the specification of csrc/rt_reproject_var.h.

The reference for every comparison is the NumPy restatement of tests/reproject_var_cases.py (held to the host twin by
tests/test_reproject_var_host.py), or the host twins composed as include/rt_amd.h says, on inputs made by kernels this feature does not
touch: the records, scenes, cameras and hostile 4-spp frames of tests/test_reproject_gpu.py, and the variance of a real frame with moments
(2 passes of 2 samples).  What is required: 0 differing 64-bit words, equal counts and equal bytes, on cornell (list), random (one BVH) and
final (media) at 23 x 11 pixels (253: three whole waves and one of 61 lanes).  Neither kernel loops: a lane takes one pixel."""
import ctypes as C
import functools

import numpy as np
import pytest

from raytracinginrust_amd import render as R

import reproject_cases as RC
import reproject_var_cases as RV
import test_reproject_gpu as TG

pytestmark = pytest.mark.gpu

GW, GH, DEPTH, SEEDS = TG.GW, TG.GH, TG.DEPTH, TG.SEEDS
INF = float("inf")
VS = R.DENOISE_VARIANCE_SIGMA


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _moments_frame(name):
    """(sums, variance of the mean) of view 0 after 2 passes of 2 samples, and the same variance with hostile entries."""
    pb, bg, cams = TG._scene(name)
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0], moments=True) as fr:
        fr.add(2); fr.add(2)
        s, v = fr.sum(), fr.variance()
    hostile = v.copy()
    f = hostile.reshape(-1, 3)
    f[2::23, 0] = np.nan; f[4::29, 1] = INF; f[6::31, 2] = -INF; f[8::37, 1] = -0.25; f[10::41] = -0.0; f[12::43, 0] = 5e-324; f[1::47, 2] = 1e300
    for a in (s, v, hostile):
        a.setflags(write=False)
    return s, v, hostile


def _agree(got, want, what=""):
    assert RC.differing_words(got[0], want[0]) == 0 and (got[1] == want[1]).all() and RC.differing_words(got[2], want[2]) == 0, what


def _known_share(hn, hv):
    return int(((hn > 0) & RV.known(hv).all(axis=-1)).sum())


# ---------------------------------------------------------------- 1. the fused kernel is the specification, per scene class
@pytest.mark.parametrize("name", TG.SCENES)
def test_reproject_variance_equals_the_numpy_restatement(name):
    _, _, cams = TG._scene(name)
    s_h, n_h = TG._frame(name)
    s_m, v_m, v_h = _moments_frame(name)
    g0, g1 = TG._records(name, 0), TG._records(name, 1)
    for s, counts, samples, var, cap, sigma in ((s_m, None, 4, v_m, RC.CAP, RC.SIGMA), (s_h, n_h, 0, v_h, RC.CAP, RC.SIGMA), (s_h, n_h, 0, v_m, 3, (0.0, INF)),
                                                (s_m, None, 2 ** 40, v_h, 2 ** 31 - 1, (1.0, 1e-3)), (s_h, n_h, 0, v_h, 0, RC.SIGMA)):
        want = RV.numpy_reproject_variance(s, counts, samples, var, g0, cams[0], g1, cap, sigma)
        what = (counts is None, var is v_h, cap, sigma)
        _agree(R.reproject_variance(s, var, g0, cams[0], g1, counts, samples, cap, sigma), want, what)
        _agree(R.reproject_variance_host(s, var, g0, cams[0], g1, counts, samples, cap, sigma), want, "host twin")
        plain = R.reproject(s, g0, cams[0], g1, counts, samples, cap, sigma)                  # the parent's kernel: the same sums and counts
        assert (bits(plain[0]) == bits(want[0])).all() and (plain[1] == want[1]).all(), what
    _, hn, hv = RV.numpy_reproject_variance(s_m, None, 4, v_m, g0, cams[0], g1, RC.CAP, RC.SIGMA)
    _, hn2, hv2 = RV.numpy_reproject_variance(s_h, n_h, 0, v_h, g0, cams[0], g1, RC.CAP, RC.SIGMA)
    print(f"{name}: {int((hn > 0).sum())} pixels with history, {_known_share(hn, hv)} with known variance; hostile: {int((hn2 > 0).sum())}, {_known_share(hn2, hv2)} known, "
          f"{int(((hn2 > 0) & (hv2 == INF).all(axis=-1)).sum())} unknown")
    # a condition on the inputs, not a measurement: a tenth of the frame's pixels carry a known variance
    assert _known_share(hn, hv) >= GW * GH / 10.0


# ---------------------------------------------------------------- 2. the _device forms
@pytest.mark.parametrize("name", ("cornell", "random"))
def test_device_forms_on_a_stream_of_the_callers(name):
    """Torch tensors on a stream of the caller's: word for word the restatement; nothing behind the last pixel of any of the three outputs
    is touched; the blend of variances out of place, in place with counts, in place without counts, and without a variance frame."""
    import torch
    _, _, cams = TG._scene(name)
    s, n = TG._frame(name)
    _, _, var = _moments_frame(name)
    g0, g1 = TG._records(name, 0), TG._records(name, 1)
    px = GW * GH
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    rs = np.random.RandomState(9)
    new_n = rs.randint(0, 5, (GH, GW)).astype(np.uint32)
    new_v = RV.variance_frame(5, np.maximum(new_n, 1), True)

    def up(a, dtype=None):
        return torch.from_numpy((a if dtype is None else a.view(dtype)).copy()).to(dev)
    with torch.cuda.stream(stream):
        d_s, d_n, d_v, d_g0, d_g1 = up(s), up(n, np.int32), up(var), up(g0), up(g1)
        d_hs = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        d_hv = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        d_hn = torch.full((px + 1,), 77, dtype=torch.int32, device=dev)
        R.reproject_variance_device(d_s, d_v, d_g0, cams[0], d_g1, GW, GH, d_hs, d_hn, d_hv, d_prev_counts=d_n, max_history=RC.CAP, sigma=RC.SIGMA, stream=stream.cuda_stream)
        d_nn, d_nv = up(new_n, np.int32), up(new_v)
        d_out = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        R.temporal_blend_variance_device(d_nv, d_hv, d_hn, px, d_out, d_counts=d_nn, stream=stream.cuda_stream)
        d_in1 = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev); d_in1[:px] = d_nv.reshape(-1, 3)
        R.temporal_blend_variance_device(d_in1, d_hv, d_hn, px, d_counts=d_nn, stream=stream.cuda_stream)              # in place, with counts
        d_in2 = d_in1.clone(); d_in2[:px] = d_nv.reshape(-1, 3)
        R.temporal_blend_variance_device(d_in2, d_hv, d_hn, px, samples=3, stream=stream.cuda_stream)                  # in place, without counts
        d_none = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        R.temporal_blend_variance_device(None, d_hv, d_hn, px, d_none, samples=3, stream=stream.cuda_stream)           # no variance frame
    stream.synchronize()
    want = RV.numpy_reproject_variance(s, n, 0, var, g0, cams[0], g1, RC.CAP, RC.SIGMA)
    hs, hv, hn = d_hs.cpu().numpy(), d_hv.cpu().numpy(), d_hn.cpu().numpy().view(np.uint32)
    _agree((hs[:px].reshape(GH, GW, 3), hn[:px].reshape(GH, GW), hv[:px].reshape(GH, GW, 3)), want)
    assert (hs[px] == canary).all() and (hv[px] == canary).all() and hn[px] == 77
    for d_got, v, counts, samples in ((d_out, new_v, new_n, 0), (d_in1, new_v, new_n, 0), (d_in2, new_v, None, 3), (d_none, None, None, 3)):
        got = d_got.cpu().numpy()
        assert RC.differing_words(got[:px].reshape(GH, GW, 3), RV.numpy_blend_variance(v, counts, samples, want[2], want[1])) == 0, (v is None, counts is None)
        assert (got[px] == canary).all()


def test_device_form_arguments(pbe):
    """What the device forms refuse before anything is launched."""
    lib = pbe.lib
    _, _, cams = TG._scene("cornell")
    sg = (C.c_double * 2)(*RC.SIGMA)
    d = C.c_void_p(0x1000)

    def err():
        return lib.rt_last_error().decode()
    cam = C.byref(cams[0])
    assert lib.rt_reproject_variance_device(d, None, 4, d, C.c_void_p(0x1008), cam, d, GW, GH, 8, sg, 0, d, d, d, None) != 0 and "16-byte aligned" in err()
    assert lib.rt_reproject_variance_device(d, None, 4, C.c_void_p(0x1004), d, cam, d, GW, GH, 8, sg, 0, d, d, d, None) != 0 and "8-byte aligned" in err()
    assert lib.rt_reproject_variance_device(d, None, 4, d, d, cam, d, GW, GH, 8, sg, 0, d, d, C.c_void_p(0x1004), None) != 0 and "8-byte aligned" in err()
    assert lib.rt_reproject_variance_device(d, C.c_void_p(0x1002), 4, d, d, cam, d, GW, GH, 8, sg, 0, d, d, d, None) != 0 and "4-byte aligned" in err()
    assert lib.rt_reproject_variance_device(d, None, 0, d, d, cam, d, GW, GH, 8, sg, 0, d, d, d, None) != 0 and "prev_samples" in err()
    assert lib.rt_reproject_variance_device(d, None, 4, None, d, cam, d, GW, GH, 8, sg, 0, d, d, d, None) != 0 and "null argument" in err()
    assert lib.rt_reproject_variance_device(d, None, 4, d, d, cam, d, GW, GH, 8, sg, 0, d, d, None, None) != 0 and "null argument" in err()
    assert lib.rt_temporal_blend_variance_device(d, None, 4, C.c_void_p(0x1004), d, 8, d, None) != 0 and "8-byte aligned" in err()
    assert lib.rt_temporal_blend_variance_device(d, C.c_void_p(0x1002), 4, d, d, 8, d, None) != 0 and "4-byte aligned" in err()
    assert lib.rt_temporal_blend_variance_device(d, None, 4, d, None, 8, d, None) != 0 and "null argument" in err()
    assert lib.rt_temporal_blend_variance_device(d, None, 4, d, d, 2 ** 31, d, None) != 0 and "2^31 - 1" in err()


# ---------------------------------------------------------------- 3. progressive frames with moments
def _resolve(s, n):
    return R.adaptive_resolve_rgb8_host(s, n)[0]


def _host_resolve(sums, samples, var, hist, guide, albedo=None, albedo_samples=0):
    """include/rt_amd.h's composition for rt_progressive_resolve_temporal_variance_rgb8, from the host twins."""
    hs, hn, hv = hist
    bs, bn = R.temporal_blend_host(sums, hs, hn, None, samples)
    bv = R.temporal_blend_variance_host(var, hv, hn, None, samples)
    den = R.denoise_frame_host(bs, guide, counts=bn, var=bv, albedo_sum=albedo, albedo_samples=albedo_samples if albedo is not None else 1, iterations=2, sigma=VS)
    return _resolve(den, bn), (bs, bn, bv)


@pytest.mark.parametrize("name,first_passes", (("cornell", 2), ("random", 2), ("cornell", 1)))
def test_a_frame_with_moments_carries_its_variance_through_two_moves(name, first_passes):
    pb, bg, cams = TG._scene(name)
    cap, sigma = 24, RC.SIGMA
    zeros, zeros_n = np.zeros((GH, GW, 3)), np.zeros((GH, GW), np.uint32)
    rec = [TG._records(name, k) for k in range(3)]
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0], moments=True) as fr:
        assert (bits(fr.history_variance()) == 0).all()
        for _ in range(first_passes):
            fr.add(2)
        n1 = 2 * first_passes
        s1 = fr.sum()
        v1 = fr.variance() if first_passes >= 2 else None           # one pass: the frame has no variance, and set_view takes NULL
        # the first move: (BV) of the frame's variance with a history that is not there, then (V)
        fr.set_view(cams[1], SEEDS[1], cap, sigma)
        pv1 = R.temporal_blend_variance_host(v1, zeros, zeros_n, None, n1)
        want1 = R.reproject_variance_host(s1, pv1, rec[0], cams[0], rec[1], None, n1, cap, sigma)
        h1 = fr.history() + (fr.history_variance(),)
        _agree(h1, want1, "the first history")
        _agree(want1, RV.numpy_reproject_variance(s1, None, n1, RV.numpy_blend_variance(v1, None, n1, zeros, zeros_n), rec[0], cams[0], rec[1], cap, sigma))
        has = h1[1] > 0
        assert fr.history_info()["pixels"] == int(has.sum()) > 50 and fr.samples == 0
        if first_passes == 1:
            assert (h1[2][has] == INF).all() and (bits(h1[2][~has]) == 0).all()
        else:
            assert _known_share(h1[1], h1[2]) >= GW * GH / 10.0
        # the resolve through the variance stop: in the instant after the move, after one pass, after two
        guide = rec[1]
        image, _ = _host_resolve(zeros, 0, None, h1, guide)
        assert (fr.rgb8_temporal(2, VS, variance=True) == image).all(), "0 new samples"
        fr.add(2)
        image, _ = _host_resolve(fr.sum(), 2, None, h1, guide)
        assert (fr.rgb8_temporal(2, VS, variance=True) == image).all(), "one pass"
        assert (fr.rgb8_temporal(2, VS, variance=True) != fr.rgb8_temporal(2)).any()                # ... which is not the plain filter's resolve
        fr.add(2)
        s2, q2, v2 = fr.sum(), fr.sq_sum(), fr.variance()
        image, (bs, bn, bv) = _host_resolve(s2, 4, v2, h1, guide)
        assert (fr.rgb8_temporal(2, VS, variance=True) == image).all(), "two passes"
        assert (fr.rgb8_temporal(2, (INF, 0.5, 0.02), variance=True) != image).any()                # the stop does something
        assert RC.differing_words(fr.sum(), s2) == 0 and RC.differing_words(fr.sq_sum(), q2) == 0 and fr.passes == 2
        _agree(fr.history() + (fr.history_variance(),), h1, "passes and resolves leave the history alone")
        # the second move: the chained state
        fr.set_view(cams[2], SEEDS[2], cap, sigma)
        want2 = R.reproject_variance_host(bs, bv, guide, cams[1], rec[2], bn, 0, cap, sigma)
        _agree(fr.history() + (fr.history_variance(),), want2, "the chained history")
        assert _known_share(want2[1], want2[2]) >= GW * GH / 10.0 and (want2[1] > 4).any()
        # max_history = 0 is a plain change of view; reset clears the history variance
        fr.add(2)
        fr.set_view(cams[0], SEEDS[0], 0, sigma)
        assert (bits(fr.history_variance()) == 0).all() and not fr.history()[1].any()
        fr.add(2); fr.add(2)
        fr.set_view(cams[1], SEEDS[1], cap, sigma)
        assert (fr.history_variance() != 0.0).any()
        fr.reset()
        assert (bits(fr.history_variance()) == 0).all() and not fr.history()[1].any()
        with pytest.raises(R.RenderError, match="0 samples and no history"):
            fr.rgb8_temporal(2, VS, variance=True)


def test_the_variance_resolve_with_albedo_demodulation_on_textures(pbe):
    from test_denoise_albedo_gpu import textured_scene
    b, cam, bg = textured_scene(pbe)
    cam2 = type(cam).from_buffer_copy(cam)
    cam2.lookfrom[:] = RC._orbit(tuple(cam.lookfrom), tuple(cam.lookat), 3.0)
    zeros, zeros_n = np.zeros((GH, GW, 3)), np.zeros((GH, GW), np.uint32)
    with R.Progressive(b, cam, bg, GW, GH, DEPTH, 41, moments=True) as fr:
        fr.add(2); fr.add(2)
        s1, v1 = fr.sum(), fr.variance()
        fr.set_view(cam2, 42, 24, RC.SIGMA)
        g0, g1 = R.query_camera(b, cam, GW, GH, 0, 41), R.query_camera(b, cam2, GW, GH, 0, 42)
        h = R.reproject_variance_host(s1, R.temporal_blend_variance_host(v1, zeros, zeros_n, None, 4), g0, cam, g1, None, 4, 24, RC.SIGMA)
        _agree(fr.history() + (fr.history_variance(),), h)
        assert _known_share(h[1], h[2]) >= GW * GH / 10.0
        fr.add(2)
        albedo = R.query_camera_albedo(b, cam2, GW, GH, 0, 4, 42)
        image, _ = _host_resolve(fr.sum(), 2, None, h, g1, albedo, 4)
        got = fr.rgb8_temporal(2, VS, variance=True, albedo_samples=4)
        assert (got == image).all()
        assert (got != _host_resolve(fr.sum(), 2, None, h, g1)[0]).any() and fr.albedo_info()[0] == 4


def test_a_frame_without_moments_takes_the_parents_path_and_refusals():
    pb, bg, cams = TG._scene("cornell")
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0]) as fr:
        fr.add(4)
        s1 = fr.sum()
        fr.set_view(cams[1], SEEDS[1], 24, RC.SIGMA)
        want = R.reproject_host(s1, TG._records("cornell", 0), cams[0], TG._records("cornell", 1), None, 4, 24, RC.SIGMA)
        h = fr.history()
        assert RC.differing_words(h[0], want[0]) == 0 and (h[1] == want[1]).all()
        fr.add(4)
        b = R.temporal_blend_host(fr.sum(), h[0], h[1], None, 4)
        assert (fr.rgb8_temporal() == _resolve(*b)).all()
        den = R.denoise_frame_host(b[0], TG._records("cornell", 1), counts=b[1], iterations=2, sigma=R.DENOISE_SIGMA)
        assert (fr.rgb8_temporal(2, R.DENOISE_SIGMA) == _resolve(den, b[1])).all()
        with pytest.raises(R.RenderError, match="no moments"):
            fr.rgb8_temporal(2, VS, variance=True)
        with pytest.raises(R.RenderError, match="no moments"):
            fr.history_variance()
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0], adaptive=True) as fr:
        fr.add(2)
        with pytest.raises(R.RenderError, match="adaptive frame"):
            fr.rgb8_temporal(2, VS, variance=True)
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0], moments=True) as fr:
        with pytest.raises(R.RenderError, match="0 samples and no history"):
            fr.rgb8_temporal(2, VS, variance=True)
        fr.add(2)
        for k in (0, 9):
            with pytest.raises(R.RenderError, match="iterations"):
                fr.rgb8_temporal(k, VS, variance=True)
        with pytest.raises(R.RenderError, match="sigma_v"):
            fr.rgb8_temporal(2, (0.0, 0.5, 0.02), variance=True)
        with pytest.raises(ValueError):
            fr.rgb8_temporal(2, albedo_samples=4)
        # without a history and with one pass every variance is unknown: the resolve is the frame filter's with an all-+inf variance frame
        s = fr.sum()
        den = R.denoise_frame_host(s, TG._records("cornell", 0), counts=np.full((GH, GW), 2, np.uint32), var=np.full((GH, GW, 3), INF), iterations=2, sigma=VS)
        assert (fr.rgb8_temporal(2, VS, variance=True) == _resolve(den, np.full((GH, GW), 2, np.uint32))).all()


def test_a_history_taken_before_the_moments_were_enabled_has_an_unknown_variance():
    """set_view on a plain frame, then rt_progressive_enable_moments at 0 samples: the history is there and knows no variance — +inf where
    H_cnt > 0, +0.0 elsewhere, as (V) writes a pixel none of whose taps is var-known — and from there everything goes on as specified."""
    pb, bg, cams = TG._scene("cornell")
    zeros = np.zeros((GH, GW, 3))
    rec = [TG._records("cornell", k) for k in range(3)]
    with R.Progressive(pb, cams[0], bg, GW, GH, DEPTH, SEEDS[0]) as fr:
        fr.add(4)
        fr.set_view(cams[1], SEEDS[1], 24, RC.SIGMA)
        hs, hn = fr.history()
        fr.enable_moments()
        hv = fr.history_variance()
        has = hn > 0
        assert has.sum() > 50 and (hv[has] == INF).all() and (bits(hv[~has]) == 0).all()
        assert RC.differing_words(fr.history()[0], hs) == 0 and (fr.history()[1] == hn).all()
        h = (hs, hn, hv)
        assert (fr.rgb8_temporal(2, VS, variance=True) == _host_resolve(zeros, 0, None, h, rec[1])[0]).all(), "0 new samples"
        fr.add(2); fr.add(2)
        image, (bs, bn, bv) = _host_resolve(fr.sum(), 4, fr.variance(), h, rec[1])                  # (BV)'s "only V known" row wherever there is history
        assert (fr.rgb8_temporal(2, VS, variance=True) == image).all() and RV.known(bv).all()
        fr.set_view(cams[2], SEEDS[2], 24, RC.SIGMA)
        _agree(fr.history() + (fr.history_variance(),), R.reproject_variance_host(bs, bv, rec[1], cams[1], rec[2], bn, 0, 24, RC.SIGMA), "the chained history")

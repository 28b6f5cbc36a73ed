"""The variance-guided denoiser on the GPU (rt_denoise_variance, rt_denoise_variance_device, rt_moments_variance_device,
rt_progressive_variance, rt_progressive_resolve_denoised_variance_rgb8; csrc/rt_denoise_var.hip) against the host twins, which
tests/test_denoise_variance_host.py holds to the specification: 0 differing 64-bit words on every frame shape, iteration count, sigma and
flag value of tests/denoise_variance_cases.py, with steps 1 and 2 both from LDS tiles and read directly."""
import os
import subprocess

import numpy as np
import pytest

from raytracinginrust_amd import _lib, render as R, scenes

import denoise_variance_cases as VC
import moments_cases as MC
from denoise_variance_cases import differing_words

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the kernels are the host twins
@pytest.mark.parametrize("no_lds", [False, True], ids=["as-shipped", "no-lds"])
@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_twin(monkeypatch, shape, no_lds):
    if no_lds:
        monkeypatch.setenv("RT_DENOISE_NO_LDS", "1")
    else:
        monkeypatch.delenv("RT_DENOISE_NO_LDS", raising=False)
    rgb, var, hits = VC.case(shape)
    for k, sigma, flags in VC.settings_for(shape):
        got, got_v = R.denoise_variance(rgb, VC.SAMPLES, var, hits, k, sigma, flags, want_var=True)
        want, want_v = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, k, sigma, flags, want_var=True)
        assert differing_words(got, want) == 0, (shape, k, sigma, flags)
        assert differing_words(got_v, want_v) == 0, (shape, k, sigma, flags)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned-16", "8-bytes-off"])
@pytest.mark.parametrize("shape", MC.SHAPES + ((67, 130),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_variance_kernel_equals_host_twin(shape, offset):
    import torch
    if shape in MC.SHAPES:
        S, Q, samples, passes = MC.state(shape)
    else:                                                       # more than one workgroup, an odd number of doubles with the offset
        rs = np.random.RandomState(3)
        S = rs.uniform(0.0, 16.0, shape + (3,)); Q = S * S / 16.0 + rs.uniform(-0.01, 0.5, shape + (3,)); samples, passes = 16, 4
    want = R.moments_variance_host(S, Q, samples, passes)
    H, W = shape
    n = H * W * 3
    canary = 12345.678
    bufs = [torch.full((n + 3,), canary, dtype=torch.float64, device="cuda") for _ in range(3)]
    d_s, d_q, d_v = (b[offset:offset + n] for b in bufs)
    assert all(b.data_ptr() % 16 == 0 for b in bufs) and d_s.data_ptr() % 16 == 8 * offset
    d_s.copy_(torch.from_numpy(S.reshape(-1).copy())); d_q.copy_(torch.from_numpy(Q.reshape(-1).copy()))
    R.moments_variance_device(d_s, d_q, samples, passes, W, H, d_v, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = bufs[2].cpu().numpy()
    assert differing_words(out[offset:offset + n].reshape(H, W, 3), want) == 0
    assert np.all(out[:offset] == canary) and np.all(out[offset + n:] == canary)
    if offset == 0:
        assert differing_words(R.moments_variance(S, Q, samples, passes), want) == 0


# ---------------------------------------------------------------- 2. device pointers, a stream and a workspace of the caller's
def test_device_form_on_a_stream_in_place_and_a_short_workspace():
    import torch
    H, W = 67, 130
    rgb, var, hits = VC.case((H, W))
    k, sigma, flags = 4, VC.SIGMAS[0], 1
    want, want_v = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, k, sigma, flags, want_var=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    need = R.denoise_variance_workspace_bytes(W, H)
    assert need == W * H * 128
    with torch.cuda.stream(stream):
        d_sum = torch.from_numpy(rgb.copy()).to(dev)
        d_var = torch.from_numpy(var.copy()).to(dev)
        d_hits = torch.from_numpy(hits.copy()).to(dev)
        d_out = torch.full((H * W + 1, 3), canary, dtype=torch.float64, device=dev)
        d_vout = torch.full((H * W + 1,), canary, dtype=torch.float64, device=dev)
        d_ws = torch.full((need // 8 + 2,), canary, dtype=torch.float64, device=dev)
        R.denoise_variance_device(d_sum, VC.SAMPLES, d_var, d_hits, W, H, d_out, d_vout, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
        d_in_place = d_sum.clone()
        R.denoise_variance_device(d_in_place, VC.SAMPLES, d_var, d_hits, W, H, None, None, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
    stream.synchronize()
    out = d_out.cpu().numpy(); vout = d_vout.cpu().numpy()
    assert differing_words(out[:-1].reshape(H, W, 3), want) == 0 and np.all(out[-1] == canary)
    assert differing_words(vout[:-1].reshape(H, W), want_v) == 0 and vout[-1] == canary
    assert np.all(d_ws.cpu().numpy()[need // 8:] == canary)                          # nothing behind the workspace's 128 bytes per pixel
    assert differing_words(d_sum.cpu().numpy(), rgb) == 0 and differing_words(d_var.cpu().numpy(), var) == 0      # the inputs are left alone
    assert differing_words(d_in_place.cpu().numpy(), want) == 0                       # in place, and without var_out
    # one byte short: refused with a message, nothing written
    with torch.cuda.stream(stream):
        d_out2 = torch.full((H * W, 3), canary, dtype=torch.float64, device=dev)
        d_vout2 = torch.full((H * W,), canary, dtype=torch.float64, device=dev)
        with pytest.raises(R.RenderError, match="workspace too small"):
            R.denoise_variance_device(d_sum, VC.SAMPLES, d_var, d_hits, W, H, d_out2, d_vout2, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need - 1)
    stream.synchronize()
    assert np.all(d_out2.cpu().numpy() == canary) and np.all(d_vout2.cpu().numpy() == canary)
    # the workspace the wrapper allocates itself
    ws = R.denoise_variance_device(d_sum, VC.SAMPLES, d_var, d_hits, W, H, d_out2, None, None, k, sigma, flags)
    torch.cuda.synchronize()
    assert ws.numel() == need and differing_words(d_out2.cpu().numpy().reshape(H, W, 3), want) == 0


# ---------------------------------------------------------------- 3. progressive frames
W_P = H_P = 40
DEPTH_P, SEED_P = 12, 0x5EED + 11


def _expected(frame, hits, k, sigma, flags):
    N = frame.samples
    V = R.moments_variance_host(frame.sum(), frame.sq_sum(), N, frame.passes)
    return R.format_image(R.denoise_variance_host(frame.sum(), N, V, hits, k, sigma, flags), N)


def test_progressive_variance_guided_resolve(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    hits = R.query_camera(b, cam, W_P, H_P, 0, SEED_P)
    k, sigma = 3, (3.0, 0.5, 0.02)
    with R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P, moments=True) as frame, R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P, moments=True) as plain, \
            R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P) as bare:
        # the error cases: no moments; 0 samples; fewer than two passes
        bare.add(3)
        with pytest.raises(R.RenderError, match="no moments"):
            bare.rgb8_denoised_variance(k, sigma)
        with pytest.raises(R.RenderError, match="no moments"):
            bare.variance()
        with pytest.raises(R.RenderError):
            frame.rgb8_denoised_variance(k, sigma)                                   # 0 samples (and 0 passes)
        for i, n in enumerate((3, 5, 8)):
            frame.add(n); plain.add(n)
            if i == 0:
                with pytest.raises(R.RenderError, match="passes must be >= 2"):
                    frame.rgb8_denoised_variance(k, sigma)
                with pytest.raises(R.RenderError, match="passes must be >= 2"):
                    frame.variance()
                continue
            before, sq_before, passes_before = frame.sum(), frame.sq_sum(), frame.passes
            got = frame.rgb8_denoised_variance(k, sigma)
            assert np.array_equal(got.astype(np.uint64), _expected(frame, hits, k, sigma, 0)), n
            assert differing_words(frame.variance(), R.moments_variance_host(before, sq_before, frame.samples, passes_before)) == 0
            assert differing_words(frame.sum(), before) == 0 and differing_words(frame.sq_sum(), sq_before) == 0 and frame.passes == passes_before
            img, changed = frame.rgb8()
            again = frame.rgb8_denoised_variance(k, sigma)                            # interleaved with the plain resolve, either way round
            assert np.array_equal(again, got)
            img_plain, changed_plain = plain.rgb8()
            assert np.array_equal(img, img_plain) and changed == changed_plain, n     # the plain resolve's images and counts are its own
            assert np.array_equal(img.astype(np.uint64), R.format_image(before, frame.samples))
        assert frame.samples == 16 and frame.passes == 3 and (got != img).any()       # the filter did something
        # the defaults, the other key, and interleaved with the plain denoised resolve, which shares the guide and the workspace
        assert np.array_equal(frame.rgb8_denoised_variance(), frame.rgb8_denoised_variance(R.DENOISE_ITERATIONS, R.DENOISE_VARIANCE_SIGMA, 0))
        assert np.array_equal(frame.rgb8_denoised_variance(2, (2.0, 0.5, float("inf")), R.RT_DENOISE_SAME_MATERIAL).astype(np.uint64),
                              _expected(frame, hits, 2, (2.0, 0.5, float("inf")), 1))
        plain_dn = frame.rgb8_denoised(k, (4.0, 0.5, 0.02))
        assert np.array_equal(frame.rgb8_denoised_variance(k, sigma), got)
        assert np.array_equal(frame.rgb8_denoised(k, (4.0, 0.5, 0.02)), plain_dn)
        with pytest.raises(R.RenderError, match="iterations"):
            frame.rgb8_denoised_variance(9, sigma)
        with pytest.raises(R.RenderError, match="sigma"):
            frame.rgb8_denoised_variance(k, (3.0, 0.0, 0.02))
        # sums loaded without their second moments: refused, until the moments are loaded too
        ck = frame.checkpoint()
        frame.load(ck["rgb_sum"], ck["samples"])
        with pytest.raises(R.RenderError, match="invalid"):
            frame.rgb8_denoised_variance(k, sigma)
        with pytest.raises(R.RenderError, match="invalid"):
            frame.variance()
        frame.restore(ck)
        assert np.array_equal(frame.rgb8_denoised_variance(k, sigma), got)


def test_progressive_variance_guided_resolve_outlives_the_scene(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    k, sigma = 2, (3.0, 0.5, 0.02)
    frame = R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P, moments=True)
    bare = R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P, moments=True)
    for f in (frame, bare):
        f.add(4); f.add(4)
    hits = R.query_camera(b, cam, W_P, H_P, 0, SEED_P)
    first = frame.rgb8_denoised_variance(k, sigma)
    assert np.array_equal(first.astype(np.uint64), _expected(frame, hits, k, sigma, 0))
    b.close()
    assert np.array_equal(frame.rgb8_denoised_variance(k, sigma), first)
    assert np.array_equal(frame.rgb8_denoised_variance(1, sigma).astype(np.uint64), _expected(frame, hits, 1, sigma, 0))
    with pytest.raises(R.RenderError, match="destroyed"):
        bare.rgb8_denoised_variance(k, sigma)                                        # it never built a guide
    assert differing_words(bare.variance(), R.moments_variance_host(bare.sum(), bare.sq_sum(), 8, 2)) == 0      # ... but its variance needs no scene
    frame.close(); bare.close()


# ---------------------------------------------------------------- 4. the command line
def test_rtrender_denoise_variance_writes_what_the_python_path_yields(pbe):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, spp, depth = 40, 40, 16, 20
    common = [exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth)]
    run = subprocess.run(common + ["--progressive", "8", "--denoise", "3", "--denoise-variance", "2.5"], check=True, capture_output=True, timeout=120)
    b, cam, bg = scenes.cornell_box(pbe)
    with R.Progressive(b, cam, bg, W, H, depth, moments=True) as frame:
        frame.add(8); frame.add(8)
        want = frame.rgb8_denoised_variance(3, (2.5,) + R.DENOISE_SIGMA[1:])
    text = f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in want.reshape(-1, 3))
    assert run.stdout == text.encode()
    one_pass = subprocess.run(common + ["--progressive", "16", "--denoise", "3", "--denoise-variance", "2.5"], capture_output=True, timeout=120)
    assert one_pass.returncode == 1 and b"at least two passes" in one_pass.stderr
    alone = subprocess.run(common + ["--denoise", "3", "--denoise-variance", "2.5"], capture_output=True, timeout=120)
    assert alone.returncode == 2 and b"--progressive" in alone.stderr

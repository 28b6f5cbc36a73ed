"""The denoiser on the GPU (rt_denoise, rt_denoise_device, rt_progressive_resolve_denoised_rgb8; csrc/rt_denoise.hip) against its host twin
rt_denoise_host, which tests/test_denoise_host.py holds to the specification: 0 differing 64-bit words on every frame shape, iteration
count, sigma and flag value of tests/denoise_cases.py — frames smaller than the halo of every dilation, a single row, sizes that are no
multiple of the kernels' tiles (64 x 4, and 16 x 16 with a halo for steps 1 and 2), and 67 x 130, which crosses two tiles on both axes even with taps 32 pixels away."""
import os
import subprocess

import numpy as np
import pytest

from conftest import build_scene
from raytracinginrust_amd import _lib, render as R, scenes

import denoise_cases as DC
from denoise_cases import differing_words

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the kernels are the host twin
@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_twin(shape):
    rgb, hits = DC.case(shape)
    for k, sigma, flags in DC.settings_for(shape):
        got = R.denoise(rgb, DC.SAMPLES, hits, k, sigma, flags)
        want = R.denoise_host(rgb, DC.SAMPLES, hits, k, sigma, flags)
        assert differing_words(got, want) == 0, (shape, k, sigma, flags)


# ---------------------------------------------------------------- 2. device pointers, a stream and a workspace of the caller's
def test_device_form_on_a_stream_in_place_and_a_short_workspace():
    import torch
    H, W = 67, 130
    rgb, hits = DC.case((H, W))
    k, sigma, flags = 4, DC.SIGMAS[0], 1
    want = R.denoise_host(rgb, DC.SAMPLES, hits, k, sigma, flags)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    need = R.denoise_workspace_bytes(W, H)
    assert need == W * H * 128
    with torch.cuda.stream(stream):
        d_sum = torch.from_numpy(rgb.copy()).to(dev)
        d_hits = torch.from_numpy(hits.copy()).to(dev)
        d_out = torch.full((H * W + 1, 3), canary, dtype=torch.float64, device=dev)
        d_ws = torch.full((need // 8 + 2,), canary, dtype=torch.float64, device=dev)
        R.denoise_device(d_sum, DC.SAMPLES, d_hits, W, H, d_out, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
        d_in_place = d_sum.clone()
        R.denoise_device(d_in_place, DC.SAMPLES, d_hits, W, H, None, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
    stream.synchronize()
    out = d_out.cpu().numpy()
    assert differing_words(out[:-1].reshape(H, W, 3), want) == 0 and np.all(out[-1] == canary)
    assert np.all(d_ws.cpu().numpy()[need // 8:] == canary)                          # nothing behind the workspace's 128 bytes per pixel
    assert differing_words(d_sum.cpu().numpy(), rgb) == 0                              # a separate output leaves the input alone
    assert differing_words(d_in_place.cpu().numpy(), want) == 0
    # one byte short: refused with a message, nothing written
    with torch.cuda.stream(stream):
        d_out2 = torch.full((H * W, 3), canary, dtype=torch.float64, device=dev)
        with pytest.raises(R.RenderError, match="workspace too small"):
            R.denoise_device(d_sum, DC.SAMPLES, d_hits, W, H, d_out2, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need - 1)
    stream.synchronize()
    assert np.all(d_out2.cpu().numpy() == canary)
    # the workspace the wrapper allocates itself
    ws = R.denoise_device(d_sum, DC.SAMPLES, d_hits, W, H, d_out2, None, k, sigma, flags)
    torch.cuda.synchronize()
    assert ws.numel() == need and differing_words(d_out2.cpu().numpy().reshape(H, W, 3), want) == 0


# ---------------------------------------------------------------- 3. progressive frames
W_P = H_P = 40
DEPTH_P, SEED_P = 12, 0x5EED + 11


def _expected(frame, hits, k, sigma, flags):
    return R.format_image(R.denoise_host(frame.sum(), frame.samples, hits, k, sigma, flags), frame.samples)


def test_progressive_denoised_resolve(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    hits = R.query_camera(b, cam, W_P, H_P, 0, SEED_P)
    k, sigma = 3, (4.0, 0.5, 0.02)
    with R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P) as frame, R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P) as plain:
        with pytest.raises(R.RenderError, match="0 samples"):
            frame.rgb8_denoised(k, sigma)
        for n in (1, 7, 8):
            frame.add(n); plain.add(n)
            before = frame.sum()
            got = frame.rgb8_denoised(k, sigma)
            assert np.array_equal(got.astype(np.uint64), _expected(frame, hits, k, sigma, 0)), n
            assert differing_words(frame.sum(), before) == 0                          # the accumulated sums are untouched
            img, changed = frame.rgb8()
            again = frame.rgb8_denoised(k, sigma)                                     # interleaved with the plain resolve, either way round
            assert np.array_equal(again, got)
            img_plain, changed_plain = plain.rgb8()
            assert np.array_equal(img, img_plain) and changed == changed_plain, n     # the plain resolve's images and counts are its own
            assert np.array_equal(img.astype(np.uint64), R.format_image(before, frame.samples))
        assert frame.samples == 16 and (got != img).any()                             # the filter did something
        # the defaults, and the other key
        assert np.array_equal(frame.rgb8_denoised(), frame.rgb8_denoised(R.DENOISE_ITERATIONS, R.DENOISE_SIGMA, 0))
        assert np.array_equal(frame.rgb8_denoised(2, (1.0, R.DENOISE_SIGMA[1], float("inf")), R.RT_DENOISE_SAME_MATERIAL).astype(np.uint64),
                              _expected(frame, hits, 2, (1.0, 0.5, float("inf")), 1))
        assert np.array_equal(frame.rgb8_denoised(k, sigma), got)
        with pytest.raises(R.RenderError, match="iterations"):
            frame.rgb8_denoised(9, sigma)
        with pytest.raises(R.RenderError, match="sigma"):
            frame.rgb8_denoised(k, (4.0, 0.0, 0.02))


def test_progressive_guide_is_rebuilt_after_reset_and_outlives_the_scene(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    k, sigma = 3, (4.0, 0.5, 0.02)
    frame = R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P)
    bare = R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P)
    frame.add(4)
    hits_before = R.query_camera(b, cam, W_P, H_P, 0, SEED_P)
    first = frame.rgb8_denoised(k, sigma)
    assert np.array_equal(first.astype(np.uint64), _expected(frame, hits_before, k, sigma, 0))
    # a sphere in front of the camera changes the scene and what sample 0's camera rays hit
    b.world.push(b.Sphere((278.0, 278.0, 100.0), 120.0, b.Lambertian(b.ConstantTexture((0.2, 0.4, 0.8)))))
    frame.reset(); bare.reset()
    frame.add(4); bare.add(4)
    hits_after = R.query_camera(b, cam, W_P, H_P, 0, SEED_P)
    assert differing_words(hits_after, hits_before) > 100
    second = frame.rgb8_denoised(k, sigma)
    assert np.array_equal(second.astype(np.uint64), _expected(frame, hits_after, k, sigma, 0))
    assert not np.array_equal(second.astype(np.uint64), _expected(frame, hits_before, k, sigma, 0))
    # the scene goes: the frame that holds a guide still resolves denoised, the one that never built one cannot
    b.close()
    assert np.array_equal(frame.rgb8_denoised(k, sigma), second)
    assert np.array_equal(frame.rgb8_denoised(1, sigma).astype(np.uint64), _expected(frame, hits_after, 1, sigma, 0))
    with pytest.raises(R.RenderError, match="destroyed"):
        bare.rgb8_denoised(k, sigma)
    img, _ = bare.rgb8()                                                              # ... while its plain resolve works as before
    assert np.array_equal(img.astype(np.uint64), R.format_image(bare.sum(), 4))
    frame.close(); bare.close()


# ---------------------------------------------------------------- 4. quality through the device path
def test_quality_through_the_device_path(pbe):
    """tests/test_denoise_host.py's quality check end to end on the device: 16 samples against 2048, guide from query_camera."""
    b, cam, bg = build_scene("cornell", pbe)
    noisy = R.render(b, cam, bg, DC.Q_W, DC.Q_H, DC.Q_SPP, DC.Q_DEPTH, DC.Q_SEED)
    truth = R.render(b, cam, bg, DC.Q_W, DC.Q_H, DC.Q_TRUTH_SPP, DC.Q_DEPTH, DC.Q_TRUTH_SEED)
    hits = R.query_camera(b, cam, DC.Q_W, DC.Q_H, 0, DC.Q_SEED)
    out = R.denoise(noisy, DC.Q_SPP, hits, DC.Q_ITERATIONS, DC.Q_SIGMA, 0)
    raw = DC.clipped_mse(noisy, DC.Q_SPP, truth, DC.Q_TRUTH_SPP)
    den = DC.clipped_mse(out, DC.Q_SPP, truth, DC.Q_TRUTH_SPP)
    print(f"clipped MSE raw {raw:.5f}, denoised {den:.5f}, ratio {den / raw:.3f}")
    assert den / raw < DC.Q_BOUND


# ---------------------------------------------------------------- 5. the command line
def test_rtrender_denoise_writes_what_the_python_path_yields(pbe):
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, spp, depth = 40, 40, 16, 20
    common = [exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth)]
    run = subprocess.run(common + ["--denoise", "3,4,0.5,0.02"], check=True, capture_output=True, timeout=120)
    b, cam, bg = scenes.cornell_box(pbe)
    hits = R.query_camera(b, cam, W, H)
    img = R.format_image(R.denoise(R.render(b, cam, bg, W, H, spp, depth), spp, hits, 3, (4.0, 0.5, 0.02), 0), spp)
    text = f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in img.reshape(-1, 3))
    assert run.stdout == text.encode()
    assert subprocess.run(common + ["--denoise", "3"], check=True, capture_output=True, timeout=120).stdout == run.stdout        # the default sigmas
    # with --progressive the frame resolves itself denoised on the device
    prog = subprocess.run(common + ["--progressive", "8", "--denoise", "3,4,0.5,0.02"], check=True, capture_output=True, timeout=120)
    with R.Progressive(b, cam, bg, W, H, depth) as frame:
        frame.add(8); frame.add(8)
        want = frame.rgb8_denoised(3, (4.0, 0.5, 0.02))
    text = f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in want.reshape(-1, 3))
    assert prog.stdout == text.encode()
    bad = subprocess.run(common + ["--denoise", "9"], capture_output=True, timeout=120)
    assert bad.returncode == 1 and b"iterations" in bad.stderr

"""Albedo-demodulated denoising on the GPU (rt_denoise_albedo, rt_denoise_albedo_device, rt_progressive_resolve_denoised_albedo_rgb8; the two
element-wise kernels of csrc/rt_albedo.hip around the unchanged filter) against its host twin rt_denoise_albedo_host, which
tests/test_denoise_albedo_host.py holds to the specification: 0 differing 64-bit words.  Shapes: one pixel (an odd number of doubles: the
scalar tail alone), 23 x 37 and 67 x 130 (no multiple of any tile; 3 W H odd and even); K = 1, 3, 5, so that the LDS iterations and the direct
ones both run.  The progressive frame is held to the host chain of include/rt_amd.h byte for byte, and on a small textured scene the
demodulated filter has to beat both the plain filter and the raw frame — the point of it all."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import build_scene, golden_path
from raytracinginrust_amd import _lib, render as R
from raytracinginrust_amd.api import Camera, Plane, Rng, SceneBuilder

import albedo_cases as AC
import denoise_cases as DC
from denoise_cases import differing_words

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (23, 37), (67, 130))
ITERATIONS = (1, 3, 5)


# ---------------------------------------------------------------- 8. the kernels are the host twin
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_twin(shape):
    rgb, hits = DC.case(shape)
    for albedo_samples in AC.ALBEDO_SAMPLES:
        alb = AC.albedo_case(shape, albedo_samples)
        for k, sigma, flags in DC.settings_for(shape):
            if k not in ITERATIONS:
                continue
            got = R.denoise_albedo(rgb, DC.SAMPLES, alb, albedo_samples, hits, k, sigma, flags)
            want = R.denoise_albedo_host(rgb, DC.SAMPLES, alb, albedo_samples, hits, k, sigma, flags)
            assert differing_words(got, want) == 0, (shape, albedo_samples, k, sigma, flags)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_form_on_a_stream_in_place_and_a_short_workspace(shape):
    import torch
    H, W = shape
    rgb, hits = DC.case(shape)
    alb = AC.albedo_case(shape, 5)
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    need = R.denoise_albedo_workspace_bytes(W, H)
    assert need == W * H * 152
    for k in ITERATIONS:
        sigma, flags = DC.SIGMAS[0], 1
        want = R.denoise_albedo_host(rgb, DC.SAMPLES, alb, 5, hits, k, sigma, flags)
        with torch.cuda.stream(stream):
            d_sum = torch.from_numpy(rgb.copy()).to(dev)
            d_alb = torch.from_numpy(alb.copy()).to(dev)
            d_hits = torch.from_numpy(hits.copy()).to(dev)
            d_out = torch.full((H * W + 1, 3), canary, dtype=torch.float64, device=dev)
            d_ws = torch.full((need // 8 + 2,), canary, dtype=torch.float64, device=dev)
            R.denoise_albedo_device(d_sum, DC.SAMPLES, d_alb, 5, d_hits, W, H, d_out, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
            d_in_place = d_sum.clone()
            R.denoise_albedo_device(d_in_place, DC.SAMPLES, d_alb, 5, d_hits, W, H, None, d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
            # buffers 8 bytes off a 16-byte boundary: the scalar kernels
            d_odd_sum = torch.empty((H * W * 3 + 1,), dtype=torch.float64, device=dev); d_odd_sum[1:] = d_sum.reshape(-1)
            d_odd_out = torch.full((H * W * 3 + 2,), canary, dtype=torch.float64, device=dev)
            R.denoise_albedo_device(d_odd_sum[1:], DC.SAMPLES, d_alb, 5, d_hits, W, H, d_odd_out[1:], d_ws, k, sigma, flags, stream=stream.cuda_stream, workspace_bytes=need)
        stream.synchronize()
        out = d_out.cpu().numpy()
        assert differing_words(out[:-1].reshape(H, W, 3), want) == 0 and np.all(out[-1] == canary), k
        assert np.all(d_ws.cpu().numpy()[need // 8:] == canary)                          # nothing behind the workspace's 152 bytes per pixel
        assert differing_words(d_sum.cpu().numpy(), rgb) == 0 and differing_words(d_alb.cpu().numpy(), alb) == 0      # the inputs are only read
        assert differing_words(d_in_place.cpu().numpy(), want) == 0, k
        odd = d_odd_out.cpu().numpy()
        assert differing_words(odd[1:-1].reshape(H, W, 3), want) == 0 and odd[0] == canary and odd[-1] == canary, k
    # one byte short: refused with a message, nothing written
    with torch.cuda.stream(stream):
        d_out2 = torch.full((H * W, 3), canary, dtype=torch.float64, device=dev)
        with pytest.raises(R.RenderError, match="workspace too small"):
            R.denoise_albedo_device(d_sum, DC.SAMPLES, d_alb, 5, d_hits, W, H, d_out2, d_ws, 3, DC.SIGMAS[0], 1, stream=stream.cuda_stream, workspace_bytes=need - 1)
    stream.synchronize()
    assert np.all(d_out2.cpu().numpy() == canary)
    ws = R.denoise_albedo_device(d_sum, DC.SAMPLES, d_alb, 5, d_hits, W, H, d_out2, None, 3, DC.SIGMAS[0], 1)       # the workspace the wrapper allocates
    torch.cuda.synchronize()
    assert ws.numel() == need and differing_words(d_out2.cpu().numpy().reshape(H, W, 3), R.denoise_albedo_host(rgb, DC.SAMPLES, alb, 5, hits, 3, DC.SIGMAS[0], 1)) == 0


# ---------------------------------------------------------------- 9. progressive frames
W_P, H_P, DEPTH_P, SEED_P = 67, 35, 8, 0x5EED + 21


def _expected(b, cam, frame, albedo_samples, hits, k, sigma, flags=0):
    alb = R.query_camera_albedo(b, cam, W_P, H_P, 0, albedo_samples, SEED_P)
    return R.format_image(R.denoise_albedo_host(frame.sum(), frame.samples, alb, albedo_samples, hits, k, sigma, flags), frame.samples)


def test_progressive_denoised_albedo_resolve(pbe):
    b, cam, bg = build_scene("random", pbe)
    hits = R.query_camera(b, cam, W_P, H_P, 0, SEED_P)
    k, sigma = 2, R.DENOISE_SIGMA
    with R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P) as frame, R.Progressive(b, cam, bg, W_P, H_P, DEPTH_P, SEED_P) as plain:
        with pytest.raises(R.RenderError, match="0 samples"):
            frame.rgb8_denoised_albedo(4, k, sigma)
        frame.add(8); plain.add(8)
        assert frame.albedo_info() == (0, 0)
        before = frame.sum()
        got = frame.rgb8_denoised_albedo(4, k, sigma)
        assert frame.albedo_info() == (4, 1)
        assert np.array_equal(got.astype(np.uint64), _expected(b, cam, frame, 4, hits, k, sigma))
        assert differing_words(frame.sum(), before) == 0                              # the accumulated sums are untouched
        # what the other resolves give is what they give without the call, interleaved either way round
        img, changed = frame.rgb8(); img_plain, changed_plain = plain.rgb8()
        assert np.array_equal(img, img_plain) and changed == changed_plain
        assert np.array_equal(frame.rgb8_denoised(k, sigma), plain.rgb8_denoised(k, sigma))
        assert np.array_equal(frame.rgb8_denoised_albedo(4, k, sigma), got)
        img, changed = frame.rgb8(); img_plain, changed_plain = plain.rgb8()
        assert np.array_equal(img, img_plain) and changed == changed_plain
        assert (got != img).any() and (got != frame.rgb8_denoised(k, sigma)).any()      # the filter did something, and something else than the plain one
        # the second call reused the albedo sums (one build so far, and no query kernel has been launched for it: a caller's tiny query in
        # between is still the scene's most recent); other iterations and flags reuse them too
        R.query_hits(b, np.array([[13.0, 2.0, 3.0, -1.0, -0.1, -0.2, 0.0]]))
        ms = R.last_query_ms(b)
        assert np.array_equal(frame.rgb8_denoised_albedo(4, k, sigma), got) and frame.albedo_info() == (4, 1) and R.last_query_ms(b) == ms
        assert np.array_equal(frame.rgb8_denoised_albedo(4, 3, (1.0, 0.5, float("inf")), R.RT_DENOISE_SAME_MATERIAL).astype(np.uint64),
                              _expected(b, cam, frame, 4, hits, 3, (1.0, 0.5, float("inf")), 1))
        assert frame.albedo_info() == (4, 1)
        # another albedo_samples rebuilds them
        other = frame.rgb8_denoised_albedo(7, k, sigma)
        assert frame.albedo_info() == (7, 2)
        assert np.array_equal(other.astype(np.uint64), _expected(b, cam, frame, 7, hits, k, sigma))
        assert np.array_equal(frame.rgb8_denoised_albedo(4, k, sigma), got) and frame.albedo_info() == (4, 3)
        # more samples: the same albedo sums serve the longer frame
        frame.add(3)
        assert np.array_equal(frame.rgb8_denoised_albedo(4, k, sigma).astype(np.uint64), _expected(b, cam, frame, 4, hits, k, sigma)) and frame.albedo_info() == (4, 3)
        # reset drops them
        frame.reset()
        assert frame.albedo_info() == (0, 3)
        frame.add(2)
        assert np.array_equal(frame.rgb8_denoised_albedo(4, k, sigma).astype(np.uint64), _expected(b, cam, frame, 4, hits, k, sigma)) and frame.albedo_info() == (4, 4)
        assert np.array_equal(frame.rgb8_denoised_albedo(), frame.rgb8_denoised_albedo(16, R.DENOISE_ITERATIONS, R.DENOISE_SIGMA, 0))     # the defaults
        with pytest.raises(R.RenderError, match="albedo_samples"):
            frame.rgb8_denoised_albedo(0, k, sigma)
        with pytest.raises(R.RenderError, match="flag"):
            frame.rgb8_denoised_albedo(4, k, sigma, 2)


# ---------------------------------------------------------------- 10. the point of it all
Q_W = Q_H = 40
Q_DEPTH, Q_SPP, Q_SEED, Q_TRUTH_SPP, Q_TRUTH_SEED, Q_ALBEDO_SAMPLES = 12, 16, 7, 2048, 99, 16
Q_ITERATIONS, Q_SIGMA = 2, R.DENOISE_SIGMA


def textured_scene(be):
    """A checker-textured ground rect, an image-textured sphere, a Perlin sphere and one rect light; a pinhole camera, no motion blur.
    (Everything in the first quadrant, away from the origin: the reference's Perlin lattice is odd at negative coordinates, and its
    checker is a product of three sines — a ground at y = 0 would have no pattern at all.)"""
    b = SceneBuilder(be)
    im = Image.open(golden_path("earthmap_256x128.png")).convert("RGB")
    ground = b.Lambertian(b.CheckTexture(b.ConstantTexture((0.15, 0.3, 0.1)), b.ConstantTexture((0.9, 0.9, 0.9))))
    globe = b.Lambertian(b.ImageTexture(im.tobytes(), im.width, im.height))
    marble = b.Lambertian(b.NoiseTexture(4.0, Rng(be, 3, 17)))
    light = b.DiffuseLight(b.ConstantTexture((7.0, 7.0, 7.0)))
    world = b.HittableList()
    world.push(b.AARect(Plane.XZ, 98.0, 108.0, 98.0, 108.0, 100.1, ground))
    world.push(b.Sphere((102.0, 101.1, 103.0), 1.0, globe))
    world.push(b.Sphere((104.2, 101.0, 102.4), 0.9, marble))
    lamp = b.FlipNormal(b.AARect(Plane.XZ, 101.5, 104.5, 101.0, 104.0, 105.0, light))
    world.push(lamp)
    b.set_scene(world, [lamp])
    cam = Camera((103.0, 103.4, 96.5), (103.0, 100.8, 102.8), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 0.0)
    return b, cam, (0.1, 0.1, 0.1)


def test_demodulation_beats_the_plain_filter_and_the_raw_frame_on_textures(pbe):
    """Both comparisons are against code that exists without this feature, on the same frame from the same build; no absolute threshold.
    Measured (one MI355X, DESIGN §15, profiles/denoise_albedo.log): clipped MSE raw 0.004530, plain filter 0.010365 (2.29 x raw),
    albedo-demodulated 0.003006 (0.66 x raw)."""
    b, cam, bg = textured_scene(pbe)
    noisy = R.render(b, cam, bg, Q_W, Q_H, Q_SPP, Q_DEPTH, Q_SEED)
    truth = R.render(b, cam, bg, Q_W, Q_H, Q_TRUTH_SPP, Q_DEPTH, Q_TRUTH_SEED)
    hits = R.query_camera(b, cam, Q_W, Q_H, 0, Q_SEED)
    alb = R.query_camera_albedo(b, cam, Q_W, Q_H, 0, Q_ALBEDO_SAMPLES, Q_SEED)
    # the scene is what it is meant to be: ground, both spheres and the light are in view, and the albedo frame shows all three textures
    mats = {int(m) for m in hits[..., 11][hits[..., 0] != 0.0]}
    assert len(mats) >= 3 and len({tuple(p) for p in (alb / Q_ALBEDO_SAMPLES).round(3).reshape(-1, 3).tolist()}) > 50
    plain = R.denoise(noisy, Q_SPP, hits, Q_ITERATIONS, Q_SIGMA, 0)
    demod = R.denoise_albedo(noisy, Q_SPP, alb, Q_ALBEDO_SAMPLES, hits, Q_ITERATIONS, Q_SIGMA, 0)
    raw_err = DC.clipped_mse(noisy, Q_SPP, truth, Q_TRUTH_SPP)
    plain_err = DC.clipped_mse(plain, Q_SPP, truth, Q_TRUTH_SPP)
    demod_err = DC.clipped_mse(demod, Q_SPP, truth, Q_TRUTH_SPP)
    print(f"clipped MSE raw {raw_err:.6f}, plain filter {plain_err:.6f}, albedo-demodulated {demod_err:.6f} "
          f"(of raw: {plain_err / raw_err:.3f}, {demod_err / raw_err:.3f})")
    assert demod_err < plain_err
    assert demod_err < raw_err


# ---------------------------------------------------------------- the command line
def test_rtrender_albedo_options_write_what_the_python_path_yields(pbe):
    from raytracinginrust_amd import scenes
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, spp, depth = 48, 27, 8, 8
    common = [exe, "--scene", "random", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth)]
    b, cam, bg = scenes.random_scene(pbe, aspect_ratio=W / H)

    def ppm(img):
        return (f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in img.reshape(-1, 3))).encode()
    for extra, n in (([], 1), (["--denoise-albedo", "4"], 4)):
        run = subprocess.run(common + ["--aov", "albedo", "-"] + extra, check=True, capture_output=True, timeout=120)
        assert run.stdout == ppm(R.albedo_image(R.query_camera_albedo(b, cam, W, H, 0, n), n)), extra
    run = subprocess.run(common + ["--denoise", "2", "--denoise-albedo", "4"], check=True, capture_output=True, timeout=120)
    hits = R.query_camera(b, cam, W, H)
    alb = R.query_camera_albedo(b, cam, W, H, 0, 4)
    want = R.format_image(R.denoise_albedo(R.render(b, cam, bg, W, H, spp, depth), spp, alb, 4, hits, 2, R.DENOISE_SIGMA, 0), spp)
    assert run.stdout == ppm(want)
    prog = subprocess.run(common + ["--progressive", "4", "--denoise", "2", "--denoise-albedo", "4"], check=True, capture_output=True, timeout=120)
    with R.Progressive(b, cam, bg, W, H, depth) as frame:
        frame.add(4); frame.add(4)
        assert prog.stdout == ppm(frame.rgb8_denoised_albedo(4, 2, R.DENOISE_SIGMA))
    bad = subprocess.run(common + ["--denoise-albedo", "4"], capture_output=True, timeout=120)
    assert bad.returncode == 2 and b"--denoise" in bad.stderr

"""The variance-guided denoiser without a GPU (rt_denoise_variance_host, rt_moments_variance_host): the filter is defined by an exact f64
specification (csrc/rt_denoise_var.h, csrc/rt_moments.h (4); + - * / and comparisons only, a fixed order), so the host twins must equal
the NumPy restatement of tests/denoise_variance_cases.py with 0 differing 64-bit words; with sigma_v = +inf the colours are the plain
filter's with sigma_c = +inf; known answers pin what the words mean; every bad argument is an error with a message; against the CPU oracle
the filter has to cut the error of a 16-sample Cornell box; and the twins run clean under AddressSanitizer + UBSan as a stand-alone
program.  tests/test_denoise_variance_gpu.py holds the HIP kernels to the twins."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, build_scene
from oracle import orc
from raytracinginrust_amd import render as R

import denoise_cases as DC
import denoise_variance_cases as VC
import moments_cases as MC
from denoise_variance_cases import INF, differing_words, sigma3


# ---------------------------------------------------------------- 1. the host twins are the specification
@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_restatement(pbe, shape):
    rgb, var, hits = VC.case(shape)
    want = VC.reference(shape)
    for k, sigma, flags in VC.settings_for(shape):
        got, got_v = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, k, sigma, flags, want_var=True)
        assert differing_words(got, want[(k, sigma, flags)][0]) == 0, (shape, k, sigma, flags)
        assert differing_words(got_v, want[(k, sigma, flags)][1]) == 0, (shape, k, sigma, flags)
        assert differing_words(R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, k, sigma, flags), got) == 0     # without var_out
    # the inputs do what they are for
    if shape[0] * shape[1] > 1:
        px = var.reshape(-1, 3)
        assert np.isnan(px).any() and np.isposinf(px).any() and (px < 0.0).any() and (px == 0.0).all(axis=1).any()
        v = VC.numpy_pack_v(var)
        assert (v == 0.0).sum() >= 4 and np.isfinite(v).all() and (v >= 0.0).all()


@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_with_sigma_v_off_the_colours_are_the_plain_filters_with_sigma_c_off(shape):
    rgb, var, hits = VC.case(shape)
    for k, sigma, flags in VC.settings_for(shape):
        off = (INF,) + tuple(sigma[1:])
        got = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, k, off, flags)
        assert differing_words(got, R.denoise_host(rgb, VC.SAMPLES, hits, k, off, flags)) == 0, (shape, k, sigma, flags)


@pytest.mark.parametrize("shape", MC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_variance_twin_equals_the_restatement_and_is_the_v_of_e2(shape):
    S, Q, samples, passes = MC.state(shape)
    V = R.moments_variance_host(S, Q, samples, passes)
    assert differing_words(V, VC.numpy_variance(S, Q, samples, passes)) == 0
    assert differing_words(V, MC.numpy_channels(S, Q, samples, passes)["V"]) == 0
    # for channels with delta <= m < 1: e2_c == V / (4 m) bit for bit; a pixel whose three channels all qualify has the largest of them as e2
    e2 = R.moments_error_host(S, Q, samples, passes)
    with np.errstate(all="ignore"):
        m = S / np.float64(samples)
        ok = ((m >= MC.DELTA) & (m < 1.0)).all(axis=2) & np.isfinite(V).all(axis=2)
        per_channel = V / (np.float64(4.0) * m)
    assert ok.any()
    want = per_channel[..., 0].copy()
    for c in (1, 2):
        want = np.where(per_channel[..., c] > want, per_channel[..., c], want)
    assert differing_words(e2[ok], want[ok]) == 0
    if shape[0] * shape[1] >= 33:                               # what a non-finite state gives: 0, or +inf from a +inf in Q
        flat = V.reshape(-1, 3)
        assert flat[MC.PX_NAN, 1] == 0.0 and flat[MC.PX_PINF, 0] == 0.0 and flat[MC.PX_OVERFLOW, 1] == 0.0 and flat[MC.PX_Q_INF, 1] == INF
        assert (V[np.isfinite(V)] >= 0.0).all()


# ---------------------------------------------------------------- 2. known answers
def _uniform_guide(H, W):
    hits = np.zeros((H, W, 16))
    hits[..., 0] = 1.0; hits[..., 1] = 1.0; hits[..., 5:8] = (0.0, 0.0, 1.0); hits[..., 8] = 1.0
    return hits


def test_the_propagated_variance_of_one_unstopped_iteration():
    """All stops off, one key, constant dyadic v, K = 1: the prefilter of a constant is the constant, every w is k, wsum = 1 and
    sum k^2 = (sum h^2)^2 = (70/256)^2, so an interior pixel's v is exactly v * 4900 / 65536."""
    H, W = 9, 11
    rs = np.random.RandomState(11)
    rgb = rs.uniform(0.0, 1.0, (H, W, 3)) * 4
    var = np.full((H, W, 3), 0.25); var[..., 2] = 0.5                               # v = 1.0
    _, v = R.denoise_variance_host(rgb, 4, var, _uniform_guide(H, W), 1, (INF, INF, INF), 0, want_var=True)
    assert differing_words(v[2:-2, 2:-2], np.full((H - 4, W - 4), 4900.0 / 65536.0)) == 0
    assert (v[0, 0] > v[4, 5])                                  # a corner averages 9 taps, not 25
    var2 = var * 0.125
    _, v2 = R.denoise_variance_host(rgb, 4, var2, _uniform_guide(H, W), 1, (INF, INF, INF), 0, want_var=True)
    assert differing_words(v2[2:-2, 2:-2], np.full((H - 4, W - 4), 0.125 * 4900.0 / 65536.0)) == 0


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_a_step_edge_of_forty_standard_deviations_comes_back_bit_for_bit(k):
    """Two flat halves, 0.25 and 0.75 in every channel, whose pixels carry a variance that makes the step 40 standard deviations of a
    difference: at sigma_v = 2 no weight crosses the edge, and the frame comes back as it went in."""
    H, W, samples = 13, 21, 8
    rgb = np.zeros((H, W, 3)); rgb[:, :10] = 0.25 * samples; rgb[:, 10:] = 0.75 * samples
    # |c_q - c_p|^2 = 0.75 across the edge; v = 0.75 / 3200 per pixel makes v_p + v_q = 0.75 / 1600: the step is sqrt(1600) = 40 standard
    # deviations of the difference.  sigma_v = 2: den = 4 (v_p + v_q + 2^-16) < 0.75, t < 0, wc = 0 across the edge; within a half d = 0, wc = 1.
    var = np.full((H, W, 3), 0.75 / 3200.0 / 3.0)
    out, v = R.denoise_variance_host(rgb, samples, var, _uniform_guide(H, W), k, (2.0, INF, INF), 0, want_var=True)
    assert differing_words(out, rgb) == 0
    assert (v < VC.numpy_pack_v(var)).all()                     # ... while each half's variance fell


def test_a_pixel_one_standard_deviation_off_is_pulled_towards_its_flat_neighbours():
    H, W, samples = 9, 9, 4
    v_px = 2.0 ** -6                                            # per pixel; sd of a difference = sqrt(2 v) = 2^-2.5 = 0.177
    rgb = np.full((H, W, 3), 0.5 * samples)
    rgb[4, 4] = (0.5 + 0.125) * samples                         # d = 3 * 2^-6 against v_p + v_q = 2^-5: 1.2 sd of the difference, all channels together
    var = np.full((H, W, 3), v_px / 4.0); var[..., 2] = v_px / 2.0
    out = R.denoise_variance_host(rgb, samples, var, _uniform_guide(H, W), 1, (2.0, INF, INF), 0)
    c = out[4, 4] / samples
    assert (c > 0.5).all() and (c < 0.5 + 0.125 / 2).all()      # wc = (1 - 0.375)^2 = 0.39 for the 24 neighbours: the centre keeps 0.30 of its offset
    assert differing_words(out, VC.numpy_denoise_variance(rgb, samples, var, _uniform_guide(H, W), 1, (2.0, INF, INF), 0)[0]) == 0
    assert (out[0, 0] == 0.5 * samples).all()                   # out of the outlier's reach
    assert (out[4, 3] > 0.5 * samples).all()                    # ... and its neighbours take a little of it


def test_output_may_alias_the_input(pbe):
    rgb, var, hits = VC.case((23, 37))
    before = rgb.copy()
    separate = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, 4, VC.SIGMAS[0], 1)
    assert differing_words(rgb, before) == 0                                       # a separate output leaves the input untouched
    in_place = rgb.copy()
    assert pbe.lib.rt_denoise_variance_host(in_place.ctypes.data, VC.SAMPLES, var.ctypes.data, hits.ctypes.data, 37, 23, 4, sigma3(VC.SIGMAS[0]), 1,
                                            in_place.ctypes.data, None) == 0
    assert differing_words(in_place, separate) == 0 and differing_words(in_place, before) != 0


# ---------------------------------------------------------------- 3. arguments
BAD = (  # (samples, W, H, iterations, sigma, flags) -> a piece of the message
    ((5, 4, 3, 0, (1.0, 1.0, 1.0), 0), "iterations"),
    ((5, 4, 3, 9, (1.0, 1.0, 1.0), 0), "iterations"),
    ((5, 4, 3, 2, (0.0, 1.0, 1.0), 0), "sigma_v"),
    ((5, 4, 3, 2, (1.0, -2.0, 1.0), 0), "sigma_v"),
    ((5, 4, 3, 2, (1.0, 1.0, float("nan")), 0), "sigma_v"),
    ((5, 4, 3, 2, (-INF, 1.0, 1.0), 0), "sigma_v"),
    ((0, 4, 3, 2, (1.0, 1.0, 1.0), 0), "samples"),
    ((5, 0, 3, 2, (1.0, 1.0, 1.0), 0), "W and H"),
    ((5, 4, 0, 2, (1.0, 1.0, 1.0), 0), "W and H"),
    ((5, 4, 3, 2, (1.0, 1.0, 1.0), 2), "flag"),
    ((5, 4, 3, 2, (1.0, 1.0, 1.0), 0x80000001), "flag"),
)


def _err(lib):
    return lib.rt_last_error().decode()


def test_bad_arguments_are_errors_with_a_message(pbe):
    lib = pbe.lib
    rgb = np.ones((3, 4, 3)); var = np.ones((3, 4, 3)); hits = np.zeros((3, 4, 16)); out = np.full((3, 4, 3), 7.0)
    dev = C.c_void_p(0x1000)                                   # never dereferenced: every call below is refused before a device is looked at
    for (samples, W, H, k, sigma, flags), text in BAD:
        sg = sigma3(sigma)
        for fn in (lib.rt_denoise_variance_host, lib.rt_denoise_variance):
            assert fn(rgb.ctypes.data, samples, var.ctypes.data, hits.ctypes.data, W, H, k, sg, flags, out.ctypes.data, None) != 0 and text in _err(lib), (fn, text)
        assert lib.rt_denoise_variance_device(dev, samples, dev, dev, W, H, k, sg, flags, dev, None, dev, 1 << 20, None) != 0 and text in _err(lib), text
    good = sigma3((1.0, 1.0, 1.0))
    for fn in (lib.rt_denoise_variance_host, lib.rt_denoise_variance):
        for hole in (0, 2, 3, 7, 9):
            args = [rgb.ctypes.data, 5, var.ctypes.data, hits.ctypes.data, 4, 3, 2, good, 0, out.ctypes.data, None]
            args[hole] = None
            assert fn(*args) != 0 and "null argument" in _err(lib)
    for hole in (0, 2, 3, 7, 9, 11):
        args = [dev, 5, dev, dev, 4, 3, 2, good, 0, dev, None, dev, 1 << 20, None]
        args[hole] = None
        assert lib.rt_denoise_variance_device(*args) != 0 and "null argument" in _err(lib)
    # the workspace: 128 bytes per pixel, refused one byte short before anything else is looked at
    assert lib.rt_denoise_variance_workspace_bytes(4, 3) == 4 * 3 * 128 and lib.rt_denoise_variance_workspace_bytes(3840, 2160) == 3840 * 2160 * 128
    assert lib.rt_denoise_variance_device(dev, 5, dev, dev, 4, 3, 2, good, 0, dev, None, dev, 4 * 3 * 128 - 1, None) != 0 and "workspace too small" in _err(lib)
    assert lib.rt_denoise_variance_device(dev, 5, dev, C.c_void_p(0x1008), 4, 3, 2, good, 0, dev, None, dev, 4 * 3 * 128, None) != 0 and "16-byte aligned" in _err(lib)
    assert lib.rt_denoise_variance_device(dev, 5, dev, dev, 4, 3, 2, good, 0, dev, None, C.c_void_p(0x1008), 4 * 3 * 128, None) != 0 and "16-byte aligned" in _err(lib)
    assert lib.rt_denoise_variance_device(dev, 5, C.c_void_p(0x1004), dev, 4, 3, 2, good, 0, dev, None, dev, 4 * 3 * 128, None) != 0 and "8-byte aligned" in _err(lib)
    assert lib.rt_denoise_variance_device(dev, 5, dev, dev, 4, 3, 2, good, 0, dev, C.c_void_p(0x1004), dev, 4 * 3 * 128, None) != 0 and "8-byte aligned" in _err(lib)
    # the variance frame: passes < 2 and samples = 0, host and device forms alike
    for samples, passes, text in ((16, 1, "passes"), (16, 0, "passes"), (0, 2, "samples")):
        assert lib.rt_moments_variance_host(rgb.ctypes.data, var.ctypes.data, samples, passes, 4, 3, out.ctypes.data) != 0 and text in _err(lib)
        assert lib.rt_moments_variance_device(dev, dev, samples, passes, 4, 3, dev, None) != 0 and text in _err(lib)
    assert lib.rt_moments_variance_host(rgb.ctypes.data, var.ctypes.data, 16, 2, 0, 3, out.ctypes.data) != 0 and "W and H" in _err(lib)
    assert lib.rt_moments_variance_host(None, var.ctypes.data, 16, 2, 4, 3, out.ctypes.data) != 0 and "null argument" in _err(lib)
    assert lib.rt_moments_variance_device(dev, dev, 16, 2, 4, 3, None, None) != 0 and "null argument" in _err(lib)
    assert lib.rt_moments_variance_device(dev, C.c_void_p(0x1004), 16, 2, 4, 3, dev, None) != 0 and "8-byte aligned" in _err(lib)
    assert (out == 7.0).all()
    # the progressive calls
    img = np.zeros(36, np.uint8)
    assert lib.rt_progressive_resolve_denoised_variance_rgb8(None, 3, good, 0, img.ctypes.data) != 0 and "null argument" in _err(lib)
    assert lib.rt_progressive_variance(None, out.ctypes.data) != 0 and "null argument" in _err(lib)
    with pytest.raises(ValueError):
        R.denoise_variance_host(np.ones((3, 4, 3)), 1, np.ones((3, 4)), np.zeros((3, 4, 16)))
    with pytest.raises(R.RenderError, match="iterations"):
        R.denoise_variance_host(np.ones((3, 4, 3)), 1, np.ones((3, 4, 3)), np.zeros((3, 4, 16)), iterations=0)
    with pytest.raises(R.RenderError, match="passes"):
        R.moments_variance_host(np.ones((3, 4, 3)), np.ones((3, 4, 3)), 4, 1)


def test_without_a_device_the_device_paths_fail_like_rt_render(pbe):
    if R.device_count() > 0:                                   # (the messages can only be seen on a machine without a device)
        return
    from raytracinginrust_amd import scenes
    b, cam, bg = scenes.cornell_box(pbe)
    with pytest.raises(R.RenderError, match="no HIP device") as one_shot:
        R.render(b, cam, bg, 8, 8, 1, 4)
    with pytest.raises(R.RenderError, match="no HIP device") as dn:
        R.denoise_variance(np.ones((3, 4, 3)), 1, np.ones((3, 4, 3)), np.zeros((3, 4, 16)))
    assert str(dn.value) == str(one_shot.value)
    dev = C.c_void_p(0x1000)
    assert pbe.lib.rt_denoise_variance_device(dev, 5, dev, dev, 4, 3, 2, sigma3((1.0, 1.0, 1.0)), 0, dev, None, dev, 4 * 3 * 128, None) != 0
    assert _err(pbe.lib) == str(one_shot.value)
    assert pbe.lib.rt_moments_variance_device(dev, dev, 16, 2, 4, 3, dev, None) != 0
    assert _err(pbe.lib) == str(one_shot.value)
    with pytest.raises(R.RenderError, match="no HIP device"):  # no frame to resolve: create is where a progressive frame fails
        R.Progressive(b, cam, bg, 8, 8, 4, moments=True).rgb8_denoised_variance()


def test_python_defaults():
    assert R.DENOISE_VARIANCE_SIGMA == (Q_SIGMA_V,) + DC.Q_SIGMA[1:]
    rgb, var, hits = VC.case((23, 37))
    assert differing_words(R.denoise_variance_host(rgb, VC.SAMPLES, var, hits),
                           R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, R.DENOISE_ITERATIONS, R.DENOISE_VARIANCE_SIGMA, 0)) == 0


# ---------------------------------------------------------------- 4. quality, against the oracle
Q_SIGMA_V = 3.0                                                 # the Python default, chosen from the figures below and DESIGN §17
Q_MEASURED = {2: 0.159, 3: 0.136}                               # the chosen setting's ratio to raw by K, measured on the CPU (the docstring below)


@functools.lru_cache(maxsize=None)
def oracle_quality_frames():
    """(S, Q, truth sums, guide records) of the set-up: the 16 samples of seed 7 as 4 passes of 4, merged by the host twin."""
    from test_denoise_host import oracle_quality_frames as plain
    _, truth, hits = plain()
    obe = orc.load()
    ob, cam, bg = build_scene("cornell", obe)
    S = np.zeros((DC.Q_H, DC.Q_W, 3)); Q = np.zeros_like(S)
    base = 0
    for n_b in VC.Q_PASSES:
        p = orc.render(ob, cam, bg, DC.Q_W, DC.Q_H, n_b, DC.Q_DEPTH, VC.pass_seed(DC.Q_SEED, base))
        R.moments_merge_host(p, n_b, S, Q)
        base += n_b
    assert base == DC.Q_SPP
    return S, Q, truth, hits


def test_quality_against_the_oracle():
    """Measured on these inputs, on the CPU (clipped MSE; raw 0.00429; the others as ratios to raw):
        K = 2: plain (4, 0.5, 0.02) 0.166;  sigma_v = 1: 0.930, 2: 0.528, 3: 0.159, 4: 0.220
        K = 3: plain (4, 0.5, 0.02) 0.248;  sigma_v = 1: 0.930, 2: 0.514, 3: 0.136, 4: 0.162
    sigma_v = 1 filters next to nothing — the stop's weight reaches 0 at ONE standard deviation of the difference, and a variance from
    four batch means is an estimate with three degrees of freedom; sigma_v = 4 lets the light bleed into the ceiling.  sigma_v = 3 is the
    Python default.  The bound is the measured ratio plus 10 %, a margin for a later change of the pass split, not for arithmetic."""
    S, Q, truth, hits = oracle_quality_frames()
    N, B = DC.Q_SPP, len(VC.Q_PASSES)
    V = R.moments_variance_host(S, Q, N, B)
    raw = DC.clipped_mse(S, N, truth, DC.Q_TRUTH_SPP)
    print(f"clipped MSE raw {raw:.5f}")
    ratios = {}
    for k in VC.Q_ITERATIONS:
        plain = DC.clipped_mse(R.denoise_host(S, N, hits, k, VC.Q_PLAIN_SIGMA, 0), N, truth, DC.Q_TRUTH_SPP)
        line = f"K = {k}: plain {VC.Q_PLAIN_SIGMA} {plain / raw:.3f}"
        for sv in VC.Q_SIGMA_VS:
            den = DC.clipped_mse(R.denoise_variance_host(S, N, V, hits, k, (sv,) + VC.Q_PLAIN_SIGMA[1:], 0), N, truth, DC.Q_TRUTH_SPP)
            ratios[(k, sv)] = den / raw
            line += f", sigma_v = {sv:g} {den / raw:.3f}"
        print(line)
    for k in VC.Q_ITERATIONS:
        assert ratios[(k, Q_SIGMA_V)] < Q_MEASURED[k] * 1.10, (k, ratios[(k, Q_SIGMA_V)])


# ---------------------------------------------------------------- 5. the host twins under AddressSanitizer + UBSan, stand-alone
def test_host_twins_under_sanitizers(tmp_path):
    """The runtimes are linked statically, so the program needs nothing from its environment.  Inside tests/test_sanitizers.py's run of
    this suite the twins are already the sanitizer build's (and a second, preloaded runtime would refuse to start beside the linked one)."""
    if os.environ.get("RT_SANITIZER_RUN") == "1":
        return
    exe = str(tmp_path / "denoise_variance_san")
    csrc = os.path.join(ROOT, "raytracinginrust_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(csrc, "rt_denoise_cpu.cpp"), os.path.join(csrc, "rt_denoise_var_cpu.cpp"), os.path.join(csrc, "rt_moments_cpu.cpp"),
                    os.path.join(ROOT, "tests", "denoise_variance_san_main.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and run.stderr == "", run.stdout + run.stderr

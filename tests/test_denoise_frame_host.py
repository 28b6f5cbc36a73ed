"""Denoising a frame as it is, without a GPU (rt_denoise_frame_host, rt_adaptive_variance_host): csrc/rt_denoise_frame.h is an exact f64
specification (+ - * / and comparisons only, a fixed order), so the host twins must equal the NumPy restatement of
tests/denoise_frame_cases.py with 0 differing 64-bit words in all eight combinations of {counts, variance, albedo}; with equal counts the
call reduces word for word to the three filters it composes; a pixel without samples behaves as a NaN pixel and comes out +0.0; every bad
argument is an error with a message; and the twins run clean under AddressSanitizer + UBSan as a stand-alone program.
tests/test_denoise_frame_gpu.py holds the HIP kernels to the twins."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracinginrust_amd import render as R

import adaptive_cases as AC
import albedo_cases as ALC
import denoise_cases as DC
import denoise_frame_cases as FC
import denoise_variance_cases as VC
import moments_cases as MC
from denoise_frame_cases import INF, differing_words, sigma3

IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}" if isinstance(s, tuple) and len(s) == 2 else FC.combo_id(s))


# ---------------------------------------------------------------- 1. the host twins are the specification
@pytest.mark.parametrize("combo", FC.COMBOS, **IDS)
@pytest.mark.parametrize("shape", FC.SHAPES, **IDS)
def test_host_twin_equals_the_numpy_restatement(shape, combo):
    rgb, n, var, alb, hits = FC.frames(shape, combo)
    want = FC.reference(shape, combo)
    for k, sigma, flags in FC.settings_for(shape, combo[1]):
        got = R.denoise_frame_host(rgb, hits, n, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, k, sigma, flags, want_var=combo[1])
        got, got_v = got if combo[1] else (got, None)
        assert differing_words(got, want[(k, sigma, flags)][0]) == 0, (shape, combo, k, sigma, flags)
        if combo[1]:
            assert differing_words(got_v, want[(k, sigma, flags)][1]) == 0, (shape, combo, k, sigma, flags)
    if shape[0] * shape[1] > 1:                                 # the inputs do what they are for
        n, b = FC.counts_case(shape)
        assert (n == 0).any() and (n == 1).any() and len(np.unique(n)) >= 4
        assert (b == 0).any() and (b == 1).any() and (b >= 2).any() and (b <= n).all()
        alb = ALC.albedo_case(shape, FC.ALBEDO_SAMPLES)
        assert not np.isfinite(rgb).all() and (alb == 0.0).any() and not np.isfinite(alb).all()


@pytest.mark.parametrize("shape", FC.VARIANCE_SHAPES, **IDS)
def test_variance_twin_equals_the_restatement(shape):
    S, Q, n, b = FC.variance_state(shape)
    V = R.adaptive_variance_host(S, Q, n, b)
    assert differing_words(V, FC.numpy_adaptive_variance(S, Q, n, b)) == 0
    assert (V[b < 2] == INF).all()
    if shape[0] * shape[1] >= 33:
        assert (b == 0).any() and (b == 1).any() and (b >= 2).any() and len(np.unique(n)) >= 4


# ---------------------------------------------------------------- 2. reductions
@pytest.mark.parametrize("shape", FC.SHAPES, **IDS)
def test_equal_counts_give_the_three_filters_word_for_word(shape):
    rgb, var, hits = VC.case(shape)
    alb = ALC.albedo_case(shape, FC.ALBEDO_SAMPLES)
    N = FC.SAMPLES
    n = np.full(shape, N, np.uint32)
    for k, sigma, flags in DC.settings_for(shape)[::2]:
        for counts in (None, n):
            assert differing_words(R.denoise_frame_host(rgb, hits, counts, N, None, None, 1, k, sigma, flags), R.denoise_host(rgb, N, hits, k, sigma, flags)) == 0
            assert differing_words(R.denoise_frame_host(rgb, hits, counts, N, None, alb, FC.ALBEDO_SAMPLES, k, sigma, flags),
                                   R.denoise_albedo_host(rgb, N, alb, FC.ALBEDO_SAMPLES, hits, k, sigma, flags)) == 0
    ones = np.full(rgb.shape, 3.0)                              # three samples of albedo 1
    for k, sigma, flags in VC.settings_for(shape)[::2]:
        want, want_v = R.denoise_variance_host(rgb, N, var, hits, k, sigma, flags, want_var=True)
        for counts in (None, n):
            got, got_v = R.denoise_frame_host(rgb, hits, counts, N, var, None, 1, k, sigma, flags, want_var=True)
            assert differing_words(got, want) == 0 and differing_words(got_v, want_v) == 0
            got, got_v = R.denoise_frame_host(rgb, hits, counts, N, var, ones, 3, k, sigma, flags, want_var=True)
            assert differing_words(got, want) == 0 and differing_words(got_v, want_v) == 0
    # with counts, `samples` is ignored
    assert differing_words(R.denoise_frame_host(rgb, hits, n, 0, None, None, 1, 2, DC.SIGMAS[0], 0), R.denoise_host(rgb, N, hits, 2, DC.SIGMAS[0], 0)) == 0


@pytest.mark.parametrize("shape", MC.SHAPES, **IDS)
def test_equal_counts_give_the_moments_variance(shape):
    S, Q, samples, passes = MC.state(shape)
    n = np.full(shape, samples, np.uint32); b = np.full(shape, passes, np.uint32)
    assert differing_words(R.adaptive_variance_host(S, Q, n, b), R.moments_variance_host(S, Q, samples, passes)) == 0


@pytest.mark.parametrize("shape", FC.VARIANCE_SHAPES, **IDS)
def test_the_adaptive_error_is_made_of_this_variance(shape):
    """For b >= 2, adaptive_error_host's e2 is what rt_moments.h (2) makes of (E)'s V: per channel V / (4 max(m, delta)), 0 where the channel is
    saturated beyond doubt, then the maximum of rt_moments.h (2) over the channels."""
    S, Q, n, b = FC.variance_state(shape)
    V = R.adaptive_variance_host(S, Q, n, b)
    e2 = R.adaptive_error_host(S, Q, n, b)
    with np.errstate(all="ignore"):
        m = S / n.astype(np.float64)[..., None]
        den = np.where(m >= MC.DELTA, m, MC.DELTA)
        c = V / (np.float64(4.0) * den)
        over = m - np.float64(1.0)
        c = np.where((m >= 1.0) & (over * over >= np.float64(9.0) * V), 0.0, c)
        e = c[..., 0].copy()
        for k in (1, 2):
            x = c[..., k]
            e = np.where(MC.finite(e) & (~MC.finite(x) | (x > e)), x, e)
    two = b >= 2
    assert two.any() and differing_words(e2[two], e[two]) == 0
    assert (e2[~two] == INF).all() and (V[~two] == INF).all()


# ---------------------------------------------------------------- 3. properties
@pytest.mark.parametrize("variance", (False, True), ids=("colour", "variance"))
def test_a_pixel_without_samples_comes_out_zero_and_acts_as_a_nan_pixel(variance):
    shape = (23, 37)
    rgb, var, hits = VC.case(shape)
    n = FC.counts_case(shape)[0]
    empty = n == 0
    assert empty.sum() >= 2
    v = var if variance else None
    sigma = (VC.SIGMAS if variance else DC.SIGMAS)[0]
    got = R.denoise_frame_host(rgb, hits, n, 1, v, None, 1, 3, sigma, 1)
    assert (got[empty].view(np.uint64) == 0).all()              # +0.0, not -0.0
    # the same frame with a NaN in the empty pixels' place, and any count there
    rgb_nan = rgb.copy(); rgb_nan[empty] = np.nan
    n_one = n.copy(); n_one[empty] = 3
    other = R.denoise_frame_host(rgb_nan, hits, n_one, 1, v, None, 1, 3, sigma, 1)
    assert differing_words(got[~empty], other[~empty]) == 0


def test_a_black_albedo_channel_stays_black_under_the_variance_stop():
    shape = (23, 37)
    rgb, var, hits = VC.case(shape)
    n = FC.counts_case(shape)[0]
    alb = ALC.albedo_case(shape, FC.ALBEDO_SAMPLES).copy()
    alb[5:9, 7:20, 1] = 0.0
    for counts in (None, n):
        out = R.denoise_frame_host(rgb, hits, counts, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, 3, VC.SIGMAS[1], 0)
        black = out[5:9, 7:20, 1]
        assert ((black == 0.0) | np.isnan(black)).all() and (black == 0.0).sum() > black.size // 2
        assert (out[5:9, 7:20, 0] != 0.0).any()


@pytest.mark.parametrize("combo", FC.COMBOS, **IDS)
def test_output_may_alias_the_input(pbe, combo):
    shape = (23, 37)
    rgb, n, var, alb, hits = FC.frames(shape, combo)
    sigma = (VC.SIGMAS if combo[1] else DC.SIGMAS)[0]
    before = rgb.copy()
    separate = R.denoise_frame_host(rgb, hits, n, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, 4, sigma, 1)
    assert differing_words(rgb, before) == 0
    in_place = rgb.copy()
    ptr = lambda a: None if a is None else a.ctypes.data
    assert pbe.lib.rt_denoise_frame_host(in_place.ctypes.data, ptr(n), FC.SAMPLES, ptr(var), ptr(alb), FC.ALBEDO_SAMPLES, hits.ctypes.data, 37, 23, 4, sigma3(sigma), 1,
                                         in_place.ctypes.data, None) == 0
    assert differing_words(in_place, separate) == 0 and differing_words(in_place, before) != 0


# ---------------------------------------------------------------- 4. arguments
BAD = (  # (samples, W, H, iterations, sigma, flags) -> a piece of the message
    ((5, 4, 3, 0, (1.0, 1.0, 1.0), 0), "iterations"),
    ((5, 4, 3, 9, (1.0, 1.0, 1.0), 0), "iterations"),
    ((5, 4, 3, 2, (0.0, 1.0, 1.0), 0), "sigma"),
    ((5, 4, 3, 2, (1.0, -2.0, 1.0), 0), "sigma"),
    ((5, 4, 3, 2, (1.0, 1.0, float("nan")), 0), "sigma"),
    ((0, 4, 3, 2, (1.0, 1.0, 1.0), 0), "samples"),
    ((5, 0, 3, 2, (1.0, 1.0, 1.0), 0), "W and H"),
    ((5, 4, 0, 2, (1.0, 1.0, 1.0), 0), "W and H"),
    ((5, 4, 3, 2, (1.0, 1.0, 1.0), 2), "flag"),
)


def _err(lib):
    return lib.rt_last_error().decode()


def test_bad_arguments_are_errors_with_a_message(pbe):
    lib = pbe.lib
    rgb = np.ones((3, 4, 3)); var = np.ones((3, 4, 3)); alb = np.ones((3, 4, 3)); hits = np.zeros((3, 4, 16)); out = np.full((3, 4, 3), 7.0)
    cnt = np.ones((3, 4), np.uint32); vout = np.full((3, 4), 7.0)
    dev = C.c_void_p(0x1000)                                   # never dereferenced: every call below is refused before a device is looked at
    ws = lib.rt_denoise_frame_workspace_bytes(4, 3)
    for (samples, W, H, k, sigma, flags), text in BAD:
        sg = sigma3(sigma)
        for v in (None, var.ctypes.data):
            for fn in (lib.rt_denoise_frame_host, lib.rt_denoise_frame):
                assert fn(rgb.ctypes.data, None, samples, v, alb.ctypes.data, 2, hits.ctypes.data, W, H, k, sg, flags, out.ctypes.data, None) != 0 and text in _err(lib), (fn, text)
            assert lib.rt_denoise_frame_device(dev, None, samples, dev if v else None, dev, 2, dev, W, H, k, sg, flags, dev, None, dev, 1 << 20, None) != 0 and text in _err(lib), text
    good = sigma3((1.0, 1.0, 1.0))
    full = lambda: [rgb.ctypes.data, cnt.ctypes.data, 5, var.ctypes.data, alb.ctypes.data, 2, hits.ctypes.data, 4, 3, 2, good, 0, out.ctypes.data, vout.ctypes.data]
    for fn in (lib.rt_denoise_frame_host, lib.rt_denoise_frame):
        for hole in (0, 6, 10, 12):
            args = full(); args[hole] = None
            assert fn(*args) != 0 and "null argument" in _err(lib)
        args = full(); args[5] = 0                              # albedo sums of no samples
        assert fn(*args) != 0 and "albedo_samples" in _err(lib)
        args = full(); args[3] = None                           # var_out without var
        assert fn(*args) != 0 and "var_out needs var" in _err(lib)
        args = full(); args[1] = None; args[2] = 0              # no counts: samples counts
        assert fn(*args) != 0 and "samples" in _err(lib)
    dfull = lambda: [dev, dev, 5, dev, dev, 2, dev, 4, 3, 2, good, 0, dev, dev, dev, ws, None]
    for hole in (0, 6, 10, 12, 14):
        args = dfull(); args[hole] = None
        assert lib.rt_denoise_frame_device(*args) != 0 and "null argument" in _err(lib)
    args = dfull(); args[3] = None
    assert lib.rt_denoise_frame_device(*args) != 0 and "var_out needs var" in _err(lib)
    # the workspace: the filter's 128 bytes per pixel and two frames of 24, each padded to 16; refused one byte short
    assert ws == 4 * 3 * (128 + 48) and lib.rt_denoise_frame_workspace_bytes(5, 3) == 15 * 128 + 2 * 368
    args = dfull(); args[15] = ws - 1
    assert lib.rt_denoise_frame_device(*args) != 0 and "workspace too small" in _err(lib)
    for hole, text in ((6, "16-byte aligned"), (14, "16-byte aligned"), (0, "8-byte aligned"), (3, "8-byte aligned"), (4, "8-byte aligned"), (12, "8-byte aligned"),
                       (13, "8-byte aligned")):
        args = dfull(); args[hole] = C.c_void_p(0x1004 if "8" == text[0] else 0x1008)
        assert lib.rt_denoise_frame_device(*args) != 0 and text in _err(lib), hole
    args = dfull(); args[1] = C.c_void_p(0x1002)
    assert lib.rt_denoise_frame_device(*args) != 0 and "4-byte aligned" in _err(lib)
    # the variance frame with counts
    assert lib.rt_adaptive_variance_host(rgb.ctypes.data, var.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, 0, 3, out.ctypes.data) != 0 and "W and H" in _err(lib)
    for hole in range(4):
        args = [rgb.ctypes.data, var.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, 4, 3, out.ctypes.data]; args[hole] = None
        assert lib.rt_adaptive_variance_host(*args) != 0 and "null argument" in _err(lib)
    assert lib.rt_adaptive_variance_host(rgb.ctypes.data, var.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, 4, 3, None) != 0 and "null argument" in _err(lib)
    assert lib.rt_adaptive_variance_device(dev, dev, dev, dev, 4, 3, None, None) != 0 and "null argument" in _err(lib)
    assert lib.rt_adaptive_variance_device(dev, C.c_void_p(0x1004), dev, dev, 4, 3, dev, None) != 0 and "8-byte aligned" in _err(lib)
    assert lib.rt_adaptive_variance_device(dev, dev, dev, C.c_void_p(0x1002), 4, 3, dev, None) != 0 and "4-byte aligned" in _err(lib)
    assert (out == 7.0).all() and (vout == 7.0).all()
    # the progressive calls
    img = np.zeros(36, np.uint8)
    assert lib.rt_progressive_resolve_denoised_frame_rgb8(None, 0, 0, 3, good, 0, img.ctypes.data) != 0 and "null argument" in _err(lib)
    assert lib.rt_progressive_variance_counts(None, out.ctypes.data) != 0 and "null argument" in _err(lib)
    with pytest.raises(ValueError):
        R.denoise_frame_host(np.ones((3, 4, 3)), np.zeros((3, 4, 16)), counts=np.ones((4, 3), np.uint32))
    with pytest.raises(ValueError):
        R.denoise_frame_host(np.ones((3, 4, 3)), np.zeros((3, 4, 16)), var=np.ones((3, 4)))
    with pytest.raises(R.RenderError, match="iterations"):
        R.denoise_frame_host(np.ones((3, 4, 3)), np.zeros((3, 4, 16)), iterations=0)


def test_python_defaults():
    rgb, n, var, alb, hits = FC.frames((23, 37), (True, True, True))
    assert differing_words(R.denoise_frame_host(rgb, hits, n, var=var), R.denoise_frame_host(rgb, hits, n, 1, var, None, 1, R.DENOISE_ITERATIONS, R.DENOISE_VARIANCE_SIGMA, 0)) == 0
    assert differing_words(R.denoise_frame_host(rgb, hits, n), R.denoise_frame_host(rgb, hits, n, 1, None, None, 1, R.DENOISE_ITERATIONS, R.DENOISE_SIGMA, 0)) == 0
    assert (R.DENOISE_STOP_COLOUR, R.DENOISE_STOP_VARIANCE) == (0, 1)


# ---------------------------------------------------------------- 5. the host twins under AddressSanitizer + UBSan, stand-alone
def test_host_twins_under_sanitizers(tmp_path):
    """The runtimes are linked statically, so the program needs nothing from its environment.  Inside tests/test_sanitizers.py's run of
    this suite the twins are already the sanitizer build's (and a second, preloaded runtime would refuse to start beside the linked one)."""
    if os.environ.get("RT_SANITIZER_RUN") == "1":
        assert R.denoise_frame_host(np.ones((3, 4, 3)), np.zeros((3, 4, 16))).shape == (3, 4, 3)
        return
    exe = str(tmp_path / "denoise_frame_san")
    csrc = os.path.join(ROOT, "raytracinginrust_amd", "csrc")
    sources = [os.path.join(csrc, f) for f in ("rt_denoise_cpu.cpp", "rt_denoise_var_cpu.cpp", "rt_moments_cpu.cpp", "rt_adaptive_cpu.cpp", "rt_denoise_frame_cpu.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"] + sources + [os.path.join(ROOT, "tests", "denoise_frame_san_main.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and run.stderr == "", run.stdout + run.stderr

"""The moments of a progressive frame without a GPU (rt_moments_*_host, csrc/rt_moments_cpu.cpp): the merge, the per-pixel error estimate
and its statistics are defined by an exact f64 specification (csrc/rt_moments.h; + - * / and comparisons only, a fixed order), so the host
twin must equal the NumPy restatement of tests/moments_cases.py with 0 differing 64-bit words; the variance is pinned against the textbook
formula; every bad argument is an error with a message; and the twin runs clean under AddressSanitizer + UBSan as a stand-alone program.
tests/test_moments_gpu.py holds the HIP kernels to the twin."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracinginrust_amd import render as R

import moments_cases as MC
from moments_cases import differing_words


def host_merge_all(passes, sizes):
    S = np.zeros_like(passes[0]); Q = np.zeros_like(passes[0])
    for p, n_b in zip(passes, sizes):
        R.moments_merge_host(p, n_b, S, Q)
    return S, Q


# ---------------------------------------------------------------- 1. the host twin is the specification
@pytest.mark.parametrize("shape", MC.SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_host_twin_equals_the_numpy_restatement(shape):
    passes = MC.case(shape)
    S, Q = host_merge_all(passes, MC.PASS_SAMPLES)
    wS, wQ = MC.numpy_merge_all(passes, MC.PASS_SAMPLES)
    assert differing_words(S, wS) == 0 and differing_words(Q, wQ) == 0
    S, Q, N, B = MC.state(shape)
    for n_passes in (2, B, 1000):                              # (the pass count enters as B - 1 only)
        e2 = R.moments_error_host(S, Q, N, n_passes)
        want = MC.numpy_error(S, Q, N, n_passes)
        assert e2.shape == shape and differing_words(e2, want) == 0
        for tau in (0.0, 1.0 / 256.0, 0.05, 1e30, MC.INF):
            assert MC.stats_words(R.moments_stats_host(e2, tau)) == MC.numpy_stats(want, tau), (n_passes, tau)


@pytest.mark.parametrize("shape", MC.SHAPES[1:], ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_inputs_do_what_they_are_for(shape):
    S, Q, N, B = MC.state(shape)
    c = {k: v.reshape(-1, 3) for k, v in MC.numpy_channels(S, Q, N, B).items()}
    e2 = MC.numpy_error(S, Q, N, B).reshape(-1)
    Sf = S.reshape(-1, 3)
    assert np.isnan(Sf[MC.PX_NAN, 1]) and Sf[MC.PX_PINF, 0] == MC.INF and Sf[MC.PX_NINF, 2] == -MC.INF
    # a non-finite sum has a NaN ssb, which the clamp sends to 0: that channel's e2 is 0 and the pixel's comes from its other channels
    for px, ch in ((MC.PX_NAN, 1), (MC.PX_PINF, 0), (MC.PX_NINF, 2), (MC.PX_OVERFLOW, 1)):
        assert np.isnan(c["ssb_raw"][px, ch]) and c["e2"][px, ch] == 0.0 and np.isfinite(e2[px]) and e2[px] > 0.0
    assert e2[MC.PX_Q_INF] == MC.INF                           # the one non-finite e2: +inf in Q beside a finite sum
    assert (~np.isfinite(e2)).sum() == 1
    assert (c["m"][MC.PX_DARK] < MC.DELTA).all() and (c["den"][MC.PX_DARK] == MC.DELTA).all() and e2[MC.PX_DARK] > 0.0
    assert c["saturated"][MC.PX_SAT_YES].all() and e2[MC.PX_SAT_YES] == 0.0 and (c["V"][MC.PX_SAT_YES] > 0.0).all()
    assert (c["m"][MC.PX_SAT_NO] >= 1.0).any() and not c["saturated"][MC.PX_SAT_NO][c["m"][MC.PX_SAT_NO] >= 1.0].any() and e2[MC.PX_SAT_NO] > 0.0
    raw = c["ssb_raw"][list(MC.PX_CONST)]
    assert (raw < 0.0).any() and (np.abs(raw) < 1e-12).all()      # the true ssb is 0; its rounding falls below zero for some, and is clamped
    assert (c["V"][list(MC.PX_CONST)][raw < 0.0] == 0.0).all()


def test_e2_exactly_equal_to_tau2_counts_as_converged():
    passes, sizes, tau = MC.exact_tau_case()
    S, Q = host_merge_all(passes, sizes)
    e2 = R.moments_error_host(S, Q, 2, 2)
    assert differing_words(e2, MC.numpy_error(S, Q, 2, 2)) == 0
    assert e2[0, 0] == tau * tau == 2.0 ** -6 and e2[0, 1] > tau * tau > e2[0, 2] > 0.0 and e2[0, 3] == 0.0
    st = R.moments_stats_host(e2, tau)
    assert (st["converged"], st["unconverged"], st["nonfinite"]) == (3, 1, 0) and st["max_e2"] == e2[0, 1] and st["max_error"] > tau
    assert MC.stats_words(st) == MC.numpy_stats(e2, tau)
    # the statistics alone, on a map with the threshold, its neighbours, zeros of both signs, non-finite and negative values
    e, tau = MC.stats_case()
    st = R.moments_stats_host(e, tau)
    assert MC.stats_words(st) == MC.numpy_stats(e, tau)
    assert (st["converged"], st["unconverged"], st["nonfinite"], st["max_e2"]) == (7, 2, 3, 3.5)
    for perm in (np.arange(e.size)[::-1], np.random.RandomState(3).permutation(e.size)):
        assert MC.stats_words(R.moments_stats_host(e[perm], tau)) == MC.stats_words(st)       # no word depends on the order of the pixels


# ---------------------------------------------------------------- 2. the formula, not only its restatement
@pytest.mark.parametrize("n_b,B", [(2, 5), (4, 7), (16, 32)])
def test_equal_passes_give_the_textbook_variance_of_the_batch_means(n_b, B):
    H, W = 6, 5
    rs = np.random.RandomState(100 * n_b + B)
    passes = [rs.uniform(0.0, 1.0, (n_b, H, W, 3)).sum(axis=0) for _ in range(B)]
    S, Q = host_merge_all(passes, [n_b] * B)
    N = n_b * B
    means = np.stack(passes) / n_b                                        # the B batch means of every channel
    V_textbook = means.var(axis=0, ddof=1) / B                            # the variance of their mean
    V = MC.numpy_channels(S, Q, N, B)["V"]
    assert np.abs(V - V_textbook).max() <= 1e-12 * V_textbook.max() and (np.abs(V - V_textbook) <= 1e-12 * V_textbook).all()
    m = means.mean(axis=0)
    assert (m < 1.0).all() and (m > MC.DELTA).all()                       # no clamp, no saturation: e2 is V / (4 m) of the worst channel
    want = (V_textbook / (4.0 * m)).max(axis=2)
    got = R.moments_error_host(S, Q, N, B)
    assert (np.abs(got - want) <= 1e-12 * want).all()
    # unequal passes estimate the same sigma^2 (one-way ANOVA): the same samples cut 1 + the rest / in halves / evenly agree in expectation,
    # so their average over many pixels agrees closely — a coarse check that the n_b weights are the right ones
    if n_b == 16:
        x = rs.uniform(0.0, 1.0, (64, 40, 40, 3))                         # 64 samples of 1600 pixels, sigma^2 = 1/12
        for cuts in ((1, 63), (8, 56), (32, 32), (16, 16, 16, 16), (3, 5, 8, 16, 32)):
            edges = np.cumsum((0,) + cuts)
            S, Q = host_merge_all([x[a:b].sum(axis=0) for a, b in zip(edges[:-1], edges[1:])], cuts)
            V = MC.numpy_channels(S, Q, 64, len(cuts))["V"]
            # E[V] = sigma^2 / N; the relative spread of the estimate over 4800 channels with B - 1 >= 1 degrees of freedom is
            # sqrt(2 / (B - 1) / 4800) <= 0.021 (normal theory; uniform samples have lighter tails): 5 sigma
            assert abs(V.mean() * 64 * 12 - 1.0) < 5 * 0.021, cuts


# ---------------------------------------------------------------- 3. arguments
def _err(lib):
    return lib.rt_last_error().decode()


def test_bad_arguments_are_errors_with_a_message(pbe):
    lib = pbe.lib
    s = np.ones((2, 3, 3)); q = np.ones((2, 3, 3)); p = np.ones((2, 3, 3)); e = np.full((2, 3), 7.0)
    st = (C.c_uint64 * 4)(7, 7, 7, 7)
    dev = C.c_void_p(0x1000)                                   # never dereferenced: every call below is refused before a device is looked at
    sp, qp, pp, ep = s.ctypes.data, q.ctypes.data, p.ctypes.data, e.ctypes.data
    # merge: n_samples = 0, null pointers
    assert lib.rt_moments_merge_host(pp, 0, sp, qp, 18) != 0 and "n_samples" in _err(lib)
    assert lib.rt_moments_merge_device(dev, 0, dev, dev, 18, None) != 0 and "n_samples" in _err(lib)
    for hole in (0, 2, 3):
        args = [pp, 1, sp, qp, 18]; args[hole] = None
        assert lib.rt_moments_merge_host(*args) != 0 and "null argument" in _err(lib)
        args = [dev, 1, dev, dev, 18, None]; args[hole] = None
        assert lib.rt_moments_merge_device(*args) != 0 and "null argument" in _err(lib)
    assert lib.rt_moments_merge_device(C.c_void_p(0x1004), 1, dev, dev, 18, None) != 0 and "8-byte aligned" in _err(lib)
    # error: passes < 2, samples = 0, an empty or too large frame, null pointers
    for (samples, passes, W, H), text in (((8, 1, 3, 2), "passes"), ((8, 0, 3, 2), "passes"), ((0, 2, 3, 2), "samples"), ((8, 2, 0, 2), "W and H"),
                                          ((8, 2, 3, 0), "W and H"), ((8, 2, 65536, 32768), "too large")):
        assert lib.rt_moments_error_host(sp, qp, samples, passes, W, H, ep) != 0 and text in _err(lib), text
        assert lib.rt_moments_error_device(dev, dev, samples, passes, W, H, dev, 0.1, dev, None) != 0 and text in _err(lib), text
    for hole in (0, 1, 6):
        args = [sp, qp, 8, 2, 3, 2, ep]; args[hole] = None
        assert lib.rt_moments_error_host(*args) != 0 and "null argument" in _err(lib)
    for hole in (0, 1):
        args = [dev, dev, 8, 2, 3, 2, dev, 0.1, dev, None]; args[hole] = None
        assert lib.rt_moments_error_device(*args) != 0 and "null argument" in _err(lib)
    # tau negative or NaN
    for tau in (-1.0, -1e-300, float("nan"), -MC.INF):
        assert lib.rt_moments_stats_host(ep, 6, tau, st) != 0 and "tau" in _err(lib)
        assert lib.rt_moments_error_device(dev, dev, 8, 2, 3, 2, dev, tau, dev, None) != 0 and "tau" in _err(lib)
    assert lib.rt_moments_stats_host(None, 6, 0.1, st) != 0 and "null argument" in _err(lib)
    assert lib.rt_moments_stats_host(ep, 6, 0.1, None) != 0 and "null argument" in _err(lib)
    # nothing was written
    assert (s == 1.0).all() and (q == 1.0).all() and (e == 7.0).all() and list(st) == [7, 7, 7, 7]
    # the frame calls
    words = (C.c_uint64 * 4)(); n = C.c_uint64(); ptr = C.c_void_p()
    for rc in (lib.rt_progressive_enable_moments(None), lib.rt_progressive_passes(None, C.byref(n)), lib.rt_progressive_read_moments(None, ep),
               lib.rt_progressive_load_moments(None, sp, qp, 1, 1), lib.rt_progressive_error_map(None, ep),
               lib.rt_progressive_error_map_device(None, C.byref(ptr), None), lib.rt_progressive_error_stats(None, 0.1, words)):
        assert rc != 0 and "null argument" in _err(lib)
    # the Python layer
    with pytest.raises(ValueError):
        R.moments_error_host(np.ones((2, 3, 3)), np.ones((2, 3, 2)), 8, 2)
    with pytest.raises(ValueError):
        R.moments_merge_host(np.ones((2, 3, 3)), 1, np.ones((2, 3, 3)), np.ones((2, 3, 3), np.float32))
    with pytest.raises(R.RenderError, match="passes"):
        R.moments_error_host(s, q, 8, 1)
    with pytest.raises(R.RenderError, match="tau"):
        R.moments_stats_host(e, -0.5)


def test_without_a_device_the_device_paths_fail_like_rt_render(pbe):
    if R.device_count() > 0:                                   # (the messages can only be seen on a machine without a device)
        return
    from raytracinginrust_amd import scenes
    b, cam, bg = scenes.cornell_box(pbe)
    with pytest.raises(R.RenderError, match="no HIP device") as one_shot:
        R.render(b, cam, bg, 8, 8, 1, 4)
    dev = C.c_void_p(0x1000)
    assert pbe.lib.rt_moments_merge_device(dev, 4, dev, dev, 18, None) != 0 and _err(pbe.lib) == str(one_shot.value)
    assert pbe.lib.rt_moments_error_device(dev, dev, 8, 2, 3, 2, dev, 0.1, dev, None) != 0 and _err(pbe.lib) == str(one_shot.value)
    with pytest.raises(R.RenderError, match="no HIP device"):  # no frame to enable moments on: create is where a progressive frame fails
        R.Progressive(b, cam, bg, 8, 8, 4, moments=True)
    with pytest.raises(R.RenderError, match="no HIP device"):
        next(R.render_progressive(b, cam, bg, 8, 8, 8, 4, passes=2, until_error=0.1))


def test_render_progressive_checks_its_stopping_arguments(pbe):
    from raytracinginrust_amd import scenes
    b, cam, bg = scenes.cornell_box(pbe)
    with pytest.raises(ValueError, match="min_passes"):
        next(R.render_progressive(b, cam, bg, 8, 8, 8, 4, passes=2, until_error=0.1, min_passes=1))


# ---------------------------------------------------------------- 4. the host twin under AddressSanitizer + UBSan, stand-alone
def test_host_twin_under_sanitizers(tmp_path):
    """The runtimes are linked statically, so the program needs nothing from its environment.  Inside tests/test_sanitizers.py's run of
    this suite the twin is already the sanitizer build's (and a second, preloaded runtime would refuse to start beside the linked one)."""
    if os.environ.get("RT_SANITIZER_RUN") == "1":
        return
    exe = str(tmp_path / "moments_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "raytracinginrust_amd", "csrc", "rt_moments_cpu.cpp"),
                    os.path.join(ROOT, "tests", "moments_san_main.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and run.stderr == "", run.stdout + run.stderr

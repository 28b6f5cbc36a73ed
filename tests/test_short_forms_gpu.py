"""The exact short forms of the lean f64 kernel on the device (csrc/rt_short.h; rt_kernel.hip div_pi_pair, div_frame, rng_u01_of,
rect_absdot — run on caller operands through rt_debug_short_forms), bit for bit against NumPy's `/`, the U01 expression of rt_rng.h and
the reference's full form of AARect::pdf_value; and whole frames of the lean f64 kernel per sample against the CPU oracle at frame sizes
whose divisors are and are not served by the short division.  tests/test_short_forms_host.py checks the same functions on the host."""

from fractions import Fraction

import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from test_fuzz_gpu import SAMPLE_RTOL, _rand_box_room_scene, _rand_list_scene

pytestmark = pytest.mark.gpu

PI = 3.14159265358979323846264338327950288
WAVES, LANES = 256, 64
N = WAVES * LANES


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def recip_for(C):
    """csrc/rt_short.h sf_recip_for, with exact rationals in place of its one fma"""
    if not (2.0 ** -32 <= C <= 2.0 ** 32):
        return 0.0
    zh = 1.0 / C
    return zh if abs(Fraction(zh) * Fraction(C) - 1) * 2 ** 53 < Fraction(1, 2) else 0.0


def numerators(rnd, n, C):
    """the four kinds of tests/short_forms_main.cpp: [0, 1), i + U01 with i < 2^15, exponents down to 2^-63, within +-3 ulp of the
    rounding midpoints of quotients by C"""
    k = n // 4
    q = rnd.uniform(1.0, 2.0, n - 3 * k) * 2.0 ** rnd.integers(-16, 16, n - 3 * k)
    mid = (words(q * C + C * (np.spacing(q) * 0.5)) + rnd.integers(-3, 4, len(q)).astype(np.uint64)).view(np.float64)     # ~ C (q + ulp(q) / 2)
    x = np.concatenate([rnd.random(k), rnd.integers(0, 2 ** 15, k) + rnd.random(k), rnd.uniform(1.0, 2.0, k) * 2.0 ** -rnd.integers(0, 64, k).astype(np.float64), mid])
    return rnd.permutation(x)


def test_divisions_by_pi(pbe):
    """64 x 256 (cosine, m) pairs; guard cases mixed into otherwise clear waves.  Every quotient equals NumPy's; a wave whose numerators
    are all served — in range, or not divided (cosine not > 0), or a zero m — takes the three instructions, any other the plain ones."""
    rnd = np.random.default_rng(9101)
    cos = numerators(rnd, N, PI).reshape(WAVES, LANES)
    m = numerators(rnd, N, PI).reshape(WAVES, LANES)
    served = np.ones(WAVES, bool)
    # waves 0-63 stay clear; 64-127: cases the short path serves by its selects; 128-255: cases that must send the wave to the division
    soft_cos = [0.0, -0.0, -0.25, -np.inf, np.nan, -1e-310, -2.0 ** -950]
    soft_m = [0.0, -0.0]
    hard_cos = [2.0 ** -901, 1e-310, 5e-324, np.inf, 2.0 ** 900, 2.0 ** -1022]
    hard_m = hard_cos + [-1.0, -2.0 ** -950]
    for w in range(64, 128):
        lanes = rnd.permutation(LANES)[:6]
        cos[w, lanes[:3]] = rnd.choice(soft_cos, 3)
        m[w, lanes[3:]] = rnd.choice(soft_m, 3)
    for w in range(128, WAVES):
        lane = rnd.integers(0, LANES)
        if w % 2:
            cos[w, lane] = hard_cos[(w // 2) % len(hard_cos)]
        else:
            m[w, lane] = hard_m[(w // 2) % len(hard_m)]
        served[w] = False
    out = R.debug_short_forms(0, cos, m)
    with np.errstate(all="ignore"):
        want_pdf = np.where(cos > 0.0, cos / PI, 0.0).reshape(-1)
        want_sc = (m / PI).reshape(-1)
    assert (words(out[:, 0]) == words(want_pdf)).all(), f"{int((words(out[:, 0]) != words(want_pdf)).sum())} pdf values differ from cosine / pi"
    assert (words(out[:, 1]) == words(want_sc)).all(), f"{int((words(out[:, 1]) != words(want_sc)).sum())} values differ from m / pi"
    took = out[:, 2].reshape(WAVES, LANES)
    assert (took == took[:, :1]).all(), "the vote is not wave-uniform"
    assert np.array_equal(took[:, 0] != 0.0, served), f"waves {np.flatnonzero((took[:, 0] != 0.0) != served).tolist()} took the other path"


def test_division_by_the_frames_constants(pbe):
    """the camera's division: numerators i + U01 (and the other kinds), divisors W - 1 the host enables (799, 255, 3839, 1, 8191 if so) and
    ones it does not (63, 399, 1919: reciprocal 0, the plain division), mixed within waves"""
    rnd = np.random.default_rng(9102)
    divisors = np.array([799.0, 255.0, 3839.0, 2159.0, 1079.0, 1.0, 63.0, 399.0, 1919.0])
    zh = np.array([recip_for(c) for c in divisors])
    assert (zh[:5] != 0.0).all() and zh[5] == 1.0 and (zh[6:] == 0.0).all()
    pick = rnd.integers(0, len(divisors), N)
    C = divisors[pick]
    x = np.empty(N)
    for i, c in enumerate(divisors):
        sel = pick == i
        x[sel] = numerators(rnd, int(sel.sum()), c)
    x[rnd.permutation(N)[:256]] = 0.0                                        # pixel 0 with a U01 of 0
    got = R.debug_short_forms(1, x, np.stack([C, zh[pick]], axis=1))
    assert (words(got) == words(x / C)).all(), f"{int((words(got) != words(x / C)).sum())} quotients differ"


def test_u01(pbe):
    rnd = np.random.default_rng(9103)
    u = rnd.integers(0, 2 ** 64, N, dtype=np.uint64)
    u[:9] = np.array([0, 2 ** 64 - 1, 0x7FF, 2 ** 64 - 1 - 0x7FF, 0x800, 0xFFFFF80000000000, 0x000007FFFFFFF800, 0x0000080000000000, 2 ** 63], np.uint64)
    v = u >> np.uint64(11)
    want = ((v >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (v & np.uint64(0xFFFFFFFF)).astype(np.float64)) * 2.0 ** -53     # rt_rng.h
    got = R.debug_short_forms(2, u)
    assert (words(got) == words(want)).all(), f"{int((words(got) != words(want)).sum())} of {N} values differ"
    assert got.max() < 1.0 and got.min() == 0.0


def _rect_pdf_full(v, t, k, area):
    """rect.rs:91-101 after the hit test, operation by operation (NumPy's *, +, /, sqrt round once each)"""
    with np.errstate(all="ignore"):
        ax = [np.where(k == a, 1.0, 0.0) for a in range(3)]
        neg = v[:, 0] * ax[0] + v[:, 1] * ax[1] + v[:, 2] * ax[2] < 0.0
        n = [np.where(neg, ax[a], -1.0 * ax[a]) for a in range(3)]
        ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        d2 = (t * t) * (ln * ln)
        cosine = np.abs(v[:, 0] * n[0] + v[:, 1] * n[1] + v[:, 2] * n[2]) / ln
        return np.where(cosine != 0.0, d2 / (cosine * area), 0.0)


def test_rect_light_pdf(pbe):
    """random finite directions, every pattern of +-0 components among them: waves of them take |v_k|; a wave with a NaN or infinite
    component (or an overflowing length) takes the two dot products; every pdf equals the full form's"""
    rnd = np.random.default_rng(9104)
    v = rnd.uniform(-1.0, 1.0, (N, 3)) * 2.0 ** rnd.integers(-16, 16, (N, 1))
    pat = np.arange(N) % 64
    for a in range(3):
        zero = ((pat >> a) & 1 == 1) & (np.arange(N) < N // 2)
        v[zero, a] = 0.0
        flip = ((pat >> (3 + a)) & 1 == 1) & (np.arange(N) < N // 2)
        v[flip, a] = -v[flip, a]
    assert (np.signbit(v) & (v == 0.0)).any()
    v = v.reshape(WAVES, LANES, 3)[rnd.permutation(WAVES)]
    finite = np.ones(WAVES, bool)
    for w in range(192, WAVES):
        v[w, rnd.integers(0, LANES), rnd.integers(0, 3)] = [np.nan, np.inf, -np.inf, 1e200][w % 4]
        finite[w] = False
    v = v.reshape(N, 3)
    t, k, area = rnd.uniform(0.001, 1000.0, N), rnd.integers(0, 3, N), rnd.uniform(0.5, 20000.0, N)
    out = R.debug_short_forms(3, v, np.stack([t, k.astype(np.float64), area], axis=1))
    want = _rect_pdf_full(v, t, k, area)
    same = (words(out[:, 0]) == words(want)) | (np.isnan(out[:, 0]) & np.isnan(want))
    assert same.all(), f"{int((~same).sum())} of {N} pdf values differ from the full form"
    took = out[:, 1].reshape(WAVES, LANES)
    assert (took == took[:, :1]).all() and np.array_equal(took[:, 0] != 0.0, finite)


def _scene(be, which):
    if which == "cornell":
        return scenes.cornell_box(be)
    kind, seed = which.split("-")
    return _rand_box_room_scene(be, int(seed))[:3] if kind == "room" else _rand_list_scene(be, int(seed))


@pytest.fixture(scope="module")
def oracle_samples(obe):
    """the oracle's samples of a (scene, W, H), rendered once"""
    from oracle import orc
    cache = {}

    def get(which, W, H, spp, depth, seed):
        key = (which, W, H, spp, depth, seed)
        if key not in cache:
            ob, ocam, obg = _scene(obe, which)
            cache[key] = orc.render(ob, ocam, obg, W, H, spp, depth, seed=seed, want_samples=True, want_counters=True)[1:]
        return cache[key]
    return get


@pytest.mark.parametrize("size", [(256, 64), (64, 256)])
@pytest.mark.parametrize("which", ["cornell", "room-704", "room-705", "list-1", "list-5"])
def test_samples_against_the_oracle(pbe, oracle_samples, which, size, monkeypatch):
    """rt_render_samples of the lean f64 kernel, 4 samples per pixel, depth 50, per sample against the CPU oracle (the suite's per-sample
    bound: 1e-9 relative, at most 2 paths diverged over a last-ulp difference of a libm-class function).  255 is a divisor the short
    division serves and 63 one it does not, on either axis.  And the same frame with RT_NO_SHORT_DIV — the plain division for both
    — has the same 64-bit words."""
    W, H = size
    spp, depth, seed = 4, 50, 41
    assert recip_for(255.0) != 0.0 and recip_for(63.0) == 0.0
    rs, cnt = oracle_samples(which, W, H, spp, depth, seed)
    assert (rs != 0.0).any(), "the oracle's frame is black"
    b, cam, bg = _scene(pbe, which)
    _, gs = R.render(b, cam, bg, W, H, spp, depth, seed=seed, want_samples=True)
    assert R.last_loop_info(b)["kernel"] == "rt::pathtrace_kernel<double, 0u>", "not the lean f64 kernel"
    assert np.array_equal(np.isnan(gs), np.isnan(rs)) and np.array_equal(np.isinf(gs), np.isinf(rs))
    fin = np.isfinite(rs)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs, 0.0)))).any(axis=-1)
    assert bad.sum() <= 2, f"{int(bad.sum())} of {W * H * spp} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"
    assert R.last_stats(b)["nonfinite_samples"] == cnt["nonfinite"]
    monkeypatch.setenv("RT_NO_SHORT_DIV", "1")
    b0, cam0, bg0 = _scene(pbe, which)
    _, plain = R.render(b0, cam0, bg0, W, H, spp, depth, seed=seed, want_samples=True)
    n_words = int((words(gs) != words(plain)).sum())
    assert n_words == 0, f"{n_words} 64-bit words differ from the frame with the plain divisions"

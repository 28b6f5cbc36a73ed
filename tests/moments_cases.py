"""What tests/test_moments_host.py and tests/test_moments_gpu.py share: the NumPy restatement of the moments' specification
(csrc/rt_moments.h, include/rt_amd.h) and the inputs both compare on.

The restatement is written from the specification, not from the C++: elementwise NumPy operations only, one IEEE operation each, in the
specification's order; comparisons with a NaN are false, as in C."""
import functools

import numpy as np

INF = float("inf")
DELTA = np.float64(2.0 ** -8)
SHAPES = ((1, 1), (11, 15), (3, 64))                         # (H, W): the issue's 1x1, 15x11 and 64x3
PASS_SAMPLES = (3, 5, 8, 16)                                   # unequal n_b


def differing_words(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape
    return int((a.view(np.uint64) != b.view(np.uint64)).sum())


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-53 (Higham): n rounding errors compounded."""
    u = 2.0 ** -53
    return n * u / (1.0 - n * u)


# ---------------------------------------------------------------- the restatement
def numpy_merge(S, Q, p, n_b):
    """(1): the new (S, Q) after pass frame p of n_b samples."""
    nb = np.float64(n_b)
    with np.errstate(all="ignore"):
        S2 = S + p
        pp = p * p
        Q2 = Q + pp / nb
    return S2, Q2


def numpy_merge_all(passes, sizes):
    S = np.zeros_like(passes[0]); Q = np.zeros_like(passes[0])
    for p, n_b in zip(passes, sizes):
        S, Q = numpy_merge(S, Q, p, n_b)
    return S, Q


def finite(v):
    with np.errstate(all="ignore"):
        return (v - v) == 0.0


def numpy_channels(S, Q, samples, passes):
    """(2) per channel: every intermediate, for the tests that look at them."""
    Nd = np.float64(samples); Bm1 = np.float64(passes - 1)
    with np.errstate(all="ignore"):
        m = S / Nd
        ss = S * S
        ssb_raw = Q - ss / Nd
        ssb = np.where(ssb_raw > 0.0, ssb_raw, 0.0)
        V = (ssb / Bm1) / Nd
        den = np.where(m >= DELTA, m, DELTA)
        e2 = V / (np.float64(4.0) * den)
        over = m - np.float64(1.0)
        saturated = (m >= 1.0) & (over * over >= np.float64(9.0) * V)
        e2 = np.where(saturated, 0.0, e2)
    return {"m": m, "ssb_raw": ssb_raw, "V": V, "den": den, "saturated": saturated, "e2": e2}


def numpy_error(S, Q, samples, passes):
    """(2): e2 of every pixel, S.shape[:-1]."""
    c = numpy_channels(S, Q, samples, passes)["e2"]
    e = c[..., 0].copy()
    for k in (1, 2):
        x = c[..., k]
        fe, fx = finite(e), finite(x)
        with np.errstate(all="ignore"):
            take = fe & (~fx | (x > e))
        e = np.where(take, x, e)
    return e


def numpy_stats(e2, tau):
    """(3): the four words as Python ints."""
    e = np.ascontiguousarray(e2, np.float64).reshape(-1)
    tau2 = np.float64(tau) * np.float64(tau)
    f = finite(e)
    with np.errstate(all="ignore"):
        conv = int((f & (e <= tau2)).sum()); unconv = int((f & (e > tau2)).sum())
    mx = np.float64(0.0)
    for v in e[f]:                                             # "replaced by a finite e2 that is > it", pixel by pixel
        if v > mx:
            mx = v
    return [conv, unconv, int((~f).sum()), int(np.array([mx]).view(np.uint64)[0])]


def stats_words(d):
    """The dict of render.moments_stats back as the four words."""
    return [d["converged"], d["unconverged"], d["nonfinite"], int(np.array([d["max_e2"]], np.float64).view(np.uint64)[0])]


# ---------------------------------------------------------------- inputs
# where the special pixels of a frame of >= 33 pixels sit (flat pixel index), and what they are for
PX_NAN, PX_PINF, PX_NINF, PX_DARK, PX_SAT_YES, PX_SAT_NO, PX_OVERFLOW, PX_Q_INF = 1, 4, 7, 9, 12, 14, 17, 18
PX_CONST = tuple(range(20, 32))                                # every pass holds n_b * c: the true ssb is 0 and its rounding falls on either side


@functools.lru_cache(maxsize=None)
def case(shape, sizes=PASS_SAMPLES):
    """The pass frames (a tuple of (H, W, 3) arrays, read-only) of passes of `sizes` samples: n_b times a uniform mean, and — in every
    frame of >= 33 pixels — the special pixels above."""
    H, W = shape
    rs = np.random.RandomState(9000 + 131 * H + W)
    passes = []
    for b, n_b in enumerate(sizes):
        p = rs.uniform(0.0, 1.0, (H, W, 3)) * n_b
        flat = p.reshape(-1, 3)
        if H * W >= 33:
            if b == 1:
                flat[PX_NAN, 1] = np.nan; flat[PX_PINF, 0] = INF; flat[PX_NINF, 2] = -INF
                flat[PX_OVERFLOW, 1] = 1e160                   # p * p and S * S both overflow: ssb = inf - inf
            flat[PX_DARK] = rs.uniform(0.0, 1.0, 3) * 1e-3 * n_b                    # a mean under delta
            flat[PX_SAT_YES] = (3.0 + 0.01 * rs.uniform(-1.0, 1.0, 3)) * n_b       # (m - 1)^2 ~ 4 against 9 V ~ 1e-5
            flat[PX_SAT_NO] = (1.05 + (0.9 if b % 2 else -0.9) + 0.01 * rs.uniform(-1.0, 1.0, 3)) * n_b      # m ~ 1.33: (m - 1)^2 ~ 0.11 against 9 V ~ 2
            for k, px in enumerate(PX_CONST):
                for c in range(3):
                    flat[px, c] = np.float64(n_b) * np.float64((0.1, 0.3, 0.7, 1.0 / 3.0, 0.013, 2.9)[(k + c) % 6] + 0.01 * k)
        p.setflags(write=False)
        passes.append(p)
    return tuple(passes)


@functools.lru_cache(maxsize=None)
def state(shape, sizes=PASS_SAMPLES):
    """(S, Q, samples, passes) for the error map: `case` merged by the restatement, and — in every frame of >= 33 pixels — one second
    moment set to +inf beside its finite sum, as a loaded checkpoint may hold: the one way to a non-finite e2 (the clamp sends a NaN ssb,
    which is what a non-finite SUM gives, to 0)."""
    S, Q = numpy_merge_all(case(shape, sizes), sizes)
    if shape[0] * shape[1] >= 33:
        Q = Q.copy(); Q.reshape(-1, 3)[PX_Q_INF, 1] = INF
    S.setflags(write=False); Q.setflags(write=False)
    return S, Q, sum(sizes), len(sizes)


def exact_tau_case():
    """Two passes of one sample, 1 x 4 pixels, every operation exact in binary: pixel 0 has e2 = 2^-6 = (2^-3)^2 exactly, pixel 1 just more,
    pixel 2 just less (a one-ulp change of one sample), pixel 3 is constant (e2 = 0).  -> (passes, sizes, tau)"""
    a = np.array([[[0.375] * 3, [0.375] * 3, [0.375] * 3, [0.25] * 3]])
    b = np.array([[[0.125] * 3, [0.125] * 3, [0.125] * 3, [0.25] * 3]])
    a[0, 1, 0] = 0.375 + 2.0 ** -40; b[0, 1, 0] = 0.125 - 2.0 ** -40      # same mean, a wider spread
    a[0, 2] = 0.375 - 2.0 ** -40; b[0, 2] = 0.125 + 2.0 ** -40             # same mean, a narrower spread, all channels
    return (a, b), (1, 1), 0.125


def stats_case():
    """An error map for rt_moments_stats_host alone, and its tau: values equal to tau^2, one ulp to either side, zeros, a NaN, both
    infinities and a negative value (no error map holds one; it is finite and not > 0)."""
    t2 = np.float64(0.25)
    e = np.array([t2, np.nextafter(t2, 1.0), np.nextafter(t2, 0.0), 0.0, -0.0, np.nan, INF, -INF, 3.5, 1e-300, -2.0, t2], np.float64)
    return e, 0.5

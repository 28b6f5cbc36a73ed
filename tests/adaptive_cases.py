"""What tests/test_adaptive_host.py and tests/test_adaptive_gpu.py share: the NumPy restatement of the adaptive frames' specification
(csrc/rt_adaptive.h, include/rt_amd.h) and the states both compare on.

The restatement is written from the specification, not from the C++: elementwise NumPy operations only, one IEEE operation each, in the
specification's order; comparisons with a NaN are false, as in C.  Counts are uint32 arrays; the frames are those of moments_cases."""
import functools

import numpy as np

import moments_cases as MC
from moments_cases import differing_words, finite  # noqa: F401  (re-exported)

INF = float("inf")
MAX_SAMPLES = 2 ** 32 - 1
SHAPES = ((1, 1), (11, 15), (3, 64), (300, 300))               # (H, W)


# ---------------------------------------------------------------- the restatement
def numpy_error(S, Q, n, b):
    """(A): e2 of every pixel with its own counts; +inf where b < 2."""
    two = b >= 2
    Nd = n.astype(np.float64)[..., None]
    Bm1 = np.where(two, b.astype(np.int64) - 1, 1).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        m = S / Nd
        ss = S * S
        ssb = Q - ss / Nd
        ssb = np.where(ssb > 0.0, ssb, 0.0)
        V = (ssb / Bm1) / Nd
        den = np.where(m >= MC.DELTA, m, MC.DELTA)
        c = V / (np.float64(4.0) * den)
        over = m - np.float64(1.0)
        c = np.where((m >= 1.0) & (over * over >= np.float64(9.0) * V), 0.0, c)
    e = c[..., 0].copy()
    for k in (1, 2):
        x = c[..., k]
        fe, fx = finite(e), finite(x)
        with np.errstate(all="ignore"):
            take = fe & (~fx | (x > e))
        e = np.where(take, x, e)
    return np.where(two, e, INF)


def numpy_need(S, Q, n, b, tau):
    e2 = numpy_error(S, Q, n, b)
    tau2 = np.float64(tau) * np.float64(tau)
    with np.errstate(all="ignore"):
        return (b < 2) | (finite(e2) & (e2 > tau2))


def dilate3(need):
    """need, or one of the 8 neighbours inside the frame."""
    H, W = need.shape
    padded = np.zeros((H + 2, W + 2), dtype=bool)
    padded[1:-1, 1:-1] = need
    out = np.zeros_like(need)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= padded[dy:dy + H, dx:dx + W]
    return out


def numpy_active(S, Q, n, b, n_b, tau, max_samples=MAX_SAMPLES, spread=1):
    """(B): the active map, (H, W) bool."""
    need = numpy_need(S, Q, n, b, tau)
    needed = dilate3(need) if spread else need
    return needed & (n.astype(np.uint64) + np.uint64(n_b) <= np.uint64(max_samples))


def numpy_select(S, Q, n, b, n_b, tau, max_samples=MAX_SAMPLES, spread=1):
    """(B): the list."""
    return np.flatnonzero(numpy_active(S, Q, n, b, n_b, tau, max_samples, spread)).astype(np.uint32)


def numpy_merge(p, n_b, S, Q, n, b, pixels):
    """(C): the new (pass, S, Q, n, b); pixels not listed keep every word."""
    p2, S2, Q2, n2, b2 = (a.copy() for a in (p, S, Q, n, b))
    fp, fS, fQ = p2.reshape(-1, 3), S2.reshape(-1, 3), Q2.reshape(-1, 3)
    idx = np.asarray(pixels, dtype=np.int64)
    nb = np.float64(n_b)
    with np.errstate(all="ignore"):
        x = fp[idx]
        fS[idx] = fS[idx] + x
        xx = x * x
        fQ[idx] = fQ[idx] + xx / nb
    fp[idx] = 0.0
    n2.reshape(-1)[idx] += np.uint32(n_b)
    b2.reshape(-1)[idx] += np.uint32(1)
    return p2, S2, Q2, n2, b2


def numpy_resolve(S, n, prev=None):
    """(D): ((H, W, 3) uint8, changed pixels)."""
    Nd = n.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        x = np.sqrt(S / Nd)
        x = np.where(x < 0.0, 0.0, np.where(x > 0.999, 0.999, x))      # f64::clamp: a NaN stays
        y = np.float64(256.0) * x
        v = np.where(y > 0.0, y, 0.0)                                   # `as u64`: NaN and everything <= 0 give 0
    out = np.where((n > 0)[..., None], v.astype(np.uint64), 0).astype(np.uint8)
    changed = out.shape[0] * out.shape[1] if prev is None else int((out != prev).any(axis=2).sum())
    return out, changed


# ---------------------------------------------------------------- states
PX_B0, PX_B1 = 2, 3                                            # a pixel without a pass, and one with a single pass
PX_CAP_AT, PX_CAP_OVER = 5, 6                                  # n + N_B = CAP exactly, and one more
N_B, CAP = 8, 4000


@functools.lru_cache(maxsize=None)
def state(shape):
    """(S, Q, n, b), read-only: moments_cases.state (NaN and infinite sums, an infinite second moment, saturated, dark and constant pixels)
    under per-pixel counts — sample counts from {32, 35, 70, 1000}, pass counts from {2, 4, 7}, and in every frame of >= 33 pixels a pixel
    that holds nothing yet, one with a single pass, and two at the sample cap CAP and one past it."""
    S, Q, _, _ = MC.state(shape)
    H, W = shape
    rs = np.random.RandomState(77 + 3 * H + W)
    n = rs.choice(np.array([32, 35, 70, 1000], np.uint32), size=(H, W)).astype(np.uint32)
    b = rs.choice(np.array([2, 4, 7], np.uint32), size=(H, W)).astype(np.uint32)
    S = S.copy(); Q = Q.copy()
    if H * W >= 33:
        fS, fQ, fn, fb = S.reshape(-1, 3), Q.reshape(-1, 3), n.reshape(-1), b.reshape(-1)
        fS[PX_B0] = 0.0; fQ[PX_B0] = 0.0; fn[PX_B0] = 0; fb[PX_B0] = 0
        fn[PX_B1] = 5; fb[PX_B1] = 1
        fn[PX_CAP_AT] = CAP - N_B; fn[PX_CAP_OVER] = CAP - N_B + 1; fb[PX_CAP_AT] = fb[PX_CAP_OVER] = 2
    for a in (S, Q, n, b):
        a.setflags(write=False)
    return S, Q, n, b


@functools.lru_cache(maxsize=None)
def pass_frame(shape):
    """A pass frame of N_B samples for `state(shape)`: uniform means, a NaN and an infinity."""
    H, W = shape
    p = np.random.RandomState(500 + 7 * H + W).uniform(0.0, 1.0, (H, W, 3)) * N_B
    if H * W >= 33:
        p.reshape(-1, 3)[8, 0] = np.nan; p.reshape(-1, 3)[10, 2] = INF
    p.setflags(write=False)
    return p


def exact_tau_state():
    """moments_cases.exact_tau_case as a state with counts: 1 x 4 pixels of two passes of one sample; pixel 0 has e2 == tau^2 exactly (NOT
    needed: the comparison is >), pixel 1 just more, pixel 2 just less, pixel 3 is constant.  -> (S, Q, n, b, tau)"""
    passes, sizes, tau = MC.exact_tau_case()
    S, Q = MC.numpy_merge_all(passes, sizes)
    n = np.full((1, 4), 2, np.uint32); b = np.full((1, 4), 2, np.uint32)
    return S, Q, n, b, tau


def border_state(shape):
    """A frame in which exactly the four corners and the middles of the four edges are needed (one pass only: b = 1) and every other pixel
    is finished beyond doubt (Q = 0: ssb clamps to 0, e2 = 0) -> (S, Q, n, b, the needed flat indices)."""
    H, W = shape
    S = np.full((H, W, 3), 16.0); Q = np.zeros((H, W, 3)); n = np.full((H, W), 32, np.uint32); b = np.full((H, W), 4, np.uint32)
    spots = sorted({(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)})
    for y, x in spots:
        b[y, x] = 1; n[y, x] = 8
    return S, Q, n, b, np.array([y * W + x for y, x in spots], np.uint32)


def lists_for(n_px):
    """The lists of the issue: empty, one pixel, the last pixel only, every other pixel, all pixels."""
    return {"empty": np.zeros(0, np.uint32), "one": np.array([0], np.uint32), "last": np.array([n_px - 1], np.uint32),
            "every_other": np.arange(0, n_px, 2, dtype=np.uint32), "all": np.arange(n_px, dtype=np.uint32)}

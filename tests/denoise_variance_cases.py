"""What tests/test_denoise_variance_host.py and tests/test_denoise_variance_gpu.py share: the NumPy restatement of the variance-guided
denoiser's specification (csrc/rt_denoise_var.h (B)-(D), csrc/rt_moments.h (4)), the variance frames both compare on beside the colour
and guide frames of tests/denoise_cases.py, and the quality set-up.

The restatement is written from the specification, not from the C++: elementwise NumPy operations only, one IEEE operation each, in the
specification's order; comparisons with a NaN are false, as in C."""
import functools

import numpy as np

import denoise_cases as DC
from denoise_cases import INF, H_B3, differing_words, sigma3  # noqa: F401  (re-exported for the two test files)

SHAPES = DC.SHAPES
# sigma = (variance, normal, plane): finite values that leave some taps of the random frames in and cut others; every stop off; a mix
SIGMAS = ((1.5, 1.2, 1.0), (INF, INF, INF), (INF, 1.2, INF))
FLAGS = DC.FLAGS
SAMPLES = DC.SAMPLES
EPS = np.float64(2.0 ** -16)
B_3 = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)
G = 0x9E3779B97F4A7C15


def settings_for(shape):
    """Every (iterations, sigma, flags) a shape is checked with: K = 1 .. 5, and 8 on the 3 x 5 frame."""
    return [(k, sg, fl) for k in DC.iterations_for(shape) for sg in SIGMAS for fl in FLAGS]


@functools.lru_cache(maxsize=None)
def case(shape):
    """(rgb_sum, var, hits): the frames of denoise_cases.case — misses, a medium's hits, NaN / +inf / -inf colour channels — and a variance
    frame (H, W, 3) on the scale of the colour differences, with — in every frame of more than one pixel — all-zero pixels, a NaN, a +inf and
    a negative entry (each of which makes its pixel's v count as 0, unless the other channels outweigh the negative one)."""
    H, W = shape
    rgb, hits = DC.case(shape)
    rs = np.random.RandomState(8000 + 131 * H + W)
    var = rs.uniform(0.0, 0.3, (H, W, 3))
    if H * W > 1:
        px = var.reshape(-1, 3)
        where = rs.choice(len(px), size=min(len(px), max(5, len(px) // 30)), replace=False)
        for k, i in enumerate(where):
            if k % 5 == 0: px[i] = 0.0
            elif k % 5 == 1: px[i, 1] = np.nan
            elif k % 5 == 2: px[i, 0] = INF
            elif k % 5 == 3: px[i, 2] = -5.0           # the sum is negative
            else: px[i, 2] = -0.01                     # a negative entry whose pixel keeps a positive sum
    var.setflags(write=False)
    return rgb, var, hits


def finite(v):
    with np.errstate(all="ignore"):
        return (v - v) == 0.0


def _stop(t):
    return np.where(t > 0.0, t * t, 0.0)


def numpy_variance(S, Q, samples, passes):
    """(A): the variance of the mean per pixel and channel."""
    Nd = np.float64(samples); Bm1 = np.float64(passes - 1)
    with np.errstate(all="ignore"):
        ssb = Q - (S * S) / Nd
        ssb = np.where(ssb > 0.0, ssb, 0.0)
        return (ssb / Bm1) / Nd


def numpy_pack_v(var):
    """(B): one scalar per pixel."""
    with np.errstate(all="ignore"):
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        return np.where((v > 0.0) & finite(v), v, 0.0)


def numpy_prefilter(v, key):
    """(C)"""
    H, W = v.shape
    acc = np.zeros((H, W)); wsum = np.zeros((H, W))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            taken = ~(key[Q] != key[P])
            k = np.float64(B_3[dy + 1]) * np.float64(B_3[dx + 1])
            acc[P] = np.where(taken, acc[P] + k * v[Q], acc[P])
            wsum[P] = np.where(taken, wsum[P] + k, wsum[P])
    return acc / wsum


def numpy_denoise_variance(rgb_sum, samples, var, hits, iterations, sigma, flags):
    """The specification, restated -> (the filtered sums (H, W, 3), the filtered variance (H, W))."""
    H, W, _ = rgb_sum.shape
    with np.errstate(all="ignore"):
        c = rgb_sum / np.float64(samples)
        n, x = hits[..., 5:8], hits[..., 2:5]
        inv_t = 1.0 / hits[..., 1]
        key = np.where(hits[..., 0] != 0.0, hits[..., 11] + 2.0 if flags & 1 else 1.0, 0.0)
        guided = key != 0.0
        v = numpy_prefilter(numpy_pack_v(var), key)
        kv = np.float64(sigma[0]) * np.float64(sigma[0])
        in_, ip = (1.0 / (np.float64(s) * np.float64(s)) for s in sigma[1:])
        for i in range(iterations):
            s = 1 << i
            acc = np.zeros((H, W, 3)); vacc = np.zeros((H, W)); wsum = np.zeros((H, W))
            cp_finite = np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2])
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue                                                   # outside the frame for every pixel
                    P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    cq, cp, vq, vp = c[Q], c[P], v[Q], v[P]
                    taken = ~(key[Q] != key[P]) & np.isfinite(cq[..., 0]) & np.isfinite(cq[..., 1]) & np.isfinite(cq[..., 2])
                    k = np.float64(H_B3[dy + 2]) * np.float64(H_B3[dx + 2])
                    e = cq - cp
                    d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                    den = kv * ((vp + vq) + EPS)
                    wc = np.where(cp_finite[P], _stop(1.0 - d / den), 1.0)
                    m = n[Q] - n[P]
                    d = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
                    wn = np.where(guided[P], _stop(1.0 - d * in_), 1.0)
                    r = x[Q] - x[P]
                    npp = n[P]
                    g = ((npp[..., 0] * r[..., 0] + npp[..., 1] * r[..., 1]) + npp[..., 2] * r[..., 2]) * inv_t[P]
                    wp = np.where(guided[P], _stop(1.0 - (g * g) * ip), 1.0)
                    w = ((k * wc) * wn) * wp
                    acc[P] = np.where(taken[..., None], acc[P] + w[..., None] * cq, acc[P])
                    vacc[P] = np.where(taken, vacc[P] + (w * w) * vq, vacc[P])
                    wsum[P] = np.where(taken, wsum[P] + w, wsum[P])
            any_ = wsum > 0.0
            c = np.where(any_[..., None], acc / wsum[..., None], c)
            v = np.where(any_, vacc / (wsum * wsum), v)
        return c * np.float64(samples), v


@functools.lru_cache(maxsize=None)
def reference(shape):
    """{(iterations, sigma, flags): (sums, variance)} of the restatement for every setting of a shape: computed once, shared by the host
    and the GPU tests, read-only."""
    rgb, var, hits = case(shape)
    out = {}
    for k, sg, fl in settings_for(shape):
        c, v = numpy_denoise_variance(rgb, SAMPLES, var, hits, k, sg, fl)
        c.setflags(write=False); v.setflags(write=False)
        out[(k, sg, fl)] = (c, v)
    return out


# ---- the quality check: Cornell box 40 x 40, depth 20; 4 passes of 4 samples — the 16 samples of seed 7, pass b being an ordinary frame
# under the folded seed of DESIGN §11 — against 2048 samples of seed 99
Q_PASSES = (4, 4, 4, 4)
Q_PLAIN_SIGMA = DC.Q_SIGMA
Q_SIGMA_VS = (1.0, 2.0, 3.0, 4.0)
Q_ITERATIONS = (2, 3)


def pass_seed(seed, base):
    """The seed under which samples [base, base + n) of `seed` are samples [0, n) (the seed fold)."""
    return (seed + 2 * base * G) % (1 << 64)

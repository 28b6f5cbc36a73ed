"""What tests/test_denoise_host.py and tests/test_denoise_gpu.py share: the NumPy restatement of the denoiser's specification
(csrc/rt_denoise.h, include/rt_amd.h), the input frames both compare on, and the quality metric.

The restatement is written from the specification, not from the C++: elementwise NumPy operations only, one IEEE operation each, dot
products spelled out in the specification's order (no np.dot, no np.sum over channels), taps added in the specification's order."""
import ctypes as C
import functools

import numpy as np

INF = float("inf")
# (H, W): one pixel; smaller than the halo of every dilation; a single row; no multiple of any tile; more than two 64 x 4 tiles on both axes
# even where the taps are 2 * 16 = 32 pixels away
SHAPES = ((1, 1), (3, 5), (1, 40), (23, 37), (67, 130))
# sigma = (colour, normal, plane): finite values that leave some taps of the random frames in and cut others; every stop off; a mix
SIGMAS = ((0.7, 1.2, 1.0), (INF, INF, INF), (INF, 1.2, INF))
FLAGS = (0, 1)
SAMPLES = 5
H_B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def iterations_for(shape):
    return (1, 2, 3, 4, 5, 8) if shape == (3, 5) else (1, 2, 3, 4, 5)


def settings_for(shape):
    """Every (iterations, sigma, flags) a shape is checked with."""
    return [(k, sg, fl) for k in iterations_for(shape) for sg in SIGMAS for fl in FLAGS]


@functools.lru_cache(maxsize=None)
def case(shape):
    """(rgb_sum (H, W, 3), hits (H, W, 16)) of SAMPLES samples per pixel: random colours, ~30 % misses, random unit normals and positions,
    materials 0 .. 2 and some -1 (a medium's hit), and — in every frame of more than one pixel — a few NaN, +inf and -inf colour channels."""
    H, W = shape
    rs = np.random.RandomState(7000 + 131 * H + W)
    rgb = rs.uniform(0.0, 1.0, (H, W, 3)) * SAMPLES
    hits = np.zeros((H, W, 16))
    hit = rs.uniform(size=(H, W)) > 0.3
    n = rs.normal(size=(H, W, 3))
    n /= np.sqrt((n * n).sum(axis=2, keepdims=True))
    mat = rs.randint(0, 3, (H, W)).astype(np.float64)
    mat[rs.uniform(size=(H, W)) < 0.1] = -1.0
    hits[..., 0] = 1.0
    hits[..., 1] = rs.uniform(0.5, 3.0, (H, W))
    hits[..., 2:5] = rs.uniform(-1.0, 1.0, (H, W, 3))
    hits[..., 5:8] = n
    hits[..., 8] = 1.0
    hits[..., 11] = mat
    hits[..., 12] = 3.0
    hits[~hit] = 0.0
    hits[~hit, 11:15] = -1.0                       # a miss as rt_query_camera writes it
    if H * W > 1:
        flat = rgb.reshape(-1)
        where = rs.choice(flat.size, size=min(6, max(3, flat.size // 40)), replace=False)
        for k, i in enumerate(where):
            flat[i] = (np.nan, INF, -INF)[k % 3]
    rgb.setflags(write=False); hits.setflags(write=False)
    return rgb, hits


def _stop(t):
    return np.where(t > 0.0, t * t, 0.0)


def numpy_denoise(rgb_sum, samples, hits, iterations, sigma, flags):
    """The specification, restated."""
    H, W, _ = rgb_sum.shape
    with np.errstate(all="ignore"):
        c = rgb_sum / np.float64(samples)
        n, x = hits[..., 5:8], hits[..., 2:5]
        inv_t = 1.0 / hits[..., 1]
        key = np.where(hits[..., 0] != 0.0, hits[..., 11] + 2.0 if flags & 1 else 1.0, 0.0)
        guided = key != 0.0
        ic, in_, ip = (1.0 / (np.float64(s) * np.float64(s)) for s in sigma)
        for i in range(iterations):
            s = 1 << i
            ic_i = ic * np.float64(4 ** i)
            acc = np.zeros((H, W, 3)); wsum = np.zeros((H, W))
            cp_finite = np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2])
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue                                                   # outside the frame for every pixel
                    P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    cq, cp = c[Q], c[P]
                    taken = ~(key[Q] != key[P]) & np.isfinite(cq[..., 0]) & np.isfinite(cq[..., 1]) & np.isfinite(cq[..., 2])
                    k = np.float64(H_B3[dy + 2]) * np.float64(H_B3[dx + 2])
                    e = cq - cp
                    d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                    wc = np.where(cp_finite[P], _stop(1.0 - d * ic_i), 1.0)
                    m = n[Q] - n[P]
                    d = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
                    wn = np.where(guided[P], _stop(1.0 - d * in_), 1.0)
                    r = x[Q] - x[P]
                    npp = n[P]
                    g = ((npp[..., 0] * r[..., 0] + npp[..., 1] * r[..., 1]) + npp[..., 2] * r[..., 2]) * inv_t[P]
                    wp = np.where(guided[P], _stop(1.0 - (g * g) * ip), 1.0)
                    w = ((k * wc) * wn) * wp
                    acc[P] = np.where(taken[..., None], acc[P] + w[..., None] * cq, acc[P])
                    wsum[P] = np.where(taken, wsum[P] + w, wsum[P])
            c = np.where((wsum > 0.0)[..., None], acc / wsum[..., None], c)
        return c * np.float64(samples)


def differing_words(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape
    return int((a.view(np.uint64) != b.view(np.uint64)).sum())


def sigma3(sigma):
    return (C.c_double * 3)(*[float(s) for s in sigma])


# ---- the quality check of the issue: Cornell box 40 x 40, depth 20, 16 samples (seed 7) against 2048 samples (seed 99)
Q_W = Q_H = 40
Q_DEPTH, Q_SPP, Q_SEED, Q_TRUTH_SPP, Q_TRUTH_SEED = 20, 16, 7, 2048, 99
Q_ITERATIONS, Q_SIGMA, Q_BOUND = 3, (4.0, 0.5, 0.02), 0.5


def clipped_mse(rgb_sum, spp, truth_sum, truth_spp):
    """The mean over pixels and channels of (clip(mean, 0, 1) - clip(truth, 0, 1))^2."""
    a = np.clip(rgb_sum / spp, 0.0, 1.0); b = np.clip(truth_sum / truth_spp, 0.0, 1.0)
    return float(np.mean((a - b) ** 2))

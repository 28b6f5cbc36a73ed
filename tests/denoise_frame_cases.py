"""What tests/test_denoise_frame_host.py and tests/test_denoise_frame_gpu.py share: the NumPy restatement of csrc/rt_denoise_frame.h — the
variance frame of a frame with per-pixel counts (E) and the frame denoise (F) around the restated filters of tests/denoise_cases.py and
tests/denoise_variance_cases.py — the per-pixel counts the colour, variance and albedo frames of those files are compared under, and the
eight combinations of {counts, variance, albedo}.

The restatement is written from the specification: elementwise NumPy operations only, one IEEE operation each, in the specification's
order; comparisons with a NaN are false, as in C."""
import functools
import itertools

import numpy as np

import adaptive_cases as AC
import albedo_cases as ALC
import denoise_cases as DC
import denoise_variance_cases as VC
from denoise_cases import INF, differing_words, sigma3  # noqa: F401  (re-exported for the two test files)

SHAPES = DC.SHAPES
VARIANCE_SHAPES = ((1, 1), (11, 15), (3, 64), (67, 130))        # (E): a pixel; odd counts of doubles; more than one workgroup's pairs
SAMPLES = DC.SAMPLES                                            # the frame's one count where there are no per-pixel counts
ALBEDO_SAMPLES = 5
EPS = np.float64(2.0 ** -8)
# (counts, variance, albedo)
COMBOS = tuple(itertools.product((False, True), repeat=3))


def combo_id(combo):
    return "+".join(name for name, on in zip(("counts", "variance", "albedo"), combo) if on) or "plain"


def settings_for(shape, variance):
    """The (iterations, sigma, flags) of denoise_cases / denoise_variance_cases (sigma[0] is a colour stop or a variance stop); on the
    largest shape every third of them, which still holds every K, every sigma and both flags."""
    all_ = VC.settings_for(shape) if variance else DC.settings_for(shape)
    return all_[::3] + all_[1:2] if shape == (67, 130) else all_


@functools.lru_cache(maxsize=None)
def counts_case(shape):
    """(n, b): per-pixel sample counts 2 .. 9 and pass counts 2 .. n, and in every frame of more than one pixel pixels with n = 0 (b = 0),
    n = 1 (b = 1) and n = 7 with b = 0, 1 (a pixel of a loaded checkpoint)."""
    H, W = shape
    rs = np.random.RandomState(6000 + 131 * H + W)
    n = rs.randint(2, 10, (H, W)).astype(np.uint32)
    b = (2 + rs.randint(0, 8, (H, W)) % (n - 1)).astype(np.uint32)
    if H * W > 1:
        fn, fb = n.reshape(-1), b.reshape(-1)
        where = rs.choice(fn.size, size=min(fn.size, max(4, fn.size // 25)), replace=False)
        for k, i in enumerate(where):
            fn[i], fb[i] = ((0, 0), (1, 1), (7, 0), (7, 1))[k % 4]
    assert (b <= n).all()
    n.setflags(write=False); b.setflags(write=False)
    return n, b


def frames(shape, combo):
    """(rgb_sum, counts or None, var or None, albedo_sum or None, hits) of a combination."""
    counts, variance, albedo = combo
    rgb, var, hits = VC.case(shape)
    return rgb, counts_case(shape)[0] if counts else None, var if variance else None, ALC.albedo_case(shape, ALBEDO_SAMPLES) if albedo else None, hits


# ---------------------------------------------------------------- the restatement
def numpy_adaptive_variance(S, Q, n, b):
    """(E): the variance of the mean per pixel and channel from the pixel's own n and b; +inf where b < 2."""
    two = b >= 2
    Nd = n.astype(np.float64)[..., None]
    Bm1 = np.where(two, b.astype(np.int64) - 1, 1).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        ss = S * S
        ssb = Q - ss / Nd
        ssb = np.where(ssb > 0.0, ssb, 0.0)
        V = (ssb / Bm1) / Nd
    return np.where(two[..., None], V, INF)


def numpy_denoise_frame(rgb_sum, counts, samples, var, albedo_sum, albedo_samples, hits, iterations, sigma, flags):
    """(F) -> (the filtered sums (H, W, 3), the filtered variance (H, W) or None)."""
    with np.errstate(all="ignore"):
        N = np.full(rgb_sum.shape, np.float64(samples)) if counts is None else np.repeat(counts.astype(np.float64)[..., None], 3, axis=2)
        if albedo_sum is None:
            m = d = np.ones(rgb_sum.shape)
        else:
            a = albedo_sum / np.float64(albedo_samples)
            m = np.where(a - a == 0.0, a, 1.0)
            d = np.where(m >= EPS, m, EPS)
        x = rgb_sum / d
        c = x / N
        if var is None:
            y, v = DC.numpy_denoise(c, 1, hits, iterations, sigma, flags), None
        else:
            Vd = var if albedo_sum is None else (var / d) / d
            y, v = VC.numpy_denoise_variance(c, 1, Vd, hits, iterations, sigma, flags)
        s = np.where(N > 0.0, y * N, 0.0)
        return s * m, v


@functools.lru_cache(maxsize=None)
def reference(shape, combo):
    """{(iterations, sigma, flags): (sums, variance or None)} of the restatement for every setting of a shape and a combination: computed
    once, shared by the host and the GPU tests, read-only."""
    rgb, n, var, alb, hits = frames(shape, combo)
    out = {}
    for k, sg, fl in settings_for(shape, combo[1]):
        c, v = numpy_denoise_frame(rgb, n, SAMPLES, var, alb, ALBEDO_SAMPLES, hits, k, sg, fl)
        c.setflags(write=False)
        if v is not None:
            v.setflags(write=False)
        out[(k, sg, fl)] = (c, v)
    return out


@functools.lru_cache(maxsize=None)
def variance_state(shape):
    """(S, Q, n, b) for (E): adaptive_cases.state — non-finite sums and moments, counts from {32 .. 1000}, pixels with b = 0 and b = 1."""
    return AC.state(shape)

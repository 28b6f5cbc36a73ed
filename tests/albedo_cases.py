"""What tests/test_denoise_albedo_host.py and tests/test_denoise_albedo_gpu.py share: the NumPy restatement of albedo-demodulated
denoising's specification (csrc/rt_albedo.h (2), include/rt_amd.h) around denoise_cases.numpy_denoise, and the albedo frames both compare on.

The restatement is written from the specification: six lines, elementwise NumPy operations only, one IEEE operation each."""
import functools

import numpy as np

import denoise_cases as DC

INF = float("inf")
EPS = 2.0 ** -8
ALBEDO_SAMPLES = (1, 5)


@functools.lru_cache(maxsize=None)
def albedo_case(shape, albedo_samples):
    """An albedo SUM frame (H, W, 3) of `albedo_samples` samples per pixel for DC.case(shape): means in [0, 1.25) — so some are >= 1 —, and in
    every frame of more than a few channels exact zeros, means below eps, and NaN, +inf and -inf channels."""
    H, W = shape
    rs = np.random.RandomState(9000 + 131 * H + W + albedo_samples)
    a = rs.uniform(0.0, 1.25, (H, W, 3)) * albedo_samples
    flat = a.reshape(-1)
    if flat.size >= 3:
        special = (0.0, 0.5 * EPS * albedo_samples, np.nan, INF, -INF, 0.0, 0.999 * EPS * albedo_samples, EPS * albedo_samples, 1.0 * albedo_samples)
        where = rs.choice(flat.size, size=min(flat.size, max(3, min(len(special) * 4, flat.size // 12))), replace=False)
        for k, i in enumerate(where):
            flat[i] = special[k % len(special)] if flat.size >= len(special) else special[k]
    a.setflags(write=False)
    return a


def numpy_denoise_albedo(rgb_sum, samples, albedo_sum, albedo_samples, hits, iterations, sigma, flags):
    """The specification, restated."""
    with np.errstate(all="ignore"):
        a = albedo_sum / np.float64(albedo_samples)
        m = np.where(a - a == 0.0, a, 1.0)
        d = np.where(m >= EPS, m, EPS)
        x = rgb_sum / d
        y = DC.numpy_denoise(x, samples, hits, iterations, sigma, flags)
        return y * m

"""Pure-numpy statistics for the tests of the RT_F32 variant (test_f32_variant_gpu.py, test_f32_stats_host.py): the settled-pixel rule
of the identity-colour scenes and the calibrated comparison of means of two per-sample arrays.  No GPU, no library: plain arrays in,
plain arrays out, so that the statistic itself is tested on the CPU."""
import numpy as np

Z_FRAME = 5.0          # |z| of the whole-frame mean, per channel
Z_BLOCK = 5.5          # max |z| over blocks x channels: at most 200 values under a normal law exceed it with P < 200 * 3.8e-8 < 1e-5
F32_EPS = 2.0 ** -23   # spacing of f32 at 1: a value that has no variance on either side may differ by its f32 rounding only


# ------------------------------------------------------------------ identity-colour scenes
def pixel_labels(samples, palette):
    """samples (H, W, spp, 3), palette (K, 3) -> (H, W) int: k where EVERY sample of the pixel is exactly palette[k], -1 elsewhere
    (mixed pixels, or a colour that is not in the palette)."""
    s = np.asarray(samples)
    lab = np.full(s.shape[:2], -1, dtype=np.int64)
    for k, c in enumerate(np.asarray(palette, dtype=s.dtype)):
        lab[(s == c).all(axis=(-1, -2))] = k
    return lab


def settled_mask(labels):
    """(H, W) labels -> bool mask: a pixel is settled when its own label is >= 0 and each of its (up to 8) neighbours inside the frame
    carries the same label.  The neighbours are the guard band: a camera ray of the other precision lands inside the same pixel's
    footprint up to rounding, never a whole pixel away."""
    lab = np.asarray(labels)
    H, W = lab.shape
    ok = lab >= 0
    pad = np.pad(lab, 1, mode="edge")          # a neighbour outside the frame repeats the border pixel: no constraint of its own
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            ok &= pad[dy:dy + H, dx:dx + W] == lab
    return ok


def settled_counts(labels, n_labels):
    """-> (settled mask, settled pixels per label)."""
    m = settled_mask(labels)
    return m, np.bincount(np.asarray(labels)[m], minlength=n_labels)


# ------------------------------------------------------------------ means of two per-sample arrays
def _finite(samples):
    """Non-finite samples (the reference's 0/0 cases) count as 0, as format_color prints them."""
    s = np.asarray(samples, dtype=np.float64)
    bad = ~np.isfinite(s).all(axis=-1)
    if bad.any():
        s = np.where(bad[..., None], 0.0, s)
    return s, int(bad.sum())


def moments(samples):
    """(H, W, spp, 3) -> what a comparison needs of every pixel: n, the mean and the sum of squared deviations from it (M2), per
    channel and (index 3) of the channel sum, and the number of non-finite samples.  Computed about the pixel's first sample, so that
    a pixel whose samples are all one value has M2 = 0 exactly (sum x^2 - n mean^2 would leave its rounding behind, and a block of
    such pixels must be recognised as having no variance).  Moments of several renders of one view under different seeds combine
    (add_moments): a scene that needs more samples than one per-sample array should hold is rendered in batches."""
    s, bad = _finite(samples)
    s = np.concatenate([s, s.sum(axis=-1, keepdims=True)], axis=-1)
    n = s.shape[2]
    pivot = s[:, :, 0, :]
    d = s - pivot[:, :, None, :]
    d1 = d.sum(axis=2)
    m2 = np.maximum((d * d).sum(axis=2) - d1 * d1 / n, 0.0)
    return {"n": n, "mean": pivot + d1 / n, "m2": m2, "nonfinite": bad}


def add_moments(a, b):
    """The pairwise update of Chan, Golub and LeVeque."""
    n = a["n"] + b["n"]
    delta = b["mean"] - a["mean"]
    return {"n": n, "mean": a["mean"] + delta * (b["n"] / n), "m2": a["m2"] + b["m2"] + delta * delta * (a["n"] * b["n"] / n),
            "nonfinite": a["nonfinite"] + b["nonfinite"]}


def _pixel_moments(m):
    """-> per-pixel mean and the variance OF that mean, s_p^2 / n (unbiased s_p^2; 0 at n = 1)."""
    n = m["n"]
    if n == 1:
        return m["mean"], np.zeros_like(m["mean"])
    return m["mean"], m["m2"] / (n - 1) / n


def _block_edges(n, g):
    return [(k * n) // g for k in range(g + 1)]


def _z(diff, se, scale):
    """diff / se; where neither side has any variance the two means must agree up to the f32 rounding of the value itself."""
    z = np.zeros_like(diff)
    pos = se > 0.0
    z[pos] = diff[pos] / se[pos]
    flat = ~pos & (np.abs(diff) > F32_EPS * scale)
    z[flat] = np.inf * np.sign(diff[flat])
    return z


def compare_moments(a, b, grid=4):
    """a, b: moments() of two renders of one view.  For the whole frame and a grid x grid partition into blocks, per channel:
    (mean a - mean b) / se with se^2 = sum_p s_p^2 / spp / n_px^2 per side, both sides added — the standard error of a mean of n_px
    independent pixel means.  Also the relative standard error of the whole-frame mean over all channels: the se of the DIFFERENCE
    of the two frame means (from the per-pixel variances of the channel sum, so that the channels' covariance is in it) over their
    common mean — what a bias has to beat, and what the power condition bounds.
    Returns a dict: z_frame (3,), z_blocks (grid, grid, 3), rel_se_frame, mean_a, mean_b (3,), nonfinite_a, nonfinite_b."""
    assert a["mean"].shape == b["mean"].shape
    H, W = a["mean"].shape[:2]
    ma, va = _pixel_moments(a)
    mb, vb = _pixel_moments(b)

    def one(sl, n):
        d = ma[sl].mean(axis=(0, 1)) - mb[sl].mean(axis=(0, 1))
        e = np.sqrt((va[sl].sum(axis=(0, 1)) + vb[sl].sum(axis=(0, 1))) / n ** 2)
        return d, e, _z(d, e, np.maximum(np.abs(ma[sl]).mean(axis=(0, 1)), np.abs(mb[sl]).mean(axis=(0, 1))))

    _, se, zf = one((slice(0, H), slice(0, W)), H * W)
    ys, xs = _block_edges(H, grid), _block_edges(W, grid)
    zb = np.zeros((grid, grid, 3))
    for i in range(grid):
        for j in range(grid):
            zb[i, j] = one((slice(ys[i], ys[i + 1]), slice(xs[j], xs[j + 1])), (ys[i + 1] - ys[i]) * (xs[j + 1] - xs[j]))[2][:3]
    mean_t = 0.5 * (ma[..., 3].mean() + mb[..., 3].mean())
    return {"z_frame": zf[:3], "z_blocks": zb, "rel_se_frame": float(se[3] / mean_t) if mean_t != 0.0 else float("inf"),
            "mean_a": ma[..., :3].mean(axis=(0, 1)), "mean_b": mb[..., :3].mean(axis=(0, 1)),
            "nonfinite_a": a["nonfinite"], "nonfinite_b": b["nonfinite"]}


def compare_means(a, b, grid=4):
    """compare_moments of two per-sample arrays (H, W, spp, 3) of the same view (spp may differ)."""
    return compare_moments(moments(a), moments(b), grid)


def within_bounds(r):
    """The two bounds every comparison is held to (module constants)."""
    return bool(np.abs(r["z_frame"]).max() <= Z_FRAME and np.abs(r["z_blocks"]).max() <= Z_BLOCK)


def describe(r):
    return (f"frame z {np.array2string(r['z_frame'], precision=2)}, max |block z| {np.abs(r['z_blocks']).max():.2f}, "
            f"5 x rel se {5.0 * r['rel_se_frame']:.4f}, non-finite {r['nonfinite_a']} / {r['nonfinite_b']}")

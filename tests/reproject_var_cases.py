"""Temporal variance (csrc/rt_reproject_var.h) restated in NumPy, and the variance frames the host and GPU tests feed it.

numpy_reproject_variance and numpy_blend_variance are the specification, not the code under test: vectorised over the pixels, every
operation one rounded NumPy operation in the order the header writes it.  (R1)-(R5) are restated as tests/reproject_cases.py restates them —
that file's function keeps its taps to itself — and the tests hold the sums and counts of this restatement to that one word for word.

A variance is KNOWN when v - v == 0 and v >= 0; everything else is unknown and is written as +inf."""
import numpy as np

from reproject_cases import INF, camera_fields, dot, finite


def known(v):
    with np.errstate(all="ignore"):
        return (v - v == 0.0) & (v >= 0.0)


def numpy_reproject_variance(prev_sum, prev_counts, prev_samples, prev_var, prev_hits, prev_cam, cur_hits, max_history, sigma, info=None):
    """-> (hist_sum (H, W, 3), hist_counts (H, W) uint32, hist_var (H, W, 3)).  info: a dict that receives "wsum" and "wv" (the weights of the
    taps that pass (R4), and of those among them that are var-known) — for the tests' own assertions."""
    prev_sum = np.asarray(prev_sum, np.float64); prev_hits = np.asarray(prev_hits, np.float64); cur_hits = np.asarray(cur_hits, np.float64)
    prev_var = np.asarray(prev_var, np.float64)
    Hh, Ww = prev_sum.shape[:2]
    f = camera_fields(prev_cam)
    o, llc, h, v = f[0:3], f[3:6], f[6:9], f[9:12]
    normal_min, sigma_p = float(sigma[0]), float(sigma[1])
    with np.errstate(all="ignore"):
        # (R0)
        F = ((o - h / 2.0) - v / 2.0) - llc
        FF, hh, vv = dot(F, F), dot(h, h), dot(v, v)
        Wm, Hm = float(Ww - 1), float(Hh - 1)
        # (R1)
        c = cur_hits
        key = c[..., 12]
        ok = ~(c[..., 0] == 0.0) & (key >= 0.0)
        P, n = c[..., 2:5], c[..., 5:8]
        # (R2)
        d = P - o
        den = 0.0 - dot(d, F)
        ok &= den > 0.0
        tau = FF / den
        q = d * tau[..., None]
        s = dot(q, h) / hh + 0.5
        t = dot(q, v) / vv + 0.5
        x = s * Wm - 0.5
        y = t * Hm - 0.5
        ok &= (x > -1.0) & (x < float(Ww)) & (y > -1.0) & (y < float(Hh))
        # (R3)
        xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
        xf, yf = np.floor(xs), np.floor(ys)
        fx, fy = xs - xf, ys - yf
        dd, nn = dot(d, d), dot(n, n)
        lim = ((sigma_p * sigma_p) * dd) * nn
        nm = (normal_min * normal_min) * nn
        xi, yi = xf.astype(np.int64), yf.astype(np.int64)
        if prev_counts is None:
            Nall = np.full((Hh, Ww), float(int(prev_samples)))
        else:
            Nall = np.asarray(prev_counts, np.uint32).astype(np.float64)
        acc = np.zeros((Hh, Ww, 3)); wsum = np.zeros((Hh, Ww)); nacc = np.zeros((Hh, Ww))
        vacc = np.zeros((Hh, Ww, 3)); wv = np.zeros((Hh, Ww))
        # (R4) and (V)
        for b in (0, 1):
            for a in (0, 1):
                col, up = xi + a, yi + b
                take = ok & (col >= 0) & (col < Ww) & (up >= 0) & (up < Hh)
                wx = fx if a else 1.0 - fx
                wy = fy if b else 1.0 - fy
                w = wx * wy
                take &= w > 0.0
                row = Hh - 1 - up
                rc, cc = np.clip(row, 0, Hh - 1), np.clip(col, 0, Ww - 1)
                g = prev_hits[rc, cc]
                take &= ~(g[..., 0] == 0.0) & ~(g[..., 12] != key)
                Nq = Nall[rc, cc]
                take &= ~(Nq == 0.0)
                S = prev_sum[rc, cc]
                take &= finite(S[..., 0]) & finite(S[..., 1]) & finite(S[..., 2])
                m = g[..., 5:8]
                dn = dot(n, m)
                take &= (dn > 0.0) & (dn * dn >= nm * dot(m, m))
                e = P - g[..., 2:5]
                pe = dot(e, n)
                take &= pe * pe <= lim
                acc = np.where(take[..., None], acc + w[..., None] * (S / Nq[..., None]), acc)
                wsum = np.where(take, wsum + w, wsum)
                nacc = np.where(take, nacc + w * Nq, nacc)
                V = prev_var[rc, cc]
                takev = take & known(V[..., 0]) & known(V[..., 1]) & known(V[..., 2])
                vacc = np.where(takev[..., None], vacc + w[..., None] * (V * Nq[..., None]), vacc)
                wv = np.where(takev, wv + w, wv)
        # (R5) and the result of (V)
        has = wsum > 0.0
        mean = acc / wsum[..., None]
        cap = float(int(max_history))
        Nh = np.where(has, np.floor(np.where(nacc < cap, nacc, cap)), 0.0).astype(np.uint32)
        has &= Nh != 0
        Nd = Nh.astype(np.float64)
        hist_sum = np.where(has[..., None], mean * Nd[..., None], 0.0)
        hist_counts = np.where(has, Nh, 0).astype(np.uint32)
        hv = (vacc / wv[..., None]) / Nd[..., None]
        hist_var = np.where(has[..., None], np.where((wv > 0.0)[..., None], hv, INF), 0.0)
    if info is not None:
        info["wsum"] = np.where(has, wsum, 0.0); info["wv"] = np.where(has, wv, 0.0)
    return hist_sum, hist_counts, hist_var


BRANCHES = ("no history", "no samples", "both", "history only", "frame only", "neither")


def numpy_blend_variance(var, counts, samples, hist_var, hist_counts, info=None):
    """(BV) -> var_out (H, W, 3).  info receives "branch": per element the index into BRANCHES of the row of the table that gave it."""
    Vh = np.asarray(hist_var, np.float64)
    hn = np.asarray(hist_counts, np.uint32)
    V = np.full(Vh.shape, INF) if var is None else np.asarray(var, np.float64)
    if counts is None:
        N_int = np.full(hn.shape, int(samples), object)
        Nd = np.full(hn.shape, float(int(samples)))
    else:
        N_int = np.asarray(counts, np.uint32).astype(object)
        Nd = np.asarray(counts, np.uint32).astype(np.float64)
    n_zero = np.array(N_int == 0, bool)[..., None] & np.ones(Vh.shape, bool)
    h_zero = (hn == 0)[..., None] & np.ones(Vh.shape, bool)
    Nd = Nd[..., None]; hd = hn.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        T = Nd + hd
        kv, kh = known(V), known(Vh)
        both = ((Nd * Nd) * V + (hd * hd) * Vh) / (T * T)
        only_h = (Vh * hd) / T
        only_v = (V * Nd) / T
    out = np.full(Vh.shape, INF)
    branch = np.full(Vh.shape, 5)
    mixed = ~h_zero & ~n_zero
    for k, (mask, value) in enumerate(((h_zero, np.where(~n_zero & kv, V, INF)), (~h_zero & n_zero, np.where(kh, Vh, INF)), (mixed & kv & kh, both),
                                       (mixed & ~kv & kh, only_h), (mixed & kv & ~kh, only_v))):
        out = np.where(mask, value, out)
        branch = np.where(mask, k, branch)
    if info is not None:
        info["branch"] = branch
    return out


def variance_frame(seed, counts, hostile=True):
    """prev_var (H, W, 3) for a frame with these counts: per-sample variances in [0.01, 2) over the count (0 where the count is 0); with
    hostile entries at fixed strides: NaN, +inf, -inf, negative, -0.0, denormal and huge channels."""
    rs = np.random.RandomState(1000 + seed)
    n = np.asarray(counts, np.uint32).astype(np.float64)
    with np.errstate(all="ignore"):
        var = np.where(n[..., None] > 0.0, rs.uniform(0.01, 2.0, n.shape + (3,)) / n[..., None], 0.0)
    if hostile:
        f = var.reshape(-1, 3)
        f[2::23, 0] = np.nan; f[4::29, 1] = INF; f[6::31, 2] = -INF; f[8::37, 1] = -0.25; f[10::41] = -0.0; f[12::43, 0] = 5e-324; f[1::47, 2] = 1e300
    var.setflags(write=False)
    return var

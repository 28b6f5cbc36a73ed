"""The oracle's Sphere::hit, MovingSphere::hit and Triangle::hit against plain exact references, and that the hostile rays of
tests/primitive_cases.py reach what they aim at — no GPU.  tests/test_primitive_hits_gpu.py requires the device's records to equal the
oracle's bit for bit on every one of these rays; this file is what makes "equal to the oracle" mean something.

Spheres: the discriminant in fractions.Fraction from the f64 inputs, the roots with mpmath at 300 bits.  A case is CLEAR when
|D| >= 2^-30 |d|^2 (2 |oc|^2 + r^2) and both roots are at least 2^-30 (scale + t_min) from t_min, scale = (|oc| |d| + sqrt D) / |d|^2.  On
clear cases the oracle's decision is the exact one and |t - t_exact| <= 2^-32 scale: about 16 roundings of 2^-53, amplified by at most
2^30.  Triangles: Möller–Trumbore in Fractions; clear as primitive_cases.exact_triangle says; |t - t_exact| <= 2^-40 T.  At most 60 % of a
whole mix may be unclear, and at most 1 % of its control families (silhouette offsets of 1e-4 and more from origins a tenth of a radius
off the surface; Dirichlet interior points and points well outside a triangle).  Everything the GPU test relies on being present — far
roots, rejections one ulp below t_min, NaN hits, the seam and the poles — is counted here from the oracle's records alone."""
import functools

import mpmath
import numpy as np
import pytest

import primitive_cases as P
from oracle import orc
from raytracinginrust_amd import render as R

UNCLEAR_CAP, CONTROL_CAP = 0.60, 0.01


def _mat(name, pred):
    """the material handle of the one primitive of a scene whose (kind, description) satisfies pred"""
    ids = [m for m, (kind, what, _) in P.oracle_scene(name).things.items() if pred(kind, what)]
    assert len(ids) >= 1
    return ids


@pytest.mark.parametrize("name", P.SCENES)
def test_scene_builds_alike_on_both_backends_and_selects_its_query_kernel(pbe, name):
    """Both builders hand out the same material handles (the GPU test identifies primitives by them); the scene has 4096 rays or fewer;
    and the flattened scene selects the instantiation of rt_query.hip the table says — all three that can hold spheres and triangles
    are reached: the mesh one, the all-features one, the nested one."""
    S, O = P.build(name, pbe), P.oracle_scene(name)
    assert S.things.keys() == O.things.keys() and [v[0] for v in S.things.values()] == [v[0] for v in O.things.values()]
    assert len(P.rays_of(name)[0]) <= 4096
    counts = R.flatten(S.b)
    rows, n_top = R.debug_object_rows(S.b)
    n_constant = sum(1 for v in S.things.values() if not v[2]) + (2 if name == "medium" else 0)
    assert P.query_class(counts, len(rows), n_top, counts["textures"] == n_constant) == P.QUERY_CLASS[name]
    if name in P.BVH_SCENES:
        assert counts["bvh_nodes"] > 8
    assert set(P.QUERY_CLASS.values()) == {"mesh", "all", "nested"}


def _spheres_of(name):
    return [what for kind, what, _ in P.oracle_scene(name).things.values() if kind == "sphere"]


@functools.lru_cache(None)
def _sphere_set(name):
    """per ray of a stand-alone sphere set: (None | (clear, hit, t, scale)) over all the scene's spheres — hit if any is, the smallest t;
    clear if the ray is clear for every sphere"""
    rays = P.rays_of(name)[0]
    out = []
    for ray in rays:
        res = [P.exact_sphere(ray, c, r) for c, r in _spheres_of(name)]
        if any(x is None for x in res):
            out.append(None)
            continue
        hits = [x for x in res if x[1]]
        best = min(hits, key=lambda x: x[2]) if hits else None
        out.append((all(x[0] for x in res), best is not None, None if best is None else best[2], None if best is None else best[3]))
    return out


@pytest.mark.parametrize("name", P.SPHERE_SETS)
def test_oracle_sphere_hit_against_the_exact_reference(name):
    rays, fam, ctl, _ = P.rays_of(name)
    rec = P.oracle_hits(name)
    exact = _sphere_set(name)
    clear = np.array([x is not None and x[0] for x in exact])
    hit_o = rec[:, 0] != 0.0
    wrong = [k for k in np.flatnonzero(clear) if exact[k][1] != hit_o[k]]
    assert not wrong, f"{name}: {len(wrong)} clear decisions differ from the exact ones, first ray {wrong[0]} ({fam[wrong[0]]}): {rays[wrong[0]].tolist()}"
    worst = 0.0
    with mpmath.workprec(300):
        for k in np.flatnonzero(clear & hit_o):
            err = abs(mpmath.mpf(float(rec[k, 1])) - exact[k][2]) / exact[k][3]
            worst = max(worst, float(err))
    unclear_ctl = float((~clear[ctl]).mean())
    print(f"{name}: {len(rays)} rays, {1.0 - clear.mean():.1%} unclear, controls {int(ctl.sum())} with {unclear_ctl:.2%} unclear, "
          f"{int((clear & hit_o).sum())} clear hits, max |t - t_exact| = 2^{np.log2(worst) if worst > 0 else -np.inf:.1f} scale")
    assert worst <= 2.0 ** -32
    assert ctl.sum() >= 200 and unclear_ctl <= CONTROL_CAP


def test_sphere_mix_is_not_mostly_unclear():
    clear = np.concatenate([[x is not None and x[0] for x in _sphere_set(name)] for name in P.SPHERE_SETS])
    print(f"spheres: {len(clear)} rays, {1.0 - clear.mean():.1%} unclear")
    assert 1.0 - clear.mean() <= UNCLEAR_CAP


def _tris_of(name):
    return [what for kind, what, _ in P.oracle_scene(name).things.values() if kind == "tri"]


@functools.lru_cache(None)
def _tri_set(name):
    rays = P.rays_of(name)[0]
    out = []
    for ray in rays:
        res = [P.exact_triangle(ray, v) for v in _tris_of(name)]
        if any(x is None for x in res):
            out.append(None)
            continue
        hits = [x for x in res if x[0] and x[1]]
        best = min(hits, key=lambda x: x[2]) if hits else None
        out.append((all(x[0] for x in res), best is not None, None if best is None else best[2], None if best is None else best[3]))
    return out


@pytest.mark.parametrize("name", P.TRI_SETS)
def test_oracle_triangle_hit_against_the_exact_reference(name):
    rays, fam, ctl, _ = P.rays_of(name)
    rec = P.oracle_hits(name)
    exact = _tri_set(name)
    clear = np.array([x is not None and x[0] for x in exact])
    hit_o = rec[:, 0] != 0.0
    wrong = [k for k in np.flatnonzero(clear) if exact[k][1] != hit_o[k]]
    assert not wrong, f"{name}: {len(wrong)} clear decisions differ from the exact ones, first ray {wrong[0]} ({fam[wrong[0]]}): {rays[wrong[0]].tolist()}"
    worst = 0.0
    with mpmath.workprec(200):
        for k in np.flatnonzero(clear & hit_o):
            worst = max(worst, float(abs(mpmath.mpf(float(rec[k, 1])) - exact[k][2]) / exact[k][3]))
    unclear_ctl = float((~clear[ctl]).mean()) if ctl.any() else 0.0
    print(f"{name}: {len(rays)} rays, {1.0 - clear.mean():.1%} unclear, controls {int(ctl.sum())} with {unclear_ctl:.2%} unclear, "
          f"{int((clear & hit_o).sum())} clear hits, max |t - t_exact| = 2^{np.log2(worst) if worst > 0 else -np.inf:.1f} T")
    assert worst <= 2.0 ** -40
    if name != "tri_degenerate":                                     # (a degenerate triangle has det = 0: never clear, and has no control family)
        assert ctl.sum() >= 200 and unclear_ctl <= CONTROL_CAP


def test_triangle_mix_is_not_mostly_unclear():
    clear = np.concatenate([[x is not None and x[0] for x in _tri_set(name)] for name in P.TRI_SETS])
    print(f"triangles: {len(clear)} rays, {1.0 - clear.mean():.1%} unclear")
    assert 1.0 - clear.mean() <= UNCLEAR_CAP


# ---------------------------------------------------------------- non-vacuity, from the oracle's records alone
@pytest.mark.parametrize("name", list(P.SPHERES))
def test_sphere_sets_reach_the_far_root_and_both_sides_of_t_min(name):
    rays, fam, _, extra = P.rays_of(name)
    rec = P.oracle_hits(name)
    c, r = P.SPHERES[name]
    hit = rec[:, 0] != 0.0
    fin = np.isfinite(rays[:, :6]).all(axis=1)
    with np.errstate(all="ignore"):
        inside = fin & (np.sqrt(((rays[:, 0:3] - c) ** 2).sum(axis=1)) < 0.99 * r)
    assert (inside & hit).sum() >= 100                                # an origin inside the sphere: only the far root can be accepted
    # the restatement the generator aims with gives the oracle's own t wherever the oracle hits
    t0, t1, _ = P.sphere_roots(rays[:, 0:3], rays[:, 3:6], np.array(c), r)
    assert (P.same(rec[hit, 1], t0[hit]) | P.same(rec[hit, 1], t1[hit])).all()
    ks, far = extra["tmin"]
    tm = fam == "tmin"
    t, h = rec[tm, 1], hit[tm]
    at = h & (np.abs(P.ulps_from(t, P.T_MIN)) <= 2)                  # the record's t is the root next to t_min
    for k in (0, 1, 2):                                               # accepted: t IS t_min + k ulp
        sel = ks == k
        assert sel.sum() >= 20 and at[sel].all() and (P.ulps_from(t[sel], P.T_MIN) == k).all(), (name, k)
    for k in (-1, -2):                                                # rejected by `root < t_min`: a near root gives way to the far one, a far root to a miss
        sel = ks == k
        assert sel.sum() >= 20 and not at[sel].any(), (name, k)
        assert (~h[sel & far]).all() and h[sel & ~far].all()
    counts = {k: int((ks == k).sum()) for k in (-2, -1, 0, 1, 2)}
    print(f"{name}: far-root hits {int((inside & hit).sum())}; t_min cases by ulp {counts}, {int(far.sum())} of them on the far root")


def test_pythagorean_tangents_have_a_zero_discriminant():
    rays, fam, _, extra = P.rays_of("pyth")
    py = rays[fam == "pyth"]
    exact = extra["exact"]
    n_zero = 0
    for k in np.flatnonzero(exact):
        i = k // 120
        c, r = P.PYTH_SPHERES[i]
        _, _, disc = P.sphere_roots(py[k, 0:3], py[k, 3:6], np.array(c), r)
        n_zero += int(disc == 0.0)
    assert n_zero == exact.sum() >= 100
    rec = P.oracle_hits("pyth")[fam == "pyth"]
    assert (rec[exact, 0] != 0.0).all() and 0 < (rec[~exact, 0] != 0.0).sum() < (~exact).sum()      # D = 0 is a hit; an ulp decides the others


def test_degenerate_spheres_do_what_the_reference_does():
    """time0 == time1: 0 / 0 in center(), every ray a hit with t = NaN, in a list and in a BVH leaf; radius 0: a finite t with a NaN
    normal; a negative radius: hit in a list, missed in a BVH (its box is inverted)."""
    name = "degenerate_nan"
    rec = P.oracle_hits(name)
    assert (rec[:, 0] != 0.0).all()
    frozen = _mat(name, lambda kind, what: kind == "msphere" and what[2] == what[3])
    m = np.isin(rec[:, 11], frozen)
    assert m.sum() >= 300 and np.isnan(rec[m, 1]).all()
    print(f"degenerate_nan: {int(m.sum())} records are the frozen sphere's NaN hit, {int((~m).sum())} were replaced by a later item")
    assert (~m).sum() >= 300                                          # ... and the items behind it are entered with that NaN and answer
    rec = P.oracle_hits("degenerate")
    zero = np.isin(rec[:, 11], _mat("degenerate", lambda kind, what: kind == "sphere" and what[1] == 0.0))
    assert zero.sum() >= 50 and np.isfinite(rec[zero, 1]).all() and not np.isfinite(rec[zero, 5:8]).all(axis=1).any()     # (p - c) / 0: NaN, or inf where p missed c by an ulp
    n_zero_nan = int(np.isnan(rec[zero, 5:8]).any(axis=1).sum())
    assert n_zero_nan >= 50
    neg = np.isin(rec[:, 11], _mat("degenerate", lambda kind, what: kind == "sphere" and what[1] < 0.0))
    assert neg.sum() >= 100 and np.isfinite(rec[neg, 1:8]).all()
    still = np.isin(rec[:, 11], _mat("degenerate", lambda kind, what: kind == "msphere" and what[0] == what[1]))
    moving = np.isin(rec[:, 11], _mat("degenerate", lambda kind, what: kind == "msphere" and what[0] != what[1]))
    assert np.isnan(rec[still, 1]).sum() >= 50 and np.isfinite(rec[still, 1]).sum() >= 50      # (c0 == c1: 0 * inf at an infinite time)
    assert np.isfinite(rec[moving, 1]).sum() >= 100
    twins = _mat("degenerate", lambda kind, what: kind == "sphere" and what[1] == 1.25)
    assert len(twins) == 2 and np.isin(rec[:, 11], twins[1:]).sum() >= 100 and not np.isin(rec[:, 11], twins[:1]).any()    # the later twin wins the tie
    print(f"degenerate: radius 0 {int(zero.sum())} hits with a non-finite normal ({n_zero_nan} NaN), negative radius {int(neg.sum())} hits, later twin {int(np.isin(rec[:, 11], twins[1:]).sum())}")
    for bvh in ("bvh16", "bvh300", "nested"):
        rec = P.oracle_hits(bvh)
        assert not np.isin(rec[:, 11], _mat(bvh, lambda kind, what: kind == "sphere" and what[1] < 0.0)).any()
        fz = np.isin(rec[:, 11], _mat(bvh, lambda kind, what: kind == "msphere" and what[2] == what[3]))
        assert fz.sum() >= 100 and np.isnan(rec[fz, 1]).all()
        tw = _mat(bvh, lambda kind, what: kind == "sphere" and what[1] > 0.0 and sum(1 for k2, w2, _ in P.oracle_scene(bvh).things.values()
                                                                                       if k2 == "sphere" and w2 == what) == 2)
        assert len(tw) == 2 and np.isin(rec[:, 11], tw).sum() >= 50
        print(f"{bvh}: negative radius never hit, frozen sphere {int(fz.sum())} NaN hits, twins hit {[int((rec[:, 11] == t).sum()) for t in tw]}")
    # the same spheres of bvh16 in a list: the negative radius is hit (without the frozen sphere, whose NaN hit replaces whatever stands before it)
    S = P.Scene(orc.load())
    S.finish(P._push_spheres(S, [spec for k, spec in enumerate(P._bvh_spheres(16)) if k != 7]))
    rec = orc.hit_records(S.b, P.rays_of("bvh16")[0], P.SEED)
    neg = [m for m, (kind, what, _) in S.things.items() if kind == "sphere" and what[1] < 0.0]
    assert np.isin(rec[:, 11], neg).sum() >= 20


def test_triangle_sets_reach_nan_barycentrics_shared_edges_and_t_min():
    n_nan = 0
    for name in P.TRI_SETS:
        rec = P.oracle_hits(name)
        hit = rec[:, 0] != 0.0
        n_nan += int((hit & np.isnan(rec[:, 9:11]).any(axis=1)).sum())
    assert n_nan >= 100
    rays, fam, _, _ = P.rays_of("tri_pair")
    alone = []
    for v in P.TRI_PAIR:
        S = P.Scene(orc.load())
        S.finish([S.tri(v)])
        alone.append(orc.hit_records(S.b, rays, P.SEED)[:, 0] != 0.0)
    edgy = np.isin(fam, ["edge", "near_edge", "vertex"])
    both, neither = alone[0] & alone[1], edgy & ~alone[0] & ~alone[1]
    print(f"triangles: {n_nan} hits with NaN barycentrics; shared edge: {int(both.sum())} rays answered by both, {int(neither.sum())} edge rays by neither")
    assert both.sum() >= 30 and neither.sum() >= 30
    rec = P.oracle_hits("tri_alone")
    tm = P.rays_of("tri_alone")[1] == "tmin"
    t = rec[tm, 1]
    at = (rec[tm, 0] != 0.0) & (np.abs(P.ulps_from(t, P.T_MIN)) <= 2)
    assert at.sum() >= 30 and (~at).sum() >= 30 and set(P.ulps_from(t[at], P.T_MIN).tolist()) == {0, 1, 2}


def test_uv_family_reaches_both_sides_of_the_seam_and_both_poles():
    rays, fam, _, _ = P.rays_of("sphere_origin")
    rec = P.oracle_hits("sphere_origin")[fam == "uv"]
    assert (rec[:, 0] != 0.0).all()
    u, v = rec[:, 9], rec[:, 10]
    counts = {"u < 1e-3": int((u < 1e-3).sum()), "u > 1 - 1e-3": int((u > 1.0 - 1e-3).sum()), "u == 0": int((u == 0.0).sum()), "u == 1": int((u == 1.0).sum()),
              "v == 0": int((v == 0.0).sum()), "v == 1": int((v == 1.0).sum())}
    print("sphere_origin uv:", counts)
    assert all(c >= 10 for c in counts.values())

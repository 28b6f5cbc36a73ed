"""The NumPy restatement of ConstantMedium::hit and of the list walk around it (tests/medium_cases.py) against the oracle, and that the rays
of medium_cases reach what they aim at — no GPU.  tests/test_medium_gpu.py feeds the same restatement the DEVICE's log and requires the
device's records to equal it word for word; this file is what pins the restatement and the case generator.

With glibc's log (orc.libm: the log the oracle calls) the restatement's records equal world.hit of the oracle, ray k on Rng(SEED, k), on
every ray of every list scene at every t_min of T_MINS: 0 differing 64-bit words, any NaN matching any NaN.  The reach counts are taken
from the oracle's boundary hits and the restatement's own numbers alone.  Minimum counts: a family at least 50 rays of what it aims at in
every scene it is part of, and at least 10 on each side of the 0.0001 step among the rays aimed within 8 x 2^-50 of it.  Lower minimums,
for what only part of a family can reach: 20 rays with both boundary hits and len = 0 (a sphere's roots are NaN with d d = 0, and a BVH's
boxes let no NaN through: bvh_boundary is exempt), 20 grazing rays past the silhouette, 10 non-finite rays that draw, 10 records with a
NaN or infinite t where an opaque item can hand one on, 5 with t = -inf (negative density, len = 0, origin on a face: 1 ray in 10 of
one medium's dscale family).  len = inf with both boundary hits is printed, not asserted: a box's second hit is lost to the step at
|d| = 1e200 (t2 < t1 + 0.0001), only a sphere's NaN roots pass."""
import numpy as np
import pytest

import medium_cases as M
from oracle import orc
from raytracinginrust_amd import render as R

OVERLAPPING = M.OVERLAPPING
WITH_OPAQUE = ("opaque_before", "opaque_between", "opaque_after", "ball_between")


def _restated(name, t_min):
    return M.restate(name, t_min, M.glibc_log(len(M.rays_of(name)[0])))


@pytest.mark.parametrize("name", M.SCENES)
def test_scene_builds_alike_on_both_backends_and_selects_its_query_kernel(pbe, name):
    """Both builders hand out the same handles; 4096 rays or fewer; the flattened scene selects the instantiation of rt_query.hip the table
    says — "all" (object_hit's medium arm) and "nested" (object_hit_nested, boundary_hit) are both reached; in a list scene item i is
    top-level object i, a medium where the item is one (the object column of a record then names the item)."""
    S, O = M.Scene(name, pbe), M.oracle_scene(name)
    assert [it["h"] for it in S.items] == [it["h"] for it in O.items] and S.things == O.things
    assert len(M.rays_of(name)[0]) <= 4096
    counts = R.flatten(S.b)
    rows, n_top = R.debug_object_rows(S.b)
    assert M.query_class(counts, rows, n_top) == M.QUERY_CLASS[name]
    assert set(M.QUERY_CLASS.values()) == {"all", "nested"}
    n_media = sum(1 for it in S.items if it["spec"][0] == "medium")
    assert counts["media"] == n_media
    if name in M.LIST_SCENES:
        assert n_top == len(S.items)
        assert [int(m) >= 0 for m in rows[:n_top, 5].astype(np.int32)] == [it["spec"][0] == "medium" for it in S.items]
    else:
        assert counts["bvh_nodes"] > 8
    if name in ("union", "three_media_list"):
        assert len(rows) > n_top                                       # the boundary list became a run of sub-objects: boundary_hit
    if name in ("tetra", "slab"):
        assert len(rows) == n_top                                      # (bare primitives of one kind are one range object: object_hit's arm)


def test_every_density_and_wrapper_form_is_in_some_scene():
    dens = [it[4] for name in M.LIST_SCENES for it in M.SPECS[name] if it[0] == "medium"]
    assert all(any(d == x or (d != d and x != x) for d in dens) for x in M.DENSITIES)
    shapes = {it[1][0] for name in M.LIST_SCENES for it in M.SPECS[name] if it[0] == "medium"}
    assert shapes == {"sphere", "cube", "tetra", "slab", "rect", "msphere", "bvh", "union"}
    for k in M.WRAPS:
        assert M.SPECS["in_" + k][0][2] == M.WRAPS[k] and M.SPECS["in_" + k][0][3] == ()
        assert M.SPECS["out_" + k][0][3] == M.WRAPS[k] and M.SPECS["out_" + k][0][2] == ()
    assert set(M.STREAM_SCENES) <= set(M.LIST_SCENES) and len(M.STREAM_SCENES) == 6


@pytest.mark.parametrize("name", M.LIST_SCENES)
def test_restatement_equals_the_oracle_word_for_word(name):
    rays = M.rays_of(name)[0]
    for t_min in M.T_MINS:
        res = _restated(name, t_min)
        ref = M.oracle_world_hits(name, t_min)
        bad = ~M.same(res["rec"][:, 0:12], ref[:, 0:12]).all(axis=1)
        hit = ref[:, 0] != 0.0
        print(f"{name}, t_min {t_min}: {len(rays)} rays, {int(res['drew'].sum())} draws, {int(hit.sum())} hits ({int((hit & (ref[:, 11] < 0)).sum())} in a medium), "
              f"{int(bad.sum())} differ")
        assert not bad.any(), M.describe(name, bad, t_min)
        med = hit & (ref[:, 11] < 0.0)
        assert (ref[med, 9:11] == 0.0).all()


def test_hit_records_and_hit_batch_agree():
    """orc_hit_batch on the world handle with (1e-5, +inf) is orc_hit_records"""
    for name in ("three_media_list", "bvh_wrapped"):
        a = M.oracle_world_hits(name, 1e-5)
        b = orc.hit_records(M.oracle_scene(name).b, M.rays_of(name)[0], M.SEED)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # ... and on one ray orc_hit
    sc = M.oracle_scene("cube")
    rays = M.rays_of("cube")[0]
    batch = orc.hit_batch(sc.b, sc.items[0]["boundary"], rays[:50], -M.F64_MAX, M.F64_MAX)
    for k in range(50):
        one = orc.hit(sc.b, sc.items[0]["boundary"], rays[k, 0:3], rays[k, 3:6], rays[k, 6], -M.F64_MAX, M.F64_MAX)
        assert (one is None) == (batch[k, 0] == 0.0)
        if one is not None:
            assert M.same([one["t"]] + one["position"], batch[k, 1:5]).all()


# ---------------------------------------------------------------- reach
def _count(mask, fam=None, f=None):
    return int(mask.sum()) if f is None else int((mask & (fam == f)).sum())


@pytest.mark.parametrize("name", M.LIST_SCENES)
def test_families_reach_what_they_aim_at(name):
    rays, fam, aimed, width = M.rays_of(name)
    res = _restated(name, M.T_MINS[0])
    r = M.reach(res, M.T_MINS[0])
    late = M.reach(_restated(name, 0.75), 0.75)
    out = {k: _count(v) for k, v in r.items()}
    print(f"{name}: {len(rays)} rays {out}")
    if name == "rect":                                                  # one rect: never a second hit, never a draw, at any t_min
        assert out["drew"] == 0 and out["lost"] >= 500 and _count(late["drew"]) == 0
        assert not _restated(name, M.T_MINS[2])["drew"].any()
        I = res["info"][0]                                              # a second "hit": the first one again (|t1| >= 2^40 absorbs the step), or a NaN one
        assert (~r["found"] | np.isnan(I["t1"]) | (I["t2"] == I["t1"])).all() and out["found"] >= 50
        for f in ("through", "inside", "behind", "graze", "dscale", "nonfinite"):
            assert _count(r["lost"], fam, f) >= 50, f
        return
    with np.errstate(all="ignore"):
        dmax = np.abs(rays[:, 3:6]).max(axis=1)
    per = {"through": r["drew"], "inside": r["clamp_t_min"], "behind": r["found"] & ~r["drew"], "graze": r["drew"], "dscale": r["drew"], "thin": r["found"]}
    for f, m in per.items():
        assert _count(m, fam, f) >= 50, (f, _count(m, fam, f))
    assert _count(r["lost"] | ~r["found"], fam, "graze") >= 20             # ... and past the silhouette, or too thin to be seen
    assert (fam == "nonfinite").sum() >= 50 and _count(~r["drew"], fam, "nonfinite") >= 50 and _count(r["drew"], fam, "nonfinite") >= 10
    assert ((fam == "dscale") & (dmax > 1e199) & (dmax < 1e201)).sum() >= 50 and ((fam == "dscale") & (dmax < 1e-199) & (dmax > 0.0)).sum() >= 50
    assert out["len_zero"] >= 20 or name == "bvh_boundary"            # (d d = 0 makes a sphere's roots NaN; a BVH's boxes let no NaN through)
    # on each side of the 0.0001 step, among the rays aimed within 8 x 2^-50 of it; and far from it on either side
    # (found: a second hit at the aimed width; lost: none, or — a boundary of several surfaces — the next surface instead)
    near = np.abs(width - 1.0) <= 9.0 * 2.0 ** -50
    thin = np.flatnonzero(fam == "thin")
    found, lost = np.zeros(len(rays), bool), np.zeros(len(rays), bool)
    for k in thin:
        I = res["info"][int(aimed[k])]
        second = bool(I["has2"][k]) and I["t2"][k] - I["t1"][k] <= 1.5 * M.STEP * width[k]
        found[k], lost[k] = second, bool(I["has1"][k]) and not second
    print(f"{name}: thin: aimed within 8 x 2^-50 of the step {int(near.sum())}: second hit found {_count(near & found)}, lost {_count(near & lost)}; "
          f"far below: lost {_count((width <= 0.5) & lost)}, above: found {_count((width >= 2.0) & found)}")
    assert _count(near & lost) >= 10 and _count(near & found) >= 10
    assert _count((width <= 0.5) & lost) >= 10 and not ((width <= 0.5) & found).any() and _count((width >= 2.0) & found) >= 10
    if name in M.STEP_EXACT:
        # one ulp decides: t1 = 0, so the second query starts at 0.0001 itself and `t < t_min` rejects t2 = 0.0001 - 1 ulp and keeps 0.0001
        step = np.flatnonzero(fam == "step")
        I = [res["info"][int(aimed[k])] for k in step]
        has1 = np.array([bool(i["has1"][k]) and i["t1"][k] == 0.0 for i, k in zip(I, step)])
        has2 = np.array([bool(i["has2"][k]) for i, k in zip(I, step)])
        t2 = np.array([i["t2"][k] for i, k in zip(I, step)])
        kk = width[step]
        at = has2 & (M.P.ulps_from(np.where(has2, t2, M.STEP), M.STEP) == kk)
        print(f"{name}: step: {len(step)} rays from a face, t1 = 0 on {int(has1.sum())}; second hit at 0.0001 + k ulp found for k >= 0: {int(at[kk >= 0].sum())} of "
              f"{int((kk >= 0).sum())}, for k < 0: {int(at[kk < 0].sum())} of {int((kk < 0).sum())}")
        assert has1.all() and (kk >= 0).sum() >= 10 and (kk < 0).sum() >= 10
        assert at[kk >= 0].all() and not at[kk < 0].any()
    # draws and none; hits and misses among the draws; clamps at t_min (more of them at t_min = 0.75)
    for k in ("drew", "hit", "miss", "lost", "clamp_t_min"):
        assert out[k] >= 50, k
    assert _count(~r["drew"]) >= 50
    print(f"{name}: t_min 0.75: clamps {_count(late['clamp_t_min'])}, of them not at 1e-5 {_count(late['clamp_t_min'] & ~r['clamp_t_min'])}, draws at 1e-5 and none at 0.75 {_count(r['drew'] & ~late['drew'])}")
    assert _count(late["clamp_t_min"]) >= 50 and _count(r["drew"] & ~late["drew"]) >= 50


@pytest.mark.parametrize("name", OVERLAPPING + ("densities_a", "densities_b"))
def test_lists_reach_the_clamp_at_closest_and_both_draw_orders(name):
    """The closest hit so far cuts a later medium's chord (t2 > closest); a later medium draws after an earlier one did, and where the
    earlier one did not: the uniform it gets is then another one."""
    res = _restated(name, M.T_MINS[0])
    r = M.reach(res, M.T_MINS[0])
    media = sorted(res["info"])
    drew = res["drew"]
    first_then = drew[:, media[0]] & drew[:, media[1]]
    second_only = ~drew[:, media[0]] & drew[:, media[1]]
    shifted = sum(int((res["info"][i]["drew"] & (res["info"][i]["cursor"] > 0)).sum()) for i in media[1:])
    print(f"{name}: clamps at closest {int(r['clamp_closest'].sum())}, first medium then second {int(first_then.sum())}, second without the first {int(second_only.sum())}, "
          f"draws of a later medium with an advanced stream {shifted}, records with a NaN t {int(r['nan_t'].sum())}, infinite {int(r['inf_t'].sum())}")
    if name in OVERLAPPING:
        assert r["clamp_closest"].sum() >= 50 and first_then.sum() >= 50 and second_only.sum() >= 50 and shifted >= 50
    else:
        assert second_only.sum() >= 50                                  # (side by side: a ray rarely meets two)
    if name in WITH_OPAQUE:
        # the opaque item relative to the first medium's chord [t1, t2] (as the boundary gives them): in front, inside, behind
        sc = M.oracle_scene(name)
        k = [i for i, it in enumerate(sc.items) if it["spec"][0] != "medium"][0]
        I = res["info"][media[0]]
        o = orc.hit_batch(sc.b, sc.items[k]["h"], M.rays_of(name)[0], M.T_MINS[0], M.INF)
        both = I["has1"] & I["has2"] & (o[:, 0] != 0.0)
        with np.errstate(invalid="ignore"):
            front, cut, behind = both & (o[:, 1] < I["t1"]), both & (o[:, 1] > I["t1"]) & (o[:, 1] < I["t2"]), both & (o[:, 1] > I["t2"])
        print(f"{name}: the opaque item in front of t1 {int(front.sum())}, cutting the chord {int(cut.sum())}, behind t2 {int(behind.sum())}")
        assert cut.sum() >= 50 and (name == "ball_between" or (front.sum() >= 50 and behind.sum() >= 50))
        rec = res["rec"]
        assert ((rec[:, 0] != 0.0) & (rec[:, 11] >= 0.0)).sum() >= 50 and ((rec[:, 0] != 0.0) & (rec[:, 11] < 0.0)).sum() >= 50
        assert r["nan_t"].sum() + r["inf_t"].sum() >= 10                # an opaque item's NaN / inf hit: the media after it are entered with it
    if name == "densities_a":
        assert r["before_t1"].sum() >= 50 and r["inf_t"].sum() >= 5     # a negative density: t < t1, and -inf with len = 0


@pytest.mark.parametrize("name", M.OUTER_ROTATED)
def test_a_rotation_outside_the_medium_changes_the_length_of_d(name):
    """|d| of the world ray and of the ray the medium receives differ as words on more than 30 % of the rays: a kernel that took the
    length on the wrong side of the wrapper cannot pass the GPU test."""
    rays = M.rays_of(name)[0]
    spec = M.SPECS[name][0]
    _, d, _ = M.received(spec, rays)
    with np.errstate(all="ignore"):
        l0 = np.sqrt(rays[:, 3] * rays[:, 3] + rays[:, 4] * rays[:, 4] + rays[:, 5] * rays[:, 5])
        l1 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    differ = ~M.same(l0, l1)
    res = _restated(name, M.T_MINS[0])
    hits = res["info"][0]["hit"]
    print(f"{name}: |d| differs as a word on {differ.mean():.1%} of {len(rays)} rays, on {int((differ & hits).sum())} of {int(hits.sum())} medium hits")
    assert differ.mean() > 0.30 and (differ & hits).sum() >= 100
    if name.startswith("in_out"):
        return                                                          # (there the wrong length has two wrong sides: the test below)
    # ... and where it does, the record would differ: t and the position are made with it
    I = res["info"][0]
    with np.errstate(all="ignore"):
        t_wrong = I["t1c"] + I["hd"] / l0
    assert (~M.same(t_wrong, res["rec"][:, 1]) & hits).sum() >= 50


@pytest.mark.parametrize("name", M.BVH_SCENES)
def test_bvh_forms_have_medium_hits_and_name_their_uniform(name):
    """Every medium hit of the oracle in a BVH form is the restated arithmetic on ONE of the ray's first draws (which one depends on the
    order the tree visits the media in): the GPU test takes t1 and q = hit_distance / len from here."""
    q = M.bvh_medium_terms(name)
    ref = M.oracle_world_hits(name, M.T_MINS[0])
    med = (ref[:, 0] != 0.0) & (ref[:, 11] < 0.0)
    print(f"{name}: {len(ref)} rays, {int((ref[:, 0] != 0.0).sum())} hits, {int(med.sum())} in a medium, by medium {np.bincount(q['item'][med]).tolist()}")
    assert med.sum() >= 300 and q["known"][med].all() and ((ref[:, 0] != 0.0) & ~med).sum() >= 20
    assert (np.bincount(q["item"][med], minlength=3)[:3] >= 50).all()


@pytest.mark.parametrize("name,item", M.INNER_ROTATED_NESTED)
def test_a_rotation_inside_the_medium_changes_the_length_of_d_again(name, item):
    """F_NESTED scenes with a Rotate between the medium and its boundary: |d| of the ray the medium receives and of the ray its boundary
    receives differ as words on more than 30 % of the rays (and, in_out_*, so do the world ray's and the medium's: the test above) — len
    taken on either wrong side of med_at cannot pass the GPU test."""
    rays = M.rays_of(name)[0]
    spec = M.SPECS[name][item]
    o, d, _ = M.received(spec, rays)
    ob, db = o, d
    for op in spec[2]:
        ob, db = M.op_forward(op, ob, db)
    with np.errstate(all="ignore"):
        l1 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        l2 = np.sqrt(db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1] + db[:, 2] * db[:, 2])
    differ = ~M.same(l1, l2)
    res = _restated(name, M.T_MINS[0])
    I = res["info"][item]
    with np.errstate(all="ignore"):
        t_wrong = I["t1c"] + I["hd"] / l2
    shown = I["hit"] & ~M.same(t_wrong, res["rec"][:, 1])
    print(f"{name}: |d| of the medium's ray and of its boundary's differ as words on {differ.mean():.1%} of {len(rays)} rays; t made with the boundary's differs on "
          f"{int(shown.sum())} of {int(I['hit'].sum())} hits of the medium")
    assert differ.mean() > 0.30 and shown.sum() >= 50

"""The oracle's libm table and the loop that fills it (oracle.cpp orc_lm, tests/libm_replay.py), on the host: no GPU.

  * Filled with glibc's own values — what the oracle itself computed at each missing site — the replayed output equals the plain output,
    0 differing words, on every set tests/test_libm_replay_gpu.py runs, and the last round misses nothing: the hook changes nothing by
    itself.
  * With one op's values moved by 1 ulp, records whose lookups touched that op change and no other record changes a word: the table is
    what the oracle computes with, at every routed site.
  * The sets reach what they are meant to reach (counts of distinct table entries per op; the sphere-light family's populations)."""
import functools

import numpy as np
import pytest

import libm_replay as L
import shade_kat_cases as K
import texture_cases as T
from oracle import orc


@functools.lru_cache(None)
def _bounce(name):
    _, scene, lights, what = next(s for s in L.bounce_sets() if s[0] == name)
    ob, mats = K.make_scene(orc.load(), scene, lights)
    rec, rays = L.bounce_records(what, mats, lambda r: orc.hit_records(ob, r))
    return ob, rec, rays, what, mats


@functools.lru_cache(None)
def _textures():
    return T.build(orc.load())


def _runs():
    """every set of the GPU tests, by name -> run_oracle"""
    runs = {}
    for name, _, _, _ in L.bounce_sets():
        ob, rec, rays, what, _ = _bounce(name)
        runs["one bounce " + name] = L.run_bounce(ob, rec, rays, what)
    ob, tex, mats = _textures()
    for name, (t, u, v, p) in L.texture_sets().items():
        rec, rays = T.records(mats[t].id, u, v, p)
        runs["texture " + name] = L.run_texture(ob, rec, rays)
    for name in L.UV_SCENES:
        runs["u, v " + name] = L.run_hits(*L.uv_scene(name, orc.load()))
    for name in L.MEDIA_SCENES:
        runs["medium " + name] = L.run_hits(*L.media_scene(name, orc.load()))
    fb, fm = K.make_scene(orc.load(), "full", "none")
    runs["brdf"] = L.run_brdf(fb, [h.id for h in fm["pbr"]], *L.brdf_inputs())
    return runs


@functools.lru_cache(None)
def _glibc_replays():
    """name -> (plain output, replayed output, Counts) with the table filled from glibc"""
    out = {}
    for name, run in _runs().items():
        plain = run()
        got, counts = L.replay(run, L.glibc_of_site, label=name + " (glibc)", wants_glibc=True)
        out[name] = (plain, got, counts)
    return out


def test_filled_with_glibc_the_hook_changes_nothing():
    for name, (plain, got, counts) in _glibc_replays().items():
        n_bad = int((~L.same(got, plain)).sum())
        assert n_bad == 0, f"{name}: {n_bad} words differ from the plain oracle"
        assert all(d == 0 for _, d in counts.values()), name
        assert counts.rounds <= 2, name                                  # glibc's values are what the first run went on with: nothing new turns up
        assert all(l == m for l, m in counts.stats.values())
    assert orc.libm_stats()[1] == 0 and not orc.libm_misses()            # no table is left behind


def test_the_sets_reach_every_op():
    """Conditions on the inputs, from the oracle alone.  The sets made for an arm must reach its ops with hundreds of distinct operands:
    the synthetic PBR sets and the sphere-light family for the principled material's six, the synthetic Lambertian sets for sincos_0_2pi.
    (The "real" sets are rays into a room with two PBR objects; they reach the same ops with 31 - 96 operands and are not counted on.)"""
    R_ = _glibc_replays()
    pbr_ops = ("sincos_0_2pi", "sin", "cos", "tan", "atan", "pow")
    for name, (_, _, c) in R_.items():
        if not name.startswith("one bounce"):
            continue
        what = name.split()[-1]
        if name.startswith("one bounce hostile") or what == "pbr":
            for op in pbr_ops:
                assert c[op][0] >= 200, (name, op, c[op])
            a2 = sorted({(0.1 * (1.0 - p[9]) + 0.001 * p[9]) ** 2 for p, _ in K.pbr_sets()})
            assert sorted(c.operands["log2"][0].tolist()) == a2, name          # one entry per parameter set's constant, and no other
        elif what == "lam":
            assert c["sincos_0_2pi"][0] >= 200, (name, c["sincos_0_2pi"])
    for name in ("u, v sphere_origin", "u, v chain3"):
        c = R_[name][2]
        assert c["atan2"][0] >= 1000 and c["acos"][0] >= 1000, (name, dict(c))
    assert R_["texture checker"][2]["sin"][0] >= 1000
    for name in L.MEDIA_SCENES:
        assert R_["medium " + name][2]["log"][0] >= 200, name


def test_the_sphere_light_family_holds_what_it_is_meant_to():
    for name, _, lights, _ in L.HOSTILE_SETS:
        ob, rec, rays, what, mats = _bounce(name)
        _, _, fam = K.sphere_light_records(mats)
        ref = _glibc_replays()["one bounce " + name][0][0]
        c, rad = np.array(K.LIGHT_SPHERE[0]), K.LIGHT_SPHERE[1]
        d = np.sqrt(((rec[:, 2:5] - c) ** 2).sum(1)) / rad
        nan_dir = np.isnan(ref[:, 3:6]).any(axis=1)
        with np.errstate(divide="ignore"):
            n = {"inside": int((d < 1.0).sum()), "surface": int((np.abs(d - 1.0) <= 1e-12).sum()), "far": int((d > 1e6).sum()),
                 "so far that 1 - r^2 / d^2 rounds to 1": int((1.0 - rad * rad / (d * rad) ** 2 == 1.0).sum()), "NaN direction": int(nan_dir.sum())}
        print(f"{name}: {len(rec)} records, {n}; Lambertian {int((rec[:, 11] == mats['lam'].id).sum())}")
        assert all(v >= 50 for v in n.values()), n
        assert (fam[nan_dir] != "far").all() and (rec[:, 11] == mats["lam"].id).sum() >= 200 and (rec[:, 11] != mats["lam"].id).sum() >= 200


def _moved(op):
    def math(o, a, b):
        v = L.host_math(o, a, b)
        if o == op:
            ok = np.isfinite(v) & (v != 0.0)
            v = np.where(ok, (v.view(np.int64) + 1).view(np.float64), v)
        return v
    return math


# (op, set): every routed site at least once — the cosine arm's and the sphere light's sincos_0_2pi; GTR_1_direction's pow, sin, cos and
# GTR_2_aniso_direction's tan, atan, sin, cos (the PBR set); mon_to_lin's pow and GTR_1's log2 alone (the brdf set generates nothing);
# get_sphere_uv's atan2, acos; the marble's sin alone and under a checker; the medium's log.  (The checker's own sin decides a branch:
# a move of 1 ulp changes no sign.  test_libm_replay_gpu.py holds it to the oracle's branch on every point.)
MOVES = [("sincos_0_2pi", "one bounce full none lam"), ("sincos_0_2pi", "one bounce hostile sphere"), ("sin", "one bounce full none pbr"),
         ("cos", "one bounce full none pbr"), ("tan", "one bounce full none pbr"), ("atan", "one bounce full none pbr"),
         ("pow", "one bounce full none pbr"), ("log2", "one bounce full none pbr"), ("pow", "brdf"), ("log2", "brdf"),
         ("atan2", "u, v sphere_origin"), ("acos", "u, v sphere_origin"), ("sin", "texture marble noise4"),
         ("sin", "texture checker over an image and a noise texture"), ("log", "medium sphere")]


@pytest.mark.parametrize("op,name", MOVES)
def test_one_op_moved_by_one_ulp(op, name):
    """Against the replay with glibc's values as they are: records whose lookups touched the moved op change — some on every routed site —
    and a record that did not look the op up keeps every word; in the last round every lookup of every op was served by the table.

    NOT asserted: "at least as many records change as looked the op up".  No 1-ulp move can do that: the next operation rounds half of
    such moves away (v = acos(..) / pi: 1330 of 1687 records change; 0.5 (1 + sin): 460 of 793), a NaN or a value multiplied by zero
    stays what it was (the sphere light seen from inside: 804 of 1837), and a branch taken on a sign does not move at all.  What every
    lookup returned is checked instead: lookups == matches per op, and the table holds nothing but the moved values."""
    run = _runs()[name]
    base, _ = L.replay(run, L.host_math)
    per_record = name != "brdf"                                          # (orc_brdf is called record by record: nothing to note)
    k = base.shape[-2]
    note = orc.libm_touched(k)

    def run_noting():
        with note:
            return run()
    got, counts = L.replay(run_noting, _moved(op))
    assert counts[op][0] >= 3 and all(l == m and l > 0 for o, (l, m) in counts.stats.items() if o in counts)
    if not per_record:
        d = ~L.same(got, base)
        assert d[..., :3].any() and bool(d[..., 3].any()) == (op == "log2")              # the BRDF moves; the pdf value with log2 alone
        return
    changed = L.differing_records(got.reshape(-1, *got.shape[-2:])[0], base.reshape(-1, *base.shape[-2:])[0])
    t = note.touched(op)[:k]
    print(f"{op} moved by 1 ulp on {name}: {int(t.sum())} of {len(t)} records looked it up, {int(changed.sum())} changed, {int((changed & ~t).sum())} changed without a lookup")
    assert t.any() and (changed & t).any()
    assert not (changed & ~t).any()


def test_whole_paths_under_threads():
    """orc_ray_color_paths on four threads with a table set: the table is only read while a batch runs and the miss list takes a lock, so
    the replayed paths are the plain ones word for word, every operand is noted once, and the last round finds them all"""
    ob, _ = K.make_scene(orc.load(), "full", "sphere")
    rays = K.real_rays(400, 7408)
    run = lambda: orc.ray_color_paths(ob, rays, 2, (0.1, 0.2, 0.3), 4, K.SEED, nthreads=4)
    plain = run()
    got, counts = L.replay(run, L.glibc_of_site, label="whole paths, 4 threads (glibc)", wants_glibc=True)
    assert L.same(got, plain).all() and counts.rounds == 2
    assert counts["sincos_0_2pi"][0] >= 200 and counts["pow"][0] >= 1 and sum(l for l, _ in counts.stats.values()) >= sum(e for e, _ in counts.values())

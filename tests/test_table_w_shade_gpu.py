"""The compact lean f64 kernel's shade_hit on the device, ONE call per record (rt_debug_shade with RT_KAT_TABLE_W: csrc/rt_kat.hip
shade_kat_table_w_kernel does what trace_shade_fill<double, 0, true> does at the top of its material section — ring_pack_signs,
ring_normal, shade_hit<double, 0, true>, whose merged arm is rt_kernel.hip merged_arms_table_w).  That function has its own order of
operations — Metal reflects into ray.d at the top, one shared normalisation, w / v / u loaded from the ONB table where they are used and w a
second time at dot(xn, w), the light count converted at its use — and the frames of every scene with the compact first-hit ring run it.

The room, the ten `lights` lists and the record families are tests/table_w_shade_cases.py's (tests/test_table_w_shade_host.py counts, by
the oracle alone, what they hold): no lights; one bare rect light in each plane; two (the divisor 2 is exact) and three (the divisor 3
rounds); two stacked rects (two non-zero terms in the mixture sum); one rect twice; a list mixing rects, a trait-default entry and a rect of
area 0; a lamp in the ceiling's own plane.  Real records and hostile ones: p on and next to a light's plane and under its edges, incoming
directions of every magnitude and with zero, denormal, infinite and NaN components; five beta, depth_left 1 and 50, RT_STOP_ON_ZERO.

1. The compact form against the lean form with and without the ONB memo and against the all-features form: 0 differing 64-bit words in all
   19 columns on every record (NaN compared as NaN).
2. Against the oracle's one level of ray_color (orc.shade_batch) under tests/test_shade_kat_gpu.py's rules: stream words, done, depth_left
   and the NaN / inf pattern equal; 0 differing words on every Metal record and every Lambertian record whose first draw picks the lights;
   |got - ref| <= 1e-9 (1 + |ref|) on the cosine arm, at most 1 % of it left out by the oracle's margin.  The largest ratio is printed.
3. Neighbours: a record's words do not depend on what the other lanes of its wave hold (the wave votes of div_pi_pair and rect_absdot),
   nor on the batch's length (the partial last wave).
4. beta scaled by powers of two scales the output exactly.
5. Whole samples of the rooms whose `lights` have 3 and 5 entries, lights in the XY and YZ planes, stacked lights and the flush lamp,
   through the kernel the frames run: 0 differing words against RT_NO_PRIMARY_PASS and against the wide ring, equal non-finite counts; against
   the oracle 0 differing words at max_depth 1, deeper 0 samples beyond SAMPLE_RTOL; the compact kernel ran."""
import numpy as np
import pytest

import shade_kat_cases as K
import table_w_shade_cases as T
from oracle import orc
from raytracinginrust_amd import render as R

from test_compact_ring_gpu import _assert_ring
from test_compact_ring_host import COMPACT, QN_W
from test_primary_pass_gpu import on_off
from test_shade_kat_gpu import differing

pytestmark = pytest.mark.gpu
SETS = list(T.LIGHT_SETS)
COMBOS = [(beta, depth, flags) for beta in T.BETAS for depth in T.DEPTHS for flags in T.FLAGS]
OTHER_FORMS = (("lean", dict()), ("lean, no ONB memo", dict(onb_table=False)), ("rest", dict(shape="rest")))
_SETS = {}


def _set(lights):
    """(product scene, oracle scene, materials, records, rays, family): the records are the device's hit query's"""
    if lights not in _SETS:
        pb, mats, _ = T.room(R._lib.load(), lights)
        assert R.debug_ring_form(pb) == COMPACT
        ob, omats, _ = T.room(orc.load(), lights)
        assert {k: v.id for k, v in mats.items()} == {k: v.id for k, v in omats.items()}
        rec, rays, fam = T.record_set(lights, mats, lambda r: R.query_hits(pb, r))
        for a in (rec, rays):
            a.setflags(write=False)
        _SETS[lights] = (pb, ob, mats, rec, rays, fam)
    return _SETS[lights]


def _compact(pb, rec, rays, **kw):
    return R.debug_shade(pb, rec, rays, seed=T.SEED, table_w=True, **kw)


# ---------------------------------------------------------------- 1.
@pytest.mark.parametrize("lights", SETS)
def test_compact_form_is_the_other_forms_word_for_word(lights):
    pb, ob, mats, rec, rays, fam = _set(lights)
    assert 2000 <= len(rec) <= 8192
    n_calls = 0
    for beta, depth, flags in COMBOS:
        got = _compact(pb, rec, rays, beta=beta, depth_left=depth, flags=flags)
        for name, kw in OTHER_FORMS:
            other = R.debug_shade(pb, rec, rays, seed=T.SEED, beta=beta, depth_left=depth, flags=flags, **kw)
            d = ~(K.same_words(got, other) | (np.isnan(got) & np.isnan(other)))
            per_family = {f: int(d[fam == f].sum()) for f in ("real", "p", "d")}
            assert not d.any(), f"{lights} beta {beta} depth_left {depth} flags {flags}: {int(d.sum())} words differ from the {name} form {per_family}; " \
                                f"first record {np.nonzero(d.any(1))[0][:3].tolist()}, columns {np.nonzero(d.any(0))[0].tolist()}"
            n_calls += 1
    print(f"{lights}: {len(rec)} records x {len(COMBOS)} (beta, depth_left, flags) x {len(OTHER_FORMS)} forms: 0 of {n_calls * rec.shape[0] * 19} words differ")


# ---------------------------------------------------------------- 2.
@pytest.mark.parametrize("lights", SETS)
def test_compact_form_against_the_oracle(obe, lights):
    pb, ob, mats, rec, rays, fam = _set(lights)
    is_metal, is_lam, to_light = T.classes(rec, mats, obe, T.SEED)
    if not T.LIGHT_SETS[lights]:
        to_light = np.zeros(len(rec), bool)                             # (no lights: no coin is drawn, deviation D2)
    exact = is_metal | to_light
    worst_of_set, left = 0.0, 0
    for beta, depth, flags in COMBOS:
        ref, margin = orc.shade_batch(ob, rec, rays, beta=beta, seed=T.SEED, depth_left=depth, flags=flags)
        got = _compact(pb, rec, rays, beta=beta, depth_left=depth, flags=flags)
        worst, n_exact, n_cmp, left_out = T.check_against_oracle(f"{lights} beta {beta} depth_left {depth} flags {flags}", got, ref, margin, exact)
        worst_of_set, left = max(worst_of_set, worst), max(left, left_out)
    print(f"{lights}: {int(exact.sum())} records exact ({int(is_metal.sum())} Metal, {int(to_light.sum())} to the lights), {int((~exact).sum())} on the cosine arm "
          f"({left} left out by the margin), max |got - ref| / (1 + |ref|) = {worst_of_set:.3e} (bound {K.SAMPLE_RTOL:.0e}) over {len(COMBOS)} (beta, depth_left, flags)")
    assert exact.any() and (~exact).any()


# ---------------------------------------------------------------- 3.
@pytest.mark.parametrize("lights", SETS)
def test_a_records_words_do_not_depend_on_its_neighbours(lights):
    pb, ob, mats, rec, rays, fam = _set(lights)
    (a_rec, a_rays), (b_rec, b_rays) = T.neighbour_sets(rec, rays)
    changed = [j for j in range(256) if j not in T.KEPT]
    assert not np.isfinite(b_rays[changed, 3:6]).all(1).any() and not np.isfinite(b_rec[changed, 2:5]).all(1).any()
    for flags in T.FLAGS:
        a, b = _compact(pb, a_rec, a_rays, flags=flags), _compact(pb, b_rec, b_rays, flags=flags)
        kept = list(T.KEPT)
        assert differing(a[kept], b[kept]) == 0, f"{lights}: records {kept} change with their neighbours: {differing(a[kept], b[kept])} words"
        assert differing(a[changed], b[changed]) > 0                    # (the neighbours did change)
        for name, kw in OTHER_FORMS:                                    # ... and the hostile array is the other forms' too
            assert differing(b, R.debug_shade(pb, b_rec, b_rays, seed=T.SEED, flags=flags, **kw)) == 0, name


@pytest.mark.parametrize("lights", ["none", "three", "mixed5"])
def test_batch_lengths_and_the_partial_last_wave(lights):
    pb, ob, mats, rec, rays, fam = _set(lights)
    whole = _compact(pb, rec, rays)
    for n in (1, 63, 65, 257):
        part = _compact(pb, rec[:n], rays[:n])
        assert part.shape == (n, 19) and differing(part, whole[:n]) == 0, n


# ---------------------------------------------------------------- 4.
@pytest.mark.parametrize("lights", SETS)
def test_beta_in_powers_of_two_scales_exactly(lights):
    pb, ob, mats, rec, rays, fam = _set(lights)
    one = _compact(pb, rec, rays)
    two = _compact(pb, rec, rays, beta=(2.0, 0.5, 4.0))
    with np.errstate(all="ignore"):
        want = one.copy()
        want[:, 7:10] = one[:, 7:10] * np.array([2.0, 0.5, 4.0])
    tiny = (np.abs(want[:, 7:10]) < 2.0 ** -1000).any(1) & (want[:, 7:10] != 0.0).any(1)      # (a denormal product does not scale exactly)
    huge = np.isfinite(one[:, 7:10]).all(1) & ~np.isfinite(want[:, 7:10]).all(1)               # (nor one that overflows)
    assert int((tiny | huge).sum()) <= len(rec) // 100
    assert differing(two[~(tiny | huge)], want[~(tiny | huge)]) == 0


# ---------------------------------------------------------------- 5.
FRAMES = [(2, 2, 333), (16, 16, 4)]
FRAME_DEPTHS = [1, 2, 50]
FRAME_SEED = 41
_BUILT, _ORACLE = {}, {}


def _built(lights, side, monkeypatch=None):
    if (lights, side) not in _BUILT:
        if side == "w":
            monkeypatch.setenv("RT_NO_ONB_TABLE", "1")                 # (read when the scene is flattened: the query below flattens it)
            b = T.room(R._lib.load(), lights)[0]
            assert R.debug_ring_form(b) == {"compact": False, "entries": QN_W, "entry_bytes": 104}
            monkeypatch.delenv("RT_NO_ONB_TABLE")
        elif side == "o":
            b = T.room(orc.load(), lights)[0]
        else:
            b = _set(lights)[0]
        _BUILT[(lights, side)] = b
    return _BUILT[(lights, side)]


def _oracle_samples(lights, W, H, spp, depth):
    key = (lights, W, H, spp, depth)
    if key not in _ORACLE:
        _, rs, cnt = orc.render(_built(lights, "o"), T.ROOM_CAM, T.background(lights), W, H, spp, depth, seed=FRAME_SEED, want_samples=True, want_counters=True)
        rs.setflags(write=False)
        _ORACLE[key] = (rs, cnt["nonfinite"])
    return _ORACLE[key]


@pytest.mark.parametrize("depth", FRAME_DEPTHS)
@pytest.mark.parametrize("W,H,spp", FRAMES)
@pytest.mark.parametrize("lights", T.FRAME_SETS)
def test_whole_samples_on_the_compact_kernel(monkeypatch, lights, W, H, spp, depth):
    b, cam, bg = _built(lights, "p"), T.ROOM_CAM, T.background(lights)
    gs = on_off(monkeypatch, b, cam, bg, W, H, spp, depth, seed=FRAME_SEED)      # against RT_NO_PRIMARY_PASS: 0 differing words, equal counts
    _assert_ring(b, "wide")
    _, again = R.render(b, cam, bg, W, H, spp, depth, seed=FRAME_SEED, want_samples=True)
    _assert_ring(b, "compact")
    n_gpu = R.last_stats(b)["nonfinite_samples"]
    assert int((again.view(np.uint64) != gs.view(np.uint64)).sum()) == 0
    bw = _built(lights, "w", monkeypatch)
    _, ws = R.render(bw, cam, bg, W, H, spp, depth, seed=FRAME_SEED, want_samples=True)
    _assert_ring(bw, "wide")
    n_diff = int((ws.view(np.uint64) != gs.view(np.uint64)).sum())
    assert n_diff == 0, f"{n_diff} of {gs.size} words differ between the compact kernel and the wide ring's"
    assert R.last_stats(bw)["nonfinite_samples"] == n_gpu
    assert (gs != 0.0).any()
    rs, n_ref = _oracle_samples(lights, W, H, spp, depth)
    assert np.array_equal(np.isnan(gs), np.isnan(rs)) and np.array_equal(np.isinf(gs), np.isinf(rs))
    fin = np.isfinite(rs)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs, 0.0))
    bad = (d > K.SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs, 0.0)))).any(axis=-1)
    n_words = int((gs.view(np.uint64) != rs.view(np.uint64)).sum())
    print(f"{lights} {W}x{H}x{spp} depth {depth}: {n_words} of {gs.size} words differ from the oracle's, max |gpu - oracle| {d.max():.3e}, "
          f"diverged {int(bad.sum())}, non-finite samples {n_gpu} (oracle {n_ref})")
    assert int(bad.sum()) == 0, f"{int(bad.sum())} of {W * H * spp} samples diverged from the oracle; first at {np.argwhere(bad)[:3].tolist()}"
    if depth == 1:
        assert n_words == 0, f"{n_words} of {gs.size} words differ from the oracle's at max_depth 1"
    assert n_gpu == n_ref
    _assert_ring(b, "compact")

"""The host's side of tests/test_table_w_shade_gpu.py (no GPU): the compact lean f64 kernel's shade_hit, one call per record
(rt_debug_shade with RT_KAT_TABLE_W), on every kind of `lights` list its code can tell apart (tests/table_w_shade_cases.py).

  * every light set's room flattens to the compact first-hit ring, with the expected n_lights;
  * rt_debug_shade refuses — before any device call, naming the record — the flag beside RT_KAT_REST_SHAPE or RT_KAT_NO_ONB_TABLE, a scene
    whose ring is not compact, a record that is neither Lambertian nor Metal, a record whose normal is not its rect's table magnitudes;
  * the record sets are deterministic, and by the oracle alone (orc.shade_batch, K.first_draw_is_light, the stream restated in NumPy and
    checked against both) they hold what the device test is there for: at least 100 to-light records per light index in every set, 100
    records of `stacked` whose mixture sum has two non-zero terms, 100 non-finite beta in `mixed5` and in `flush`, 50 Metal records that
    run the rejection loop again, 50 absorbed Metal records; and at most 1 % of any set's cosine-arm records lie below the oracle's margin."""
import ctypes as C

import numpy as np
import pytest

import shade_kat_cases as K
import table_w_shade_cases as T
from oracle import orc
from raytracinginrust_amd import render as R

from test_compact_ring_host import COMPACT, _one_rect_scene, rotate_x

SETS = list(T.LIGHT_SETS)


# ---------------------------------------------------------------- the flattener
@pytest.mark.parametrize("lights", SETS)
def test_every_light_set_gets_the_compact_ring(pbe, lights):
    b, mats, handles = T.room(pbe, lights)
    assert R.debug_ring_form(b) == COMPACT
    assert R.flatten(b)["lights"] == len(handles) == len(T.LIGHT_SETS[lights])     # n_lights: the divisor of hit.rs:90-92
    mag, _, n_valid = R.debug_onb_table(b)
    # the walls (5), three Cubes (18) and the set's lamps in the world have entries (the flattener may keep further records of its own)
    n_lamps = len({L for L in T.LIGHT_SETS[lights] if L != T.CUBE and L[1] != L[2]})
    assert 5 + 18 + n_lamps <= n_valid <= len(mag), (n_valid, len(mag))
    wmag = R.debug_onb_table_w(b)
    assert int((wmag != mag).any(axis=1).sum()) >= 8                   # the side faces of both rotated Cubes: w != n in bits


# ---------------------------------------------------------------- the refusals
def _valid_records(b, mats, n=3):
    """n synthetic records that pass every check: a rect with a table entry, its magnitudes with a sign pattern as the normal, Lambertian"""
    mag, _, _ = R.debug_onb_table(b)
    i = int(np.flatnonzero(mag[:, 0] != np.uint64(R.ONB_MAG_INVALID))[-1])          # (the last one: a face of the bare Cube)
    nrm = mag[i].view(np.float64) * np.array([-1.0, 1.0, -1.0])
    rec = np.zeros((n, 16))
    rec[:, 0] = 1.0; rec[:, 1] = 10.0; rec[:, 2:5] = (50.0, 50.0, 50.0); rec[:, 5:8] = nrm; rec[:, 8] = 1.0
    rec[:, 11] = mats["white"].id; rec[:, 14] = i
    rays = np.tile(np.array([40.0, 45.0, 40.0, 1.0, 0.5, 1.0, 0.0]), (n, 1))
    return rec, rays, i


def test_refusals_name_the_record(pbe, monkeypatch):
    b, mats, _ = T.room(pbe, "three")
    rec, rays, i = _valid_records(b, mats)
    for shape, table in (("rest", True), ("lean", False)):
        with pytest.raises(R.RenderError, match="neither RT_KAT_REST_SHAPE nor RT_KAT_NO_ONB_TABLE"):
            R.debug_shade(b, rec, rays, shape=shape, onb_table=table, table_w=True)
    bad = rec.copy(); bad[2, 11] = mats["light"].id
    with pytest.raises(R.RenderError, match="record 2: RT_KAT_TABLE_W takes Lambertian and Metal records only"):
        R.debug_shade(b, bad, rays, table_w=True)
    for col, v in ((5, np.nan), (6, 0.5), (7, -K.step(float(rec[1, 7]), 1)), (5, 0.0 if rec[1, 5] != 0.0 else 1.0)):
        bad = rec.copy(); bad[1, col] = v
        with pytest.raises(R.RenderError, match=f"record 1: the normal's magnitudes are not those of rect {i}'s ONB-table entry"):
            R.debug_shade(b, bad, rays, table_w=True)
    bad = rec.copy(); bad[0, 14] = 1e6
    with pytest.raises(R.RenderError, match="record 0: rect index out of range"):
        R.debug_shade(b, bad, rays, table_w=True)
    with pytest.raises(R.RenderError, match="RT_KAT_NO_ONB_TABLE and RT_KAT_TABLE_W only"):      # a flag rt_debug_shade does not know is still refused
        R.debug_shade(b, rec, rays, flags=0x800, table_w=True)
    # a scene whose ring is not compact: a rect under RotateX, and the room flattened without the table
    wide = _one_rect_scene(pbe, rotate_x)
    assert not R.debug_ring_form(wide)["compact"]
    with pytest.raises(R.RenderError, match="RT_KAT_TABLE_W serves scenes with the compact first-hit ring only"):
        R.debug_shade(wide, rec, rays, table_w=True)
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")
    b2, mats2, _ = T.room(pbe, "three")
    assert not R.debug_ring_form(b2)["compact"]
    monkeypatch.delenv("RT_NO_ONB_TABLE")
    with pytest.raises(R.RenderError, match="RT_KAT_TABLE_W serves scenes with the compact first-hit ring only"):
        R.debug_shade(b2, rec, rays, table_w=True)


# ---------------------------------------------------------------- the sets, by the oracle alone
def test_the_stream_restated_in_numpy_is_the_oracles(obe):
    n = 3000
    s = T.streams(T.SEED, n)
    st = (C.c_uint32 * 4)()
    for k in (0, 1, 2, 63, 64, 255, 256, 1000, n - 1):
        obe.lib.orc_rng_path(C.c_uint64(T.SEED), C.c_uint32(k), C.c_uint32(0), st)
        assert list(st) == s[k].tolist(), k
    coin, _ = T.light_index(T.SEED, n, 5)
    assert np.array_equal(coin, K.first_draw_is_light(obe, T.SEED, n))


def test_an_empty_range_draws_the_same_number_from_both_streams(obe, pbe):
    """R(a, a) — the reference's rand panics on it; `mixed5`'s rect light of zero width samples it on every pick — is the largest double below
    a in the oracle's stream and in the library's (oracle/orc_rng.h, csrc/rt_rng.h): the device test found the oracle returning a itself,
    so that the two sampled different points of that light.  Ordinary ranges are unchanged (tests/test_host_logic.py)."""
    from raytracinginrust_amd.api import Rng
    for a in (20.0, -3.0, 0.0, 1e-300, 99.5):
        x, y = Rng(obe, T.SEED, 3).gen_range(a, a), Rng(pbe, T.SEED, 3).gen_range(a, a)
        assert K.words(x) == K.words(y) == K.words(np.nextafter(a, -np.inf)), (a, x, y)
    x, y = Rng(obe, T.SEED, 4), Rng(pbe, T.SEED, 4)
    assert [x.gen_range(10.0, 90.0) for _ in range(200)] == [y.gen_range(10.0, 90.0) for _ in range(200)]


def test_the_record_sets_are_deterministic():
    ob, mats, _, rec, rays, fam = T.oracle_set("mixed5")
    rec2, rays2, fam2 = T.record_set("mixed5", mats, lambda r: orc.hit_records(ob, r))
    same = lambda a, b: (K.same_words(a, b) | (np.isnan(a) & np.isnan(b))).all()
    assert same(rec, rec2) and same(rays, rays2) and (fam == fam2).all()
    assert {"real", "p", "d"} == set(fam.tolist())


@pytest.mark.parametrize("lights", SETS)
def test_family_counts_and_margin(obe, lights):
    ob, mats, handles, rec, rays, fam = T.oracle_set(lights)
    n, n_lights = len(rec), len(handles)
    is_metal, is_lam, to_light = T.classes(rec, mats, obe, T.SEED)
    out, margin = orc.shade_batch(ob, rec, rays, seed=T.SEED)
    # the arm the oracle took is the arm the first draw names: a to-light record with no lights does not exist
    if n_lights == 0:
        to_light = np.zeros(n, bool)
    coin, idx = T.light_index(T.SEED, n, n_lights)
    assert np.array_equal(coin & is_lam & (n_lights != 0), to_light)
    per_index = [int((to_light & (idx == i)).sum()) for i in range(n_lights)]
    cosine = is_lam & ~to_light
    below = int((cosine & (margin < K.MARGIN)).sum())
    # Metal: b1, b2 and the third component are three u64 draws, six words; a longer way means the rejection loop ran again
    s6 = T.advance(T.streams(T.SEED, n), 6)
    again = is_metal & (out[:, 15:19] != s6.astype(np.float64)).any(axis=1)
    absorbed = is_metal & (out[:, 13] == 1.0)
    bad_beta = ~np.isfinite(out[:, 7:10]).all(axis=1)
    print(f"{lights}: {n} records ({int((fam == 'real').sum())} real, {int((fam == 'p').sum())} moved p, {int((fam == 'd').sum())} changed d), "
          f"{int(is_lam.sum())} Lambertian, to-light per index {per_index}, cosine arm {int(cosine.sum())} with {below} below the margin, "
          f"Metal {int(is_metal.sum())}: {int(again.sum())} reject again, {int(absorbed.sum())} absorbed; non-finite beta {int(bad_beta.sum())}")
    assert n <= 8192 and (fam == "real").sum() >= 2000
    assert all(c >= 100 for c in per_index), per_index
    assert int(again.sum()) >= 50 and int(absorbed.sum()) >= 50
    assert below <= K.MARGIN_CAP * int(cosine.sum())
    for f in ("real", "p", "d"):                                       # ... in every family of the set, too
        m = cosine & (fam == f)
        assert int((m & (margin < K.MARGIN)).sum()) <= K.MARGIN_CAP * int(m.sum()), f
    if lights in ("mixed5", "flush"):
        assert int(bad_beta.sum()) >= 100
    if lights == "flush":                                              # where they come from: to-light records on the ceiling's plane (0 / 0 in the rect test)
        on_plane = to_light & (rec[:, 3] == 100.0)
        assert int((bad_beta & on_plane).sum()) >= 100
    if lights == "stacked":
        two_terms = 0
        for k in np.flatnonzero(is_lam):
            p0, p1 = (orc.pdf_value(ob, h, out[k, 0:3], out[k, 3:6]) for h in handles)
            two_terms += int(p0 != 0.0 and p1 != 0.0 and np.isfinite(p0) and np.isfinite(p1))
        print(f"stacked: {two_terms} records whose mixture sum has two non-zero terms")
        assert two_terms >= 100

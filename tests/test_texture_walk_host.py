"""The oracle's side of the texture walk cases (tests/texture_cases.py), no GPU: that the hostile (u, v, p) reach what they are meant to
reach, that the exact rules the GPU test holds the device to are rules glibc's own results obey, and that the DiffuseLight trick —
orc_shade_batch's emitted colour of a synthetic front-face record — is Texture::mapping(u, v, p) word for word, which ties it to
ray_color.  tests/test_texture_walk_gpu.py holds the device's tex_eval to the same oracle."""
import functools

import numpy as np
import pytest

import texture_cases as T
from oracle import orc


@functools.lru_cache(None)
def _scene():
    return T.build(orc.load())


def test_both_builders_number_the_handles_alike(pbe, obe):
    _, ptex, pmats = T.build(pbe)
    _, otex, omats = _scene()
    assert {k: h.id for k, h in ptex.items()} == {k: h.id for k, h in otex.items()}
    assert {k: h.id for k, h in pmats.items()} == {k: h.id for k, h in omats.items()}


@pytest.mark.parametrize("name", list(T.SMALL_IMAGES))
def test_image_cases_reach_every_texel_the_clamps_and_nan(name):
    """From the oracle's colours alone: the hostile set reaches every texel; the texel is texture.rs:105-116 in exact terms on every case
    (the uniform ones included); u = 1 and beyond land on column w - 1, v = 0 and below on row h - 1 (the integer clamp); NaN u, v land
    on column 0 and row 0 of the stored image — `NaN as usize` is 0 —, which is texel (0, h - 1) counted from the bottom."""
    ob, tex, _ = _scene()
    w, h = T.SMALL_IMAGES[name]
    u, v, n_hostile = T.image_cases(name)
    got = T.oracle_values(ob, tex[name].id, u, v, np.zeros((len(u), 3)))
    i, j = T.texel_of(got)
    wi, wj = T.image_index(u, v, w, h)
    assert np.array_equal(i, wi) and np.array_equal(j, wj)
    assert {(a, b) for a, b in zip(i[:n_hostile], j[:n_hostile])} == {(a, b) for a in range(w) for b in range(h)}
    one_up = u >= 1.0
    assert one_up.sum() >= 4 and (i[one_up] == w - 1).all()
    v_low = v <= 0.0
    assert v_low.sum() >= 4 and (j[v_low] == h - 1).all()
    nan = np.isnan(u) & np.isnan(v)
    assert nan.sum() >= 1 and (i[nan] == 0).all() and (j[nan] == 0).all()
    assert (i[np.isnan(u)] == 0).all() and (j[np.isnan(v)] == 0).all()
    # one ulp to either side of a boundary lands on both of its sides
    if w > 1:
        k = 1
        near = [float(np.nextafter(k / w, 0.0)), k / w]
        cols = {float(x): int(c) for x, c in zip(u, i) if float(x) in near}
        assert cols[near[0]] == k - 1 and cols[near[1]] == k


def test_the_emitted_colour_of_a_front_face_record_is_the_texture_value():
    """orc_shade_batch — the code ray_color runs after a hit — on synthetic DiffuseLight records: e is orc_texture_value(u, v, p), the
    path ends, and a back face emits nothing."""
    ob, tex, mats = _scene()
    for name in ("img3x5", "earth", "check2", "noise4", "chain"):
        u, v, _ = T.image_cases("img3x5")
        p = T.noise_points(4.0)[:len(u)]
        n = min(len(u), len(p), 400)
        u, v, p = u[:n], v[:n], p[:n]
        rec, rays = T.records(mats[name].id, u, v, p)
        out, _ = orc.shade_batch(ob, rec, rays, seed=1)
        want = T.oracle_values(ob, tex[name].id, u, v, p)
        assert T.same(out[:, 10:13], want).all(), name
        assert (out[:, 13] == 1.0).all()
        rec[:, 8] = 0.0
        back, _ = orc.shade_batch(ob, rec, rays, seed=1)
        assert (back[:, 10:13] == 0.0).all()


def test_checker_rule_holds_for_glibc_and_leaves_out_little():
    """The branch the oracle takes (two distinct constants name it) equals the one decided from the signs of the exact sines on EVERY
    decided case, and at most 2 % of the set is undecided (an argument +-0, or an f64 product of sines that underflows to 0)."""
    ob, tex, _ = _scene()
    p = T.checker_points()
    odd, decided = T.checker_decisions()
    assert (~decided).sum() <= 0.02 * len(p), f"{int((~decided).sum())} of {len(p)} left out"
    assert (~decided).sum() >= 5 and odd[decided].sum() > 500 and (~odd[decided]).sum() > 500
    got = T.oracle_values(ob, tex["check2"].id, np.zeros(len(p)), np.zeros(len(p)), p)
    took_odd = (got == np.array(T.CONSTS[0])).all(axis=1)
    assert (took_odd | (got == np.array(T.CONSTS[1])).all(axis=1)).all()
    assert np.array_equal(took_odd[decided], odd[decided])
    # the cases do sit on the zeros: the nearest sine of most cases is below 1e-10 in magnitude
    with np.errstate(all="ignore"):
        smallest = np.abs(np.sin(10.0 * p)).min(axis=1)
    assert (smallest < 1e-10).mean() > 0.9
    print(f"checker: {len(p)} points, {int((~decided).sum())} undecided, {int(odd[decided].sum())} odd")


@pytest.mark.parametrize("name", list(T.NOISE_SCALES))
def test_noise_cases_reach_the_saturating_index_and_both_sin_ranges(name):
    ob, tex, _ = _scene()
    scale = T.NOISE_SCALES[name]
    p = T.noise_points(scale)
    got = T.oracle_values(ob, tex[name].id, np.zeros(len(p)), np.zeros(len(p)), p)
    assert (got[:, 0] == got[:, 1]).all() | np.isnan(got).any()
    fin = np.isfinite(got).all(axis=1)
    assert ((got[fin] >= 0.0) & (got[fin] <= 1.0)).all()
    with np.errstate(all="ignore"):
        sx = scale * p
    if scale != 0.0:
        assert (np.abs(sx) >= 2.0 ** 64).any() and ((np.abs(sx) >= 2.0 ** 32) & (np.abs(sx) < 2.0 ** 64)).any() and (sx < 0.0).any()
        assert (~fin).sum() >= 3 and fin.sum() > 500
        small = T.in_measured_sin_range(scale, p)
        assert (small & fin).sum() > 300 and (~small & fin).sum() > 20
        # crossing 2^32 within the seven doublings: some component in [2^25, 2^32)
        assert ((np.abs(sx) >= 2.0 ** 25) & (np.abs(sx) < 2.0 ** 32)).any() and ((np.abs(sx) >= 2.0 ** 57) & (np.abs(sx) < 2.0 ** 64)).any()
    else:
        assert (got[np.isfinite(p).all(axis=1)] == 0.5).all()      # scale 0: sin(0 + 10 |0|) = 0 wherever 0 * p is a number


def test_the_chain_reads_the_image_at_the_records_own_uv():
    """70 CheckTextures over the 3 x 5 image, both children the next one down: the value is the image's texel at (u, v), whatever p."""
    ob, tex, _ = _scene()
    u, v, _ = T.image_cases("img3x5")
    p = np.random.RandomState(5).uniform(-5.0, 5.0, (len(u), 3))
    a = T.oracle_values(ob, tex["chain"].id, u, v, p)
    b = T.oracle_values(ob, tex["img3x5"].id, u, v, p)
    assert T.same(a, b).all()
    assert len({tuple(x) for x in a.tolist()}) == 15

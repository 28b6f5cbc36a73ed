"""The per-face ONB memo on the device (rt_kernel.hip onb_memo_probe / onb_memo_load, the lean f64 kernel's merged Lambertian arm): the
device functions on given (rect, normal) pairs through rt_debug_onb, and whole frames with and without the table (RT_NO_ONB_TABLE),
sample by sample.  The reference is the numpy restatement of onb.rs:8-20 in tests/test_onb_table_host.py; everything is bit for bit."""

import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from test_fuzz_gpu import _list_hits_gpu, _list_hits_oracle, _rand_box_room_scene, _rand_list_scene
from test_cube_division_only_gpu import _cornell
from test_onb_table_host import INVALID, SIGN, bounce_rays, onb_numpy, plain_rays, same_words

pytestmark = pytest.mark.gpu


def _check_pairs(b, rects, normals, mag, must_hit=None):
    """every pair is a miss, or a hit whose v, u are the numpy ONB of that very normal; a hit implies |normal| == the entry's mag; returns hit"""
    hit, v, u = R.debug_onb(b, rects, normals)
    absw = np.ascontiguousarray(normals, np.float64).view(np.uint64) & ~SIGN
    match = (absw == mag[np.asarray(rects, int)]).all(axis=1)
    assert np.array_equal(hit, match), f"{int((hit != match).sum())} pairs: hit flag differs from the bit-for-bit comparison with mag"
    rv, ru = onb_numpy(normals)
    ok = same_words(v[hit], rv[hit]).all(axis=1) & same_words(u[hit], ru[hit]).all(axis=1)
    assert ok.all(), f"{int((~ok).sum())} of {int(hit.sum())} memo hits differ from the numpy ONB, e.g. normal {np.asarray(normals)[hit][~ok][0].tolist()}"
    assert not v[~hit].any() and not u[~hit].any()
    if must_hit is not None:
        assert hit[must_hit].all(), f"{int((~hit[must_hit]).sum())} pairs on valid rects missed"
    return hit


@pytest.fixture(scope="module")
def cornell_normals(pbe, obe):
    """64 x 160 plain rays into the Cornell box and one generation of bounces off their hit points: the oracle's hit normals, and the rect
    record of each hit as the kernels' own search names it (rt_debug_list_hit; the same hits: tests/test_cube_division_only_gpu.py)"""
    pb, ob = _cornell(pbe), _cornell(obe)
    rnd = np.random.default_rng(8801)
    mn, mx = (np.asarray(v, np.float64) for v in pb.box)
    n = 64 * 160
    first = plain_rays(rnd, mn, mx, n)
    ref = _list_hits_oracle(ob, first, 1e-5)
    second = bounce_rays(rnd, mn, mx, ref[:, 0] != 0.0, ref[:, 2:5])[: 64 * 40]
    rays = np.ascontiguousarray(np.concatenate([first, second]))
    ref = np.concatenate([ref, _list_hits_oracle(ob, second, 1e-5)])
    got = _list_hits_gpu(pbe, pb, rays, 1e-5)
    h = ref[:, 0] != 0.0
    assert np.array_equal(h, got[:, 0] != 0.0)
    return pb, got[h, 10].astype(int), np.ascontiguousarray(ref[h, 5:8])


def test_memo_on_oracle_normals(pbe, cornell_normals):
    pb, rects, normals = cornell_normals
    mag, _, n_valid = R.debug_onb_table(pb)
    assert n_valid > 0 and len(rects) >= 64 * 160
    valid = mag[rects, 0] != INVALID
    assert valid.all(), "a hit on a rect of the Cornell box without an entry"
    hit = _check_pairs(pb, rects, normals, mag, must_hit=valid)
    assert hit.all()
    assert len(set(rects.tolist())) >= 14, "the rays do not reach the faces of the box"


def test_memo_on_hostile_inputs(pbe, cornell_normals):
    pb, rects, normals = cornell_normals
    mag, _, _ = R.debug_onb_table(pb)
    rnd = np.random.default_rng(8802)
    k = rnd.permutation(len(rects))[:2048]
    r0, n0 = rects[k], normals[k]
    cases_r, cases_n = [], []

    def add(r, n):
        cases_r.append(np.asarray(r, int)); cases_n.append(np.ascontiguousarray(n, np.float64))

    for axis in range(3):                                                   # one magnitude off by one ulp, either way
        for step in (1, -1):
            w = n0.copy().view(np.uint64)
            w[:, axis] = np.where((w[:, axis] & ~SIGN) == 0, w[:, axis] + np.uint64(1), (w[:, axis].astype(np.int64) + step).astype(np.uint64))
            add(r0, w.view(np.float64))
    for axis in range(3):                                                   # a NaN, an infinity
        for bad in (np.nan, -np.nan, np.inf):
            n = n0.copy(); n[:, axis] = bad
            add(r0, n)
    for s in range(8):                                                      # all eight sign variants, -0 components included: memo hits
        w = n0.copy().view(np.uint64) & ~SIGN
        for axis in range(3):
            if (s >> axis) & 1:
                w[:, axis] |= SIGN
        add(r0, w.view(np.float64))
    n_signs = 8 * len(r0)
    add(rnd.integers(0, len(mag), len(r0)), n0)                             # a valid normal presented with another rect's index
    invalid = np.flatnonzero(mag[:, 0] == INVALID)
    assert len(invalid) > 0
    add(rnd.choice(invalid, len(r0)), n0)                                   # an invalid rect
    add(rnd.choice(invalid, 64), np.full((64, 3), -np.nan))                 # ... with all-ones words
    add(rnd.choice(invalid, 64), np.full((64, 3), np.uint64(0x7FFFFFFFFFFFFFFF)).view(np.float64))
    add(r0, rnd.normal(size=n0.shape))                                      # any vector
    add(r0, n0 * 2.0)                                                       # the right direction, not a unit vector
    add(r0, np.zeros_like(n0))
    R_, N_ = np.concatenate(cases_r), np.concatenate(cases_n)
    hit = _check_pairs(pb, R_, N_, mag)
    start = 6 * len(r0) + 9 * len(r0)
    assert hit[start:start + n_signs].all(), "a sign variant of a valid normal missed"
    assert not hit[:start].any(), "an off-by-one-ulp magnitude or a non-finite component was a hit"
    assert not hit[start + n_signs + len(r0):].any(), "an invalid rect or a vector that is no normal of the rect was a hit"


def test_a_scene_without_entries_misses_everywhere(pbe, cornell_normals, monkeypatch):
    _, rects, normals = cornell_normals
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")
    b = _cornell(pbe)
    assert R.debug_onb_table(b)[2] == 0
    hit, v, u = R.debug_onb(b, rects[:4096], normals[:4096])
    assert not hit.any() and not v.any() and not u.any()


def _scene(pbe, which):
    if which == "cornell":
        return scenes.cornell_box(pbe)
    kind, seed = which.split("-")
    return _rand_box_room_scene(pbe, int(seed))[:3] if kind == "room" else _rand_list_scene(pbe, int(seed))


@pytest.mark.parametrize("which", ["cornell", "room-704", "room-705", "list-1", "list-5"])
def test_samples_with_the_table_are_the_arithmetics(pbe, which, monkeypatch):
    """rt_render_samples of the lean f64 kernel, 64 x 64 x 16, depth 50, with the table and with RT_NO_ONB_TABLE: 0 differing 64-bit words.
    The box rooms and the Cornell box have an entry for nearly every rect (waves of memo hits); the random list scenes mix the fused idiom
    with chains that have none, so their waves mix hits and misses and take the arithmetic."""
    W, H, spp, depth = 64, 64, 16, 50
    b, cam, bg = _scene(pbe, which)
    mag, _, n_valid = R.debug_onb_table(b)
    assert n_valid > 0
    if which.startswith("list"):
        assert n_valid < len(mag) - 1, "no rect without an entry: the waves of this scene never mix"
    _, with_table = R.render(b, cam, bg, W, H, spp, depth, seed=23, want_samples=True)
    assert R.last_loop_info(b)["kernel"] == "rt::pathtrace_kernel<double, 0u>", "not the lean f64 kernel"
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")
    b0, cam0, bg0 = _scene(pbe, which)
    assert R.debug_onb_table(b0)[2] == 0
    _, plain = R.render(b0, cam0, bg0, W, H, spp, depth, seed=23, want_samples=True)
    words = int((with_table.view(np.uint64) != plain.view(np.uint64)).sum())
    assert words == 0, f"{words} differing 64-bit words"

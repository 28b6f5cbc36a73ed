"""The ONB table's companion records as the flattener builds them (rt_ir.h DOnbW, rt_flatten.cpp build_onb_table; host only): per rect
record the magnitudes of w = normalized(n) (onb.rs:10) for the hit normal n that rect's owner produces.  The compact lean f64 kernel takes
w from them — these words with the sign bits of n — instead of normalising n on every Lambertian hit.  That is Lemma W (rt_kernel.hip,
above ring_w): the squares, the sum and the root of a normalisation do not see signs, and IEEE division is sign-symmetric.

Everything here is bit for bit.  The reference is the NumPy restatement below: one float64 operation per step, x*x + y*y + z*z in that
order, the square root, three divisions.  It is run on ALL EIGHT sign patterns of every entry's normal, so that the symmetry is shown and
not assumed: each pattern's |w| must be the stored words, and w's sign bits the pattern's.

Not vacuous: for the idiom at -18, 7 and -71 degrees the rotated normal's length is 0.9999999999999999 and w differs from n in bits (the
Cornell box's short box is the -18 degree case); at 15, 30, 45 and 60 degrees w == n.  Both facts are asserted on the NumPy side."""
import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from raytracinginrust_amd.api import Axis, Plane

from test_compact_ring_host import BOX_ROOM_SEEDS, _one_rect_scene, rotate_x
from test_fuzz_gpu import _rand_box_room_scene, _rand_list_scene
from test_onb_table_host import signed

INVALID = np.uint64(R.ONB_MAG_INVALID)
SIGN = np.uint64(0x8000000000000000)
MASK = np.uint64(0x7FFFFFFFFFFFFFFF)


def normalized_numpy(n):
    """vec.rs:56-58 as the kernels and the flattener write it: n (3,) float64 -> n / sqrt(n.x n.x + n.y n.y + n.z n.z), a rounding per step"""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        xx, yy, zz = n[0] * n[0], n[1] * n[1], n[2] * n[2]
        s = xx + yy
        s = s + zz
        l = np.sqrt(s)
        return np.array([n[0] / l, n[1] / l, n[2] / l], np.float64)


def angle_idiom(angle):
    return lambda b, h: b.Translate(b.Rotate(Axis.Y, h, angle), (1.0, 2.0, 3.0))


def check_w(b):
    """every valid entry's wmag is |normalized(n)| for each of the eight sign patterns of n, whose signs come through unchanged; an invalid
    entry's is all ones.  Returns (mag, wmag)."""
    mag, _, n_valid = R.debug_onb_table(b)
    wmag = R.debug_onb_table_w(b)
    assert wmag.shape == mag.shape
    valid = mag[:, 0] != INVALID
    assert int(valid.sum()) == n_valid
    assert (wmag[~valid] == INVALID).all(), "an invalid entry with a w"
    for i in np.flatnonzero(valid):
        assert not (wmag[i] & SIGN).any(), f"rect {i}: a w magnitude with its sign bit set"
        for s in range(8):
            n = signed(mag[i], s)
            w = normalized_numpy(n).view(np.uint64)
            assert ((w & MASK) == wmag[i]).all(), f"rect {i}, signs {s}: |normalized({n.tolist()})| = {(w & MASK).tolist()}, table {wmag[i].tolist()}"
            assert ((w & SIGN) == (n.view(np.uint64) & SIGN)).all(), f"rect {i}, signs {s}: normalising moved a sign bit"
    return mag, wmag


def test_cornell_box(pbe):
    mag, wmag = check_w(scenes.cornell_box(pbe)[0])
    assert int((mag[:, 0] != INVALID).sum()) == len(mag) - 2
    # the short box (records 6..11, -18 degrees): its side faces' normals are not of length one, and normalising them changes bits
    differs = (wmag[6:12] != mag[6:12]).any(axis=1)
    assert differs.any(), "no entry of the -18 degree box has wmag != mag: the test would not tell w from n"
    assert (wmag[:6] == mag[:6]).all(), "an axis vector is its own normalisation"


@pytest.mark.parametrize("seed", BOX_ROOM_SEEDS)
def test_box_rooms(pbe, seed):
    mag, _ = check_w(_rand_box_room_scene(pbe, seed)[0])
    assert (mag[:, 0] != INVALID).any()


@pytest.mark.parametrize("angle,same", [(-18.0, False), (7.0, False), (-71.0, False), (15.0, True), (30.0, True), (45.0, True), (60.0, True)])
def test_the_idiom_at_an_angle(pbe, angle, same):
    b = _one_rect_scene(pbe, angle_idiom(angle))
    mag, wmag = check_w(b)
    assert (mag[:, 0] != INVALID).all() and len(mag) == 2
    n = mag[1].view(np.float64)                                        # the rotated rect's |normal|: (|sin|, 0, |cos|)
    assert np.allclose(n, [abs(np.sin(np.radians(angle))), 0.0, abs(np.cos(np.radians(angle)))], rtol=1e-15, atol=0)
    length = float(np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]))
    if same:
        assert (wmag[1] == mag[1]).all(), f"{angle} degrees: w != n"
    else:
        assert length == 0.9999999999999999 and (wmag[1] != mag[1]).any(), f"{angle} degrees: length {length!r}, w == n"
    assert (wmag[0] == mag[0]).all()                                   # the bare floor


def test_invalid_entries_and_the_switch(pbe, monkeypatch):
    """a rect under RotateX has no entry and no w; a mixed scene's valid entries carry one; RT_NO_ONB_TABLE: none anywhere"""
    b = _one_rect_scene(pbe, rotate_x)
    mag, wmag = check_w(b)
    assert (mag[1] == INVALID).all() and (wmag[1] == INVALID).all() and (wmag[0] != INVALID).all()
    mag, wmag = check_w(_rand_list_scene(pbe, 1)[0])
    assert (mag[:, 0] == INVALID).any() and (mag[:, 0] != INVALID).any()
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")
    mag0, wmag0 = check_w(scenes.cornell_box(pbe)[0])
    assert (mag0 == INVALID).all() and (wmag0 == INVALID).all()

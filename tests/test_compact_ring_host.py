"""Which form of the first-hit ring a scene gets from the lean f64 kernels (csrc/rt_launch.h; rt_flatten.cpp HostFlat::onb_all; host only).

The compact record (80 B, 98 to a wave) leaves the hit normal out: the kernel rebuilds it from the rect's entry in the per-face ONB table
and three sign bits that ride in the record's rect word.  That is only right where every rect an object owns has a valid entry, so the
flattener decides: the Cornell box, the box rooms, a rect under the fused Translate(RotateY(..)) idiom get the compact ring; a rect under
another chain, a rect reachable through two chains, a chain three deep, a scene with a feature bit, RT_NO_ONB_TABLE, RT_NO_PRIMARY_PASS and
f32 keep the wide one (104 B, 76 to a wave) or have no ring at all.  Read through rt_debug_ring_form.

The pack and unpack of the three sign bits are restated in NumPy on all eight sign patterns, with +-0 components too: the word must keep
the rect index and the front-face bit, and the rebuilt normal must equal the original word for word."""
import os
import re

import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from raytracinginrust_amd.api import Axis, Plane, SceneBuilder
from test_fuzz_gpu import _rand_box_room_scene

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracinginrust_amd", "csrc", "rt_launch.h")


def _header_constant(name):
    with open(HDR) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, f.read(), re.M)
    assert m, name
    return int(m.group(1))


QN_C, FILL_C = _header_constant("RT_HIT_RING_QN_COMPACT"), _header_constant("RT_HIT_RING_FILL_AT_COMPACT")
QN_W, FILL_W = _header_constant("RT_HIT_RING_QN"), _header_constant("RT_HIT_RING_FILL_AT")
COMPACT = {"compact": True, "entries": QN_C, "entry_bytes": 80}
WIDE = {"compact": False, "entries": QN_W, "entry_bytes": 104}
NONE = {"compact": False, "entries": 0, "entry_bytes": 0}
BOX_ROOM_SEEDS = (3, 62)          # tests/test_shade_fill_gpu.py's and tests/test_onb_table_host.py's


def _one_rect_scene(be, wrap, extra=None):
    """a floor rect, bare, and one rect under `wrap`"""
    b = SceneBuilder(be)
    m = b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5)))
    w = b.HittableList()
    w.push(b.AARect(Plane.XZ, -50.0, 50.0, -50.0, 50.0, 0.0, m))
    w.push(wrap(b, b.AARect(Plane.XY, 0.0, 10.0, 0.0, 10.0, 5.0, m)))
    if extra:
        extra(b, w, m)
    b.set_scene(w, [])
    return b


def idiom(b, h):
    return b.Translate(b.Rotate(Axis.Y, h, 30.0), (1.0, 2.0, 3.0))


def rotate_x(b, h):
    return b.Translate(b.Rotate(Axis.X, h, 30.0), (1.0, 2.0, 3.0))


def three_deep(b, h):
    return b.FlipNormal(b.Translate(b.Rotate(Axis.Y, h, 30.0), (1.0, 2.0, 3.0)))


def two_chains_scene(be):
    b = SceneBuilder(be)
    m = b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5)))
    shared = b.AARect(Plane.XY, 0.0, 10.0, 0.0, 10.0, 5.0, m)
    w = b.HittableList()
    w.push(idiom(b, shared))
    w.push(b.FlipNormal(shared))
    b.set_scene(w, [])
    return b


def sphere_scene(be):
    return _one_rect_scene(be, idiom, lambda b, w, m: w.push(b.Sphere((0.0, 0.0, 5.0), 1.0, m)))


def test_the_constants_fit_five_workgroups_per_cu():
    """what the header's static_assert checks at compile time, on the committed constants: either form's four rings within 31 616 B, room
    for the 5120 B camera-path view of RT_NO_PRIMARY_PASS, and a pass that always finds room for a path"""
    for qn, nb, fill in ((QN_C, 80, FILL_C), (QN_W, 104, FILL_W)):
        assert qn * nb * 4 <= 31616 and qn * nb >= 64 * (7 * 8 + 6 * 4) and qn >= 64 and 1 <= fill <= qn
    assert (QN_W, FILL_W) == (76, 26)


@pytest.mark.parametrize("name,build", [("cornell", lambda be: scenes.cornell_box(be)[0]),
                                        ("box_room_3", lambda be: _rand_box_room_scene(be, BOX_ROOM_SEEDS[0])[0]),
                                        ("box_room_62", lambda be: _rand_box_room_scene(be, BOX_ROOM_SEEDS[1])[0]),
                                        ("idiom", lambda be: _one_rect_scene(be, idiom))])
def test_scenes_with_the_compact_ring(pbe, name, build):
    assert R.debug_ring_form(build(pbe)) == COMPACT


@pytest.mark.parametrize("name,build", [("rotate_x", lambda be: _one_rect_scene(be, rotate_x)), ("two_chains", two_chains_scene),
                                        ("three_deep", lambda be: _one_rect_scene(be, three_deep))])
def test_scenes_with_the_wide_ring(pbe, name, build):
    b = build(pbe)
    assert R.debug_ring_form(b) == WIDE
    mag, _, n_valid = R.debug_onb_table(b)
    assert n_valid < len(mag), "some rect of the scene has no entry: that is why"


def test_a_scene_with_a_sphere_has_no_ring(pbe):
    assert R.debug_ring_form(sphere_scene(pbe)) == NONE


def test_the_switches_give_the_wide_ring(pbe, monkeypatch):
    assert R.debug_ring_form(scenes.cornell_box(pbe)[0]) == COMPACT
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")                       # (read when the scene is flattened)
    assert R.debug_ring_form(scenes.cornell_box(pbe)[0]) == WIDE
    monkeypatch.delenv("RT_NO_ONB_TABLE")
    b = scenes.cornell_box(pbe)[0]
    monkeypatch.setenv("RT_NO_PRIMARY_PASS", "1")                    # (read at every launch)
    assert R.debug_ring_form(b) == WIDE
    monkeypatch.delenv("RT_NO_PRIMARY_PASS")
    assert R.debug_ring_form(b) == COMPACT
    assert R.debug_ring_form(b, R.RT_F32) == NONE


# ---- the record's rect word, restated: rect (28 bits) | sign(n.x) << 28 | sign(n.y) << 29 | sign(n.z) << 30 | front << 31
SIGN = np.uint64(0x8000000000000000)


def pack(rect, front, n):
    w = np.asarray(n, np.float64).view(np.uint64)
    return int(rect) | (int(front) << 31) | sum(int(w[k] >> np.uint64(63)) << (28 + k) for k in range(3))


def unpack(word, mag_words):
    n = np.array([mag_words[k] | (SIGN if (word >> (28 + k)) & 1 else np.uint64(0)) for k in range(3)], np.uint64).view(np.float64)
    return word & 0x0FFFFFFF, word >> 31, n


@pytest.mark.parametrize("mags", [(0.0, 1.0, 0.0), (np.sin(np.radians(18.0)), 0.0, np.cos(np.radians(18.0))), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0)])
def test_pack_and_unpack_on_all_sign_patterns(mags):
    mag_words = np.abs(np.array(mags, np.float64)).view(np.uint64)
    for s in range(8):
        n = np.array([mag_words[k] | (SIGN if (s >> k) & 1 else np.uint64(0)) for k in range(3)], np.uint64).view(np.float64)
        for rect in (0, 1, 17, 0x0FFFFFFF):
            for front in (0, 1):
                word = pack(rect, front, n)
                assert 0 <= word < 2 ** 32
                r2, f2, n2 = unpack(word, mag_words)
                assert (r2, f2) == (rect, front)
                assert (n2.view(np.uint64) == n.view(np.uint64)).all(), (s, n.tolist(), n2.tolist())       # -0.0 and +0.0 are different words

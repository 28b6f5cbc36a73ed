"""The per-face ONB memo of the lean f64 list-scene kernel as the flattener builds it (rt_flatten.cpp build_onb_table, rt_ir.h DOnbEntry;
host only).  One entry per rect record: the magnitudes |n| of the hit normal that rect's owner produces, and for each of the eight sign
combinations v and u of ONB::build_from_w (onb.rs:8-20).  Everything here is bit for bit.  The reference is the numpy f64 restatement of
onb.rs:8-20 below (numpy's sqrt and / are IEEE-correct, its * and + are separate roundings)."""

import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from raytracinginrust_amd.api import Axis, Plane, SceneBuilder
from test_fuzz_gpu import _rand_box_room_scene, _rand_list_scene

INVALID = np.uint64(R.ONB_MAG_INVALID)
SIGN = np.uint64(0x8000000000000000)


def onb_numpy(n):
    """onb.rs:8-20 as shade_hit's merged Lambertian arm writes it: n (..., 3) float64 -> (v, u), each (..., 3)"""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        x, y, z = n[..., 0], n[..., 1], n[..., 2]
        l = np.sqrt(x * x + y * y + z * z)
        w0, w1, w2 = x / l, y / l, z / l
        steep = np.abs(w0) > 0.9
        a0, a1, a2 = np.where(steep, 0.0, 1.0), np.where(steep, 1.0, 0.0), np.zeros_like(w0)
        c0, c1, c2 = w1 * a2 - w2 * a1, w2 * a0 - w0 * a2, w0 * a1 - w1 * a0
        lc = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
        v0, v1, v2 = c0 / lc, c1 / lc, c2 / lc
        u0, u1, u2 = w1 * v2 - w2 * v1, w2 * v0 - w0 * v2, w0 * v1 - w1 * v0
    return np.stack([v0, v1, v2], axis=-1), np.stack([u0, u1, u2], axis=-1)


def same_words(a, b):
    return np.ascontiguousarray(a, np.float64).view(np.uint64) == np.ascontiguousarray(b, np.float64).view(np.uint64)


def signed(mag_words, s):
    """the normal with magnitudes mag_words (3 uint64) and sign bits s = sx | sy << 1 | sz << 2"""
    w = np.array([mag_words[k] | (SIGN if (s >> k) & 1 else np.uint64(0)) for k in range(3)], np.uint64)
    return w.view(np.float64)


def check_slots(mag, slots):
    """every valid entry's eight slots are the numpy ONB of the sign-applied magnitudes, word for word; returns the number of valid entries"""
    valid = np.flatnonzero(mag[:, 0] != INVALID)
    for i in valid:
        assert not (mag[i] & SIGN).any(), f"rect {i}: a magnitude with its sign bit set"
        for s in range(8):
            v, u = onb_numpy(signed(mag[i], s))
            assert same_words(slots[i, s, 0], v).all() and same_words(slots[i, s, 1], u).all(), \
                f"rect {i}, signs {s}: v {slots[i, s, 0].tolist()} u {slots[i, s, 1].tolist()}, numpy v {v.tolist()} u {u.tolist()}"
    for i in np.flatnonzero(mag[:, 0] == INVALID):
        assert (mag[i] == INVALID).all()
    return len(valid)


def cornell_with_faces(be):
    """scenes.cornell_box (main.rs:278-311), and beside it — built, never pushed — every rect of it as a Hittable of its own under its
    owner's wrappers, in the order of the flattened rect records: the six bare items, then each Cube's faces in cube.rs:17-24 order.
    Hitting them one by one tells which rect record a world hit came from."""
    b = SceneBuilder(be)
    red, white, green = (b.Lambertian(b.ConstantTexture(c)) for c in ((0.65, 0.05, 0.05), (0.73, 0.73, 0.73), (0.12, 0.45, 0.15)))
    metal = b.Metal((0.8, 0.85, 0.88), 0.0)
    lamp = b.FlipNormal(b.AARect(Plane.XZ, 213.0, 343.0, 227.0, 332.0, 554.0, b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))))
    items = [b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 555.0, green), b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 0.0, red), lamp,
             b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white), b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white),
             b.AARect(Plane.XY, 0.0, 555.0, 0.0, 555.0, 555.0, white)]
    w = b.HittableList()
    for it in items:
        w.push(it)
    cubes = (((165.0, 165.0, 165.0), white, -18.0, (130.0, 0.0, 65.0)), ((165.0, 330.0, 165.0), metal, 15.0, (265.0, 0.0, 295.0)))
    faces = list(items)
    for mx, m, angle, off in cubes:
        w.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), mx, m), angle), off))
        for plane, a1, b1, k in ((Plane.XY, mx[0], mx[1], mx[2]), (Plane.XY, mx[0], mx[1], 0.0), (Plane.XZ, mx[0], mx[2], mx[1]),
                                 (Plane.XZ, mx[0], mx[2], 0.0), (Plane.YZ, mx[1], mx[2], mx[0]), (Plane.YZ, mx[1], mx[2], 0.0)):      # cube.rs:17-24
            faces.append(b.Translate(b.Rotate(Axis.Y, b.AARect(plane, 0.0, a1, 0.0, b1, k, m), angle), off))
    b.set_scene(w, [lamp])
    b.world_handle, b.box, b.faces = w, (np.zeros(3), np.full(3, 555.0)), faces
    return b


def plain_rays(rnd, mn, mx, n):
    """the first generation of tests/test_cube_division_only_gpu.py: from outside the open front into the box"""
    ext = mx - mn
    eye = mn + ext * np.array([0.5, 0.5, -1.45]) + rnd.normal(size=(n, 3)) * ext * 0.01
    tgt = mn + rnd.uniform(0.0, 1.0, (n, 3)) * ext
    return np.ascontiguousarray(np.concatenate([eye, (tgt - eye) * 10.0 ** rnd.uniform(-1, 1, (n, 1))], axis=1))


def bounce_rays(rnd, mn, mx, hit, pos):
    """its later generations: from the hit points (a miss starts again inside), random directions of random length"""
    n = len(hit)
    o = np.where(hit[:, None], pos, mn + rnd.uniform(0.05, 0.95, (n, 3)) * (mx - mn))
    return np.ascontiguousarray(np.concatenate([o, rnd.normal(size=(n, 3)) * 10.0 ** rnd.uniform(-1, 1, (n, 1))], axis=1))


def oracle_hits_with_rect(ob, rays):
    """per ray: (hit, position[3], normal[3], rect record) of the oracle's world.hit; the rect is the LAST of ob.faces whose own hit has
    the world's t bit for bit (HittableList::hit gives an exact tie to the later item, hit.rs:62-68)"""
    from oracle import orc
    out = np.zeros((len(rays), 8))
    for i, r in enumerate(rays):
        o, d = tuple(r[:3]), tuple(r[3:])
        h = orc.hit(ob, ob.world_handle, o, d, t_min=1e-5)
        if h is None:
            continue
        rect = -1
        for j, f in enumerate(ob.faces):
            hf = orc.hit(ob, f, o, d, t_min=1e-5)
            if hf is not None and np.float64(hf["t"]).view(np.uint64) == np.float64(h["t"]).view(np.uint64):
                rect = j
        out[i] = [1.0, *h["position"], *h["normal"][:3], rect]
    return out


def test_cornell_entries_are_the_numpy_onb(pbe):
    b = scenes.cornell_box(pbe)[0]
    mag, slots, n_valid = R.debug_onb_table(b)
    assert check_slots(mag, slots) == n_valid
    assert n_valid == len(mag) - 2, "every rect of the Cornell box but the room's two box records (never hit) has a valid entry"
    # the records the reference's list names: 6 bare items, then the two Cubes' faces; the lamp's and the walls' normals are axis vectors
    one = np.float64(1.0).view(np.uint64)
    assert [int(np.flatnonzero(m == one)[0]) for m in mag[:6]] == [0, 0, 1, 1, 1, 2] and all((np.sort(m) == [0, 0, one]).all() for m in mag[:6])
    # a rotated Cube's side faces carry |sin|, |cos| of its angle; its top and bottom stay (0, 1, 0)
    for first, angle in ((6, -18.0), (12, 15.0)):
        sn, cs = np.abs(np.sin(np.radians(angle))), np.abs(np.cos(np.radians(angle)))
        got = mag[first:first + 6].view(np.float64)
        assert np.allclose(got[0], [sn, 0, cs], rtol=1e-15, atol=0) and np.allclose(got[4], [cs, 0, sn], rtol=1e-15, atol=0) and (got[2] == [0, 1, 0]).all()
        assert (mag[first] == mag[first + 1]).all() and (mag[first + 2] == mag[first + 3]).all() and (mag[first + 4] == mag[first + 5]).all()


@pytest.mark.parametrize("seed", [2, 3])
def test_box_room_entries_are_the_numpy_onb(pbe, seed):
    b = _rand_box_room_scene(pbe, 60 + seed)[0]
    mag, slots, n_valid = R.debug_onb_table(b)
    assert check_slots(mag, slots) == n_valid and n_valid > 0


def _chains(b):
    """per rect record: the set of (n_ops, every wrapper a FlipNormal) of the objects that own it"""
    rows, _ = R.debug_object_rows(b)
    own = {}
    for geom_kind, first, count, _first_op, n_ops, _medium, _is_cube, nest in rows.tolist():
        if geom_kind == 0:
            for r in range(first, first + count):
                own.setdefault(r, set()).add((n_ops, bool(nest & 0x10000)))
    return own


@pytest.mark.parametrize("seed", [1, 5])
def test_random_list_scene_entries(pbe, seed, monkeypatch):
    """Mixed chains (tests/test_fuzz_gpu.py _rand_list_scene: the idiom, the idiom about another axis, the two the other way round, one, three
    and four wrappers): valid entries are the numpy ONB; a rect under no wrapper or FlipNormals only has an entry; a rect under one wrapper
    that is no FlipNormal, or under three or four, has none — both seeds hold such rects; and with RT_NO_ONB_TABLE no rect has one."""
    b = _rand_list_scene(pbe, seed)[0]
    mag, slots, n_valid = R.debug_onb_table(b)
    assert check_slots(mag, slots) == n_valid and n_valid > 0
    n_other = 0
    for r, chains in _chains(b).items():
        valid = mag[r, 0] != INVALID
        if all(n == 0 or flips for n, flips in chains):
            assert valid, f"rect {r} ({chains}) has no entry"
        if any(n not in (0, 2) and not flips for n, flips in chains):
            assert not valid, f"rect {r} ({chains}) has an entry"
            n_other += 1
    assert n_other > 0, "the seed has no rect under a chain that is not the fused idiom"
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")
    mag0, _, n_valid0 = R.debug_onb_table(_rand_list_scene(pbe, seed)[0])
    assert n_valid0 == 0 and (mag0 == INVALID).all() and len(mag0) == len(mag)


def test_which_chains_get_an_entry(pbe):
    """one rect under each shape: bare, FlipNormal, the fused idiom Translate(RotateY(..)) — an entry; the idiom about another axis, the two
    the other way round, three and four deep, and one rect reachable through two chains — none"""
    b = SceneBuilder(pbe)
    m = b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5)))

    def rect(k):
        return b.AARect(Plane.XY, 0.0, 10.0, 0.0, 10.0, float(k), m)

    shared = rect(20)
    shapes = [(rect(0), True), (b.FlipNormal(rect(1)), True), (b.Translate(b.Rotate(Axis.Y, rect(2), 30.0), (1.0, 2.0, 3.0)), True),
              (b.Translate(b.Rotate(Axis.X, rect(3), 30.0), (1.0, 2.0, 3.0)), False), (b.Rotate(Axis.Y, b.Translate(rect(4), (1.0, 2.0, 3.0)), 30.0), False),
              (b.FlipNormal(b.Translate(b.Rotate(Axis.Y, rect(5), 30.0), (1.0, 2.0, 3.0))), False),
              (b.Translate(b.Rotate(Axis.Y, b.Translate(b.Rotate(Axis.Y, rect(6), 10.0), (1.0, 0.0, 0.0)), 20.0), (0.0, 1.0, 0.0)), False),
              (b.Translate(b.Rotate(Axis.Y, shared, 30.0), (1.0, 2.0, 3.0)), False), (b.FlipNormal(shared), False)]
    w = b.HittableList()
    for h, _ in shapes:
        w.push(h)
    b.set_scene(w, [])
    mag, slots, n_valid = R.debug_onb_table(b)
    check_slots(mag, slots)
    rows, n_top = R.debug_object_rows(b)
    assert n_top == len(shapes)
    for (geom_kind, first, count, *_), (_, want) in zip(rows.tolist(), shapes):
        assert geom_kind == 0 and count == 1
        assert (mag[first, 0] != INVALID) == want, f"rect {first}: entry {'missing' if want else 'present'}"
    sn, cs = np.sin(np.radians(30.0)), np.cos(np.radians(30.0))
    assert np.allclose(mag[2].view(np.float64), [sn, 0.0, cs], rtol=1e-15, atol=0)


def test_a_scene_with_a_feature_bit_has_no_entry(pbe):
    b = SceneBuilder(pbe)
    w = b.HittableList()
    w.push(b.AARect(Plane.XY, 0.0, 10.0, 0.0, 10.0, 0.0, b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5)))))
    w.push(b.Sphere((0.0, 0.0, 5.0), 1.0, b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5)))))
    b.set_scene(w, [])
    assert R.debug_onb_table(b)[2] == 0


def test_oracle_normals_have_the_entrys_magnitudes(pbe, obe):
    """Rays that hit every face of the Cornell box — plain rays into the box, then two generations of bounces off the hit points, as
    tests/test_cube_division_only_gpu.py makes them —: the oracle's hit normal has |n| equal to the mag of the rect record it hit, for
    100 % of the hits (one rotation of a signed axis vector: the magnitudes are fixed), and every rect record is hit."""
    ob = cornell_with_faces(obe)
    pb = cornell_with_faces(pbe)
    mag, _, _ = R.debug_onb_table(pb)
    assert (mag == R.debug_onb_table(scenes.cornell_box(pbe)[0])[0]).all()
    rows, n_top = R.debug_object_rows(pb)
    ref_list = rows[n_top:].tolist()              # the world list as the reference has it, behind the list with the room
    assert [(o[1], o[2]) for o in ref_list] == [(0, 2), (2, 1), (3, 3), (6, 6), (12, 6)], ref_list
    rnd = np.random.default_rng(4242)
    mn, mx = ob.box
    rays = plain_rays(rnd, mn, mx, 64 * 12)
    seen, n_hits = set(), 0
    for generation in range(3):
        h = oracle_hits_with_rect(ob, rays)
        hit = h[:, 0] != 0.0
        rect = h[hit, 7].astype(int)
        assert (rect >= 0).all()
        absn = np.abs(h[hit, 4:7]).view(np.uint64)
        assert (mag[rect, 0] != INVALID).all()
        bad = (absn != mag[rect]).any(axis=1)
        assert not bad.any(), f"generation {generation}: {int(bad.sum())} of {len(rect)} hits, e.g. rect {rect[bad][0]} normal {h[hit, 4:7][bad][0].tolist()}"
        seen |= set(rect.tolist()); n_hits += len(rect)
        rays = bounce_rays(rnd, mn, mx, hit, h[:, 1:4])
    # (the floor hides the two Cubes' bottom faces, records 9 and 15; the lamp and every other record is hit)
    assert seen >= set(range(18)) - {9, 15}, sorted(seen)
    assert n_hits > 64 * 12 * 1.5

"""ConstantMedium::hit (medium.rs:27-61) per ray (shared by tests/test_medium_host.py and tests/test_medium_gpu.py): the scenes, their seeded
ray families, and a NumPy restatement of the medium's arithmetic that takes log(r) from the caller.

The restatement asks the oracle for what is NOT the medium's: the boundary's two raw hits (orc.hit_batch on the boundary handle with
(-f64::MAX, f64::MAX) and (t1 + 0.0001, f64::MAX)) and the records of opaque list items.  Everything between — the wrappers outside the
medium applied to the ray (translate.rs:23, rotate.rs:82-86) and to the record on the way back (translate.rs:24-28, rotate.rs:88-104), the
two clamps, t1 < t2, len = sqrt(x x + y y + z z), (t2 - t1) len, (-(1.0 / density)) log, <, t1 + hd / len, o + t d, and HittableList::hit's
walk (hit.rs:59-71) with the stream of Rng(SEED, k) advancing only where a medium draws — is one float64 NumPy operation per step, written
straight from the reference: one code path for every scene form, no case split by where a wrapper stands.

A scene is a list of item specs (SPECS): ("rect", ..) and ("ball", ..) opaque, each with a material of its own, and
("medium", shape, inner ops, outer ops, density) with ops outermost first.  Rays are made in the boundary's own frame and carried to the
world through the inverse wrappers (to AIM only: the rays are then what they are).  A medium's record can have t = -inf (a negative density with
len = 0) but never a NaN t with these densities: hd / len is NaN only for hd = +-inf with len = inf, or hd = 0 with len = 0, and hd = +inf (density
0, 5e-324) never passes hd < distance, hd = 0 needs log r = 0.  NaN and inf t come in from opaque items, as the closest hit so far.  Families, per target:
through — from outside through the boundary; inside — origin inside (t1 < 0, clamped to t_min); behind — the boundary wholly behind the
origin (t2 < t_min: no draw); graze — silhouettes of spheres (the offsets of primitive_cases.OFFSETS; the shortest chord f64 can express
there is about 1e-8 R) and edges of cubes, tetrahedra and rects at depths of 10^U(-12, -1) of the size to either side; thin — |d| scaled so
that the chord's width in t is 0.0001 (1 + j 2^-50), j in -8 .. 8, and 0.5, 1e-1, 1e-3, 1e-8 and 2, 16 times 0.0001; step (boxes) — from a
point ON a face straight to the opposite one, t1 = 0 exactly and t2 = 0.0001 + k ulp, k in -2 .. 2: the second hit is there for k >= 0; dscale — |d| from
1e-150 to 1e150, and 1e200 and 1e-200 (len = inf, len = 0); nonfinite — zero, -0, inf, NaN direction components, NaN and inf origins.
T_MINS are separate calls on all rays of a scene."""
import functools
import math

import numpy as np

import primitive_cases as P
from oracle import orc
from raytracinginrust_amd.api import Axis, Plane, Rng, SceneBuilder

T_MINS = (1e-5, 0.75, float("nan"))
SEED = 8080                      # ray k draws from Rng(SEED, k)
BG = (0.3, 0.4, 0.5)
F64_MAX = float(np.finfo(np.float64).max)
STEP = 0.0001                    # medium.rs:30
MAX_DRAWS = 5                    # a ray draws once per medium of the list at the most, and no list has more media
INF, NAN = float("inf"), float("nan")
DENSITIES = (0.3, 0.01, 5.0, 0.0, INF, -0.5, 1e-300, 1e300, 5e-324, NAN)
THIN_J = tuple(range(-8, 9))
THIN_OTHER = (0.5, 1e-1, 1e-3, 1e-8, 2.0, 16.0)
TIMES = (0.0, 0.5, 1.0)

same = P.same

# ---------------------------------------------------------------- shapes (in the boundary's own frame)
SPHERE = ("sphere", (0.3, -0.2, 0.5), 2.0)
CUBE = ("cube", (-1.5, -1.0, -2.0), (1.5, 1.25, 1.75))
TETRA_V = np.array([[-2.0, -1.5, -1.5], [2.0, -1.5, -1.25], [0.25, 2.0, -1.0], [0.0, -0.5, 2.25]])
TETRA = ("tetra",)
SLAB = ("slab", -2.0, 2.0, -1.5, 1.5, -0.5, 0.625)              # two XY rects over the same (x, y) ranges at z = k0 and z = k1
RECT = ("rect", -2.0, 2.0, -1.5, 1.5, 0.25)                     # one XY rect
MSPHERE = ("msphere", (0.0, 0.0, 0.0), (0.75, 0.25, -0.5), 0.0, 1.0, 1.75)
BVH_BALLS = ("bvh", (((-1.2, 0.0, 0.0), 1.0), ((0.0, 0.3, 0.2), 1.1), ((1.2, -0.2, 0.1), 0.9), ((0.2, 1.3, -0.3), 0.8), ((0.0, -1.2, 0.6), 0.7)))
SMALL_CUBE = ("cube", (-0.75, -1.5, -1.0), (2.25, 1.0, 1.25))
OFF_SPHERE = ("sphere", (1.0, 0.5, -0.5), 1.75)
# a list of a Cube and a Sphere: several objects, HittableList::hit over them.  The two hits of such a boundary are the first two surfaces
# along the line, whichever object's: with both behind the origin nothing is drawn.  "inside" origins lie about the last field, in the Cube only.
UNION = ("union", CUBE, ("sphere", (1.25, 0.5, 0.25), 1.5), (-1.0, 0.125, -0.25))


def frame_of(shape):
    """(centre, bounding radius, a radius about the centre that lies inside) of a shape"""
    k = shape[0]
    if k == "sphere":
        return np.array(shape[1]), shape[2], 0.9 * shape[2]
    if k == "cube":
        mn, mx = np.array(shape[1]), np.array(shape[2])
        return 0.5 * (mn + mx), float(np.sqrt((((mx - mn) * 0.5) ** 2).sum())), 0.45 * float((mx - mn).min())
    if k == "tetra":
        return TETRA_V.mean(axis=0), 2.6, 0.5
    if k == "union":
        return np.array([0.5, 0.25, 0.0]), 3.2, 0.4
    if k == "slab":
        return np.array([0.0, 0.0, 0.5 * (shape[5] + shape[6])]), 2.5, 0.45 * (shape[6] - shape[5])
    if k == "rect":
        return np.array([0.0, 0.0, shape[5]]), 2.5, 0.4
    if k == "msphere":
        return 0.5 * (np.array(shape[1]) + np.array(shape[2])), shape[5] + 0.5, 0.6 * shape[5]
    if k == "bvh":
        return np.array([0.1, 0.1, 0.1]), 2.4, 0.6
    raise KeyError(k)


def _edges(shape):
    """[(point on the edge, unit vector along it, its length, unit vector into the solid / into the rect)]"""
    k = shape[0]
    out = []
    if k == "union":
        return _edges(shape[1])
    if k == "cube":
        mn, mx = np.array(shape[1]), np.array(shape[2])
        for ax in range(3):
            a, b = [i for i in range(3) if i != ax]
            for sa in (0, 1):
                for sb in (0, 1):
                    p = mn.copy(); p[a] = (mn, mx)[sa][a]; p[b] = (mn, mx)[sb][b]
                    e = np.zeros(3); e[ax] = 1.0
                    m = np.zeros(3); m[a] = (1.0, -1.0)[sa]; m[b] = (1.0, -1.0)[sb]
                    out.append((p, e, mx[ax] - mn[ax], m / math.sqrt(2.0)))
    elif k == "tetra":
        c = TETRA_V.mean(axis=0)
        for i in range(4):
            for j in range(i + 1, 4):
                p, q = TETRA_V[i], TETRA_V[j]
                e = (q - p) / np.sqrt(((q - p) ** 2).sum())
                m = c - p; m = m - (m @ e) * e
                out.append((p, e, float(np.sqrt(((q - p) ** 2).sum())), m / np.sqrt((m * m).sum())))
    elif k in ("slab", "rect"):
        a0, a1, b0, b1 = shape[1:5]
        for z in shape[5:]:
            out += [(np.array([a0, b0, z]), np.array([1.0, 0.0, 0.0]), a1 - a0, np.array([0.0, 1.0, 0.0])),
                    (np.array([a0, b1, z]), np.array([1.0, 0.0, 0.0]), a1 - a0, np.array([0.0, -1.0, 0.0])),
                    (np.array([a0, b0, z]), np.array([0.0, 1.0, 0.0]), b1 - b0, np.array([1.0, 0.0, 0.0])),
                    (np.array([a1, b0, z]), np.array([0.0, 1.0, 0.0]), b1 - b0, np.array([-1.0, 0.0, 0.0]))]
    return out


# ---------------------------------------------------------------- scenes
def _m(shape, density=0.3, inner=(), outer=()):
    return ("medium", shape, tuple(inner), tuple(outer), density)


TR = ("translate", (0.75, -0.5, 1.25))
TR2 = ("translate", (-1.5, 0.25, 0.5))
# (angles at which |d| before and after the rotation differ as words on more than 30 % of a scene's rays — tests/test_medium_host.py; it
# is 20 to 34 % over the angles, lowest about z: x x + y y is rounded before z z is added)
ROT = {"x": ("rotate", Axis.X, 46.0), "y": ("rotate", Axis.Y, -40.0), "z": ("rotate", Axis.Z, -31.5)}
WRAPS = {"translate": (TR,), "rot_x": (ROT["x"],), "rot_y": (ROT["y"],), "rot_z": (ROT["z"],), "tr_roty": (TR2, ("rotate", Axis.Y, 63.0))}
CUT_RECT = ("rect", Plane.XY, -3.5, 3.5, -3.5, 3.5, 0.375)
BALL = ("ball", (0.5, 0.25, 0.25), 0.625)


def _spread(shapes_densities, inner=()):
    """media side by side, 9 apart along x: a ray aimed at one rarely meets another"""
    return [_m(sh, dn, inner=(("translate", (9.0 * (i - (len(shapes_densities) - 1) / 2.0), 0.0, 0.0)),) + tuple(inner)) for i, (sh, dn) in enumerate(shapes_densities)]


SPECS = {
    "sphere": [_m(SPHERE)], "cube": [_m(CUBE)], "tetra": [_m(TETRA)], "slab": [_m(SLAB)], "rect": [_m(RECT)], "msphere": [_m(MSPHERE)], "union": [_m(UNION)],
    "bvh_boundary": [_m(BVH_BALLS)],
    "densities_a": _spread([(SPHERE, 0.01), (CUBE, 5.0), (SPHERE, 0.0), (SPHERE, INF), (CUBE, -0.5)]),
    "densities_b": _spread([(CUBE, 1e-300), (SPHERE, 1e300), (CUBE, 5e-324), (SPHERE, NAN)]),
    "two_media": [_m(SPHERE), _m(SMALL_CUBE)],
    "three_media": [_m(SPHERE), _m(SMALL_CUBE), _m(OFF_SPHERE, 0.3)],
    "three_media_list": [_m(UNION), _m(SPHERE), _m(OFF_SPHERE)],
    "opaque_before": [CUT_RECT, _m(SPHERE), _m(SMALL_CUBE)],
    "opaque_between": [_m(SPHERE), CUT_RECT, _m(SMALL_CUBE)],
    "opaque_after": [_m(SPHERE), _m(SMALL_CUBE), CUT_RECT],
    "ball_between": [_m(SPHERE), BALL, _m(SMALL_CUBE)],
}
for _k, _w in WRAPS.items():
    SPECS["in_" + _k] = [_m(CUBE if "rot" in _k else SPHERE, inner=_w)]
    SPECS["out_" + _k] = [_m(CUBE if _k in ("translate", "rot_x", "tr_roty") else SPHERE, outer=_w)]
# a Rotate inside AND a Rotate outside the same medium: len belongs between them (object_hit_nested: after the ops outside, before those
# inside); and a medium with a Rotate inside and nothing outside (med_at = 0) beside a boundary list, which the F_NESTED kernel then serves
ROT_IN = ("rotate", Axis.X, 31.5)
SPECS["in_out_rot"] = [_m(CUBE, inner=(ROT_IN,), outer=(ROT["y"],))]
SPECS["in_out_tr_rot"] = [_m(SPHERE, inner=(TR, ROT_IN), outer=(TR2, ("rotate", Axis.Y, 63.0)))]
SPECS["union_in_rot"] = [_m(UNION, inner=(("translate", (-4.5, 0.0, 0.0)),)), _m(CUBE, inner=(("translate", (4.5, 0.0, 0.0)), ROT_IN))]
LIST_SCENES = tuple(SPECS)
# BVH forms (compared with the oracle's records): media as children of a BVH; media under wrappers as children of a BVH
_FILL = [("ball", (6.0 * math.cos(a), 5.0 + 0.5 * i, 6.0 * math.sin(a)), 0.5 + 0.05 * i) for i, a in enumerate(np.linspace(0.0, 5.5, 9))]
BVH_SPECS = {
    "bvh_media": _spread([(SPHERE, 0.3), (CUBE, 0.8), (OFF_SPHERE, 0.05)]) + _FILL,
    "bvh_wrapped": [_m(CUBE, 0.3, inner=(("translate", (-9.0, 0.0, 0.0)),), outer=(TR2, ("rotate", Axis.Y, 18.0))),
                    _m(SPHERE, 0.8, outer=(ROT["x"],)), _m(SMALL_CUBE, 0.2, inner=(("translate", (9.0, 0.0, 0.0)),), outer=(TR,))] + _FILL,
}
BVH_SCENES = tuple(BVH_SPECS)
SCENES = LIST_SCENES + BVH_SCENES
# the rt_query.hip instantiation a scene selects (primitive_cases.query_class): "all" object_hit's arm; "nested" object_hit_nested / boundary_hit
QUERY_CLASS = {s: "all" for s in SCENES}
QUERY_CLASS.update({s: "nested" for s in ("union", "three_media_list", "bvh_media", "bvh_wrapped", "in_out_rot", "in_out_tr_rot", "union_in_rot") + tuple("out_" + k for k in WRAPS)})
# scenes whose wrappers are translations by dyadic offsets or none: the step family's t1 is exactly 0 there
STEP_EXACT = ("cube", "slab", "union", "three_media_list", "out_translate", "densities_a", "densities_b")
STREAM_SCENES = ("two_media", "three_media", "three_media_list", "out_rot_y", "out_tr_roty", "union")
OUTER_ROTATED = tuple("out_" + k for k in ("rot_x", "rot_y", "rot_z", "tr_roty")) + ("in_out_rot", "in_out_tr_rot")
# (scene, item) of the F_NESTED scenes with a Rotate INSIDE the medium: |d| changes again between the medium and its boundary
INNER_ROTATED_NESTED = (("in_out_rot", 0), ("in_out_tr_rot", 0), ("union_in_rot", 1))
OVERLAPPING = ("two_media", "three_media", "three_media_list", "opaque_before", "opaque_between", "opaque_after", "ball_between")


def specs_of(name):
    return SPECS[name] if name in SPECS else BVH_SPECS[name]


class Scene:
    """A scene built on one backend: items[i] = {"spec", "h"[, "boundary"]}; things[material id] = the opaque item's index."""

    def __init__(self, name, be):
        self.name, self.b = name, SceneBuilder(be)
        b = self.b
        self.items, self.things = [], {}
        for i, spec in enumerate(specs_of(name)):
            item = {"spec": spec}
            if spec[0] == "medium":
                h = self._wrap(self._shape(spec[1], i), spec[2])
                item["boundary"] = h
                h = b.ConstantMedium(h, spec[4], b.ConstantTexture((0.9 - 0.1 * (i % 5), 0.85, 0.6 + 0.08 * (i % 5))))
                item["h"] = self._wrap(h, spec[3])
            elif spec[0] == "rect":
                item["h"] = b.AARect(*spec[1:], self._mat(i))
            else:
                item["h"] = b.Sphere(spec[1], spec[2], self._mat(i))
            self.items.append(item)
        if name in BVH_SPECS:
            self.world = b.BVH([it["h"] for it in self.items], 0.0, 1.0)
        else:
            self.world = b.HittableList()
            for it in self.items:
                self.world.push(it["h"])
        b.set_scene(self.world, [])

    def _mat(self, i):
        m = self.b.Lambertian(self.b.ConstantTexture((0.2 + 0.07 * (i % 9), 0.5, 0.8 - 0.06 * (i % 9))))
        self.things[m.id] = i
        return m

    def _wrap(self, h, ops):
        for op in reversed(ops):
            h = self.b.Translate(h, op[1]) if op[0] == "translate" else self.b.Rotate(op[1], h, op[2])
        return h

    def _shape(self, shape, i):
        b, k = self.b, shape[0]
        mat = self.b.Lambertian(self.b.ConstantTexture((0.5, 0.5, 0.5)))             # a boundary's material is never seen
        if k == "sphere":
            return b.Sphere(shape[1], shape[2], mat)
        if k == "cube":
            return b.Cube(shape[1], shape[2], mat)
        if k == "msphere":
            return b.MovingSphere(*shape[1:], mat)
        if k == "rect":
            return b.AARect(Plane.XY, *shape[1:], mat)
        if k == "bvh":
            return b.BVH([b.Sphere(c, r, mat) for c, r in shape[1]], 0.0, 1.0)
        lst = b.HittableList()
        if k == "union":
            lst.push(self._shape(shape[1], i)); lst.push(self._shape(shape[2], i))
        elif k == "tetra":
            for f in ((0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)):
                lst.push(b.Triangle([tuple(float(x) for x in TETRA_V[j]) for j in f], mat))
        else:
            for z in shape[5:]:
                lst.push(b.AARect(Plane.XY, *shape[1:5], z, mat))
        return lst


@functools.lru_cache(None)
def oracle_scene(name):
    return Scene(name, orc.load())


# ---------------------------------------------------------------- the wrappers restated
_AB = {Axis.X: (1, 2), Axis.Y: (0, 2), Axis.Z: (0, 1)}                      # rotate.rs:14-20


@functools.lru_cache(None)
def _sin_cos(angle):
    s, c = orc.sincos([(math.pi / 180.0) * angle])                           # rotate.rs:33-36
    return np.float64(s[0]), np.float64(c[0])


def op_forward(op, o, d):
    """the ray a wrapper hands to its child (translate.rs:23, rotate.rs:82-86): (n, 3) origins and directions -> new ones"""
    with np.errstate(all="ignore"):
        if op[0] == "translate":
            return o - np.array(op[1], np.float64), d
        a, b = _AB[op[1]]
        s, c = _sin_cos(op[2])
        o2, d2 = o.copy(), d.copy()
        o2[:, a] = c * o[:, a] - s * o[:, b]; o2[:, b] = s * o[:, a] + c * o[:, b]
        d2[:, a] = c * d[:, a] - s * d[:, b]; d2[:, b] = s * d[:, a] + c * d[:, b]
        return o2, d2


def op_back(op, child_d, p, n, front):
    """a child's record on its way up through a wrapper (translate.rs:24-28, rotate.rs:88-104 with hit.rs:34-41); child_d: the direction
    of the ray the wrapper handed down"""
    with np.errstate(all="ignore"):
        if op[0] == "translate":
            return p + np.array(op[1], np.float64), n, front
        a, b = _AB[op[1]]
        s, c = _sin_cos(op[2])
        p2, n2 = p.copy(), n.copy()
        p2[:, a] = c * p[:, a] + s * p[:, b]; p2[:, b] = (-s) * p[:, a] + c * p[:, b]
        n2[:, a] = c * n[:, a] + s * n[:, b]; n2[:, b] = (-s) * n[:, a] + c * n[:, b]
        front2 = (child_d[:, 0] * n2[:, 0] + child_d[:, 1] * n2[:, 1] + child_d[:, 2] * n2[:, 2]) < 0.0
        return p2, np.where(front2[:, None], n2, (-1.0) * n2), front2


def received(spec, rays):
    """(origins, directions) of the ray the medium of an item receives, and the directions each outer wrapper handed down (outermost first)"""
    o, d = rays[:, 0:3].copy(), rays[:, 3:6].copy()
    handed = []
    for op in spec[3]:
        o, d = op_forward(op, o, d)
        handed.append(d)
    return o, d, handed


def boundary_pair(sc, i, rays):
    """the boundary's two raw hits for the medium item i, from the oracle (medium.rs:29-30) -> (has1, t1, has2, t2, received o, d, handed)"""
    spec = sc.items[i]["spec"]
    o, d, handed = received(spec, rays)
    mr = np.concatenate([o, d, rays[:, 6:7]], axis=1)
    h1 = orc.hit_batch(sc.b, sc.items[i]["boundary"], mr, -F64_MAX, F64_MAX)
    with np.errstate(all="ignore"):
        h2 = orc.hit_batch(sc.b, sc.items[i]["boundary"], mr, h1[:, 1] + STEP, F64_MAX)
    return h1[:, 0] != 0.0, h1[:, 1], h2[:, 0] != 0.0, h2[:, 1], o, d, handed


def medium_hit(has1, t1, has2, t2, t_min, t_max, o, d, density, log_r):
    """medium.rs:31-55 for n rays -> (drew, hit, t, position, the clamped t1, hit_distance, distance_inside_boundary, len).  t_min: a
    number; t_max: (n,); log_r: (n,) log of the uniform each ray WOULD draw (read only where drew)."""
    with np.errstate(all="ignore"):
        t1 = np.where(t1 < t_min, t_min, t1)
        t2 = np.where(t2 > t_max, t_max, t2)
        drew = has1 & has2 & (t1 < t2)
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        inside = (t2 - t1) * ln
        hd = (-(np.float64(1.0) / np.float64(density))) * log_r
        hit = drew & (hd < inside)
        t = t1 + hd / ln
        p = o + t[:, None] * d
    return drew, hit, t, p, t1, hd, inside, ln


@functools.lru_cache(None)
def uniforms(n):
    """U[k, j]: draw j of Rng(SEED, k), k < n"""
    be = orc.load()
    out = np.zeros((n, MAX_DRAWS))
    for k in range(n):
        g = Rng(be, SEED, k)
        out[k] = [g.gen_f64() for _ in range(MAX_DRAWS)]
    out.setflags(write=False)
    return out


def glibc_log(n):
    return orc.libm("log", uniforms(n).reshape(-1)).reshape(n, MAX_DRAWS)


def restate(name, t_min, log_u, rays=None):
    """HittableList::hit (hit.rs:59-71) over the items of a LIST scene for all its rays with world.hit(ray, t_min, +inf): -> dict with
    rec (n, 16) in rt_query_hits' layout (object column = the item's index; the primitive columns -1; an opaque item's record as the
    oracle gives it), drew (n, items), and per medium item the intermediate numbers.  log_u: (n, MAX_DRAWS), the log of uniforms(n)."""
    sc = oracle_scene(name)
    rays = rays_of(name)[0] if rays is None else rays
    n = len(rays)
    U = uniforms(n)
    rec = np.zeros((n, 16)); rec[:, 11:15] = -1.0
    closest = np.full(n, INF)
    cursor = np.zeros(n, int)
    drew_all = np.zeros((n, len(sc.items)), bool)
    info = {}
    for i, item in enumerate(sc.items):
        spec = item["spec"]
        if spec[0] != "medium":
            r = orc.hit_batch(sc.b, item["h"], rays, t_min, closest)
            hit = r[:, 0] != 0.0
            r[:, 12] = float(i)
        else:
            has1, t1, has2, t2, o, d, handed = boundary_pair(sc, i, rays)
            lg = log_u[np.arange(n), np.minimum(cursor, MAX_DRAWS - 1)]
            drew, hit, t, p, t1c, hd, inside, ln = medium_hit(has1, t1, has2, t2, t_min, closest, o, d, spec[4], lg)
            assert not (drew & (cursor >= MAX_DRAWS)).any()
            nrm = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1)); front = np.zeros(n, bool)
            for op, cd in zip(reversed(spec[3]), reversed(handed)):
                p, nrm, front = op_back(op, cd, p, nrm, front)
            r = np.zeros((n, 16)); r[:, 11:15] = -1.0
            r[:, 0] = 1.0; r[:, 1] = t; r[:, 2:5] = p; r[:, 5:8] = nrm; r[:, 8] = front; r[:, 12] = float(i)
            info[i] = dict(has1=has1, t1=t1, has2=has2, t2=t2, drew=drew, hit=hit, t1c=t1c, hd=hd, inside=inside, len=ln, d=d, d_world=rays[:, 3:6],
                           closest_in=closest.copy(), u=U[np.arange(n), np.minimum(cursor, MAX_DRAWS - 1)], cursor=cursor.copy())
            drew_all[:, i] = drew
            cursor = cursor + drew
        rec[hit] = r[hit]
        closest = np.where(hit, r[:, 1], closest)
    return dict(rec=rec, drew=drew_all, info=info)


# ---------------------------------------------------------------- rays
def _to_world(ops, o, d):
    """rays of a child's frame carried out through wrappers (outermost first), approximately: to aim with"""
    for op in reversed(ops):
        if op[0] == "translate":
            o = o + np.array(op[1])
        else:
            a, b = _AB[op[1]]
            s, c = math.sin(math.radians(op[2])), math.cos(math.radians(op[2]))
            for v in (o, d):
                va, vb = v[:, a].copy(), v[:, b].copy()
                v[:, a] = c * va + s * vb; v[:, b] = -s * va + c * vb
    return o, d


def _local_families(rs, shape, n, n_thin=14):
    """{family: (origins, directions)} in the shape's own frame, about n rays each"""
    c, R, r_in = frame_of(shape)
    u = P._unit
    fam = {}
    o = c + (R * 10.0 ** rs.uniform(0.2, 1.0, n))[:, None] * u(rs.normal(size=(n, 3)))
    aim = c + (0.9 * R * rs.uniform(0.0, 1.0, n))[:, None] * u(rs.normal(size=(n, 3)))
    fam["through"] = (o, (aim - o) * (10.0 ** rs.uniform(-1.0, 1.0, n))[:, None])
    m = (4 * n) // 5
    fam["inside"] = ((np.array(shape[3]) if shape[0] == "union" else c) + (r_in * rs.uniform(0.0, 1.0, m))[:, None] * u(rs.normal(size=(m, 3))), rs.normal(size=(m, 3)) * (10.0 ** rs.uniform(-1.0, 1.0, m))[:, None])
    m = n // 3
    o = c + (R * rs.uniform(1.3, 4.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    aim = c + (0.7 * R * rs.uniform(0.0, 1.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    fam["behind"] = (o, (o - aim) * (10.0 ** rs.uniform(-1.0, 1.0, m))[:, None])
    m = (4 * n) // 5
    edges = _edges(shape)
    if edges:
        k = rs.randint(0, len(edges), m)
        p = np.array([edges[i][0] for i in k]); e = np.array([edges[i][1] for i in k]); ln = np.array([edges[i][2] for i in k]); inw = np.array([edges[i][3] for i in k])
        depth = R * 10.0 ** rs.uniform(-12.0, -1.0, m) * np.where(np.arange(m) % 4 == 3, -1.0, 1.0)
        q = p + (ln * rs.uniform(0.05, 0.95, m))[:, None] * e + depth[:, None] * inw
        g = np.cross(e, inw) * rs.choice([-1.0, 1.0], m)[:, None] + (0.2 * rs.uniform(-1.0, 1.0, m))[:, None] * e
        # (a chord of about 2 |depth|: |d| such that its width in t is 10^U(-0.5, 3) STEP — most second hits are then found)
        fam["graze"] = (q - (R * rs.uniform(0.5, 3.0, m))[:, None] * g, g * (2.0 * np.abs(depth) / (STEP * 10.0 ** rs.uniform(-0.5, 3.0, m)))[:, None])
    else:
        balls = {"sphere": lambda: [(shape[1], shape[2])], "msphere": lambda: [(shape[1], shape[5])], "bvh": lambda: list(shape[1])}[shape[0]]()
        parts = [P.fam_silhouette(rs, np.array(cc, np.float64), rr, m // len(balls) + 1)[0] for cc, rr in balls]
        r = np.concatenate(parts)[:m]
        fam["graze"] = (r[:, 0:3], u(r[:, 3:6]) * (10.0 ** rs.uniform(-7.0, 1.0, m))[:, None])
    m = (3 * n) // 4
    o = c + (R * rs.uniform(0.0, 3.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    aim = c + (0.8 * r_in * rs.uniform(0.0, 1.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    k = np.arange(m)
    # (t1 + 0.0001 == t1 from |t1| = 2^40 on, and a chord narrower than 0.0001 in t has no second hit: a medium is seen for |d| of about
    # 1e-10 .. 1e4 only, so half the family lies there)
    scale = np.where(k % 2 == 0, 10.0 ** rs.uniform(-150.0, 150.0, m), 10.0 ** rs.uniform(-13.0, 6.0, m))
    scale[k % 8 == 0] = 1e200
    scale[k % 8 == 2] = 1e-200
    d = u(aim - o) * scale[:, None]
    box = shape[1] if shape[0] == "union" else shape
    if box[0] == "cube":
        # |t| >= 2^40 absorbs the 0.0001 step (the second query finds the first face again: t2 == t1, nothing drawn), so len = 0 and a draw
        # meet only where t1 is exactly 0: origins ON a face, going in.  A negative density then gives t = t_min + hd / 0 = -inf.
        mn, mx = np.array(box[1]), np.array(box[2])
        for j in np.flatnonzero(k % 10 == 3):
            ax = int(j // 10) % 3
            o[j] = mn + (mx - mn) * rs.uniform(0.2, 0.8, 3); o[j, ax] = mn[ax]
            d[j] = u(rs.normal(size=3)) * 1e-200; d[j, ax] = abs(d[j, ax])
    fam["dscale"] = (o, d)
    m = n // 3
    o = c + (R * rs.uniform(0.0, 3.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    aim = c + (0.8 * r_in * rs.uniform(0.0, 1.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    d = (aim - o)
    k = np.arange(m)
    d[k % 8 == 0] = 0.0
    d[k % 8 == 1, 0] = 0.0
    d[k % 8 == 2, 1] = -0.0
    d[k % 8 == 3, 2] = INF
    d[k % 8 == 4, 0] = -INF
    d[k % 8 == 5, 1] = NAN
    o[k % 8 == 6, 2] = NAN
    o[k % 8 == 7, 0] = INF
    fam["nonfinite"] = (o, d)
    # bases of the thin family: from close by (|t1| of the order of the chord), unit directions
    m = n_thin * (len(THIN_J) + len(THIN_OTHER))
    o = c + (R * rs.uniform(1.1, 1.8, m))[:, None] * u(rs.normal(size=(m, 3)))
    aim = c + (0.6 * r_in * rs.uniform(0.0, 1.0, m))[:, None] * u(rs.normal(size=(m, 3)))
    fam["thin"] = (o, u(aim - o))
    # step: t1 exactly 0 and t2 = w / d within 2 ulp of 0.0001 — from a point ON one face of a box straight to the opposite face (the other
    # four planes are at +-inf), d found by scaling as primitive_cases.fam_tmin does.  The second query's t_min is then 0.0001 itself.
    span = {"cube": lambda: (shape[1], shape[2], (0, 1, 2), (2, 7)), "union": lambda: (shape[1][1], shape[1][2], (2,), (1, 3)),
            "slab": lambda: ((shape[1], shape[3], shape[5]), (shape[2], shape[4], shape[6]), (2,), (2, 7))}.get(shape[0])
    if span is not None:
        mn, mx, axes, eighths = span()
        mn, mx = np.array(mn, np.float64), np.array(mx, np.float64)
        rows, ks = [], []
        for turn in range(6 if len(axes) == 3 else 20):
            for ax in axes:
                w = mx[ax] - mn[ax]
                cand = w / STEP * (1.0 + np.arange(-40, 41) * 2.0 ** -53)
                got = P.ulps_from(w / cand, STEP)
                for kk in (-2, -1, 0, 1, 2):
                    j = np.flatnonzero(got == kk)
                    if not len(j):
                        continue
                    o = mn + (mx - mn) * rs.randint(eighths[0], eighths[1], 3) / 8.0           # (eighths of the widths: exact)
                    d = np.zeros(3)
                    o[ax], d[ax] = (mn[ax], cand[j[0]]) if turn % 2 == 0 else (mx[ax], -cand[j[0]])
                    rows.append(np.concatenate([o, d])); ks.append(float(kk))
        rows = np.array(rows)
        fam["step"] = (rows[:, 0:3], rows[:, 3:6], np.array(ks))
    return fam


N_PER_FAMILY = 560


@functools.lru_cache(None)
def rays_of(name):
    """(rays (n, 7), family per ray, the item each ray was aimed at, the thin family's aimed width in t over STEP, the step
    family's aimed distance of t2 from STEP in ulps — NaN elsewhere): n <= 4096"""
    sc = oracle_scene(name)
    rs = np.random.RandomState(9000 + SCENES.index(name))
    media = [i for i, it in enumerate(sc.items) if it["spec"][0] == "medium"]
    targets = media[:1] if name in OVERLAPPING else media
    parts = {}
    for i in targets:
        spec = sc.items[i]["spec"]
        for f, made in _local_families(rs, spec[1], max(N_PER_FAMILY // len(targets), 150), 14 if len(targets) == 1 else 6).items():
            o, d = _to_world(spec[3] + spec[2], made[0].copy(), made[1].copy())
            t = np.array(TIMES)[rs.randint(0, len(TIMES), len(o))] if spec[1][0] == "msphere" and f != "graze" else 0.0
            r = P._rays(o, d, t)
            w = np.full(len(r), NAN) if f != "step" else made[2]
            if f == "thin":
                r, w = _thin(sc, i, r)
            if len(r):
                parts.setdefault(f, []).append((r, np.full(len(r), i), w))
    order = ("through", "inside", "behind", "graze", "thin", "step", "dscale", "nonfinite")
    rays = np.concatenate([p[0] for f in order for p in parts.get(f, [])])
    fam = np.concatenate([np.full(len(p[0]), f, dtype=object) for f in order for p in parts.get(f, [])])
    aimed = np.concatenate([p[1] for f in order for p in parts.get(f, [])])
    width = np.concatenate([p[2] for f in order for p in parts.get(f, [])])
    assert len(rays) <= 4096, (name, len(rays))
    rays = np.ascontiguousarray(rays)
    rays.setflags(write=False)
    return rays, fam, aimed, width


def _thin(sc, i, base):
    """|d| of each base ray scaled so that the chord's width in t, t2 - t1 as the oracle's boundary gives them for the unit direction, becomes
    STEP (1 + j 2^-50) or STEP times a factor of THIN_OTHER (t scales inversely with |d|)"""
    has1, t1, has2, t2, *_ = boundary_pair(sc, i, base)
    with np.errstate(all="ignore"):
        ok = has1 & has2 & np.isfinite(t2 - t1) & (t2 - t1 > 1e-3)
    base, w0 = base[ok], (t2 - t1)[ok]
    k = np.arange(len(base)) % (len(THIN_J) + len(THIN_OTHER))
    width = np.where(k < len(THIN_J), STEP * (1.0 + (k - 8) * 2.0 ** -50), STEP * np.array(THIN_J + THIN_OTHER, np.float64)[k])
    out = base.copy()
    out[:, 3:6] = base[:, 3:6] * (w0 / width)[:, None]
    return out, width / STEP


def describe(name, bad, t_min=None):
    rays, fam = rays_of(name)[:2]
    idx = np.flatnonzero(bad)
    if not len(idx):
        return f"{name}: nothing differs"
    return f"{name} (t_min {t_min}): {len(idx)} rays differ, families {sorted(set(fam[idx]))}, first ray {int(idx[0])}: {rays[idx[0]].tolist()}"


@functools.lru_cache(None)
def oracle_world_hits(name, t_min):
    """world.hit(ray, t_min, +inf) of the oracle for every ray of a scene, ray k on Rng(SEED, k)"""
    sc = oracle_scene(name)
    rec = orc.hit_batch(sc.b, sc.world, rays_of(name)[0], t_min, INF, SEED)
    rec.setflags(write=False)
    return rec


def query_class(counts, rows, n_top):
    """primitive_cases.query_class, and a ConstantMedium under a wrapper (med_at, bits 8-15 of DObject::nest, not 0) selects F_NESTED too
    (rt_flatten.cpp emit_object)"""
    med_at = (rows[:, 7] >> 8) & 0xFF
    if ((rows[:, 5].astype(np.int32) >= 0) & (med_at != 0)).any():
        return "nested"
    return P.query_class(counts, len(rows), n_top, True)


def reach(res, t_min):
    """what the rays of one restated call reached, as masks over the rays, from the oracle's boundary hits and the restatement's numbers"""
    n = len(res["rec"])
    m = {k: np.zeros(n, bool) for k in ("drew", "hit", "lost", "found", "clamp_t_min", "clamp_closest", "before_t1", "len_inf", "len_zero")}
    with np.errstate(all="ignore"):
        for I in res["info"].values():
            m["drew"] |= I["drew"]
            m["hit"] |= I["hit"]
            m["lost"] |= I["has1"] & ~I["has2"]                       # the second boundary hit lost to the 0.0001 step (or never there)
            m["found"] |= I["has1"] & I["has2"]
            m["clamp_t_min"] |= I["drew"] & (I["t1"] < t_min)
            m["clamp_closest"] |= I["has1"] & I["has2"] & (I["t2"] > I["closest_in"])
            m["before_t1"] |= I["hit"] & (I["hd"] < 0.0)               # t < t1: a negative density
            m["len_inf"] |= I["has1"] & I["has2"] & np.isinf(I["len"])
            m["len_zero"] |= I["has1"] & I["has2"] & (I["len"] == 0.0)
    m["miss"] = m["drew"] & ~m["hit"]
    hit = res["rec"][:, 0] != 0.0
    m["nan_t"] = hit & np.isnan(res["rec"][:, 1])
    m["inf_t"] = hit & np.isinf(res["rec"][:, 1])
    return m


def world_centre(spec):
    """about where a medium item lies in the world, and its bounding radius"""
    c, R, _ = frame_of(spec[1])
    o, _ = _to_world(spec[3] + spec[2], c[None, :].copy(), np.zeros((1, 3)))
    return o[0], R


@functools.lru_cache(None)
def bvh_medium_terms(name):
    """For a BVH form, per ray whose oracle record (t_min = T_MINS[0]) is a medium's: the medium `item` and the draw j of the ray's stream
    for which the restated t1c + q, with glibc's log, IS the oracle's t (the tree decides in which order the media are visited), and
    that medium's t1c, q = hit_distance / len, hd, t2 and the direction it received; known — such a pair exists."""
    sc = oracle_scene(name)
    rays = rays_of(name)[0]
    n = len(rays)
    ref = oracle_world_hits(name, T_MINS[0])
    med = (ref[:, 0] != 0.0) & (ref[:, 11] < 0.0)
    media = [i for i, it in enumerate(sc.items) if it["spec"][0] == "medium"]
    lg = glibc_log(n)
    out = dict(item=np.zeros(n, int), known=np.zeros(n, bool), t1c=np.zeros(n), q=np.zeros(n), hd=np.zeros(n), d=np.zeros((n, 3)), t2=np.zeros(n))
    for i in media:
        has1, t1, has2, t2, o, d, _ = boundary_pair(sc, i, rays)
        for j in range(MAX_DRAWS):
            _, _, t, _, t1c, hd, _, ln = medium_hit(has1, t1, has2, t2, T_MINS[0], np.full(n, INF), o, d, sc.items[i]["spec"][4], lg[:, j])
            m = med & ~out["known"] & same(t, ref[:, 1]) & has1 & has2
            with np.errstate(all="ignore"):
                out["known"][m] = True; out["item"][m] = i; out["t1c"][m] = t1c[m]; out["q"][m] = (hd / ln)[m]; out["hd"][m] = hd[m]; out["d"][m] = d[m]; out["t2"][m] = t2[m]
    return out

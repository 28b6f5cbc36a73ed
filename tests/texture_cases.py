"""Textures, hostile (u, v, p) and exact branch decisions shared by tests/test_texture_walk_host.py (the oracle's side, no GPU) and
tests/test_texture_walk_gpu.py (the device's tex_eval, perlin_noise, perlin_turb, sat_index, sat_u64).

A DiffuseLight hit with front_face set returns Texture::mapping(u, v, p) verbatim as the emitted colour (mat.rs:395-401), so a synthetic
hit record hands the texture walk the caller's own u, v, p: one DiffuseLight per texture, records in rt_query_hits' layout.  Everything
is generated deterministically.  The small images give every texel a colour of its own — byte (i + 1, j + 1, 10 i + j) — so a colour
names the texel it came from."""
import ctypes as C
import functools

import mpmath
import numpy as np
from PIL import Image

from conftest import golden_path
from raytracinginrust_amd.api import Plane, Rng, SceneBuilder

MP_PREC = 160
SMALL_IMAGES = {"img1x1": (1, 1), "img2x2": (2, 2), "img3x5": (3, 5), "img7x1": (7, 1)}       # (width, height)
NOISE_SCALES = {"noise0.1": 0.1, "noise4": 4.0, "noise0": 0.0, "noise-1": -1.0}
CHAIN = 70                                                     # CheckTextures over one image, more than the flattener's old depth limit of 64
N_UNIFORM = 2000
PI = 3.14159265358979323846264338327950288
SIN_RANGE = 1e4                                                # |scale p.z| up to which DESIGN §6 measured the device's sin
CONSTS = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.9, 0.9, 0.1), (0.1, 0.9, 0.9), (0.5, 0.25, 0.125), (0.3, 0.6, 0.7)]


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """bit patterns, except that any NaN matches any NaN"""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def small_image(w, h):
    """(h, w, 3) bytes, row j from the top as texture.rs:113 indexes them: texel (i, j) = (i + 1, j + 1, 10 i + j)"""
    a = np.zeros((h, w, 3), np.uint8)
    for j in range(h):
        for i in range(w):
            a[j, i] = (i + 1, j + 1, 10 * i + j)
    return a


def texel_of(colour):
    """(i, j) of a small image's texel from its colour (n, 3)"""
    c = np.rint(np.asarray(colour) * 255.0).astype(np.int64)
    return c[:, 0] - 1, c[:, 1] - 1


def earth():
    im = Image.open(golden_path("earthmap_256x128.png")).convert("RGB")
    return im.tobytes(), im.width, im.height


def build(be):
    """-> (builder, {name: texture handle}, {name: DiffuseLight over that texture}).  Both builders number their handles alike (asserted
    by the tests)."""
    b = SceneBuilder(be)
    tex = {}
    for k, c in enumerate(CONSTS):
        tex[f"const{k}"] = b.ConstantTexture(c)
    for name, (w, h) in SMALL_IMAGES.items():
        tex[name] = b.ImageTexture(small_image(w, h).tobytes(), w, h)
    data, w, h = earth()
    tex["earth"] = b.ImageTexture(data, w, h)
    for k, (name, scale) in enumerate(NOISE_SCALES.items()):
        tex[name] = b.NoiseTexture(scale, Rng(be, 31, k))
    tex["check2"] = b.CheckTexture(tex["const0"], tex["const1"])
    tex["check_mixed"] = b.CheckTexture(tex["earth"], tex["noise4"])
    # three deep: the same p decides at every level, so only the all-odd and the all-even leaves are ever reached
    tex["check3"] = b.CheckTexture(b.CheckTexture(b.CheckTexture(tex["const2"], tex["const3"]), tex["const4"]),
                                   b.CheckTexture(tex["const5"], b.CheckTexture(tex["const0"], tex["const6"])))
    t = tex["img3x5"]
    for _ in range(CHAIN):
        t = b.CheckTexture(t, t)
    tex["chain"] = t
    mats = {name: b.DiffuseLight(h) for name, h in tex.items()}
    world = b.HittableList()
    world.push(b.AARect(Plane.XZ, -1.0, 1.0, -1.0, 1.0, 0.0, b.Lambertian(tex["const0"])))
    b.set_scene(world, [])
    return b, tex, mats


def records(mat, u, v, p):
    """(records (n, 16), rays (n, 7)) in rt_query_hits' layout: front_face 1, normal (0, 1, 0), the ray straight down onto p"""
    n = len(u)
    rec = np.zeros((n, 16)); rays = np.zeros((n, 7))
    rec[:, 0] = 1.0; rec[:, 1] = 1.0; rec[:, 2:5] = p; rec[:, 6] = 1.0; rec[:, 8] = 1.0; rec[:, 9] = u; rec[:, 10] = v; rec[:, 11] = mat
    rays[:, 0:3] = np.asarray(p) + (0.0, 1.0, 0.0); rays[:, 4] = -1.0
    return rec, rays


def oracle_values(ob, tex, u, v, p):
    """orc_texture_value per case -> (n, 3)"""
    lib = ob.b.lib
    out = np.zeros((len(u), 3))
    o3 = (C.c_double * 3)()
    for k in range(len(u)):
        lib.orc_texture_value(ob.h, int(tex), float(u[k]), float(v[k]), (C.c_double * 3)(*[float(x) for x in p[k]]), o3)
        out[k] = o3[:]
    return out


# ---------------------------------------------------------------- image lookups
def _near(x):
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


def _grid(n):
    """k / n exactly and one ulp to either side, k = 0 .. n"""
    return [y for k in range(n + 1) for y in _near(k / n)]


UV_SPECIAL = [0.0, -0.0, 1.0, float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0)), -2.0 ** -53, -5e-324, 5e-324, 2.0, -1.0, 0.5,
              float("nan"), float("inf"), float("-inf")]


@functools.lru_cache(None)
def image_cases(name):
    """(u, v, number of hostile cases at the front) for an image: the special values and every texel boundary k / w, k / h (+- 1 ulp) in
    all combinations — for the earth map the specials in all combinations and its 257 column boundaries against random v —, then N_UNIFORM
    uniform (u, v).  v's boundaries are where (1 - v) h is an integer: v = (h - k) / h, the same set."""
    rs = np.random.RandomState(9100 + len(name))
    if name == "earth":
        uu, vv = np.meshgrid(UV_SPECIAL, UV_SPECIAL, indexing="ij")
        gu = np.array(_grid(256)); gv = np.array(_grid(128))
        u = np.concatenate([uu.ravel(), gu, rs.uniform(0.0, 1.0, len(gv))])
        v = np.concatenate([vv.ravel(), rs.uniform(0.0, 1.0, len(gu)), gv])
    else:
        w, h = SMALL_IMAGES[name]
        uu, vv = np.meshgrid(UV_SPECIAL + _grid(w), UV_SPECIAL + _grid(h), indexing="ij")
        u, v = uu.ravel(), vv.ravel()
    n_hostile = len(u)
    u = np.concatenate([u, rs.uniform(0.0, 1.0, N_UNIFORM)]); v = np.concatenate([v, rs.uniform(0.0, 1.0, N_UNIFORM)])
    return u, v, n_hostile


def image_index(u, v, w, h):
    """texture.rs:105-116 in exact terms: clamp, times the size, `as usize` (NaN and negatives 0, saturating), the integer clamp"""
    def idx(x, n):
        if np.isnan(x):
            return 0
        x = min(max(x, 0.0), 1.0) * float(n)                   # one f64 rounding, as in the reference
        return min(int(x), n - 1)
    return np.array([idx(float(a), w) for a in u]), np.array([idx(1.0 - float(b), h) for b in v])


# ---------------------------------------------------------------- checker decisions
def _step(x, k):
    return float((np.array([x], np.float64).view(np.int64) + np.int64(k)).view(np.float64)[0])


@functools.lru_cache(None)
def checker_points():
    """p (n, 3): components at fl(k pi / 10) and 1, 2 ulp to either side of it — the zeros of sin(10 p) —, |k| <= 10^5, every case with at
    least one such component and the others such, ordinary, or tiny (+-0, denormals, 1e-300: about one case in a hundred, so that what has to
    be left out — the product of a tiny sine and one next to a zero underflows — stays under the cap)."""
    rs = np.random.RandomState(9201)
    ks = np.concatenate([np.arange(-20, 21), rs.randint(-100000, 100001, 400), [100000, -100000, 99999, -99999]])
    ks = ks[ks != 0]
    zeros = np.array([_step(float(k) * PI / 10.0, j) for k in ks for j in (-2, -1, 0, 1, 2)])
    n = len(zeros)
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.0 ** -1030, 1e-300, -1e-300])
    p = np.zeros((n, 3))
    for i in range(n):
        comp = [zeros[i]]
        for _ in range(2):
            r = rs.rand()
            comp.append(zeros[rs.randint(n)] if r < 0.5 else (tiny[rs.randint(len(tiny))] if r < 0.506 else rs.uniform(-600.0, 600.0)))
        p[i] = np.array(comp)[rs.permutation(3)]
    # and the tiny values together: the product of three such sines underflows
    extra = np.array([[a, 0.3, -0.7] for a in tiny] + [[1e-300, 1e-300, 0.3], [5e-324, 5e-324, 5e-324]])
    return np.concatenate([p, extra])


@functools.lru_cache(None)
def checker_decisions():
    """Per point of checker_points(): (odd, decided) — odd: the product of the three exact sines sin(fl(10 p_i)) is negative (mpmath, 160
    bits: a sin within 1.3 ulp keeps the sign of a non-zero sine); decided: False where an argument is +-0 or the f64 product of the
    three correctly rounded sines underflows to 0 — the only cases a test may leave out."""
    p = checker_points()
    odd = np.zeros(len(p), bool); decided = np.ones(len(p), bool)
    with mpmath.workprec(MP_PREC), np.errstate(all="ignore"):
        for i in range(len(p)):
            args = 10.0 * p[i]                                  # one f64 rounding each, as texture.rs:47 forms them
            if (args == 0.0).any():
                decided[i] = False
                continue
            s = [mpmath.sin(mpmath.mpf(float(a))) for a in args]
            prod = np.float64(float(s[0])) * np.float64(float(s[1])) * np.float64(float(s[2]))
            if prod == 0.0:
                decided[i] = False
                continue
            odd[i] = sum(1 for x in s if x < 0) % 2 == 1
    return odd, decided


# ---------------------------------------------------------------- noise
@functools.lru_cache(None)
def noise_points(scale):
    """p (n, 3) for a NoiseTexture of this scale: lattice points n / scale, negative coordinates (the reference's `as usize` takes them to
    index 0: quirk B10), +-0, components whose scaled value is 2^31, 2^32, 2^53, 2^63, 2^64, 1e300 and their neighbours, +-inf, NaN,
    and values that cross 2^32 or 2^64 within turb's seven doublings; ordinary points between them."""
    rs = np.random.RandomState(9300 + int(scale * 10) % 97)
    inv = 1.0 / scale if scale != 0.0 else 1.0
    xs = [float(k) for k in range(-6, 260, 7)] + [255.0, 256.0, 257.0, -1.0, -255.0, -256.0]                      # lattice points (scaled)
    big = [2.0 ** 31, 2.0 ** 32, 2.0 ** 53, 2.0 ** 63, 2.0 ** 64, 1e300]
    xs += [y for x in big for y in _near(x)] + [-x for x in big]
    xs += [2.0 ** (e - d) * f for e in (32, 64) for d in range(1, 8) for f in (1.0 - 2.0 ** -40, 1.0, 1.0 + 2.0 ** -40, 0.75)]
    xs += [0.0, -0.0, 5e-324, -5e-324, float("inf"), float("-inf"), float("nan")]
    xs = np.array(xs)
    hostile = xs * inv
    n = 3 * len(hostile)
    p = rs.uniform(-40.0, 40.0, (n, 3)) * inv
    for i in range(n):                                          # each hostile value on each axis once; a fifth of the cases get a second one
        p[i, i % 3] = hostile[i // 3]
        if rs.rand() < 0.2:
            p[i, (i + 1) % 3] = hostile[rs.randint(len(hostile))]
    plain = np.concatenate([rs.uniform(-40.0, 40.0, (300, 3)) * inv, rs.uniform(-1e4, 1e4, (100, 3)) * abs(inv)])
    return np.concatenate([p, plain])


def in_measured_sin_range(scale, p):
    """|scale p.z| <= 1e4: the final sin's argument lies where DESIGN §6 measured the device's sin (turb adds at most 20)"""
    with np.errstate(all="ignore"):
        return np.abs(scale * p[:, 2]) <= SIN_RANGE


@functools.lru_cache(None)
def large_sin_arguments():
    """3000 log-uniform arguments in [1e4, 1e300], both signs"""
    rs = np.random.RandomState(9400)
    return 10.0 ** rs.uniform(4.0, 300.0, 3000) * rs.choice([-1.0, 1.0], 3000)


def sin_ulp_errors(got, x):
    """|got - sin x| in ulps of the exact value (mpmath)"""
    out = np.zeros(len(x))
    with mpmath.workprec(1200):                                 # the reduction of 1e300 mod pi needs ~ 1000 bits
        for i in range(len(x)):
            ref = mpmath.sin(mpmath.mpf(float(x[i])))
            out[i] = float(abs(mpmath.mpf(float(got[i])) - ref) / mpmath.mpf(float(np.spacing(abs(float(ref))))))
    return out


# ---------------------------------------------------------------- an image behind a chain of checkers, on spheres
CHAIN_SPHERES = [((0.0, 0.0, 0.0), 1.0), ((2.5, 0.5, -1.0), 0.75), ((-2.0, -0.5, 1.5), 1.25), ((0.5, 2.5, 0.5), 0.5)]


def chain_scene(be, n_checkers):
    """Four spheres with one Lambertian over n_checkers CheckTextures over the earth map, both children of each the next one down (the
    image's texel whatever p) -> (builder, the top texture's handle, (width, height))."""
    b = SceneBuilder(be)
    data, w, h = earth()
    t = b.ImageTexture(data, w, h)
    for _ in range(n_checkers):
        t = b.CheckTexture(t, t)
    mat = b.Lambertian(t)
    world = b.HittableList()
    for c, r in CHAIN_SPHERES:
        world.push(b.Sphere(c, r, mat))
    b.set_scene(world, [])
    return b, t.id, (w, h)


@functools.lru_cache(None)
def chain_rays():
    """2048 rays from a shell of radius 8 at points inside the spheres"""
    rs = np.random.RandomState(9500)
    n = 2048
    o = rs.normal(size=(n, 3)); o *= 8.0 / np.sqrt((o * o).sum(1))[:, None]
    which = rs.randint(0, len(CHAIN_SPHERES), n)
    c = np.array([CHAIN_SPHERES[k][0] for k in which]); r = np.array([CHAIN_SPHERES[k][1] for k in which])
    aim = rs.normal(size=(n, 3)); aim *= (r * rs.uniform(0.0, 1.1, n) / np.sqrt((aim * aim).sum(1)))[:, None]
    rays = np.zeros((n, 7))
    rays[:, 0:3] = o; rays[:, 3:6] = c + aim - o
    rays.setflags(write=False)
    return rays

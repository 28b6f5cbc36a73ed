"""Argument sets, exact references and scenes shared by tests/test_shade_kat_host.py (the oracle's side, no GPU) and
tests/test_shade_kat_gpu.py (the device's): everything is generated deterministically, and a reference is computed once per process."""
import functools

import mpmath
import numpy as np

from raytracinginrust_amd.api import SceneBuilder

PI = 3.14159265358979323846264338327950288
MP_PREC = 160                      # bits of the mpmath references (>= 120)
N_RAND = 2000                      # random arguments per libm set
SAMPLE_RTOL = 1e-9                 # the project's per-sample bound, tests/test_parity_gpu.py: |got - ref| <= 1e-9 (1 + |ref|)
MARGIN = 1e-9                      # an input whose oracle margin is below this may be left out of the value comparison
MARGIN_CAP = 0.01                  # ... and at most this share of any set may be


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def step(x, k):
    """x moved by k ulps away from zero (k < 0: towards it); x finite and non-zero"""
    return float((np.array([x], np.float64).view(np.int64) + np.int64(k)).view(np.float64)[0])


def same_words(a, b):
    return words(a) == words(b)


def kinds(x):
    """0 NaN, 1 +inf, 2 -inf, 3 +0, 4 -0, 5 positive finite, 6 negative finite"""
    x = np.asarray(x, np.float64)
    neg = np.signbit(x)
    k = np.where(neg, 6, 5)
    k = np.where(x == 0.0, np.where(neg, 4, 3), k)
    k = np.where(np.isinf(x), np.where(neg, 2, 1), k)
    return np.where(np.isnan(x), 0, k)


# ---------------------------------------------------------------- sincos_0_2pi
@functools.lru_cache(None)
def r1_set():
    """r1 of phi = 2 pi r1: 0, the two ends, k/8 +- {0..3} ulp (the rint ties and the quadrant changes), 8000 random multiples of 2^-53"""
    edge = [0.0, 2.0 ** -53, 1.0 - 2.0 ** -53] + [step(k / 8.0, j) for k in range(1, 8) for j in range(-3, 4)]
    rnd = np.random.default_rng(7001).integers(0, 2 ** 53, 8000).astype(np.float64) * 2.0 ** -53
    return np.concatenate([np.array(edge), rnd]), len(edge)


# ---------------------------------------------------------------- the libm functions on the kernel's own domains
@functools.lru_cache(None)
def libm_sets():
    """name -> (function, a, b or None).  The domains are those of rt_kernel.hip's call sites."""
    r = np.random.default_rng(7101)
    N = N_RAND
    s = {}
    checker = 10.0 * np.concatenate([r.uniform(-1e4, 1e4, N), r.uniform(-600.0, 600.0, N // 2), [0.0, -0.0, 1e4, -1e4, 555.0, 1e-300]])   # texture.rs:45-54: sin(10 p)
    phi_edges = [v for c in (-0.5 * PI, 0.5 * PI, PI, 1.5 * PI) for v in (step(c, -2), step(c, -1), c, step(c, 1), step(c, 2))] + [0.0, -0.0]
    phi = np.concatenate([r.uniform(-0.5 * PI, 1.5 * PI, N), phi_edges])                 # pdf.rs:38-60: atan(..) (+ pi)
    for f in ("sin", "cos"):
        s[f + " 10p"] = (f, checker, None)
        s[f + " phi"] = (f, phi, None)
    r2 = np.concatenate([r.integers(0, 2 ** 53, N).astype(np.float64) * 2.0 ** -53, [0.0, 2.0 ** -53, 2.0 ** -52, 3 * 2.0 ** -53, 1.0 - 2.0 ** -53],
                         [step(v, j) for v in (0.25, 0.5, 0.75) for j in range(-3, 4)]])
    s["tan 2pi r2 + pi/2"] = ("tan", 2.0 * PI * r2 + 0.5 * PI, None)                     # pdf.rs:47
    mag = np.ldexp(r.uniform(1.0, 2.0, N), r.integers(-1074, 1024, N).astype(np.int32)) * r.choice([-1.0, 1.0], N)
    s["atan all magnitudes"] = ("atan", np.concatenate([mag, [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 5e-324, -5e-324, 1.7976931348623157e308]]), None)
    v = r.normal(size=(N, 3))
    v /= np.sqrt((v * v).sum(1))[:, None]
    z0 = [(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324)] + [(a, b) for a in (1.0, -1.0, 5e-324, -5e-324) for b in (0.0, -0.0)]
    s["atan2(-z, x)"] = ("atan2", np.concatenate([-v[:, 2], [p[0] for p in z0]]), np.concatenate([v[:, 0], [p[1] for p in z0]]))   # sphere.rs:11-25
    near1 = [1.0 - 2.0 ** -k for k in range(1, 54)] + [step(1.0, -j) for j in (1, 2, 3)]
    s["acos [-1, 1]"] = ("acos", np.concatenate([r.uniform(-1.0, 1.0, N), near1, [-x for x in near1], [1.0, -1.0, 0.0, -0.0, step(1.0, 1), -step(1.0, 1)]]), None)
    s["log [0, 1)"] = ("log", np.concatenate([r.random(N), r.integers(1, 2 ** 53, N // 2).astype(np.float64) * 2.0 ** -53 * 2.0 ** -r.integers(0, 60, N // 2).astype(np.float64),
                                              [0.0, 5e-324, 1e-310, 2.0 ** -1022, step(1.0, -1), 0.5]]), None)            # medium.rs:42
    gl = np.concatenate([r.random(N), [0.0, 1.0, 0.5]])
    a = 0.1 * (1.0 - gl) + 0.001 * gl                                                    # mixf(0.1, 0.001, clearcoat_gloss)
    s["log2 [1e-6, 1e-2]"] = ("log2", np.concatenate([np.exp(r.uniform(np.log(1e-6), np.log(1e-2), N)), a * a, [1e-6, 1e-2]]), None)   # mat.rs:16-24
    x22 = np.concatenate([r.uniform(0.0, 4.0, N), r.random(N // 2) ** 8, [0.0, -0.0, -1.0, -0.5, -5e-324, 1.0, 4.0, 1e-300, 5e-324, step(1.0, 1), step(1.0, -1)]])
    s["pow(x, 2.2)"] = ("pow", x22, np.full(len(x22), 2.2))                              # mat.rs:46-48
    r1 = np.concatenate([r.integers(0, 2 ** 53, len(a) - 2).astype(np.float64) * 2.0 ** -53, [0.0, 1.0 - 2.0 ** -53]])
    s["pow(a^2, 1 - r1)"] = ("pow", a * a, 1.0 - r1)                                     # pdf.rs:27-29
    return s


_MP = {"sin": mpmath.sin, "cos": mpmath.cos, "tan": mpmath.tan, "atan": mpmath.atan, "atan2": mpmath.atan2, "acos": mpmath.acos,
       "log": mpmath.log, "log2": lambda x: mpmath.log(x, 2), "pow": mpmath.power}


def _exact(fn, a, b):
    """the function's exact values (mpf) where arguments and value are finite reals and the value is not zero, else None"""
    f = _MP[fn]
    out = []
    with mpmath.workprec(MP_PREC):
        for i in range(len(a)):
            args = (a[i],) if b is None else (a[i], b[i])
            if not all(np.isfinite(x) for x in args):
                out.append(None)
                continue
            if (fn in ("log", "log2") and a[i] <= 0.0) or (fn == "acos" and abs(a[i]) > 1.0) or (fn == "pow" and a[i] <= 0.0) or \
                    (fn == "atan2" and a[i] == 0.0):      # (a zero y: the result's sign is the zero's, which mpmath does not keep — compared by kind)
                out.append(None)
                continue
            v = f(*[mpmath.mpf(float(x)) for x in args])
            out.append(v if v != 0 else None)
    return out


@functools.lru_cache(None)
def libm_exact(name):
    fn, a, b = libm_sets()[name]
    return _exact(fn, a, b)


def ulp_errors(got, exact):
    """|got - exact| in units of the spacing of doubles at the exact value; NaN where there is no finite non-zero exact value or got
    is not finite"""
    out = np.full(len(got), np.nan)
    with mpmath.workprec(MP_PREC):
        for i, ref in enumerate(exact):
            if ref is None or not np.isfinite(got[i]):
                continue
            r = float(ref)
            u = np.spacing(abs(r)) if np.isfinite(r) and r != 0.0 else 5e-324
            out[i] = float(abs(mpmath.mpf(float(got[i])) - ref) / mpmath.mpf(float(u)))
    return out


def max_ulp(got, exact):
    e = ulp_errors(got, exact)
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


# ---------------------------------------------------------------- Vec3 / f64
@functools.lru_cache(None)
def div_cases():
    """(numerators (n, 3), denominators (n,), want_shared (n,): 1 the shared-denominator form is required, 0 the plain one, -1 either)"""
    r = np.random.default_rng(7201)
    n_rand = 8000
    a = r.normal(size=(n_rand, 3)) * np.ldexp(1.0, r.integers(-30, 31, (n_rand, 3)).astype(np.int32))
    d = r.normal(size=n_rand) * np.ldexp(1.0, r.integers(-30, 31, n_rand).astype(np.int32))
    want = np.ones(n_rand, np.int64)                                    # ordinary operands: no v_div_scale rescales
    E = [s * 2.0 ** e for e in (1022, -1022, 1000, -1000, 900, -900) for s in (1.0, -1.0)]
    ea, ed = [], []
    for i, den in enumerate(E):                                         # the ends of the exponent range, numerators and denominators
        for j, num in enumerate(E):
            ea.append((num, E[(i + j) % len(E)] * 0.75, 1.5)); ed.append(den)
            ea.append((num, num * 0.5, num * 0.25)); ed.append(den)
    fa, fd = [], []
    for den in (2.0 ** 100, 3.0, -7.0 * 2.0 ** -200, 2.0 ** 200, 1.0):  # the numerators far apart: one 768 or more binades above the denominator, one ordinary
        hi = den * 2.0 ** 800
        for perm in ((hi, den * 3.0, den * 0.3), (den * 5.0, hi, -den), (den, den * 1.25, -hi)):
            fa.append(perm); fd.append(den)
    sp = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-310, 2.0 ** -1022, 1.7976931348623157e308]
    sa, sd = [], []
    for x in sp:
        for y in sp:
            sa.append((x, 1.0, -2.5)); sd.append(y)
            sa.append((3.0, y, x)); sd.append(7.0)
    A = np.concatenate([a, np.array(ea), np.array(fa), np.array(sa)])
    D = np.concatenate([d, np.array(ed), np.array(fd), np.array(sd)])
    W = np.concatenate([want, -np.ones(len(ea), np.int64), np.zeros(len(fa), np.int64), -np.ones(len(sa), np.int64)])
    # mixed within a wave: the special records go between the ordinary ones
    perm = np.random.default_rng(7202).permutation(len(D))
    return A[perm], D[perm], W[perm]


# ---------------------------------------------------------------- onb_from_w and the BRDF helpers
@functools.lru_cache(None)
def onb_normals():
    r = np.random.default_rng(7301)
    v = r.normal(size=(1500, 3))
    unit = v / np.sqrt((v * v).sum(1))[:, None]
    scaled = v * np.ldexp(1.0, r.integers(-40, 41, (1500, 1)).astype(np.int32))
    edge = []
    for j in range(-8, 9):                                              # |w.x| at 0.9 +- ulps (onb.rs:12), both signs, unit and not
        x = step(0.9, j)
        for sg in (1.0, -1.0):
            y = np.sqrt(1.0 - x * x)
            edge += [(sg * x, y, 0.0), (sg * x, 0.0, -y), (sg * x * 4.0, y * 4.0, 0.0), (sg * x, y * np.sqrt(0.5), y * np.sqrt(0.5))]
    axes = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.9, 0.0, 0.0), (-0.0, 0.0, 2.0)]
    return np.concatenate([unit, scaled, np.array(edge), np.array(axes)])


@functools.lru_cache(None)
def helper_cases():
    """operands of GTR_1, GTR_2_aniso, smithG_GGX, smithG_GGX_aniso, schlick_fresnel"""
    r = np.random.default_rng(7302)
    N = 3000
    c = {}
    gl = r.random(N)
    a = np.concatenate([0.1 * (1.0 - gl) + 0.001 * gl, [step(1.0, -1), 1.0, step(1.0, 1), 2.0, 0.1, 0.001, 0.5]])
    c["GTR_1"] = (np.concatenate([r.uniform(-1.0, 1.0, N), [0.0, 1.0, 1.0, 0.5, 1.0, 0.0, -1.0]]), a)
    ax = np.concatenate([r.uniform(0.001, 1.0, N - 4), [0.001, 0.001, 1.0, 0.31622776601683794]])
    ay = np.concatenate([r.uniform(0.001, 1.0, N - 4), [0.001, 1.0, 0.001, 3.1622776601683795]])
    c["GTR_2_aniso"] = (r.uniform(-1.0, 1.0, (N, 3)), np.stack([ax, ay], 1))
    c["smithG_GGX_aniso"] = (np.concatenate([r.uniform(-1.0, 1.0, (N - 2, 3)), [[0.0, 0.0, 0.0], [1e-12, 1.0, 0.0]]]), np.stack([ax, ay], 1))
    c["smithG_GGX"] = (np.concatenate([r.uniform(-1.0, 1.0, N), [0.0, 1e-12, 1.0, -0.0]]), np.concatenate([np.full(N, 0.25), [0.25, 0.25, 0.0, 1.0]]))
    c["schlick_fresnel"] = (np.concatenate([r.uniform(-0.5, 1.5, N), [0.0, 1.0, -0.0, np.nan, np.inf, -np.inf, 1e-300, step(1.0, -1)]]), None)
    return c


def np_helper(name, a, b):
    """the helper restated in NumPy: + - * / sqrt, each rounded once (log2 through `log2`, the caller's)"""
    with np.errstate(all="ignore"):
        if name == "schlick_fresnel":
            m = 1.0 - a
            m = np.where(m < 0.0, 0.0, np.where(m > 1.0, 1.0, m))       # f64::clamp: NaN stays
            m2 = m * m
            return m2 * m2 * m
        if name == "GTR_2_aniso":
            p, q = a[:, 1] / b[:, 0], a[:, 2] / b[:, 1]
            s = p * p + q * q + a[:, 0] * a[:, 0]
            return 1.0 / (PI * b[:, 0] * b[:, 1] * (s * s))
        if name == "smithG_GGX":
            aa, bb = b * b, a * a
            return 1.0 / (a + np.sqrt(aa + bb - aa * bb))
        if name == "smithG_GGX_aniso":
            p, q = a[:, 1] * b[:, 0], a[:, 2] * b[:, 1]
            return 1.0 / (a[:, 0] + np.sqrt(p * p + q * q + a[:, 0] * a[:, 0]))
    raise KeyError(name)


# ---------------------------------------------------------------- the principled material's parameter sets and the scenes
def pbr_sets():
    """(ten parameters, base colour): a middle set, each parameter at 0 and at 1, and the corners the issue names"""
    mid = [0.5] * 10
    base = (0.8, 0.6, 0.4)
    sets = [(tuple(mid), base)]
    for k in range(10):
        for v in (0.0, 1.0):
            p = list(mid); p[k] = v
            sets.append((tuple(p), base))
    rough0 = list(mid); rough0[3] = 0.0; rough0[5] = 1.0               # roughness 0 with anisotropic 1: both 0.001 clamps of ax, ay
    sets.append((tuple(rough0), base))
    sets.append((tuple(mid), (0.0, 0.0, 0.0)))                          # black base colour: cd_lum <= 0
    sets.append((tuple(mid), (1.5, 1.2, 1.1)))                          # base > 1 from a light-coloured texture
    sets.append(((0.0,) * 10, base))
    sets.append(((1.0,) * 10, (1.0, 1.0, 1.0)))
    gloss1 = list(mid); gloss1[9] = 1.0; gloss1[8] = 1.0
    sets.append((tuple(gloss1), (0.2, 0.9, 0.1)))
    return sets


LIGHT_RECT = (1, 213.0, 343.0, 227.0, 332.0, 554.0)                     # Plane.XZ
LIGHT_SPHERE = ((400.0, 300.0, 150.0), 45.0)


def list_scene(be, lights):
    """A LIST scene (no feature bit: the lean kernels' class): Lambertian and Metal walls, a Cube, a rect light.  lights: "none" | "rect"."""
    b = SceneBuilder(be)
    m = {"lam": b.Lambertian(b.ConstantTexture((0.73, 0.73, 0.73))), "lam2": b.Lambertian(b.ConstantTexture((0.12, 0.45, 0.15))),
         "metal": b.Metal((0.8, 0.85, 0.88), 0.3), "mirror": b.Metal((0.9, 0.6, 0.2), 0.0), "light": b.DiffuseLight(b.ConstantTexture((15.0, 14.0, 13.0)))}
    w = b.HittableList()
    light = b.AARect(*LIGHT_RECT, m["light"])
    for h in (b.AARect(1, 0.0, 555.0, 0.0, 555.0, 0.0, m["lam"]), b.AARect(0, 0.0, 555.0, 0.0, 555.0, 555.0, m["lam2"]),
              b.AARect(2, 0.0, 555.0, 0.0, 555.0, 555.0, m["metal"]), b.AARect(2, 0.0, 555.0, 0.0, 555.0, 0.0, m["mirror"]), b.FlipNormal(light),
              b.Cube((130.0, 0.0, 65.0), (295.0, 165.0, 230.0), m["lam"])):
        w.push(h)
    b.set_scene(w, [light] if lights == "rect" else [])
    return b, m


def full_scene(be, lights):
    """One material per kind and every PBR parameter set.  lights: "none" | "rect" | "sphere" | "nested" (both, in a list inside `lights`)."""
    b = SceneBuilder(be)
    white = b.ConstantTexture((0.73, 0.73, 0.73))
    m = {"lam": b.Lambertian(white), "metal": b.Metal((0.8, 0.85, 0.88), 0.3), "mirror": b.Metal((0.9, 0.6, 0.2), 0.0), "glass": b.Dielectric(1.5),
         "glass1": b.Dielectric(1.0), "light": b.DiffuseLight(b.ConstantTexture((15.0, 14.0, 13.0))), "iso": b.Isotropic(b.ConstantTexture((0.3, 0.5, 0.7)))}
    m["pbr"] = [b.PBR(b.ConstantTexture(base), *p) for p, base in pbr_sets()]
    w = b.HittableList()
    lr = b.AARect(*LIGHT_RECT, m["light"])
    ls = b.Sphere(*LIGHT_SPHERE, m["light"])
    for h in (b.AARect(1, 0.0, 555.0, 0.0, 555.0, 0.0, m["lam"]), b.AARect(0, 0.0, 555.0, 0.0, 555.0, 555.0, m["pbr"][0]), b.FlipNormal(lr), ls,
              b.Sphere((150.0, 80.0, 150.0), 80.0, m["metal"]), b.Sphere((300.0, 80.0, 380.0), 80.0, m["glass"]),
              b.Sphere((450.0, 60.0, 300.0), 60.0, m["pbr"][3])):
        w.push(h)
    if lights == "nested":
        inner = b.HittableList()
        inner.push(lr); inner.push(ls)
        ll = [inner]
    else:
        ll = {"none": [], "rect": [lr], "sphere": [ls]}[lights]
    b.set_scene(w, ll)
    return b, m


def real_rays(n, seed):
    """rays from inside the room towards its objects"""
    r = np.random.default_rng(seed)
    o = r.uniform(20.0, 535.0, (n, 3)) * (1.0, 0.9, 1.0) + (0.0, 30.0, 0.0)
    t = r.uniform(0.0, 555.0, (n, 3))
    t[: n // 3] *= (1.0, 0.0, 1.0)                                       # a third at the floor
    t[n // 3: n // 2] = np.array([278.0, 554.0, 280.0]) + r.uniform(-60.0, 60.0, (n // 2 - n // 3, 3)) * (1.0, 0.0, 1.0)   # some at the light
    return np.concatenate([o, t - o, np.zeros((n, 1))], 1)


def synthetic_records(mats, n, seed, graze=(1e-3, 1e-6, 1e-9, 1e-12), graze_share=0.15, ir=1.5):
    """(records (n, 16), rays (n, 7)) for the material handles `mats` in turn: axis-aligned and 0.9-boundary normals, grazing incoming
    directions (dot(d, n) / |d| down to graze[-1]), unnormalised d of length 1e-8 ... 1e8, back faces, and incidence at and around the
    critical angle of a dielectric of index ir."""
    r = np.random.default_rng(seed)
    rec = np.zeros((n, 16)); rays = np.zeros((n, 7))
    special = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    for j in (-2, -1, 0, 1, 2):
        x = step(0.9, j)
        special.append((x, np.sqrt(1.0 - x * x), 0.0)); special.append((-x, 0.0, np.sqrt(1.0 - x * x)))
    for i in range(n):
        nrm = np.array(special[r.integers(len(special))]) if r.random() < 0.4 else r.normal(size=3)
        nrm = nrm / np.sqrt((nrm * nrm).sum())
        tng = np.cross(nrm, r.normal(size=3)); tng /= np.sqrt((tng * tng).sum())
        u = r.random()
        if u < graze_share:
            c = graze[r.integers(len(graze))]
        elif u < graze_share + 0.1:                                     # around the critical angle: sin(theta) = 1 / ir +- a few 1e-16
            s = 1.0 / ir + r.integers(-3, 4) * 2.0 ** -53
            c = np.sqrt(1.0 - s * s)
        else:
            c = r.uniform(0.02, 1.0)
        d = (np.sqrt(max(0.0, 1.0 - c * c)) * tng - c * nrm) * 10.0 ** r.uniform(-8.0, 8.0)
        p = r.uniform(5.0, 550.0, 3)
        rec[i, 0] = 1.0; rec[i, 1] = r.uniform(0.5, 500.0); rec[i, 2:5] = p; rec[i, 5:8] = nrm; rec[i, 8] = float(r.random() < 0.7)
        rec[i, 9:11] = r.random(2); rec[i, 11] = mats[i % len(mats)]; rec[i, 12] = 0.0; rec[i, 13] = 0.0; rec[i, 14] = 0.0
        rays[i, 0:3] = p - d; rays[i, 3:6] = d; rays[i, 6] = r.random()
    return rec, rays


EXACT_MATS = ("metal", "mirror", "glass", "glass1", "light", "iso")      # no libm call on their arms: 0 differing words
SEED = 0x5EED


def bounce_sets():
    """The inputs of the one-bounce tests: (name, scene, lights, what) — what = "real" (rays into the scene, records from the hit query),
    "exact" / "lam" / "pbr" (synthetic records of those materials)."""
    out = []
    for lights in ("none", "rect"):
        out += [("list " + lights + " " + w, "list", lights, w) for w in ("real", "listsyn")]
    for lights in ("none", "rect", "sphere", "nested"):
        out += [("full " + lights + " " + w, "full", lights, w) for w in ("real", "exact", "lam", "pbr")]
    return out


def make_scene(be, scene, lights):
    return list_scene(be, lights) if scene == "list" else full_scene(be, lights)


def set_records(what, mats, hits_fn):
    """(records, rays) of one set; hits_fn(rays) -> (n, 16) records (the product's hit query on the device, the oracle's on the host)"""
    if what == "real":
        rays = real_rays(1500, 7401)
        rec = hits_fn(rays)
        keep = (rec[:, 0] != 0.0) & (rec[:, 11] >= 0.0)
        return rec[keep], rays[keep]
    if what == "listsyn":
        return synthetic_records([mats[k].id for k in ("lam", "lam2", "metal", "mirror", "light")], 1000, 7402)
    if what == "exact":
        return synthetic_records([mats[k].id for k in EXACT_MATS], 1200, 7403)
    if what == "lam":
        return synthetic_records([mats["lam"].id], 600, 7404)
    ids = [h.id for h in mats["pbr"]]
    a = synthetic_records(ids, 60 * len(ids), 7405, graze=(1e-3, 1e-6, 1e-8))
    b = synthetic_records(ids, 8, 7406, graze=(1e-9, 1e-12), graze_share=1.0)       # (0.5 % of the set: below the margin by construction)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def sphere_light_records(mats, n=2400, seed=7407):
    """(records, rays, family per record) for full_scene(.., "sphere") and "nested": Lambertian and PBR records whose shading point lies
    where Sphere::random and Sphere::pdf_value (sphere.rs:104-119) are hostile — "inside" the light (1 - r^2 / d^2 < 0: the sampled
    direction is NaN), at its "centre" (d = 0), on its "surface" within 1e-12 radii (1 - r^2 / d^2 about 0, either sign), "far" away
    at 1e6 ... 1e9 radii (from 1.35e8 radii on 1 - r^2 / d^2 rounds to 1) — and "near" ones, 1.01 ... 100 radii, between them.  Normals, incoming rays and the
    rest of a record are synthetic_records'."""
    r = np.random.default_rng(seed)
    pbr = [h.id for h in mats["pbr"]]
    # a third Lambertian, the rest every PBR set in turn: half of those draw from the BRDF's pdf and a third of that from each of its
    # arms, n / 9 records, so that each arm's libm calls see some 260 operands
    ids = [mats["lam"].id if i % 3 == 0 else pbr[(i - i // 3) % len(pbr)] for i in range(n)]
    rec, rays = synthetic_records(ids, n, seed)
    c, rad = np.array(LIGHT_SPHERE[0]), LIGHT_SPHERE[1]
    fam = np.array(["inside"] * (n * 3 // 8) + ["centre"] * (n // 40) + ["surface"] * (n // 8) + ["far"] * (n // 8), dtype=object)
    fam = np.concatenate([fam, np.array(["near"] * (n - len(fam)), dtype=object)])[r.permutation(n)]
    u = r.normal(size=(n, 3)); u /= np.sqrt((u * u).sum(1))[:, None]
    dist = np.select([fam == "inside", fam == "centre", fam == "surface", fam == "far"],
                     [rad * r.uniform(0.001, 0.999, n), 0.0, rad * (1.0 + r.integers(-4, 5, n) * 2.0e-13), rad * 10.0 ** r.uniform(6.1, 9.0, n)],
                     rad * 10.0 ** r.uniform(np.log10(1.01), 2.0, n))
    p = c + dist[:, None] * u
    rays[:, 0:3] = p - rays[:, 3:6]
    rec[:, 2:5] = p
    return rec, rays, fam


def first_draw_is_light(obe, seed, n):
    """per record k whether the first draw of rng_path(seed, k, 0) — the mixture pdf's coin, pdf.rs:167-173 — picks the lights"""
    import ctypes as C
    st = (C.c_uint32 * 4)()
    out = np.zeros(n, bool)
    for k in range(n):
        obe.lib.orc_rng_path(C.c_uint64(seed), C.c_uint32(k), C.c_uint32(0), st)
        x = (st[0] + st[3]) & 0xFFFFFFFF
        out[k] = ((((x << 7) | (x >> 25)) + st[0]) & 0xFFFFFFFF) >> 31 != 0
    return out


def within(got, ref):
    """the project's per-sample bound on every value, NaN / inf patterns equal"""
    got, ref = np.asarray(got), np.asarray(ref)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        ok = np.where(fin, np.abs(got - ref) <= SAMPLE_RTOL * (1.0 + np.abs(ref)), same_words(got, ref) | (np.isnan(got) & np.isnan(ref)))
    return ok

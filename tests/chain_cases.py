"""Specular-chain guides (csrc/rt_chain.h) restated in NumPy, the test scene, and the rays the host and GPU tests send through it.

numpy_step and numpy_chain are the specification (C2)-(C8), not the code under test: vectorised over the items, every operation one NumPy
operation on float64 (one rounding), in the written order.  The searches (C1) are NOT restated: a chain is composed with a `search`
callback that is not under test — the oracle's orc.hit_records on the CPU, render.query_albedo(want_hits) / render.query_camera on the GPU,
which tests/test_ray_query_gpu.py and tests/test_albedo_query_gpu.py pin to the oracle."""
import contextlib

import numpy as np

from guide_cases import differing_words, numpy_guide      # noqa: F401  (the reduction of (C8), unchanged)

INF = float("inf")
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
METAL, DIELECTRIC = 1, 2
# status words of rt_chain_step_host; END_MAX_LINKS is this file's own mark for "l == max_links, and the step would have gone on"
CONTINUE, END_SURFACE, END_MISS, END_ABSORBED, END_NONFINITE, END_FUZZ, END_MAX_LINKS = 0, 1, 2, 3, 4, 5, 6
W, H = 23, 11
T_MIN = 1e-5


def link_seed(seed, sample_index, l):
    """(C1)"""
    return (seed + ((((sample_index << 8) | l) * GOLDEN) & MASK64)) & MASK64


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def finite3(v):
    return ((v - v) == 0.0).all(axis=-1)


class Materials:
    """What the step reads of a scene's materials, by handle: kind, param (fuzz or index), albedo."""

    def __init__(self, log, n):
        self.kind = np.zeros(n, np.int64); self.param = np.zeros(n); self.albedo = np.zeros((n, 3))
        for m, (kind, param, albedo) in log.items():
            self.kind[m] = kind; self.param[m] = param; self.albedo[m] = albedo


@contextlib.contextmanager
def recorded_materials(log):
    """While active, every SceneBuilder.Metal / .Dielectric call notes its handle and arguments in `log`: the library's scene functions build
    their own SceneBuilder, and the C-ABI does not give a material's fuzz or index back."""
    from raytracinginrust_amd.api import SceneBuilder
    metal, dielectric = SceneBuilder.Metal, SceneBuilder.Dielectric

    def rec_metal(self, albedo, fuzz):
        h = metal(self, albedo, fuzz); log[h.id] = (METAL, float(fuzz), tuple(float(x) for x in albedo)); return h

    def rec_dielectric(self, ir):
        h = dielectric(self, ir); log[h.id] = (DIELECTRIC, float(ir), (0.0, 0.0, 0.0)); return h
    SceneBuilder.Metal, SceneBuilder.Dielectric = rec_metal, rec_dielectric
    try:
        yield log
    finally:
        SceneBuilder.Metal, SceneBuilder.Dielectric = metal, dielectric


def build_recorded(fn, *args, **kw):
    """fn(*args) -> (builder, camera, background) with the materials it made -> (builder, camera, Materials)."""
    log = {}
    with recorded_materials(log):
        b, cam, _ = fn(*args, **kw)
    return b, cam, Materials(log, max(log, default=0) + 64)


# ---------------------------------------------------------------- (C2)-(C5): one link
def numpy_step(rays, hits, mats, max_fuzz):
    """rays (n, 7), hits (n, 16) -> next rays (n, 7), this link's weight factor (n, 3), status (n,) as rt_chain_step_host gives them."""
    rays = np.asarray(rays, np.float64); hits = np.asarray(hits, np.float64)
    n = len(rays)
    d = rays[:, 3:6]; nrm = hits[:, 5:8]
    hit = hits[:, 0] != 0.0
    mword = hits[:, 11]
    surface = hit & (mword >= 0.0)
    m = np.where(surface, mword, 0.0).astype(np.int64)
    kind = np.where(surface, mats.kind[m], -1)
    param = mats.param[m]
    status = np.full(n, END_SURFACE, np.int64)
    status[~hit] = END_MISS
    new_d = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        # (C3)
        metal = kind == METAL
        s = (-dot(d, nrm)) * 2.0
        dn = d + s[:, None] * nrm
        r_metal = dn / np.sqrt(dot(dn, dn))[:, None]
        fuzzy = metal & ~(param <= max_fuzz)
        ok = metal & ~fuzzy
        nonfinite = ok & ~finite3(r_metal)
        absorbed = ok & ~nonfinite & ~(dot(r_metal, nrm) > 0.0)
        status[fuzzy] = END_FUZZ; status[nonfinite] = END_NONFINITE; status[absorbed] = END_ABSORBED
        go_metal = ok & ~nonfinite & ~absorbed
        # (C4)
        glass = kind == DIELECTRIC
        front = hits[:, 8] != 0.0
        ratio = np.where(front, 1.0 / param, param)
        u = d / np.sqrt(dot(d, d))[:, None]
        cos_theta = np.fmin(dot(-1.0 * u, nrm), 1.0)
        sin_theta = np.sqrt(1.0 - cos_theta * cos_theta)
        cannot_refract = ratio * sin_theta > 1.0
        q = (1.0 - ratio) / (1.0 + ratio)
        r0 = q * q
        m1 = 1.0 - cos_theta; m2 = m1 * m1
        refl = r0 + (1.0 - r0) * (m1 * (m2 * m2))
        will_reflect = refl > 0.5
        su = (-dot(u, nrm)) * 2.0
        reflected = u + su[:, None] * nrm
        perp = ratio[:, None] * (u + cos_theta[:, None] * nrm)
        ln = np.sqrt(dot(perp, perp))
        para = (-1.0 * np.sqrt(np.fabs(1.0 - ln * ln)))[:, None] * nrm
        refracted = perp + para
        r_glass = np.where((cannot_refract | will_reflect)[:, None], reflected, refracted)
        bad_glass = glass & ~finite3(r_glass)
        status[bad_glass] = END_NONFINITE
        go_glass = glass & ~bad_glass
    status[go_metal | go_glass] = CONTINUE
    new_d[go_metal] = r_metal[go_metal]; new_d[go_glass] = r_glass[go_glass]
    go = status == CONTINUE
    nxt = rays.copy()
    nxt[go, 0:3] = hits[go, 2:5]; nxt[go, 3:6] = new_d[go]        # (C5); time unchanged
    factor = np.ones((n, 3))
    factor[go_metal] = mats.albedo[m[go_metal]]
    info = {"cannot_refract": glass & cannot_refract, "reflects_by_fresnel": glass & ~cannot_refract & will_reflect}
    return nxt, factor, status.astype(np.uint32), info


# ---------------------------------------------------------------- (C1), (C6), (C7): whole chains over a search that is not under test
def numpy_chain(search, rays, mats, max_links, max_fuzz, seed, sample_index=0, first=None):
    """search(l, rays, seed_l) -> (hits (n, 16), albedo (n, 3) or None): link l of ALL items (ended items repeat their last ray, as the kernel's
    ended lanes do: item k's stream is keyed by k).  first: link 0's (hits, albedo) where the caller has them (the camera form).
    -> dict: hits (n, 16) chain records, albedo (n, 3) or None, links (n,), end (n,) END_* words, live (links + 1 counts of items searched as
    part of their chain at link l), seen (per-item or-ed step info)."""
    rays = np.asarray(rays, np.float64)
    n = len(rays)
    cur = rays.copy()
    live = np.ones(n, bool)
    weight = np.ones((n, 3)); S = np.zeros(n); L0 = np.ones(n)
    links = np.zeros(n, np.int64); end = np.full(n, -1, np.int64)
    out = np.zeros((n, 16)); alb = np.ones((n, 3)); have_albedo = True
    seen = {"cannot_refract": np.zeros(n, bool), "reflects_by_fresnel": np.zeros(n, bool)}
    live_counts = []
    with np.errstate(all="ignore"):
        for l in range(max_links + 1):
            if not live.any():
                break
            live_counts.append(int(live.sum()))
            hits, a = first if (l == 0 and first is not None) else search(l, cur, link_seed(seed, sample_index, l) if l else seed)
            hits = np.asarray(hits, np.float64)
            nxt, factor, status, info = numpy_step(cur, hits, mats, max_fuzz)
            status = status.astype(np.int64)
            if l == max_links:
                status = np.where(status == END_MISS, END_MISS, np.where(status == CONTINUE, END_MAX_LINKS, END_SURFACE))
            d = cur[:, 3:6]
            L = np.sqrt(dot(d, d))
            hit = hits[:, 0] != 0.0
            if l == 0:
                S = hits[:, 1] * L; L0 = L
                t_word = hits[:, 1].copy()
            else:
                S = np.where(live & hit, S + hits[:, 1] * L, S)
                t_word = S / L0
            ended = live & (status != CONTINUE)
            rec = hits.copy(); rec[:, 1] = t_word; rec[:, 15] = links.astype(np.float64)
            out[ended] = rec[ended]; end[ended] = status[ended]
            if a is None:
                have_albedo = False
            else:
                alb[ended] = weight[ended] * np.asarray(a, np.float64)[ended]
            go = live & (status == CONTINUE)
            for key in seen:
                seen[key] |= go & info[key]
            weight[go] = weight[go] * factor[go]
            cur[go] = nxt[go]
            links[go] += 1
            live = go
    assert not live.any()
    return {"hits": out, "albedo": alb if have_albedo else None, "weight": weight, "links": links, "end": end, "live": live_counts, "seen": seen}


def numpy_camera_chain_guide(per_sample):
    """(C8) from the per-sample chains (numpy_chain results, ascending samples): guide, albedo sums, links."""
    guide = numpy_guide(np.stack([c["hits"] for c in per_sample]))
    alb = np.zeros_like(per_sample[0]["albedo"])
    links = np.zeros(len(alb), np.int64)
    for c in per_sample:                                        # ascending, into +0.0
        alb = alb + c["albedo"]
        links = links + c["links"]
    return guide, alb, links.astype(np.uint32)


# ---------------------------------------------------------------- the test scene
MIRROR_TINT = (0.9, 0.8, 0.7)
BALL_TINT = (0.6, 0.9, 0.9)


def chain_scene(be):
    """A diffuse room open towards the camera with a light, a checker floor, two facing fuzz-0 mirrors (x = 1 and x = 4), a fuzz-0.3 metal
    sphere, a fuzz-0 metal sphere, hollow glass (index 1.5 around index 1/1.5) and one ConstantMedium box -> (builder, camera, Materials)."""
    from raytracinginrust_amd.api import Camera, Plane, SceneBuilder
    log = {}
    with recorded_materials(log):
        b = SceneBuilder(be)
        white = b.Lambertian(b.ConstantTexture((0.73, 0.73, 0.73)))
        red = b.Lambertian(b.ConstantTexture((0.65, 0.05, 0.05)))
        green = b.Lambertian(b.ConstantTexture((0.12, 0.45, 0.15)))
        checker = b.Lambertian(b.CheckTexture(b.ConstantTexture((0.2, 0.3, 0.1)), b.ConstantTexture((0.9, 0.9, 0.9))))
        light = b.DiffuseLight(b.ConstantTexture((7.0, 7.0, 7.0)))
        mirror = b.Metal(MIRROR_TINT, 0.0)
        ball = b.Metal(BALL_TINT, 0.0)
        rough = b.Metal((0.8, 0.6, 0.2), 0.3)
        glass = b.Dielectric(1.5)
        air = b.Dielectric(1.0 / 1.5)
        world = b.HittableList()
        world.push(b.AARect(Plane.XZ, 0.0, 10.0, 0.0, 10.0, 0.0, checker))
        world.push(b.AARect(Plane.XZ, 0.0, 10.0, 0.0, 10.0, 10.0, white))
        world.push(b.AARect(Plane.XY, 0.0, 10.0, 0.0, 10.0, 10.0, white))
        world.push(b.AARect(Plane.YZ, 0.0, 10.0, 0.0, 10.0, 0.0, red))
        world.push(b.AARect(Plane.YZ, 0.0, 10.0, 0.0, 10.0, 10.0, green))
        lamp = b.FlipNormal(b.AARect(Plane.XZ, 4.0, 6.0, 4.0, 6.0, 9.99, light))
        world.push(lamp)
        world.push(b.AARect(Plane.YZ, 1.0, 5.0, 2.0, 8.0, 1.0, mirror))
        world.push(b.AARect(Plane.YZ, 1.0, 5.0, 2.0, 8.0, 4.0, mirror))
        world.push(b.Sphere((7.0, 1.5, 3.0), 1.5, rough))
        world.push(b.Sphere((7.0, 8.0, 3.0), 1.5, ball))
        world.push(b.Sphere((7.0, 5.0, 6.5), 1.5, glass))
        world.push(b.Sphere((7.0, 5.0, 6.5), 1.2, air))
        world.push(b.ConstantMedium(b.Cube((1.0, 6.0, 6.0), (4.0, 9.0, 9.0), white), 0.5, b.ConstantTexture((0.9, 0.9, 0.9))))
        b.set_scene(world, [lamp])
    cam = Camera((5.0, 5.0, -14.0), (5.0, 5.0, 5.0), (0.0, 1.0, 0.0), 40.0, W / H, 0.1, 19.0, 0.0, 1.0)
    return b, cam, Materials(log, max(log) + 64)


def _ray(o, d, tm=0.5):
    return [float(x) for x in o] + [float(x) for x in d] + [float(tm)]


def aimed_rays():
    """Rays aimed at the mirrors, the glass and the metal spheres of chain_scene, the hand-made ones first (NAMED gives their rows)."""
    rays = [
        _ray((5.0, 0.5, -1.0), (0.0, 0.3, 1.0)),                 # 0: the back wall, no link
        _ray((0.5, 3.0, -1.0), (0.1, 0.0, 1.0)),                 # 1: one mirror from its outer side, then the red wall
        _ray((2.5, 3.0, 2.5), (1.0, 0.0, 0.2)),                  # 2: between the mirrors, many links
        _ray((2.5, 3.0, 5.0), (1.0, 0.0, 0.0)),                  # 3: between the mirrors for ever: ended by max_links
        _ray((7.0, 8.0, -1.0), (0.0, 0.0, 1.0)),                 # 4: the mirror ball head-on, back out of the room: a miss
        _ray((8.5, 8.0, 1.0), (0.0, 0.0, 1.0)),                  # 5: tangent to the mirror ball (|oc| = 2.5, exactly): absorbed
        _ray((7.0, 1.5, -1.0), (0.0, 0.0, 1.0)),                 # 6: the fuzzy sphere: status 5 under max_fuzz = 0
        _ray((8.35, 5.0, -1.0), (0.0, 0.0, 1.0)),                # 7: the glass shell at offset 1.35: total internal reflection at the inner sphere
        _ray((8.495, 5.0, -1.0), (0.0, 0.0, 1.0)),               # 8: the glass at offset 1.495: grazing, refl > 0.5
        _ray((7.0, 5.0, -1.0), (0.0, 0.0, 1.0)),                 # 9: the glass head-on: straight through four surfaces
        _ray((2.5, 7.5, -1.0), (0.0, 0.0, 1.0)),                 # 10: the medium box
        _ray((2.5, 3.0, 2.5), (1.0, 0.0, 0.8)),                  # 11: both mirrors once, then the back wall
    ]
    rs = np.random.RandomState(11)
    for k in range(52):
        o = np.array([rs.uniform(1.0, 9.0), rs.uniform(1.0, 9.0), rs.uniform(-2.0, 0.5)])
        kind = k % 4
        if kind == 0:      # a point on a mirror, from between them
            o[0] = rs.uniform(1.5, 3.5)
            target = np.array([1.0 if rs.randint(2) else 4.0, rs.uniform(1.5, 4.5), rs.uniform(2.5, 7.5)])
        elif kind == 1:    # a point in the glass
            target = np.array([7.0, 5.0, 6.5]) + rs.uniform(-1.4, 1.4, 3) * np.array([1.0, 1.0, 0.0])
        elif kind == 2:    # a point in the mirror ball
            target = np.array([7.0, 8.0, 3.0]) + rs.uniform(-1.0, 1.0, 3)
        else:              # anywhere on the back wall
            target = np.array([rs.uniform(0.0, 10.0), rs.uniform(0.0, 10.0), 10.0])
        rays.append(_ray(o, target - o, rs.uniform(0.0, 1.0)))
    return np.array(rays, np.float64)


NAMED = {"no_link": 0, "one_link": 1, "many_links": 2, "for_ever": 3, "miss": 4, "absorbed": 5, "fuzz": 6, "tir": 7, "fresnel": 8, "through": 9, "medium": 10, "two_links": 11}


def camera_rays(be_render, b, cam, seed=5):
    """The camera rays of sample 0 of the W x H view, (W * H, 7): rt_camera_ray, host only."""
    return np.array([be_render.camera_ray(cam, W, H, i, j, seed, 0) for j in range(H - 1, -1, -1) for i in range(W)], np.float64)


def hostile_records(mats_ids):
    """(rays, hits) for the step alone: NaN and infinite directions, zero and short normals, -0.0, a medium, a miss, both faces, on a Metal
    (mats_ids[0]), a fuzzy Metal ([1]), a Dielectric ([2]) and a Lambertian ([3])."""
    nan = float("nan")
    dirs = [(0.0, 0.0, 1.0), (0.3, -0.8, 0.5), (nan, 0.0, 1.0), (INF, 0.0, 1.0), (-INF, INF, 0.0), (0.0, 0.0, 0.0), (-0.0, -0.0, -1.0), (1e-200, 0.0, 1e-200),
            (1e200, 1e200, -1e200), (0.0, 1.0, 0.0)]
    normals = [(0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0.0, 0.0, -0.25), (-0.0, 0.6, -0.8), (nan, 0.0, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)]
    rays, hits = [], []
    for mi, m in enumerate(list(mats_ids) + [-1.0, None]):
        for d in dirs:
            for nv in normals:
                for front in (1.0, 0.0):
                    r = np.zeros(16)
                    if m is None:
                        r[11:15] = -1.0
                    else:
                        r[0] = 1.0; r[1] = 2.5; r[2:5] = (1.0, -0.0, 3.0); r[5:8] = nv; r[8] = front; r[9:11] = (0.25, 0.75)
                        r[11] = m; r[12] = 4.0; r[13] = -1.0 if m < 0 else 1.0; r[14] = -1.0 if m < 0 else 2.0
                    rays.append(_ray((0.5, 0.25, -0.0), d, 0.125)); hits.append(r)
    return np.array(rays), np.array(hits)

"""Randomised scene fuzzing: GPU (C-ABI) vs CPU oracle on scenes drawn from the whole builder surface — every primitive,
wrapper chain (Translate / Rotate X,Y,Z / FlipNormal in any order), BVHs with every leaf kind (incl. AARect leaves with
the reference's plane-blind bbox), constant media around several boundary shapes, every texture and material, and
`lights` lists mixing rect, sphere and trait-default entries.  Same seeded stream on both sides; per-sample tolerance as
in test_parity_gpu.py."""
import numpy as np
import pytest

from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Axis, Camera, Plane, Rng, SceneBuilder

pytestmark = pytest.mark.gpu

SAMPLE_RTOL = 1e-9


def _rand_scene(be, seed, earth):
    rs = np.random.RandomState(seed)
    b = SceneBuilder(be)
    rng = Rng(be, 1000 + seed, 40)

    def col(lo=0.05, hi=0.95):
        return tuple(float(x) for x in rs.uniform(lo, hi, 3))

    def texture():
        k = rs.randint(0, 6)
        if k <= 2:
            return b.ConstantTexture(col())
        if k == 3:
            return b.CheckTexture(b.ConstantTexture(col()), b.ConstantTexture(col()))
        if k == 4:
            return b.NoiseTexture(float(rs.uniform(0.05, 0.5)), rng)
        return b.ImageTexture(*earth)

    def material(allow_light=False):
        k = rs.randint(0, 9 if allow_light else 8)
        if k <= 2:
            return b.Lambertian(texture())
        if k == 3:
            return b.Metal(col(0.4, 1.0), float(rs.choice([0.0, 0.1, 0.5, 1.0])))
        if k == 4:
            return b.Dielectric(float(rs.choice([1.3, 1.5, 2.4])))
        if k == 5:
            return b.Isotropic(texture())
        if k == 6:
            return b.PBR(b.ConstantTexture(col()), *[float(x) for x in rs.uniform(0.0, 1.0, 10)])
        if k == 7:
            return b.Lambertian(b.ConstantTexture(col()))
        return b.DiffuseLight(b.ConstantTexture(col(1.0, 6.0)))

    def pos(s=60.0):
        return tuple(float(x) for x in rs.uniform(-s, s, 3))

    def prim():
        k = rs.randint(0, 6)
        m = material()
        if k == 0:
            return b.Sphere(pos(), float(rs.uniform(4, 18)), m)
        if k == 1:
            c = pos()
            return b.MovingSphere(c, tuple(c[i] + float(rs.uniform(-6, 6)) for i in range(3)), 0.0, 1.0, float(rs.uniform(4, 14)), m)
        if k == 2:
            a0, b0 = rs.uniform(-60, 30, 2)
            return b.AARect(int(rs.randint(0, 3)), float(a0), float(a0 + rs.uniform(10, 50)), float(b0), float(b0 + rs.uniform(10, 50)), float(rs.uniform(-50, 50)), m)
        if k == 3:
            mn = np.array(pos(40.0))
            return b.Cube(tuple(mn), tuple(mn + rs.uniform(8, 35, 3)), m)
        if k == 4:
            p0 = np.array(pos())
            return b.Triangle([tuple(p0), tuple(p0 + rs.uniform(-30, 30, 3)), tuple(p0 + rs.uniform(-30, 30, 3))], m)
        verts = [tuple(rs.uniform(-50, 50, 3)) for _ in range(5)]
        return b.Mesh(verts, [int(x) for x in rs.randint(0, 5, 9)], m)

    def wrap(h, depth=None):
        n = rs.randint(0, 4) if depth is None else depth
        for _ in range(n):
            k = rs.randint(0, 3)
            if k == 0:
                h = b.Translate(h, pos(30.0))
            elif k == 1:
                h = b.Rotate(int(rs.randint(0, 3)), h, float(rs.uniform(-80, 80)))
            else:
                h = b.FlipNormal(h)
        return h

    world = b.HittableList()
    lights = []
    # emitters (also candidates for `lights`)
    glow = b.DiffuseLight(b.ConstantTexture(col(2.0, 9.0)))
    rect_light = b.AARect(Plane.XZ, -25.0, 25.0, -25.0, 25.0, 75.0, glow)
    if rs.rand() < 0.5:
        rect_light = b.FlipNormal(rect_light)
    world.push(rect_light)
    bulb = b.Sphere((float(rs.uniform(-40, 40)), 55.0, float(rs.uniform(-40, 40))), float(rs.uniform(3, 8)), glow)
    world.push(bulb)
    for _ in range(rs.randint(3, 9)):
        world.push(wrap(prim()))
    # a nested list inside wrappers
    inner = b.HittableList()
    inner.push(prim())
    inner.push(b.Sphere(pos(), 6.0, material()))
    world.push(wrap(inner, 1))
    # BVHs: bare leaves of every kind, optionally inside wrappers
    leaves = []
    for _ in range(rs.randint(4, 24)):
        k = rs.randint(0, 5)
        m = material()
        p = np.array(pos(70.0))
        if k == 0:
            leaves.append(b.Sphere(tuple(p), float(rs.uniform(2, 7)), m))
        elif k == 1:
            leaves.append(b.MovingSphere(tuple(p), tuple(p + rs.uniform(-3, 3, 3)), 0.0, 1.0, float(rs.uniform(2, 6)), m))
        elif k == 2:
            leaves.append(b.Cube(tuple(p), tuple(p + rs.uniform(3, 12, 3)), m))
        elif k == 3:
            leaves.append(b.Triangle([tuple(p), tuple(p + rs.uniform(-12, 12, 3)), tuple(p + rs.uniform(-12, 12, 3))], m))
        else:
            leaves.append(b.AARect(Plane.XY, float(p[0]), float(p[0] + 10), float(p[1]), float(p[1] + 10), float(p[2]), m))   # bbox is right only for XY (quirk B4)
    world.push(wrap(b.BVH(leaves, 0.0, 1.0), int(rs.randint(0, 3))))
    # media: boundary = sphere / wrapped cube / wrapped sphere
    for _ in range(rs.randint(0, 3)):
        k = rs.randint(0, 3)
        if k == 0:
            bd = b.Sphere(pos(), float(rs.uniform(8, 25)), b.Dielectric(1.5))
        elif k == 1:
            mn = np.array(pos(30.0))
            bd = wrap(b.Cube(tuple(mn), tuple(mn + rs.uniform(10, 30, 3)), b.Lambertian(b.ConstantTexture(col()))), 2)
        else:
            bd = b.Translate(b.Sphere((0.0, 0.0, 0.0), float(rs.uniform(8, 20)), b.Dielectric(1.5)), pos(40.0))
        world.push(b.ConstantMedium(bd, float(rs.choice([0.005, 0.02, 0.1])), texture()))
    # lights list
    mode = rs.randint(0, 4)
    if mode >= 1:
        lights.append(rect_light)
    if mode >= 2:
        lights.append(bulb)
    if mode == 3:
        lights.append(b.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), glow))      # trait-default pdf_value / random (hit.rs:29-30)
    b.set_scene(world, lights)
    cam = Camera((float(rs.uniform(-30, 30)), float(rs.uniform(10, 60)), -170.0), (0.0, 10.0, 0.0), (0.0, 1.0, 0.0), 45.0, 1.0,
                 float(rs.choice([0.0, 0.5, 2.0])), 170.0, 0.0, 1.0)
    return b, cam, col(0.0, 0.6)


@pytest.mark.parametrize("seed", list(range(24)))
def test_random_scene_parity(pbe, obe, earth, seed):
    from oracle import orc
    ob, ocam, obg = _rand_scene(obe, seed, earth)
    pb, pcam, pbg = _rand_scene(pbe, seed, earth)
    W, H, spp, depth = 40, 40, 8, 12
    ref, rs_, cnt = orc.render(ob, ocam, obg, W, H, spp, depth, seed=77 + seed, want_samples=True, want_counters=True)
    got, gs = R.render(pb, pcam, pbg, W, H, spp, depth, seed=77 + seed, want_samples=True)
    assert np.array_equal(np.isnan(gs), np.isnan(rs_)), "NaN pattern differs"
    assert np.array_equal(np.isinf(gs), np.isinf(rs_)) and np.array_equal(np.signbit(gs[np.isinf(gs)]), np.signbit(rs_[np.isinf(rs_)]))
    fin = np.isfinite(rs_)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs_, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs_, 0.0)))).any(axis=-1)
    assert bad.sum() <= 2, f"seed {seed}: {int(bad.sum())} of {W * H * spp} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"
    assert R.last_stats(pb)["nonfinite_samples"] == cnt["nonfinite"]


def _rand_list_scene(be, seed):
    """A list scene (no BVH, no sphere, constant textures, Lambertian / Metal / DiffuseLight): what the lean kernels serve — their
    straight-line paths for wrapper-less objects and for `Translate(RotateY(..))`, the generic wrapper loops for every other chain,
    the merged Lambertian / Metal arms with 0, 1 or 2 lights.  (rt_kernel.hip: object_hit / finalize_hit's FEATS == 0 blocks, MERGE_ARMS; since round 5 also the Cube fast path, cube_fast.)"""
    rs = np.random.RandomState(9000 + seed)
    b = SceneBuilder(be)

    def col(lo=0.05, hi=0.95):
        return tuple(float(x) for x in rs.uniform(lo, hi, 3))

    def material():
        k = rs.randint(0, 4)
        if k <= 1:
            return b.Lambertian(b.ConstantTexture(col()))
        if k == 2:
            return b.Metal(col(0.4, 1.0), float(rs.choice([0.0, 0.1, 0.5, 1.0])))
        return b.DiffuseLight(b.ConstantTexture(col(0.5, 3.0)))

    def prim():
        m = material()
        if rs.rand() < 0.5:
            a0, b0 = rs.uniform(-60, 30, 2)
            return b.AARect(int(rs.randint(0, 3)), float(a0), float(a0 + rs.uniform(10, 60)), float(b0), float(b0 + rs.uniform(10, 60)), float(rs.uniform(-50, 50)), m)
        mn = rs.uniform(-40, 20, 3)
        return b.Cube(tuple(mn), tuple(mn + rs.uniform(8, 35, 3)), m)

    def off(s=30.0):
        return tuple(float(x) for x in rs.uniform(-s, s, 3))

    def ang():
        return float(rs.uniform(-80, 80))

    def wrap(h):
        k = rs.randint(0, 10)
        if k == 0: return h
        if k <= 3: return b.Translate(b.Rotate(1, h, ang()), off())                      # the instance idiom (main.rs:300-309)
        if k == 4: return b.Translate(b.Rotate(int(rs.choice([0, 2])), h, ang()), off())  # same shape, another axis
        if k == 5: return b.Rotate(1, b.Translate(h, off()), ang())                      # the two the other way round
        if k == 6: return b.Translate(h, off())
        if k == 7: return b.Rotate(int(rs.randint(0, 3)), h, ang())
        if k == 8: return b.FlipNormal(b.Translate(b.Rotate(1, h, ang()), off()))         # three wrappers
        return b.Translate(b.Rotate(1, b.Translate(b.Rotate(1, h, ang()), off()), ang()), off())   # the idiom twice

    world = b.HittableList()
    glow = b.DiffuseLight(b.ConstantTexture(col(4.0, 12.0)))
    l1 = b.FlipNormal(b.AARect(Plane.XZ, -30.0, 30.0, -30.0, 30.0, 70.0, glow))
    l2 = b.AARect(Plane.XY, -20.0, 20.0, 0.0, 40.0, 65.0, glow)
    world.push(l1)
    world.push(l2)
    world.push(b.AARect(Plane.XZ, -200.0, 200.0, -200.0, 200.0, -55.0, b.Lambertian(b.ConstantTexture(col()))))
    for _ in range(rs.randint(3, 10)):
        world.push(wrap(prim()))
    b.set_scene(world, [l1, l2][:int(rs.randint(0, 3))])
    cam = Camera((float(rs.uniform(-30, 30)), float(rs.uniform(0, 50)), -170.0), (0.0, 5.0, 0.0), (0.0, 1.0, 0.0), 45.0, 1.0,
                 float(rs.choice([0.0, 1.0])), 170.0, 0.0, 1.0)
    return b, cam, col(0.0, 0.5)


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_list_scene_parity(pbe, obe, seed):
    from oracle import orc
    ob, ocam, obg = _rand_list_scene(obe, seed)
    pb, pcam, pbg = _rand_list_scene(pbe, seed)
    W, H, spp, depth = 40, 40, 8, 12
    ref, rs_, cnt = orc.render(ob, ocam, obg, W, H, spp, depth, seed=31 + seed, want_samples=True, want_counters=True)
    got, gs = R.render(pb, pcam, pbg, W, H, spp, depth, seed=31 + seed, want_samples=True)
    info = R.last_launch_info(pb)
    assert info["threads"] == 256 and info["bvh_nodes"] == 0, "not the lean list-scene kernel"
    assert np.array_equal(np.isnan(gs), np.isnan(rs_)), "NaN pattern differs"
    assert np.array_equal(np.isinf(gs), np.isinf(rs_))
    fin = np.isfinite(rs_)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs_, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs_, 0.0)))).any(axis=-1)
    assert bad.sum() <= 2, f"seed {seed}: {int(bad.sum())} of {W * H * spp} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"
    assert R.last_stats(pb)["nonfinite_samples"] == cnt["nonfinite"]


def _rand_nested_scene(be, seed, kinds=None):
    """BVHs whose children are ANY Hittable (BVH::new takes Vec<Box<dyn Hittable>> and needs only bounding_box, bvh.rs:18-31): bare
    primitives beside wrapped ones (Translate / Rotate — whose box is all of space, quirk B3, so the wave walks the exact f64 nodes —
    / FlipNormal, chains of them), HittableLists (of primitives, of wrapped objects, wrapped themselves), ConstantMedia (around a sphere,
    a wrapped cube; under wrappers of their own), nested BVHs (of primitives and of wrapped objects), the whole BVH under 0-2 wrappers;
    and at the top level a ConstantMedium under wrappers.  `kinds`: restrict the children to these kinds (the per-kind tests)."""
    rs = np.random.RandomState(5000 + seed)
    b = SceneBuilder(be)

    def col(lo=0.05, hi=0.95):
        return tuple(float(x) for x in rs.uniform(lo, hi, 3))

    def material():
        k = rs.randint(0, 6)
        if k <= 2:
            return b.Lambertian(b.ConstantTexture(col()))
        if k == 3:
            return b.Metal(col(0.4, 1.0), float(rs.choice([0.0, 0.3])))
        if k == 4:
            return b.Dielectric(1.5)
        return b.Lambertian(b.CheckTexture(b.ConstantTexture(col()), b.ConstantTexture(col())))

    def pos(s=60.0):
        return tuple(float(x) for x in rs.uniform(-s, s, 3))

    def prim(s=60.0):
        k = rs.randint(0, 5)
        m = material()
        p = np.array(pos(s))
        if k == 0:
            return b.Sphere(tuple(p), float(rs.uniform(3, 10)), m)
        if k == 1:
            return b.MovingSphere(tuple(p), tuple(p + rs.uniform(-3, 3, 3)), 0.0, 1.0, float(rs.uniform(3, 8)), m)
        if k == 2:
            return b.Cube(tuple(p), tuple(p + rs.uniform(5, 18, 3)), m)
        if k == 3:
            return b.Triangle([tuple(p), tuple(p + rs.uniform(-20, 20, 3)), tuple(p + rs.uniform(-20, 20, 3))], m)
        return b.AARect(Plane.XY, float(p[0]), float(p[0] + 14), float(p[1]), float(p[1] + 14), float(p[2]), m)

    def wrap(h, n=None, no_rotate=False):
        for _ in range(rs.randint(1, 3) if n is None else n):
            k = rs.randint(0, 2 if no_rotate else 3)
            if k == 0:
                h = b.Translate(h, pos(25.0))
            elif k == 1:
                h = b.FlipNormal(h)
            else:
                h = b.Rotate(int(rs.randint(0, 3)), h, float(rs.uniform(-60, 60)))
        return h

    def medium(s=50.0):
        if rs.rand() < 0.5:
            bd = b.Sphere(pos(s), float(rs.uniform(8, 20)), b.Dielectric(1.5))
        else:
            mn = np.array(pos(s * 0.6))
            bd = wrap(b.Cube(tuple(mn), tuple(mn + rs.uniform(10, 25, 3)), b.Lambertian(b.ConstantTexture(col()))), int(rs.randint(0, 3)))
        return b.ConstantMedium(bd, float(rs.choice([0.01, 0.05, 0.2])), b.ConstantTexture(col()))

    def child(kind):
        if kind == "prim":
            return prim()
        if kind == "translate":
            return b.Translate(prim(40.0), pos(25.0))
        if kind == "flip":
            return b.FlipNormal(prim())
        if kind == "rotate":
            return b.Rotate(int(rs.randint(0, 3)), prim(40.0), float(rs.uniform(-60, 60)))
        if kind == "chain":
            return wrap(prim(40.0), int(rs.randint(2, 4)))
        if kind == "list":
            l = b.HittableList()
            for _ in range(rs.randint(1, 4)):
                l.push(prim() if rs.rand() < 0.6 else wrap(prim(40.0), 1, no_rotate=True))
            return l if rs.rand() < 0.6 else wrap(l, 1, no_rotate=True)
        if kind == "medium":
            return medium() if rs.rand() < 0.6 else wrap(medium(35.0), 1, no_rotate=True)
        if kind == "bvh":
            inner = [prim() if rs.rand() < 0.7 else wrap(prim(40.0), 1, no_rotate=True) for _ in range(rs.randint(1, 7))]
            h = b.BVH(inner, 0.0, 1.0)
            return h if rs.rand() < 0.6 else wrap(h, 1, no_rotate=True)
        raise KeyError(kind)

    all_kinds = ["prim", "translate", "flip", "rotate", "chain", "list", "medium", "bvh"]
    world = b.HittableList()
    glow = b.DiffuseLight(b.ConstantTexture(col(3.0, 9.0)))
    lamp = b.FlipNormal(b.AARect(Plane.XZ, -30.0, 30.0, -30.0, 30.0, 80.0, glow))
    world.push(lamp)
    world.push(b.AARect(Plane.XZ, -300.0, 300.0, -300.0, 300.0, -70.0, b.Lambertian(b.ConstantTexture(col()))))
    for _ in range(rs.randint(0, 3)):
        world.push(prim())
    n_children = rs.randint(3, 14)
    pool = kinds if kinds is not None else all_kinds
    children = [child(pool[rs.randint(0, len(pool))]) if rs.rand() < 0.7 else prim() for _ in range(n_children)]
    bvh = b.BVH(children, 0.0, 1.0)
    world.push(wrap(bvh, int(rs.randint(0, 3)), no_rotate=rs.rand() < 0.7))
    if kinds is None or "medium" in kinds:
        if rs.rand() < 0.5:
            world.push(wrap(medium(40.0), int(rs.randint(1, 3))))          # a ConstantMedium under wrappers at the top level
    b.set_scene(world, [lamp] if rs.rand() < 0.7 else [])
    cam = Camera((float(rs.uniform(-30, 30)), float(rs.uniform(10, 60)), -190.0), (0.0, 5.0, 0.0), (0.0, 1.0, 0.0), 45.0, 1.0,
                 float(rs.choice([0.0, 1.0])), 190.0, 0.0, 1.0)
    return b, cam, col(0.1, 0.6)


def _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, seed, W=40, H=40, spp=8, depth=12, max_bad=2):
    from oracle import orc
    ref, rs_, cnt = orc.render(ob, ocam, obg, W, H, spp, depth, seed=seed, want_samples=True, want_counters=True)
    got, gs = R.render(pb, pcam, pbg, W, H, spp, depth, seed=seed, want_samples=True)
    assert np.array_equal(np.isnan(gs), np.isnan(rs_)), "NaN pattern differs"
    assert np.array_equal(np.isinf(gs), np.isinf(rs_))
    fin = np.isfinite(rs_)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs_, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs_, 0.0)))).any(axis=-1)
    assert bad.sum() <= max_bad, f"{int(bad.sum())} of {W * H * spp} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"
    assert R.last_stats(pb)["nonfinite_samples"] == cnt["nonfinite"]
    return cnt


@pytest.mark.parametrize("kind", ["translate", "flip", "rotate", "chain", "list", "medium", "bvh"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bvh_children_of_every_hittable_kind(pbe, obe, kind, seed):
    """One kind of non-primitive BVH child at a time (beside bare primitives), against the oracle per sample: BVH::new accepts any
    Hittable (bvh.rs:18-31); until round 6 rt_bvh refused everything but Sphere / MovingSphere / AARect / Cube / Triangle."""
    ob, ocam, obg = _rand_nested_scene(obe, 100 * seed + 7, [kind])
    pb, pcam, pbg = _rand_nested_scene(pbe, 100 * seed + 7, [kind])
    _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, 11 + seed)
    li = R.last_loop_info(pb)
    assert li["feats"] == 639 and li["shape"] == "lock-step", li        # F_ALL | F_NESTED: the one instantiation with object leaves


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_nested_scene_parity(pbe, obe, seed):
    ob, ocam, obg = _rand_nested_scene(obe, seed)
    pb, pcam, pbg = _rand_nested_scene(pbe, seed)
    _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, 53 + seed)


def _rand_room_scene(be, seed):
    """Rooms made of parallel pairs of equal AARects (the Cornell room's left / right walls and floor / ceiling, main.rs:281-286) around
    boxes and a light: 1-3 pairs on different axes, sometimes a third wall behind a pair, sometimes two pairs in one run; the camera
    inside the room, outside it (both walls of a pair in front), or EXACTLY on a wall's plane (`t = 0 < t_min` rejects).  (Written for
    round 6's pair rule — one division for the two rects of a pair, exact by the sign of the numerator — which was measured slower and
    taken out again, docs/history.md; the family stays: rays that start ON rect planes are what a Cornell bounce is.)"""
    rs = np.random.RandomState(7000 + seed)
    b = SceneBuilder(be)

    def col(lo=0.05, hi=0.95):
        return tuple(float(x) for x in rs.uniform(lo, hi, 3))

    def lam():
        return b.Lambertian(b.ConstantTexture(col()))

    L = float(rs.choice([100.0, 555.0, 37.5]))
    world = b.HittableList()
    glow = b.DiffuseLight(b.ConstantTexture(col(5.0, 15.0)))
    lamp = b.FlipNormal(b.AARect(Plane.XZ, 0.3 * L, 0.6 * L, 0.35 * L, 0.6 * L, L * (1.0 - 2.0 ** -9), glow))
    axes = [a for a in (Plane.YZ, Plane.XZ, Plane.XY) if rs.rand() < 0.8] or [Plane.YZ]
    light_at = rs.randint(0, len(axes) + 1)
    for n, plane in enumerate(axes):
        if n == light_at:
            world.push(lamp)
        lo, hi = (0.0, L) if rs.rand() < 0.7 else (float(rs.uniform(-0.2, 0.1) * L), float(rs.uniform(0.9, 1.3) * L))
        ks = [L, 0.0] if rs.rand() < 0.5 else [0.0, L]
        m1, m2 = lam(), (lam() if rs.rand() < 0.5 else b.Metal(col(0.5, 1.0), float(rs.choice([0.0, 0.2]))))
        world.push(b.AARect(plane, lo, hi, lo, hi, ks[0], m1))
        world.push(b.AARect(plane, lo, hi, lo, hi, ks[1], m2))
        if rs.rand() < 0.3:
            world.push(b.AARect(plane, lo, hi, lo, hi, float(rs.uniform(1.05, 1.5) * L), lam()))      # a third parallel wall behind: pair + single
    if light_at >= len(axes):
        world.push(lamp)
    for _ in range(rs.randint(0, 3)):
        sz = rs.uniform(0.15, 0.35, 3) * L
        box = b.Cube((0.0, 0.0, 0.0), tuple(float(x) for x in sz), lam())
        world.push(b.Translate(b.Rotate(1, box, float(rs.uniform(-40, 40))), tuple(float(x) for x in rs.uniform(0.1, 0.6, 3) * L)))
    b.set_scene(world, [lamp] if rs.rand() < 0.8 else [])
    where = rs.randint(0, 4)
    if where == 0:      # inside
        frm = tuple(float(x) for x in rs.uniform(0.2, 0.8, 3) * L)
    elif where == 1:    # outside, looking in through the open side (or through a wall)
        frm = (float(rs.uniform(0.3, 0.7) * L), float(rs.uniform(0.3, 0.7) * L), -1.5 * L)
    elif where == 2:    # exactly on the plane of a wall
        frm = [float(x) for x in rs.uniform(0.2, 0.8, 3) * L]
        frm[rs.randint(0, 3)] = float(rs.choice([0.0, L]))
        frm = tuple(frm)
    else:               # outside past a corner: two slabs in front
        frm = (-0.7 * L, 1.6 * L, -0.9 * L)
    cam = Camera(frm, (0.5 * L, 0.45 * L, 0.55 * L), (0.0, 1.0, 0.0), float(rs.uniform(35, 70)), 1.0, float(rs.choice([0.0, 0.0, 0.02 * L])), L, 0.0, 1.0)
    return b, cam, col(0.0, 0.3)


@pytest.mark.parametrize("seed", list(range(24)))
def test_random_room_scene_parity(pbe, obe, seed):
    ob, ocam, obg = _rand_room_scene(obe, seed)
    pb, pcam, pbg = _rand_room_scene(pbe, seed)
    _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, 91 + seed, max_bad=2)
    info = R.last_launch_info(pb)
    assert info["threads"] == 256 and info["bvh_nodes"] == 0 and R.last_loop_info(pb)["feats"] == 0, "not the lean list-scene kernel"


def _rand_box_room_scene(be, seed):
    """Walls that are EXACT faces of one axis-aligned box — what rt_flatten.cpp's form_room turns into one object tested through the Cube
    fast path's ROOM form (round 6: the Cornell room's five walls, main.rs:291-296) — in a random list order, 3 to 6 of the six faces
    (three: no room is formed), between and around them whatever can stand in a list scene: the lamp, rotated boxes, a bare Cube, and
    the things that TIE with a wall bit for bit — a patch in a wall's own plane (bare, or under a FlipNormal), a second wall on the
    same face — placed before, between and after the walls, so that HittableList::hit's later-item-wins rule (hit.rs:62-68) decides
    samples whichever way the room's index-aware tie rule could get wrong.  Cameras: inside, outside looking through an absent face,
    outside looking at a wall's back, on a wall's plane, in a corner, on an edge line of the box."""
    rs = np.random.RandomState(9100 + seed)
    b = SceneBuilder(be)

    def col(lo=0.05, hi=0.95):
        return tuple(float(x) for x in rs.uniform(lo, hi, 3))

    def mat():
        return b.Lambertian(b.ConstantTexture(col())) if rs.rand() < 0.75 else b.Metal(col(0.5, 1.0), float(rs.choice([0.0, 0.3])))

    L = float(rs.choice([100.0, 555.0, 12.5]))
    mn = np.array([0.0, 0.0, 0.0]) if rs.rand() < 0.5 else rs.uniform(-0.5, 0.3, 3) * L
    mx = mn + rs.uniform(0.6, 1.4, 3) * L
    axes = {Plane.XY: (2, 0, 1), Plane.XZ: (1, 0, 2), Plane.YZ: (0, 1, 2)}       # plane -> (k, a, b) axes, rect.rs:26-32

    def face(plane, hi, m):
        k, a_, b_ = axes[plane]
        return b.AARect(plane, float(mn[a_]), float(mx[a_]), float(mn[b_]), float(mx[b_]), float(mx[k] if hi else mn[k]), m)

    def patch(plane, hi, m):
        """a smaller rect in the same plane as a face: every hit on it ties with the wall's, bit for bit"""
        k, a_, b_ = axes[plane]
        lo_a, hi_a = sorted(rs.uniform(0.1, 0.9, 2)); lo_b, hi_b = sorted(rs.uniform(0.1, 0.9, 2))
        ext_a, ext_b = mx[a_] - mn[a_], mx[b_] - mn[b_]
        return b.AARect(plane, float(mn[a_] + lo_a * ext_a), float(mn[a_] + hi_a * ext_a), float(mn[b_] + lo_b * ext_b), float(mn[b_] + hi_b * ext_b),
                        float(mx[k] if hi else mn[k]), m)

    all_faces = [(p, h) for p in (Plane.XY, Plane.XZ, Plane.YZ) for h in (True, False)]
    n_faces = int(rs.choice([3, 4, 5, 5, 5, 6]))
    chosen = [all_faces[i] for i in rs.permutation(6)[:n_faces]]
    glow = b.DiffuseLight(b.ConstantTexture(col(4.0, 15.0)))
    ky = mx[1] - (mx[1] - mn[1]) * 2.0 ** -9
    lamp = b.FlipNormal(b.AARect(Plane.XZ, float(mn[0] + 0.3 * (mx[0] - mn[0])), float(mn[0] + 0.6 * (mx[0] - mn[0])),
                                 float(mn[2] + 0.35 * (mx[2] - mn[2])), float(mn[2] + 0.6 * (mx[2] - mn[2])), float(ky), glow))
    items = [face(p, h, mat()) for p, h in chosen]
    extras = [lamp]
    for _ in range(rs.randint(0, 4)):
        p, h = all_faces[rs.randint(0, 6)]
        kind = rs.randint(0, 4)
        if kind == 0:
            extras.append(patch(p, h, mat()))                                   # a bare patch: joins a run of rects, never a wall
        elif kind == 1:
            extras.append(b.FlipNormal(patch(p, h, mat())))                     # a wrapped patch: an object of its own
        elif kind == 2:
            extras.append(face(p, h, mat()))                                    # a second (or first) wall on a face: ties everywhere
        else:
            extras.append(b.FlipNormal(face(p, h, mat())))
    for _ in range(rs.randint(0, 3)):
        sz = rs.uniform(0.15, 0.35, 3) * (mx - mn)
        box = b.Cube((0.0, 0.0, 0.0), tuple(float(x) for x in sz), mat())
        at = tuple(float(x) for x in mn + rs.uniform(0.1, 0.55, 3) * (mx - mn))
        extras.append(b.Translate(b.Rotate(1, box, float(rs.uniform(-40, 40))), at) if rs.rand() < 0.7 else
                      b.Cube(at, tuple(float(x) for x in np.array(at) + sz), mat()))
    for e in extras:                                                            # anywhere in the list: before, between, after the walls
        items.insert(rs.randint(0, len(items) + 1), e)
    world = b.HittableList()
    for it in items:
        world.push(it)
    b.set_scene(world, [lamp] if rs.rand() < 0.8 else [])
    b.world_handle, b.box = world, (mn.copy(), mx.copy())                       # (for the single-ray known-answer test of the list search)
    ctr, ext = 0.5 * (mn + mx), mx - mn
    where = rs.randint(0, 6)
    if where == 0:      # inside
        frm = mn + rs.uniform(0.2, 0.8, 3) * ext
    elif where == 1:    # outside, in front of one face (absent: looks in; present: looks at its back)
        frm = ctr.copy(); ax = rs.randint(0, 3); frm[ax] = (mn[ax] - 1.5 * ext[ax]) if rs.rand() < 0.5 else (mx[ax] + 1.5 * ext[ax])
    elif where == 2:    # exactly on the plane of a face
        frm = mn + rs.uniform(0.2, 0.8, 3) * ext; ax = rs.randint(0, 3); frm[ax] = mn[ax] if rs.rand() < 0.5 else mx[ax]
    elif where == 3:    # outside past a corner
        frm = mn - rs.uniform(0.5, 1.2, 3) * ext
    elif where == 4:    # exactly in a corner of the box
        frm = np.where(rs.rand(3) < 0.5, mn, mx)
    else:               # on the line of an edge, outside
        frm = mn.copy(); frm[rs.randint(0, 3)] -= 0.8 * L
    at = ctr + rs.uniform(-0.1, 0.1, 3) * ext
    cam = Camera(tuple(float(x) for x in frm), tuple(float(x) for x in at), (0.0, 1.0, 0.0), float(rs.uniform(35, 80)), 1.0,
                 float(rs.choice([0.0, 0.0, 0.02 * L])), float(L), 0.0, 1.0)
    return b, cam, col(0.0, 0.3), n_faces


@pytest.mark.parametrize("seed", list(range(32)))
def test_random_box_room_scene_parity(pbe, obe, seed):
    ob, ocam, obg, _ = _rand_box_room_scene(obe, seed)
    pb, pcam, pbg, n_faces = _rand_box_room_scene(pbe, seed)
    _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, 131 + seed, max_bad=2)
    assert R.last_loop_info(pb)["feats"] == 0, "not the lean list-scene kernel"
    rooms = [o for o in R.debug_objects(pb) if o["is_cube"] & 2]
    assert len(rooms) <= 1 and (n_faces >= 3 or not rooms), (n_faces, rooms)   # (a room needs four walls — an extra one may stand on a fourth face — and nothing rotated between them)


def test_the_box_room_family_does_form_rooms(pbe):
    """(what the parity test above is for) of its 32 scenes a good part flattens to a list with a room — and some do not: fewer than four
    walls, or a rotated box between two walls (rt_flatten.cpp form_room)."""
    n = sum(any(o["is_cube"] & 2 for o in R.debug_objects(_rand_box_room_scene(pbe, seed)[0])) for seed in range(32))
    assert 10 <= n < 32, n


def _hostile_rays(rnd, n, mn, mx, planes_y=()):
    """Rays for the list search's known-answer test: origins inside / outside the box, exactly ON the planes of its faces (and of the given
    extra y planes: a lamp), in its corners; directions random, aimed at edges and corners, with one or two components EXACTLY zero (a plane
    distance of an origin on that plane is then 0 / 0 = NaN: accepted by `t < t_min || t > t_max`, and HittableList::hit's answer depends
    on the order of its items — what the room form must not change), denormal / 1e-30 / 1e30 components, and a few rays that are not finite."""
    ext = mx - mn
    o = mn + rnd.uniform(-0.6, 1.6, (n, 3)) * ext
    inside = rnd.integers(0, 2, n) == 0
    o[inside] = (mn + rnd.uniform(0.02, 0.98, (n, 3)) * ext)[inside]
    ys = np.array(list(planes_y) + [mn[1], mx[1]])
    for ax in range(3):                                                         # exactly on a plane (about half of the rays, often on two)
        on = rnd.integers(0, 4, n) == 0
        vals = ys if ax == 1 else np.array([mn[ax], mx[ax]])
        o[on, ax] = rnd.choice(vals, on.sum())
    tgt = mn + rnd.choice([0.0, 1.0, 0.5, 0.3], (n, 3), p=[0.3, 0.3, 0.2, 0.2]) * ext
    d = np.where((rnd.integers(0, 2, n) == 0)[:, None], tgt - o, rnd.normal(size=(n, 3)))
    d *= 10.0 ** rnd.uniform(-2, 2, (n, 1))
    for ax in range(3):                                                         # exact zeros: one component for a third of the rays, two for a tenth
        z = rnd.integers(0, 5, n) == 0
        d[z, ax] = rnd.choice([0.0, -0.0], z.sum())
    odd = rnd.integers(0, 40, n) == 0
    d[odd, rnd.integers(0, 3, odd.sum())] = rnd.choice([5e-324, -1e-310, 1e-45, 1e-39, -1e-30, 1e30, 1e300], odd.sum())
    bad = rnd.integers(0, 200, n) == 0
    which = rnd.integers(0, 6, bad.sum())
    vals = rnd.choice([np.nan, np.inf, -np.inf], bad.sum())
    both = np.concatenate([o, d], axis=1)
    both[np.flatnonzero(bad), which] = vals
    d_all_zero = (both[:, 3:] == 0.0).all(axis=1)
    both[d_all_zero, 3] = 1.0
    return np.ascontiguousarray(both)


def _list_hits_gpu(pbe, b, rays, t_min):
    n = len(rays)
    out = np.zeros((n, 12))
    tm = np.full(n, t_min)
    assert pbe.lib.rt_debug_list_hit(b.h, n, rays.ctypes.data, tm.ctypes.data, out.ctypes.data) == 0, pbe.lib.rt_last_error()
    return out


def _list_hits_oracle(ob, rays, t_min):
    from oracle import orc
    out = np.zeros((len(rays), 9))
    for i, r in enumerate(rays):
        h = orc.hit(ob, ob.world_handle, tuple(r[:3]), tuple(r[3:]), t_min=t_min)
        if h is not None:
            out[i] = [1.0, h["t"], *h["position"], *h["normal"][:3], 1.0 if h["front_face"] else 0.0][:9]
    return out


def _same(a, b):
    """equal as numbers, NaN == NaN, +0 == -0 NOT assumed: bit patterns except that any NaN matches any NaN"""
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("seed", list(range(12)))
def test_list_search_ray_by_ray_on_hostile_rays(pbe, obe, seed):
    """world.hit (main.rs:48) of a list scene for single rays, the kernels' own search (rt_debug_list_hit: world_hit + finalize_hit of the
    lean kernel) against the oracle's HittableList::hit: the same hit-or-miss, the same t, position, normal and front_face bit for bit
    (any NaN equals any NaN) on rays chosen to break the room form's order argument — see _hostile_rays.  Seeds 0-1: the Cornell box
    (the lamp between the walls); the others: random box rooms with patches and second walls that tie with the walls."""
    rnd = np.random.default_rng(500 + seed)
    if seed < 2:
        from raytracinginrust_amd import scenes

        def cornell(be):
            b = SceneBuilder(be)
            red, white, green = (b.Lambertian(b.ConstantTexture(c)) for c in ((0.65, 0.05, 0.05), (0.73, 0.73, 0.73), (0.12, 0.45, 0.15)))
            metal = b.Metal((0.8, 0.85, 0.88), 0.0)
            lamp = b.FlipNormal(b.AARect(Plane.XZ, 213.0, 343.0, 227.0, 332.0, 554.0, b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))))
            w = b.HittableList()                                                # main.rs:291-309
            w.push(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 555.0, green)); w.push(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 0.0, red)); w.push(lamp)
            w.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white)); w.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white))
            w.push(b.AARect(Plane.XY, 0.0, 555.0, 0.0, 555.0, 555.0, white))
            w.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white), -18.0), (130.0, 0.0, 65.0)))
            w.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), metal), 15.0), (265.0, 0.0, 295.0)))
            b.set_scene(w, [lamp])
            b.world_handle, b.box = w, (np.zeros(3), np.full(3, 555.0))
            return b
        pb, ob = cornell(pbe), cornell(obe)
        extra_y = (554.0,)
    else:
        pb = _rand_box_room_scene(pbe, 40 + seed)[0]
        ob = _rand_box_room_scene(obe, 40 + seed)[0]
        mn, mx = pb.box
        extra_y = (float(mx[1] - (mx[1] - mn[1]) * 2.0 ** -9),)
    n = 40000
    rays = _hostile_rays(rnd, n, pb.box[0], pb.box[1], extra_y)
    got = _list_hits_gpu(pbe, pb, rays, 1e-5)
    ref = _list_hits_oracle(ob, rays, 1e-5)
    hit_g, hit_r = got[:, 0] != 0.0, ref[:, 0] != 0.0
    assert np.array_equal(hit_g, hit_r), f"hit-or-miss differs for {int((hit_g != hit_r).sum())} rays, e.g. ray {rays[np.flatnonzero(hit_g != hit_r)[0]].tolist()}"
    h = hit_r
    ok = _same(got[h, 1], ref[h, 1]) & _same(got[h, 2:5], ref[h, 2:5]).all(axis=1) & _same(got[h, 5:8], ref[h, 5:8]).all(axis=1) & (got[h, 8] == ref[h, 8])
    assert ok.all(), f"{int((~ok).sum())} of {int(h.sum())} hits differ, e.g. ray {rays[np.flatnonzero(h)[np.flatnonzero(~ok)[0]]].tolist()}: " \
                     f"gpu {got[np.flatnonzero(h)[np.flatnonzero(~ok)[0]]].tolist()} oracle {ref[np.flatnonzero(h)[np.flatnonzero(~ok)[0]]].tolist()}"
    # the cases the test is for did occur: NaN hits (a 0 / 0 plane distance accepted), and rays with zero components that hit something
    assert np.isnan(ref[h, 1]).sum() >= (5 if seed < 2 else 0)
    assert ((rays[:, 3:] == 0.0).any(axis=1) & h).sum() > 1000
    if seed < 2:
        assert any(o["is_cube"] & 2 for o in R.debug_objects(pb))
        # and the path that serves them is what makes the answers equal: with it switched off (a test knob) the room's order shows —
        # a NaN hit of the lamp or of a wall "forgets" what was found before it, and the room is searched after the lamp, not around it
        import os
        os.environ["RT_ROOM_NO_NAN_PATH"] = "1"
        try:
            off = _list_hits_gpu(pbe, pb, rays, 1e-5)
        finally:
            del os.environ["RT_ROOM_NO_NAN_PATH"]
        differ = ((off[:, 0] != 0.0) != hit_r) | (hit_r & ~(_same(off[:, 1], ref[:, 1]) & _same(off[:, 5:8], ref[:, 5:8]).all(axis=1)))
        assert differ.sum() > 0, "the hostile rays never reach an order-dependent NaN hit: the test does not test what it says"
        assert not differ[~(rays[:, 3:] == 0.0).any(axis=1) & np.isfinite(rays).all(axis=1)].any(), "a finite ray without a zero component depends on the order"


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5, 8])
def test_room_form_in_the_f32_variant_is_the_plain_list(pbe, seed, monkeypatch):
    """The f32 throughput variant (RT_F32: statistical parity only, no Cube fast path) meets a room too: it searches the room's walls by
    their rect tests in list order, with the same tie rule and the same choice of list — its samples must be the plain list's word for word."""
    def mk():
        from raytracinginrust_amd import scenes
        return scenes.cornell_box(pbe) if seed == 0 else _rand_box_room_scene(pbe, 300 + seed)[:3]
    W, H, spp, depth = 48, 48, 8, 20
    b, cam, bg = mk()
    _, with_room = R.render(b, cam, bg, W, H, spp, depth, seed=7 + seed, flags=R.RT_F32, want_samples=True)
    has_room = any(o["is_cube"] & 2 for o in R.debug_objects(b))
    monkeypatch.setenv("RT_NO_ROOM", "1")
    b0, cam0, bg0 = mk()
    assert not any(o["is_cube"] & 2 for o in R.debug_objects(b0))
    _, plain = R.render(b0, cam0, bg0, W, H, spp, depth, seed=7 + seed, flags=R.RT_F32, want_samples=True)
    assert np.array_equal(with_room.view(np.uint64), plain.view(np.uint64)), f"room formed: {has_room}"
    assert seed != 0 or has_room

"""The scene forms the flattener used to refuse, rendered on the GPU against the oracle per sample: HittableLists inside `lights` (both
call sites of the light sampling: the Lambertian mixture and the PBR Microfacet arm), ConstantMedium boundaries of several objects (at the
top level, under Translate(Rotate(..)), as a BVH leaf; with a BVH and a mesh inside), wrapper chains longer than 8, and a random family
mixing all three.  Every such scene runs the all-features instantiation with object leaves (FEATS = F_ALL | F_NESTED = 639).  The lights'
pdf_value is also checked on the device bit for bit (rt_debug_light_pdf)."""
import numpy as np
import pytest

from oracle import orc
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Axis, Plane, SceneBuilder

from test_scene_forms_host import cornell_light_tree, long_chain_scene, medium_boundary_scene, random_forms_scene

pytestmark = pytest.mark.gpu

SAMPLE_RTOL = 1e-9
NESTED_FEATS = 639


def _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, seed, W=40, H=40, spp=8, depth=12, max_bad=2):
    ref, rs_, cnt = orc.render(ob, ocam, obg, W, H, spp, depth, seed=seed, want_samples=True, want_counters=True)
    got, gs = R.render(pb, pcam, pbg, W, H, spp, depth, seed=seed, want_samples=True)
    assert np.array_equal(np.isnan(gs), np.isnan(rs_)), "NaN pattern differs"
    assert np.array_equal(np.isinf(gs), np.isinf(rs_))
    fin = np.isfinite(rs_)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs_, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs_, 0.0)))).any(axis=-1)
    assert bad.sum() <= max_bad, f"{int(bad.sum())} of {W * H * spp} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"
    assert R.last_stats(pb)["nonfinite_samples"] == cnt["nonfinite"]
    return ref, got


def _check(make, seed, *args):
    ob, ocam, obg = make(orc.load(), *args)
    pb, pcam, pbg = make(R._lib.load(), *args)
    ref, got = _compare_with_oracle(pb, pcam, pbg, ob, ocam, obg, seed)
    assert R.last_loop_info(pb)["feats"] == NESTED_FEATS
    assert np.nansum(np.abs(ref)) > 0.0                    # (something is lit: the scene is not all background)
    return pb, pcam, pbg


@pytest.mark.parametrize("pbr", [False, True])
def test_light_tree_cornell(pbr):
    _check(cornell_light_tree, 31 + pbr, pbr)


@pytest.mark.parametrize("where", ["top", "wrapped", "bvh"])
def test_medium_boundary_of_several_objects(where):
    _check(medium_boundary_scene, 41, where)


@pytest.mark.parametrize("n", [9, 16, 40])
def test_long_wrapper_chains(n):
    _check(long_chain_scene, 51, n)


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_scene_forms(seed):
    _check(random_forms_scene, 61 + seed, seed)


@pytest.mark.parametrize("make,args", [(cornell_light_tree, (False,)), (cornell_light_tree, (True,)),
                                       (medium_boundary_scene, ("top",)), (medium_boundary_scene, ("wrapped",)),
                                       (medium_boundary_scene, ("bvh",)), (long_chain_scene, (40,)), (random_forms_scene, (3,))])
def test_f32_variant_renders_the_new_forms(make, args):
    """RT_F32 renders every new form (its accuracy claim stays the statistical one of test_parity_gpu.py)."""
    pb, cam, bg = make(R._lib.load(), *args)
    img = R.render(pb, cam, bg, 32, 32, 8, 12, flags=R.RT_F32)
    li = R.last_loop_info(pb)
    assert li["feats"] == NESTED_FEATS and li["kernel"].startswith("rt::pathtrace_kernel<float,")
    assert np.isfinite(img).any() and np.nansum(np.abs(img)) > 0.0      # (PBR scenes have 0/0 samples in the reference too: quirk B8)


def _kat_scene(be):
    """A light tree of every entry kind: rects on all three planes (under FlipNormals too), spheres, trait-default entries (Translate,
    Rotate, Cube, BVH, MovingSphere, Triangle), lists of one, lists under FlipNormal, four levels deep."""
    b = SceneBuilder(be)
    glow = b.DiffuseLight(b.ConstantTexture((4.0, 4.0, 4.0)))
    rxz = b.AARect(Plane.XZ, 213.0, 343.0, 227.0, 332.0, 554.0, glow)
    rxy = b.AARect(Plane.XY, 100.0, 200.0, 300.0, 420.0, 500.0, glow)
    ryz = b.AARect(Plane.YZ, 50.0, 150.0, 60.0, 260.0, 30.0, glow)
    s1 = b.Sphere((400.0, 100.0, 150.0), 45.0, glow)
    s2 = b.Sphere((150.0, 400.0, 300.0), 20.0, glow)
    world = b.HittableList()
    for h in (rxz, rxy, ryz, s1, s2):
        world.push(h)
    others = [b.Translate(s1, (1.0, 0.0, 0.0)), b.Rotate(Axis.Y, rxz, 10.0), b.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), glow),
              b.BVH([s1, s2], 0.0, 1.0), b.MovingSphere((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.0, 1.0, 5.0, glow),
              b.Triangle([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)], glow)]

    def lst(*items):
        l = b.HittableList()
        for h in items:
            l.push(h)
        return l

    deep = lst(rxy, lst(s2, lst(b.FlipNormal(ryz), others[2])), others[3])
    lights = [lst(b.FlipNormal(rxz)), lst(s1, lst(rxz), others[0]), rxy, b.FlipNormal(lst(ryz, others[4], deep)),
              lst(lst(lst(s2))), others[1], lst(others[5], s1, s2, rxz, ryz, rxy)]
    b.set_scene(world, lights)
    return b, {"rects": [(Plane.XZ, 213.0, 343.0, 227.0, 332.0, 554.0), (Plane.XY, 100.0, 200.0, 300.0, 420.0, 500.0),
                         (Plane.YZ, 50.0, 150.0, 60.0, 260.0, 30.0)],
               "spheres": [((400.0, 100.0, 150.0), 45.0), ((150.0, 400.0, 300.0), 20.0)]}


def _kat_pairs(geo, n, seed=5):
    """(origin, direction) pairs: uniform directions, directions to points ON rect edges and corners (grazing the boundaries of
    rect.rs:91-101's hit test), tangent to sphere silhouettes (sphere.rs:104-112), and directions with zero components."""
    rs = np.random.RandomState(seed)
    o = rs.uniform(-50.0, 600.0, (n, 3))
    d = rs.normal(size=(n, 3))
    kind = rs.randint(0, 5, n)
    for i in np.nonzero(kind == 1)[0]:                       # a point on a rect's edge (or a corner)
        plane, a0, a1, b0, b1, k = geo["rects"][rs.randint(0, 3)]
        a = rs.choice([a0, a1, rs.uniform(a0, a1)])
        bb = rs.choice([b0, b1]) if a not in (a0, a1) else rs.choice([b0, b1, rs.uniform(b0, b1)])
        p = {Plane.XY: (a, bb, k), Plane.XZ: (a, k, bb), Plane.YZ: (k, a, bb)}[plane]        # rect.rs:26-32
        d[i] = np.asarray(p) - o[i]
    for i in np.nonzero(kind == 2)[0]:                       # tangent to a sphere's silhouette
        c, r = geo["spheres"][rs.randint(0, 2)]
        w = np.asarray(c) - o[i]
        dist = np.linalg.norm(w)
        if dist <= r * 1.01:
            continue
        u = np.cross(w, rs.normal(size=3))
        u /= np.linalg.norm(u)
        ang = np.arcsin(r / dist) * rs.choice([1.0, 1.0 - 1e-12, 1.0 + 1e-12])
        d[i] = np.cos(ang) * w / dist + np.sin(ang) * u
    zero = np.nonzero(kind == 3)[0]                          # zero components
    for i in zero:
        d[i, rs.randint(0, 3)] = 0.0
        if rs.rand() < 0.3:
            d[i, rs.randint(0, 3)] = 0.0
    d[np.all(d == 0.0, axis=1)] = (0.0, 1.0, 0.0)
    return o, d


def test_light_pdf_device_known_answers():
    """rt_debug_light_pdf — the function the 639 kernels run — against the oracle's lights.pdf_value, bit for bit, on 100 000 pairs."""
    pb, geo = _kat_scene(R._lib.load())
    ob, _ = _kat_scene(orc.load())
    o, d = _kat_pairs(geo, 100_000)
    got = R.debug_light_pdf(pb, o, d)
    olib = orc.load().lib
    ref = np.array([olib.orc_lights_pdf_value(ob.h, orc._d(*o[i]), orc._d(*d[i])) for i in range(len(o))])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    diff = np.nonzero(got[fin].view(np.uint64) != ref[fin].view(np.uint64))[0]
    assert diff.size == 0, f"{diff.size} pairs differ; first: {o[fin][diff[:3]].tolist()} {d[fin][diff[:3]].tolist()}"
    assert (ref > 0.0).mean() > 0.05                          # (the pairs do hit lights)


def test_light_pdf_device_flat_list_matches_oracle():
    """A flat `lights` list through the same function: the Cornell box's one light."""
    from raytracinginrust_amd import scenes
    pb, _, _ = scenes.cornell_box(R._lib.load())
    ob, _, _ = scenes.cornell_box(orc.load())
    rs = np.random.RandomState(9)
    o = rs.uniform(0.0, 555.0, (4000, 3))
    d = np.array([278.0, 554.0, 280.0]) + rs.uniform(-80.0, 80.0, (4000, 3)) * (1.0, 0.0, 1.0) - o
    got = R.debug_light_pdf(pb, o, d)
    olib = orc.load().lib
    ref = np.array([olib.orc_lights_pdf_value(ob.h, orc._d(*o[i]), orc._d(*d[i])) for i in range(len(o))])
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))

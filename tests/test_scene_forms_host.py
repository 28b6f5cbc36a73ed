"""Scene forms the reference accepts that the flattener used to refuse (host only, no GPU): HittableLists inside `lights` (a light
tree), ConstantMedium boundaries that flatten to several objects, wrapper chains longer than 8.  What stays refused stays refused.
The scene builders here are shared with test_scene_forms_gpu.py, which renders them against the oracle."""
import numpy as np
import pytest

from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Axis, Camera, Plane, SceneBuilder

G_OBJ = 5                                       # rt_ir.h GeomKind: a run of sub-objects


def _cornell_room(b, light_mat):
    """The Cornell room of src/main.rs:278-296 (walls and the ceiling light) -> (world list, white, the light's AARect)."""
    red = b.Lambertian(b.ConstantTexture((0.65, 0.05, 0.05)))
    white = b.Lambertian(b.ConstantTexture((0.73, 0.73, 0.73)))
    green = b.Lambertian(b.ConstantTexture((0.12, 0.45, 0.15)))
    rect = b.AARect(Plane.XZ, 213.0, 343.0, 227.0, 332.0, 554.0, light_mat)
    world = b.HittableList()
    world.push(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 555.0, green))
    world.push(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 0.0, red))
    world.push(b.FlipNormal(rect))
    world.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white))
    world.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white))
    world.push(b.AARect(Plane.XY, 0.0, 555.0, 0.0, 555.0, 555.0, white))
    return world, white, rect


def _cornell_cam():
    return Camera((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.05, 10.0, 0.0, 1.0)


def cornell_light_tree(be, pbr=False):
    """The Cornell box with lights [List[FlipNormal(light)], List[Sphere light, List[rect]]] and a glowing sphere in the room.
    pbr: the tall box and a sphere are principled (PBR) materials, so the Microfacet arm's light sampling runs too."""
    b = SceneBuilder(be)
    light = b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))
    world, white, rect = _cornell_room(b, light)
    glow = b.Sphere((420.0, 90.0, 120.0), 45.0, b.DiffuseLight(b.ConstantTexture((4.0, 4.0, 4.0))))
    world.push(glow)
    tall_mat = b.PBR(b.ConstantTexture((0.8, 0.6, 0.3)), 0.7, 0.0, 0.5, 0.3, 0.0, 0.0, 0.0, 0.5, 0.2, 0.8) if pbr else white
    world.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white), -18.0), (130.0, 0.0, 65.0)))
    world.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), tall_mat), 15.0), (265.0, 0.0, 295.0)))
    if pbr:
        world.push(b.Sphere((190.0, 260.0, 190.0), 60.0, b.PBR(b.ConstantTexture((0.2, 0.5, 0.9)), 0.1, 0.3, 0.5, 0.6, 0.2, 0.0, 0.4,
                                                                  0.5, 0.0, 0.0)))
    first = b.HittableList()
    first.push(b.FlipNormal(rect))
    inner = b.HittableList()
    inner.push(rect)
    second = b.HittableList()
    second.push(glow)
    second.push(inner)
    b.set_scene(world, [first, second])
    return b, _cornell_cam(), (0.0, 0.0, 0.0)


def _grey(b, v=0.6):
    return b.Lambertian(b.ConstantTexture((v, v, v)))


def _small_bvh(b, center, n=5, r=12.0):
    c = np.asarray(center, float)
    items = [b.Sphere(tuple(c + (30.0 * k - 60.0, 8.0 * (k % 2), 5.0 * k)), r, _grey(b, 0.3 + 0.1 * k)) for k in range(n)]
    return b.BVH(items, 0.0, 1.0)


def _small_mesh(b, center, s=50.0):
    """A closed tetrahedron as a Mesh (the `tris` HittableList)."""
    c = np.asarray(center, float)
    pos = np.array([[0.0, 0.0, 0.0], [s, 0.0, 0.0], [0.0, s, 0.0], [0.0, 0.0, s]]) + c
    idx = np.array([0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3], np.uint32)
    return b.Mesh(pos, idx, _grey(b, 0.5))


def medium_boundary_scene(be, where="top"):
    """Cornell room with ConstantMedia whose boundaries are lists of several objects (ConstantMedium<H: Hittable>, medium.rs:10-24):
    where = "top": [Sphere, Translate(Rotate(Cube))] and [BVH, AARect] at the top level; "wrapped": the same under Translate(Rotate(..));
    "bvh": [Mesh, Sphere] and [BVH, Translate(Cube)] media as BVH leaves beside bare primitives."""
    b = SceneBuilder(be)
    light = b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))
    world, white, rect = _cornell_room(b, light)
    glass = b.Dielectric(1.5)

    def mixed():
        l = b.HittableList()
        l.push(b.Sphere((200.0, 150.0, 200.0), 80.0, glass))
        l.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (120.0, 200.0, 120.0), white), 25.0), (300.0, 0.0, 250.0)))
        return b.ConstantMedium(l, 0.01, b.ConstantTexture((0.9, 0.9, 0.9)))

    def with_bvh():
        l = b.HittableList()
        l.push(_small_bvh(b, (280.0, 380.0, 300.0)))
        l.push(b.AARect(Plane.XY, 100.0, 450.0, 50.0, 300.0, 420.0, white))
        return b.ConstantMedium(l, 0.005, b.ConstantTexture((0.2, 0.4, 0.9)))

    def with_mesh():
        l = b.HittableList()
        l.push(_small_mesh(b, (120.0, 40.0, 150.0), 160.0))
        l.push(b.Sphere((420.0, 120.0, 330.0), 70.0, white))
        return b.ConstantMedium(l, 0.02, b.ConstantTexture((0.9, 0.3, 0.2)))

    if where == "top":
        world.push(mixed())
        world.push(with_bvh())
    elif where == "wrapped":
        world.push(b.Translate(b.Rotate(Axis.Y, mixed(), -10.0), (20.0, 0.0, 10.0)))
        world.push(b.Translate(b.Rotate(Axis.X, with_bvh(), 4.0), (0.0, -15.0, 0.0)))
    elif where == "bvh":
        leaves = [with_mesh(), b.Sphere((100.0, 400.0, 400.0), 40.0, white), b.Sphere((450.0, 450.0, 150.0), 30.0, glass)]
        l = b.HittableList()
        l.push(_small_bvh(b, (300.0, 300.0, 350.0), 4, 15.0))
        l.push(b.Translate(b.Cube((0.0, 0.0, 0.0), (60.0, 60.0, 60.0), white), (380.0, 20.0, 80.0)))
        leaves.append(b.ConstantMedium(l, 0.01, b.ConstantTexture((0.5, 0.9, 0.5))))
        world.push(b.BVH(leaves, 0.0, 1.0))
    else:
        raise KeyError(where)
    b.set_scene(world, [rect])
    return b, _cornell_cam(), (0.0, 0.0, 0.0)


def _chain(b, h, n, seed):
    """n wrappers around h: Translate / Rotate (every axis) / FlipNormal, small enough that the object stays in the room."""
    rs = np.random.RandomState(seed)
    for k in range(n):
        kind = k % 3 if k < 3 else rs.randint(0, 3)
        if kind == 0:
            h = b.Translate(h, tuple(float(x) for x in rs.uniform(-6.0, 6.0, 3)))
        elif kind == 1:
            h = b.Rotate(int(rs.randint(0, 3)), h, float(rs.uniform(-4.0, 4.0)))
        else:
            h = b.FlipNormal(h)
    return h


def long_chain_scene(be, n):
    """A Cube and a BVH each under a chain of n wrappers (rotations included) in the Cornell room."""
    b = SceneBuilder(be)
    light = b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))
    world, white, rect = _cornell_room(b, light)
    world.push(_chain(b, b.Cube((150.0, 0.0, 150.0), (300.0, 200.0, 300.0), white), n, 10 + n))
    world.push(_chain(b, _small_bvh(b, (330.0, 380.0, 300.0)), n, 20 + n))
    b.set_scene(world, [rect])
    return b, _cornell_cam(), (0.0, 0.0, 0.0)


def random_forms_scene(be, seed):
    """A random mix of the three forms: a light tree (rects, spheres, trait-default entries, FlipNormals, 1-4 levels), 1-2 media over
    mixed boundary lists (top level, wrapped, or as a BVH leaf), objects under chains of 9-40 wrappers."""
    rs = np.random.RandomState(7000 + seed)
    b = SceneBuilder(be)
    light = b.DiffuseLight(b.ConstantTexture((12.0, 12.0, 12.0)))
    world, white, rect = _cornell_room(b, light)

    def col():
        return tuple(float(x) for x in rs.uniform(0.1, 0.9, 3))

    def mat():
        k = rs.randint(0, 4)
        if k == 0:
            return b.Metal(col(), float(rs.choice([0.0, 0.3])))
        if k == 1:
            return b.Dielectric(1.5)
        return b.Lambertian(b.ConstantTexture(col()))

    def pos(lo=80.0, hi=470.0):
        return rs.uniform(lo, hi, 3)

    def prim(size=60.0):
        k = rs.randint(0, 4)
        p = pos()
        if k == 0:
            return b.Sphere(tuple(p), float(rs.uniform(20.0, size)), mat())
        if k == 1:
            return b.Cube(tuple(p - size), tuple(p + rs.uniform(0.3, 1.0, 3) * size), mat())
        if k == 2:
            return b.Translate(b.Rotate(int(rs.randint(0, 3)), b.Cube((0.0, 0.0, 0.0), (size, size, size), mat()),
                                        float(rs.uniform(-40, 40))), tuple(p))
        return _small_bvh(b, tuple(p), int(rs.randint(2, 6)), float(rs.uniform(8.0, 20.0)))

    glow = b.Sphere(tuple(pos(150.0, 400.0)), 25.0, b.DiffuseLight(b.ConstantTexture(col())))
    world.push(glow)
    for _ in range(rs.randint(1, 3)):
        l = b.HittableList()
        for _ in range(rs.randint(2, 4)):
            l.push(prim())
        m = b.ConstantMedium(l, float(rs.choice([0.003, 0.01, 0.03])), b.ConstantTexture(col()))
        w = rs.randint(0, 3)
        if w == 0:
            world.push(m)
        elif w == 1:
            world.push(b.Translate(b.Rotate(int(rs.randint(0, 3)), m, float(rs.uniform(-5, 5))), tuple(rs.uniform(-10, 10, 3))))
        else:
            world.push(b.BVH([m, prim(40.0), prim(40.0)], 0.0, 1.0))
    for _ in range(rs.randint(1, 3)):
        world.push(_chain(b, prim(50.0), int(rs.choice([9, 12, 25, 40])), int(rs.randint(0, 1 << 30))))

    def light_node(depth):
        k = rs.randint(0, 6 if depth < 3 else 4)
        if k == 0:
            return rect
        if k == 1:
            return b.FlipNormal(rect)
        if k == 2:
            return glow
        if k == 3:
            return b.Translate(glow, (1.0, 0.0, 0.0)) if rs.rand() < 0.5 else b.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), white)
        l = b.HittableList()
        for _ in range(rs.randint(1, 4)):
            l.push(light_node(depth + 1))
        return l if k == 4 else b.FlipNormal(l)

    lights = [light_node(1) for _ in range(rs.randint(1, 3))]
    nested = b.HittableList()
    nested.push(rect)
    lights.append(nested)                        # (at least one list inside `lights`)
    b.set_scene(world, lights)
    return b, _cornell_cam(), (0.0, 0.0, 0.0)


# ---------------------------------------------------------------- the flattener accepts the new forms


def test_flatten_light_tree(pbe):
    b, _, _ = cornell_light_tree(pbe)
    got = R.flatten(b)
    assert got["lights"] == 2 + 1 + 2 + 1          # top [first, second]; first = [flip(rect)]; second = [glow, inner]; inner = [rect]
    b2, _, _ = cornell_light_tree(pbe, pbr=True)
    assert R.flatten(b2)["lights"] == 6


def test_flat_lights_keep_their_table(pbe):
    from raytracinginrust_amd import scenes
    b, _, _ = scenes.cornell_box(pbe)
    assert R.flatten(b)["lights"] == 1


def test_flatten_light_tree_depth_limit(pbe):
    b = SceneBuilder(pbe)
    light = b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))
    world, _, rect = _cornell_room(b, light)

    def nest(levels):
        h = rect
        for _ in range(levels):
            l = b.HittableList()
            l.push(h)
            h = l
        return h

    b.set_scene(world, [nest(16)])
    assert R.flatten(b)["lights"] == 17
    b2 = SceneBuilder(pbe)
    world2, _, rect2 = _cornell_room(b2, b2.DiffuseLight(b2.ConstantTexture((1.0, 1.0, 1.0))))
    h = rect2
    for _ in range(17):
        l = b2.HittableList()
        l.push(h)
        h = l
    b2.set_scene(world2, [h])
    with pytest.raises(R.RenderError, match="RT_MAX_LIGHT_NEST"):
        R.flatten(b2)


def test_empty_nested_light_list_raises(pbe):
    """The reference panics on choose(..).unwrap() of an empty list (hit.rs:95): an error at flatten time (deviation D16)."""
    for under_flip in (False, True):
        b = SceneBuilder(pbe)
        light = b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))
        world, _, rect = _cornell_room(b, light)
        inner = b.HittableList()
        outer = b.HittableList()
        outer.push(rect)
        outer.push(b.FlipNormal(inner) if under_flip else inner)
        b.set_scene(world, [outer])
        with pytest.raises(R.RenderError, match="empty HittableList inside `lights`"):
            R.flatten(b)


@pytest.mark.parametrize("where", ["top", "wrapped", "bvh"])
def test_flatten_multi_object_medium_boundary(pbe, where):
    b, _, _ = medium_boundary_scene(pbe, where)
    R.flatten(b)
    objs = R.debug_objects(b, top_only=False)
    media = [o for o in objs if o["medium"] != 0xFFFFFFFF]
    runs = [o for o in media if o["geom_kind"] == G_OBJ]
    assert len(runs) == 2
    n = len(objs)
    for o in runs:
        assert o["geom_count"] >= 2 and o["geom_first"] + o["geom_count"] <= n
        for sub in objs[o["geom_first"]: o["geom_first"] + o["geom_count"]]:
            assert sub["medium"] == 0xFFFFFFFF                          # no medium inside a boundary
            assert sub["nest"] & 0xFF == o["n_ops"]                     # the medium object's ops lie outside every sub-object's own


def test_flatten_medium_over_sphere_and_wrapped_cube(pbe):
    b = SceneBuilder(pbe)
    m = _grey(b)
    l = b.HittableList()
    l.push(b.Sphere((0.0, 0.0, 0.0), 1.0, m))
    l.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m), 30.0), (3.0, 0.0, 0.0)))
    world = b.HittableList()
    world.push(b.ConstantMedium(l, 0.1, b.ConstantTexture((1.0, 1.0, 1.0))))
    b.set_scene(world, [])
    R.flatten(b)
    top = R.debug_objects(b)
    assert len(top) == 1 and top[0]["geom_kind"] == G_OBJ and top[0]["geom_count"] == 2


def test_single_object_boundaries_keep_their_form(pbe):
    """A boundary list that is one object (one item, or a run of bare primitives of one kind) flattens as it always did."""
    b = SceneBuilder(pbe)
    m = _grey(b)
    world = b.HittableList()
    world.push(b.ConstantMedium(_small_mesh(b, (0.0, 0.0, 0.0)), 0.1, b.ConstantTexture((1.0, 1.0, 1.0))))
    one = b.HittableList()
    one.push(b.Translate(b.Sphere((0.0, 0.0, 0.0), 1.0, m), (1.0, 0.0, 0.0)))
    world.push(b.ConstantMedium(one, 0.1, b.ConstantTexture((1.0, 1.0, 1.0))))
    b.set_scene(world, [])
    R.flatten(b)
    assert [o["geom_kind"] for o in R.debug_objects(b, top_only=False)] == [3, 1]      # G_TRI range, G_SPHERE


@pytest.mark.parametrize("n", [9, 32, 200, 255])
def test_flatten_long_wrapper_chains(pbe, n):
    b = SceneBuilder(pbe)
    m = _grey(b)
    h = _chain(b, b.Cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m), n, n)
    g = _chain(b, _small_bvh(b, (0.0, 0.0, 0.0)), n, n + 1)
    world = b.HittableList()
    world.push(h)
    world.push(g)
    b.set_scene(world, [])
    assert R.flatten(b)["ops"] == 2 * n
    assert [o["n_ops"] for o in R.debug_objects(b)] == [n, n]


def test_wrapper_chain_limit_still_an_error(pbe):
    b = SceneBuilder(pbe)
    h = _chain(b, b.Sphere((0.0, 0.0, 0.0), 1.0, _grey(b)), 256, 3)
    b.set_scene(h, [])
    with pytest.raises(R.RenderError, match="RT_MAX_OPS"):
        R.flatten(b)


def test_long_chain_inside_bvh_leaf_and_medium(pbe):
    """Chain positions are packed into 8 bits each (DObject::nest): a medium under 100 wrappers inside a BVH leaf, whose boundary items
    carry 50 more."""
    b = SceneBuilder(pbe)
    m = _grey(b)
    l = b.HittableList()
    l.push(_chain(b, b.Sphere((0.0, 0.0, 0.0), 1.0, m), 50, 1))
    l.push(b.Sphere((3.0, 0.0, 0.0), 1.0, m))
    med = _chain(b, b.ConstantMedium(l, 0.1, b.ConstantTexture((1.0, 1.0, 1.0))), 100, 2)
    b.set_scene(b.BVH([med, b.Sphere((9.0, 0.0, 0.0), 1.0, m)], 0.0, 1.0), [])
    R.flatten(b)
    objs = R.debug_objects(b, top_only=False)
    run = [o for o in objs if o["geom_kind"] == G_OBJ and o["medium"] != 0xFFFFFFFF]
    assert len(run) == 1 and run[0]["n_ops"] == 100 and (run[0]["nest"] >> 8) & 0xFF == 100
    subs = objs[run[0]["geom_first"]: run[0]["geom_first"] + 2]
    assert [s["n_ops"] for s in subs] == [150, 100] and all(s["nest"] & 0xFF == 100 for s in subs)


@pytest.mark.parametrize("seed", range(4))
def test_random_forms_flatten(pbe, seed):
    b, _, _ = random_forms_scene(pbe, seed)
    R.flatten(b)


# ---------------------------------------------------------------- what stays refused


def test_deeper_bvh_nesting_still_refused(pbe):
    b = SceneBuilder(pbe)
    m = _grey(b)
    lvl2 = b.BVH([b.Sphere((0, 0, 0), 1.0, m), b.Sphere((3, 0, 0), 1.0, m)], 0.0, 1.0)
    lvl1 = b.BVH([lvl2, b.Sphere((6, 0, 0), 1.0, m)], 0.0, 1.0)
    b.set_scene(b.BVH([lvl1, b.Sphere((9, 0, 0), 1.0, m)], 0.0, 1.0), [])
    with pytest.raises(R.RenderError, match="RT_MAX_NEST"):
        R.flatten(b)
    # a boundary list counts at the level its medium stands at: a BVH inside a BVH inside the boundary of a medium in a BVH leaf
    b2 = SceneBuilder(pbe)
    m2 = _grey(b2)
    l = b2.HittableList()
    l.push(b2.BVH([b2.BVH([b2.Sphere((0, 0, 0), 1.0, m2), b2.Sphere((2, 0, 0), 1.0, m2)], 0.0, 1.0), b2.Sphere((5, 0, 0), 1.0, m2)], 0.0, 1.0))
    l.push(b2.Sphere((8, 0, 0), 1.0, m2))
    b2.set_scene(b2.BVH([b2.ConstantMedium(l, 0.1, b2.ConstantTexture((1, 1, 1))), b2.Sphere((20, 0, 0), 1.0, m2)], 0.0, 1.0), [])
    with pytest.raises(R.RenderError, match="RT_MAX_NEST"):
        R.flatten(b2)


@pytest.mark.parametrize("where", ["list", "bvh", "wrapped"])
def test_medium_in_medium_boundary_still_refused(pbe, where):
    b = SceneBuilder(pbe)
    m = _grey(b)
    tex = b.ConstantTexture((1.0, 1.0, 1.0))
    inner = b.ConstantMedium(b.Sphere((0.0, 0.0, 0.0), 1.0, m), 0.1, tex)
    l = b.HittableList()
    l.push(b.Sphere((4.0, 0.0, 0.0), 1.0, m))
    if where == "list":
        l.push(inner)
    elif where == "bvh":
        l.push(b.BVH([inner, b.Sphere((8.0, 0.0, 0.0), 1.0, m)], 0.0, 1.0))
    else:
        l.push(b.Translate(inner, (1.0, 0.0, 0.0)))
    b.set_scene(b.ConstantMedium(l, 0.1, tex), [])
    with pytest.raises(R.RenderError, match="nested ConstantMedium"):
        R.flatten(b)


# ---------------------------------------------------------------- which materials read (u, v)
def test_needs_uv_sees_an_image_behind_any_number_of_checkers(tmp_path):
    """MAT_NEEDS_UV (rt_flatten.cpp) decides whether finalize_hit computes u, v at all; without it an ImageTexture is sampled at (0, 0).  The
    flag used to be found by a recursion that gave up 65 levels down and memoised the answer, so an image under more than 64 CheckTextures
    lost it (on the device: tests/test_texture_walk_gpu.py::test_image_behind_a_chain_of_checkers_on_a_sphere).  No C-ABI call shows a
    flattened material, so tests/reads_uv_main.cpp reads the flattened scene behind the handle: every chain over an image has the flag —
    as both children, as the odd one, as the even one, under Lambertian, DiffuseLight, Isotropic and PBR — and no chain over a constant."""
    import os
    import subprocess
    from conftest import ROOT
    from raytracinginrust_amd import _lib
    if os.environ.get("RT_SANITIZER_RUN") == "1":      # (the library in use is the sanitizer build: a program without its runtime cannot load it)
        return
    exe = str(tmp_path / "reads_uv")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "reads_uv_main.cpp"), "-o", exe,
                    "-L" + libdir, "-lrt_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    flags = dict(line.split() for line in run.stdout.splitlines())
    assert len(flags) == 4 * 9 + 1
    wrong = sorted(name for name, f in flags.items() if f != ("0" if name.startswith("constant") else "1"))
    assert not wrong, f"MAT_NEEDS_UV wrong for {wrong}"

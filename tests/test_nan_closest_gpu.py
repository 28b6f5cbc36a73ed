"""Every hit search of the kernels entered with a NaN closest hit, against the oracle (cases: tests/nan_closest_cases.py; that they do
reach the searches with a NaN: tests/test_nan_closest_host.py).

Per structure, through the known-answer entry points, with t_max from {NaN, +inf, -inf, 0, -1, t_hit} and t_min from {1e-5, NaN, +inf,
-inf}: AABB::hit and its NaN-free and f32-filter forms, the Cube fast path, its room form with face masks (the form the mesh kernels'
room site runs too).  Per ray: the lean kernel's own search (rt_debug_list_hit) on every list scene — rooms of four, five and six walls,
objects between the walls, sources before the first, between and behind the last wall —, rt_query_hits on every scene class (BVHs of
triangles, of spheres, with object leaves, media, a mesh room; the BVHs with the whole tree staged in LDS, with part of it, with none),
and whole paths (rt_query_radiance, depth 4) on the same rays.  Everything also runs on the control rays, one ulp off the plane.

rt_query_hits and rt_query_radiance serve the reference's traversal order only (flags other than the radiance flags are an error), so the
near-first order has no entry for caller rays and is not run here.

What would flip if `t > t_max` were written `!(t <= t_max)` somewhere: every case with a NaN t_max that hits (the item would reject
everything: hit -> miss), and every NaN t under a numeric t_max (accepted now, rejected then); `t < t_min` against `!(t >= t_min)` the
same with a NaN t_min.  Both kinds are a third and more of the known-answer cases and every source ray of the scene tests."""
import functools

import numpy as np
import pytest

import nan_closest_cases as N
from oracle import orc
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Rng

from test_parity_gpu import _cube_kat_cases
from test_radiance_query_gpu import oracle_seed
from test_ray_query_gpu import MAX_BAD, SAMPLE_RTOL

pytestmark = pytest.mark.gpu

N_KAT = 20000
DEPTH = 4
RADIANCE_SEED = 2026


def _same(a, b):
    """bit patterns, except that any NaN matches any NaN"""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def _slab_t(boxes, rays):
    """A distance at which the ray meets a face's plane, computed as rect.rs:50 computes it — (k - o_k) / d_k, so t_max = t_hit ties with
    the reference's own t bit for bit: the entry distance of the box if positive, else the exit distance; 1.0 where that is no number."""
    with np.errstate(all="ignore"):
        t0 = (boxes[:, :3] - rays[:, :3]) / rays[:, 3:6]
        t1 = (boxes[:, 3:] - rays[:, :3]) / rays[:, 3:6]
        t_in = np.nanmax(np.where(np.isnan(t0) | np.isnan(t1), -np.inf, np.minimum(t0, t1)), axis=1)
        t_out = np.nanmin(np.where(np.isnan(t0) | np.isnan(t1), np.inf, np.maximum(t0, t1)), axis=1)
    t = np.where(t_in > 0.0, t_in, t_out)
    return np.where(np.isfinite(t), t, 1.0)


def _kinds(kmin, kmax, mask):
    idx = np.flatnonzero(mask)[:5]
    return [(int(i), N.T_MIN_KINDS[kmin[i]], N.T_MAX_KINDS[kmax[i]]) for i in idx]


# ------------------------------------------------------------------ per structure
def test_aabb_hit_with_nan_and_infinite_limits(pbe, obe):
    """AABB::hit (aabb.rs:19-36) on the device against the oracle's on the cases of test_aabb_hit_on_the_device_against_the_oracle with
    NaN / infinite limits: f64::max / min ignore a NaN, so a NaN t_max leaves the far planes alone to decide and a NaN t_min the near ones.
    The NaN-free form and the f32 filter are used by the kernels whatever the closest hit is: they must stay exact / conservative."""
    rnd = np.random.default_rng(70)
    n = N_KAT
    lo = rnd.uniform(-10, 10, (n, 3)); ext = rnd.uniform(0, 5, (n, 3))
    boxes = np.concatenate([lo, lo + ext], axis=1)
    o = rnd.uniform(-20, 20, (n, 3)); d = rnd.normal(size=(n, 3))
    special = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-320, 1e300, -1e300, 1e308]
    for i in range(0, n, 4):                 # every 4th case gets hostile components
        k = rnd.integers(0, 3)
        which = rnd.integers(0, 6)
        if which == 0: d[i, k] = rnd.choice([0.0, -0.0])
        elif which == 1: o[i, k] = boxes[i, k]; d[i, (k + 1) % 3] = 0.0          # origin on the min face, axis-parallel: 0 * inf
        elif which == 2: o[i, k] = rnd.choice(special)
        elif which == 3: d[i, k] = rnd.choice(special)
        elif which == 4: boxes[i, k], boxes[i, 3 + k] = boxes[i, 3 + k], boxes[i, k] - 1.0   # inverted box
        else: o[i] = boxes[i, :3]; d[i] = boxes[i, 3:] - boxes[i, :3]             # through two corners
    aimed = np.arange(n) % 4 == 1                                                  # a quarter aimed into the box: most random rays miss it
    d[aimed] = (lo + rnd.uniform(0.1, 0.9, (n, 3)) * ext - o)[aimed]
    rays = np.concatenate([o, d], axis=1)
    tl, kmin, kmax = N.kat_limits(rnd, _slab_t(boxes, rays))
    assert np.isnan(tl[:, 1]).sum() >= n // 3
    out = R.debug_aabb_hit(boxes, rays, tl)
    d3 = lambda v: orc._d(*v)
    ref = np.array([obe.lib.orc_aabb_hit(d3(boxes[i, :3]), d3(boxes[i, 3:]), d3(rays[i, :3]), d3(rays[i, 3:]), tl[i, 0], tl[i, 1]) for i in range(n)])
    differ = (out & 1) != ref
    assert not differ.any(), f"{int(differ.sum())} of {n} box tests differ from the oracle, (case, t_min, t_max): {_kinds(kmin, kmax, differ)}"
    nan_max, nan_min = np.isnan(tl[:, 1]), np.isnan(tl[:, 0])
    assert (ref[nan_max] == 1).sum() > 500 and (ref[nan_max] == 0).sum() > 500 and (ref[nan_min] == 1).sum() > 50
    box_tame = (boxes[:, :3] <= boxes[:, 3:]).all(axis=1) & np.isfinite(boxes).all(axis=1)
    use = ((out & 4) != 0) & box_tame
    assert use.sum() > n // 2 and (use & nan_max).sum() > n // 6
    wrong = use & (((out >> 1) & 1) != ref)
    assert not wrong.any(), f"the NaN-free form disagrees where it would be used: {_kinds(kmin, kmax, wrong)}"
    filt = use & ((out & 8) != 0)
    assert filt.sum() > n // 2 and (filt & nan_max).sum() > n // 6
    culled = filt & (ref == 1) & ((out & 16) == 0)
    assert not culled.any(), f"the f32 filter culled a box AABB::hit passes: {_kinds(kmin, kmax, culled)}"
    # the f32 kernels' pair (statistical parity only, but their filter must still contain their exact test)
    use32 = box_tame & ((out & 64) != 0)
    culled32 = use32 & ((out & 32) != 0) & ((out & 128) == 0)
    assert not culled32.any(), f"the f32 kernels' filter culled a box their exact test passes: {_kinds(kmin, kmax, culled32)}"


def _check_fast_path(out, oracle_out, kmin, kmax, what):
    t_ref, face_ref, t_fast, code = out[:, 0], out[:, 1].astype(int), out[:, 2], out[:, 3].astype(int)
    clear = (code & 8) != 0
    face_fast = (code & 7) - 1
    bad = clear & ((face_fast != face_ref) | ~_same(t_fast, t_ref))
    assert not bad.any(), f"{what}: {int(bad.sum())} clear cases differ from the rect tests, (case, t_min, t_max): {_kinds(kmin, kmax, bad)}"
    t_orc, face_orc = oracle_out[:, 0], oracle_out[:, 1].astype(int)
    assert (face_orc >= -1).all()
    differ = (face_orc != face_ref) | ~_same(t_orc, t_ref)
    assert not differ.any(), f"{what}: {int(differ.sum())} cases: the device's rect tests differ from the oracle's, {_kinds(kmin, kmax, differ)}"
    return clear, face_ref


def _fast_path_cases(seed):
    rnd = np.random.default_rng(seed)
    boxes, rays, _, about = _cube_kat_cases(rnd, N_KAT)
    boxes, rays = (np.ascontiguousarray(x, dtype=np.float64) for x in (boxes, rays))
    tl, kmin, kmax = N.kat_limits(rnd, _slab_t(boxes, rays))
    assert np.isnan(tl[:, 1]).sum() >= N_KAT // 3
    return rnd, boxes, rays, tl, kmin, kmax, about


def test_cube_fast_path_with_nan_and_infinite_limits(pbe, obe):
    """The Cube fast path (rt_kernel.hip: cube_fast) with the limits a NaN closest hit and hostile callers give it, on the hostile cases of
    test_cube_fast_path_against_the_six_rect_tests: wherever it calls a case clear, face and t are the six rect tests' bit for bit, and
    those are the oracle's Cube::hit on every case.  A NaN t_max accepts what +inf accepts (rect.rs:51), so it costs no clear case."""
    rnd, boxes, rays, tl, kmin, kmax, about = _fast_path_cases(71)
    n = N_KAT
    rect_m = float(np.abs(boxes).max()) * 1.0000002
    out = R.debug_cube_hit(boxes, rays, tl, rect_m)
    ref = np.zeros((n, 2))
    obe.lib.orc_cube_hit_batch(n, boxes.ctypes.data, rays.ctypes.data, tl.ctypes.data, ref.ctypes.data)
    clear, face_ref = _check_fast_path(out, ref, kmin, kmax, "Cube")
    nan_max = np.isnan(tl[:, 1]) & (kmin == 0)
    inf_max = np.isposinf(tl[:, 1]) & (kmin == 0)
    print(f"Cube: clear {clear.mean():.3f}; NaN t_max {clear[nan_max].mean():.3f} of {int(nan_max.sum())}, +inf t_max {clear[inf_max].mean():.3f} of {int(inf_max.sum())}; "
          f"hits with a NaN t_max {int((nan_max & (face_ref >= 0)).sum())}, NaN t {int(np.isnan(ref[face_ref >= 0, 0]).sum())}")
    assert (clear & nan_max).sum() > 1000 and (clear & nan_max & (face_ref >= 0)).sum() > 300
    assert clear[nan_max].mean() > clear[inf_max].mean() - 0.05, "a NaN t_max is classed unclear where +inf is clear"
    assert (np.isnan(tl[:, 0]) & (face_ref >= 0)).sum() > 100 and ((kmax == 5) & (face_ref >= 0)).sum() > 100


def test_room_form_with_nan_and_infinite_limits(pbe, obe):
    """The same for the room form with face masks (every set of faces; the Cornell room's; all six) — the form that serves the lean kernel's
    rooms and the mesh kernels' room site — against the oracle's HittableList over the AARects of the faces that exist."""
    rnd, boxes, rays, tl, kmin, kmax, about = _fast_path_cases(72)
    n = N_KAT
    masks = rnd.integers(0, 64, n).astype(np.uint32)
    masks[rnd.integers(0, 5, n) == 0] = 0x3D
    masks[rnd.integers(0, 10, n) == 0] = 0x3E
    masks[rnd.integers(0, 20, n) == 0] = 0x3F
    rect_m = float(np.abs(boxes).max()) * 1.0000002
    out = R.debug_room_hit(boxes, rays, tl, rect_m, masks)
    ref = np.zeros((n, 2))
    obe.lib.orc_room_hit_batch(n, boxes.ctypes.data, rays.ctypes.data, tl.ctypes.data, masks.ctypes.data, ref.ctypes.data)
    clear, face_ref = _check_fast_path(out, ref, kmin, kmax, "room")
    hit = face_ref >= 0
    assert (((masks[hit] >> face_ref[hit]) & 1) == 1).all(), "a face that does not exist was hit"
    nan_max = np.isnan(tl[:, 1]) & (kmin == 0)
    inf_max = np.isposinf(tl[:, 1]) & (kmin == 0)
    print(f"room: clear {clear.mean():.3f}; NaN t_max {clear[nan_max].mean():.3f}, +inf t_max {clear[inf_max].mean():.3f}; hits with a NaN t_max {int((nan_max & hit).sum())}")
    assert (clear & nan_max).sum() > 1000 and (clear & nan_max & hit).sum() > 200
    assert clear[nan_max].mean() > clear[inf_max].mean() - 0.05, "a NaN t_max is classed unclear where +inf is clear"
    # every face there: the room form says what the Cube form says
    six = masks == 0x3F
    full = R.debug_cube_hit(boxes[six], rays[six], tl[six], rect_m)
    assert six.sum() > 500 and (out[six, 3] == full[:, 3]).all() and _same(out[six, 2], full[:, 2]).all()


# ------------------------------------------------------------------ per ray
@functools.lru_cache(maxsize=None)
def _product_scene(scene):
    return N.build(scene, _lib.load())


def _rays(scene):
    return N.rays_of(N.families_of(scene))[0]


def _list_differs(got, ref):
    """rt_debug_list_hit's records against the oracle's: hit-or-miss, t, position, normal bit for bit (NaN = NaN), front_face."""
    hit_g, hit_r = got[:, 0] != 0.0, ref[:, 0] != 0.0
    both = hit_g & hit_r
    return (hit_g != hit_r) | (both & ~(_same(got[:, 1:8], ref[:, 1:8]).all(axis=1) & (got[:, 8] == ref[:, 8])))


@pytest.mark.parametrize("scene", N.LIST_SCENES)
def test_list_search_entered_with_a_nan_closest_hit(scene, pbe):
    """The lean kernel's search (rt_debug_list_hit: world_hit_list + finalize_hit) ray by ray against the oracle's world.hit; zero rays
    differ.  The rotated sources' rays have no zero component: their waves search the list WITH the room (its walls moved behind what
    stood between them) and reach it with closest = NaN — what the order argument above world_hit_list claims is harmless."""
    pb = _product_scene(scene)
    assert R.flatten(pb)["bvh_nodes"] == 0
    if scene in N.ROOM_SCENES:
        assert any(o["is_cube"] & 2 for o in R.debug_objects(pb)), "no room was formed: the test does not test what it says"
    rays = np.ascontiguousarray(_rays(scene))
    got = R.debug_list_hit(pb, rays[:, :6], 1e-5)
    bad = _list_differs(got, N.oracle_hits(scene))
    assert not bad.any(), N.describe(scene, bad)
    # the search that rt_query_hits runs on a list scene is its own instantiation of the same code
    again = R.query_hits(pb, rays, 1e-5, N.SEED)
    bad = _query_differs(again, N.oracle_hits(scene))
    assert not bad.any(), N.describe(scene, bad)


def test_the_list_scenes_do_depend_on_the_nan_path(pbe, monkeypatch):
    """Teeth: with the route to the list as the reference has it switched off (RT_ROOM_NO_NAN_PATH, a test knob), rays with a zero
    component that start on the plane of a source BETWEEN the walls meet the room in the wrong order and differ from the oracle — and only
    those: no ray without a zero component changes, which is the claim about the rotated sources once more."""
    seen = set()
    for scene in ("room5_sources", "room5_between"):
        pb = _product_scene(scene)
        rays = np.ascontiguousarray(_rays(scene))
        _, names, control = N.rays_of(N.families_of(scene))
        monkeypatch.setenv("RT_ROOM_NO_NAN_PATH", "1")
        off = R.debug_list_hit(pb, rays[:, :6], 1e-5)
        monkeypatch.delenv("RT_ROOM_NO_NAN_PATH")
        bad = _list_differs(off, N.oracle_hits(scene))
        seen |= set(names[bad & ~control])
        zero = (rays[:, 3:6] == 0.0).any(axis=1)
        assert not (bad & ~zero).any(), N.describe(scene, bad & ~zero)
    assert seen, "no family depends on the order of the list: the cases never reach an order-dependent NaN hit"
    print("families that differ without the NaN path:", sorted(seen))


def _query_differs(got, ref):
    """rt_query_hits' records against the oracle's by the rules of tests/test_ray_query_gpu.py (_compare): hit-or-miss identical; t,
    position, normal bit for bit and front_face equal; a ConstantMedium's t / position and u, v within SAMPLE_RTOL (1 + |ref|)."""
    hit_g, hit_r = got[:, 0] != 0.0, ref[:, 0] != 0.0
    bad = hit_g != hit_r
    both = hit_g & hit_r
    medium = both & (got[:, 13] == -1.0)
    exact = _same(got[:, 1:8], ref[:, 1:8]).all(axis=1)
    with np.errstate(invalid="ignore"):
        close = (np.abs(got[:, 1:8] - ref[:, 1:8]) <= SAMPLE_RTOL * (1.0 + np.abs(ref[:, 1:8]))).all(axis=1)
        uv_set = (got[:, 9:11] != 0.0).any(axis=1)
        uv_ok = ~uv_set | (np.abs(got[:, 9:11] - ref[:, 9:11]) <= SAMPLE_RTOL * (1.0 + np.abs(ref[:, 9:11]))).all(axis=1)
    bad |= both & ~np.where(medium, close, exact)
    bad |= both & (got[:, 8] != ref[:, 8])
    bad |= both & ~uv_ok
    bad |= ~hit_g & ((got[:, 0:11] != 0.0).any(axis=1) | (got[:, 11:15] != -1.0).any(axis=1))
    bad |= got[:, 15] != 0.0
    return bad


@pytest.mark.parametrize("scene", N.QUERY_SCENES)
def test_world_hit_entered_with_a_nan_closest_hit(scene, pbe, monkeypatch):
    """world_hit<FEATS> of every other scene class (rt_query_hits) ray by ray against the oracle: make_filter with a NaN bound, bvh_accept,
    the exact and the NaN-free box tests, the object-leaf walk, ConstantMedium's `t2 > closest`, spheres, the mesh kernels' room.  The BVH
    scenes three ways — the tree staged in LDS as the launch plans it, 8 nodes of it, none: where a node comes from changes no word."""
    pb = _product_scene(scene)
    rays = np.ascontiguousarray(_rays(scene))
    media = scene in N.MEDIA_SCENES
    got = R.query_hits(pb, rays, 1e-5, N.SEED)
    bad = _query_differs(got, N.oracle_hits(scene))
    print(f"{scene}: {len(rays)} rays, {int((got[:, 0] != 0).sum())} hits, {int((got[:, 13] == -1.0).sum() - (got[:, 0] == 0).sum())} medium, {int(bad.sum())} differ")
    assert bad.sum() <= (MAX_BAD if media else 0), N.describe(scene, bad)
    if scene in N.BVH_SCENES:
        assert R.flatten(pb)["bvh_nodes"] > 8
        for limit in ("8", "0"):
            monkeypatch.setenv("RT_NODE_CACHE_MAX", limit)
            part = R.query_hits(pb, rays, 1e-5, N.SEED)
            changed = (part.view(np.uint64) != got.view(np.uint64)).any(axis=1)
            assert not changed.any(), f"RT_NODE_CACHE_MAX={limit}: " + N.describe(scene, changed)
        monkeypatch.delenv("RT_NODE_CACHE_MAX")


# ------------------------------------------------------------------ whole paths
@functools.lru_cache(maxsize=None)
def _oracle_radiance(scene):
    """The oracle's ray_color at depth DEPTH for every ray of the scene, ray k on the stream the product gives (ray k, sample 0)."""
    obe = orc.load()
    ob = N.oracle_scene(scene)
    rays = _rays(scene)
    out = np.zeros((len(rays), 3))
    for k, r in enumerate(rays):
        out[k] = orc.ray_color(ob, r[0:3], r[3:6], r[6], N.BG, DEPTH, Rng(obe, oracle_seed(RADIANCE_SEED, k), 0))
    return out


@pytest.mark.parametrize("scene", N.SCENES)
def test_paths_that_start_with_a_nan_closest_hit(scene, pbe):
    """ray_color along the same rays (rt_query_radiance, one sample, depth 4) against the oracle's with the same streams: the record made
    from a NaN hit — position NaN, the normal from set_face_normal on NaN — goes through the shading that follows it.  Per sample
    |d| <= 1e-9 (1 + |ref|); NaN and inf where the oracle has them and nowhere else; on the scenes with a medium at most MAX_BAD samples
    may diverge (a free-flight distance an ulp to the other side of a boundary: tests/test_radiance_query_gpu.py)."""
    pb = _product_scene(scene)
    rays = np.ascontiguousarray(_rays(scene))
    ref = _oracle_radiance(scene)
    _, samples, nonfinite = R.query_radiance(pb, rays, 1, DEPTH, N.BG, RADIANCE_SEED, want_samples=True)
    got = samples[:, 0, :]
    kinds = (np.isnan(got) != np.isnan(ref)).any(axis=1) | (np.isinf(got) != np.isinf(ref)).any(axis=1) | ((got == np.inf) != (ref == np.inf)).any(axis=1)
    fin = np.isfinite(ref) & np.isfinite(got)
    d = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0))
    bad = kinds | (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, ref, 0.0)))).any(axis=1)
    print(f"{scene}: {len(rays)} samples, {int((ref != 0.0).any(axis=1).sum())} non-zero, {int((~np.isfinite(ref)).any(axis=1).sum())} non-finite, "
          f"{int(bad.sum())} diverged, largest |d| / (1 + |ref|) = {float((d / (1.0 + np.abs(np.where(fin, ref, 0.0)))).max()):.3g}")
    assert (~np.isfinite(ref)).any(axis=1).sum() >= 100 and np.isfinite(ref).all(axis=1).sum() >= 1000      # NaN paths and ordinary ones, both
    assert bad.sum() <= (MAX_BAD if scene in N.MEDIA_SCENES else 0), N.describe(scene, bad)
    assert nonfinite == int((~np.isfinite(got)).any(axis=1).sum())

"""Ray queries on the GPU (rt_query_hits, rt_query_camera and their _device forms) against the oracle, ray by ray: world.hit (main.rs:48,
Hittable::hit) of every scene class — a list scene with a room (Cornell), a mesh scene whose tree is larger than the LDS share of a
workgroup (teapot room), one BVH with moving spheres that fits it (random spheres), media / image texture / noise (final scene), and a BVH
with object leaves (medium_boundary_scene("bvh")).

What is required: identical hit-or-miss; t, position and normal bit-identical (any NaN equals any NaN), front_face equal.  Exceptions, as
DESIGN §6 has them: a ConstantMedium hit goes through the device's `log`, and u, v through `atan2` / `acos`, which differ from glibc in
the last ulp — there SAMPLE_RTOL = 1e-9 (1 + |ref|) applies; and on the two scenes with media at most MAX_BAD = 2 rays of a batch may
differ in hit-or-miss or exceed that (a free-flight distance one ulp to the other side of a boundary: max_bad of
test_scene_forms_gpu.py).  Everywhere else the allowance is 0.

Camera mode is checked on the scenes without media only: the oracle exposes no way to continue a path's stream past the camera's draws,
which is the stream a ConstantMedium would draw from there; media are covered by the caller-ray tests."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import build_scene
from oracle import orc
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R
from raytracinginrust_amd import scenes
from raytracinginrust_amd.api import Camera, Plane, Rng, SceneBuilder

from test_scene_forms_host import medium_boundary_scene

pytestmark = pytest.mark.gpu

SAMPLE_RTOL = 1e-9
MAX_BAD = 2
N_RAYS = 4133                                   # 16 workgroups of 256 and a partial one whose last wave is partial too
SEED = 2024
MEDIA_SCENES = ("final", "medium_bvh")
SCENES = ("cornell", "teapot", "random", "final", "medium_bvh")
F = R.HIT_FIELDS


def _same(a, b):
    """bit patterns, except that any NaN matches any NaN (tests/test_fuzz_gpu.py)"""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(product scene, oracle scene, camera) of one of SCENES, built once."""
    pbe, obe = _lib.load(), orc.load()
    if name == "medium_bvh":
        pb, cam, _ = medium_boundary_scene(pbe, "bvh")
        ob, _, _ = medium_boundary_scene(obe, "bvh")
    else:
        earth = scenes.load_earthmap() if name == "final" else None
        pb, cam, _ = build_scene(name, pbe, earth)
        ob, _, _ = build_scene(name, obe, earth)
    return pb, ob, cam


def _world_box(ob):
    """The world's bounding box (orc_bounding_box).  A world with a Rotate in it has the whole-space box of rotate.rs:40-57: those are the
    Cornell-sized scenes, and the room's [0, 555]^3 stands in for the bounds that are not finite."""
    out = (C.c_double * 6)()
    assert orc.load().lib.orc_bounding_box(ob.h, ob.world.id, 0.0, 1.0, out)
    lo, hi = np.array(out[0:3]), np.array(out[3:6])
    return np.where(np.abs(lo) < 1e5, lo, 0.0), np.where(np.abs(hi) < 1e5, hi, 555.0)


@functools.lru_cache(maxsize=None)
def _rays(name):
    """N_RAYS rays for a scene: a third camera rays (rt_camera_ray, the scene's own camera at 64 x 36), a third with random origins in the
    world's bounding box and random directions, a third hostile — one or two direction components exactly zero, or the origin exactly on a
    face of the world's box (in the rooms: on a wall's plane), sometimes both (0 / 0 plane distances)."""
    _, ob, cam = _scene(name)
    rs = np.random.RandomState(1000 + SCENES.index(name))
    n_cam = N_RAYS // 3
    rays = np.zeros((N_RAYS, 7))
    for k in range(n_cam):
        rays[k] = R.camera_ray(cam, 64, 36, int(rs.randint(0, 64)), int(rs.randint(0, 36)), 77, int(rs.randint(0, 16)))
    lo, hi = _world_box(ob)
    # (the random scene's box is the ground sphere's, 2000 across: keep most origins near the things in it)
    span_lo, span_hi = np.maximum(lo, -600.0), np.minimum(hi, 700.0)
    rest = N_RAYS - n_cam
    rays[n_cam:, 0:3] = rs.uniform(span_lo, span_hi, (rest, 3))
    rays[n_cam:, 3:6] = rs.normal(size=(rest, 3))
    rays[n_cam:, 6] = rs.uniform(0.0, 1.0, rest)
    first_hostile = n_cam + rest // 2
    for k in range(first_hostile, N_RAYS):
        mode = rs.randint(0, 4)
        if mode in (0, 3):
            rays[k, 3 + rs.randint(0, 3)] = 0.0
        if mode == 1:
            a = rs.randint(0, 3)
            rays[k, 3 + a] = 0.0; rays[k, 3 + (a + 1 + rs.randint(0, 2)) % 3] = 0.0
        if mode in (2, 3):
            a = rs.randint(0, 3)
            rays[k, a] = (lo if rs.rand() < 0.5 else hi)[a]
    return rays


def _zero_component(rays):
    return (rays[:, 3:6] == 0.0).any(axis=1)


@functools.lru_cache(maxsize=None)
def _oracle_hits(name):
    """The oracle's answer for _rays(name), ray k with the stream of Rng(SEED, k): (hit mask, (n, 10) position[3] normal[3] t u v front)."""
    _, ob, _ = _scene(name)
    return _oracle(ob, _rays(name), SEED)


def _oracle(ob, rays, seed):
    obe = orc.load()
    hit = np.zeros(len(rays), bool); rec = np.zeros((len(rays), 10))
    for k, r in enumerate(rays):
        h = orc.hit(ob, ob.world, r[0:3], r[3:6], r[6], 1e-5, float("inf"), rng=Rng(obe, seed, k))
        if h is not None:
            hit[k] = True
            rec[k] = h["position"] + h["normal"] + [h["t"], h["u"], h["v"], 1.0 if h["front_face"] else 0.0]
    return hit, rec


def _certain_medium_hits(rays, hit, rec):
    """Hits that can only be a ConstantMedium's, from the oracle's record alone: medium.rs:45-55 sets normal (1, 0, 0) and front_face false
    whatever the ray; a surface's set_face_normal (hit.rs:34-41) leaves dot(direction, normal) <= 0.  So normal == (1, 0, 0), front_face
    false and direction.x > 0 is a medium hit (about half of them)."""
    return hit & (rec[:, 3] == 1.0) & (rec[:, 4] == 0.0) & (rec[:, 5] == 0.0) & (rec[:, 9] == 0.0) & (rays[:, 3] > 0.0)


def _compare(name, got, rays, hit, rec):
    """The number of rays of the batch that differ from the oracle (see the module docstring), and a description of the first few."""
    g_hit = got[:, 0] != 0.0
    bad = g_hit != hit
    both = g_hit & hit
    medium = both & (got[:, F["prim_kind"]][:, 0] == -1.0)
    geo_ref = np.concatenate([rec[:, 6:7], rec[:, 0:6]], axis=1)               # t, position, normal
    geo_got = got[:, 1:8]
    exact = _same(geo_got, geo_ref).all(axis=1)
    with np.errstate(invalid="ignore"):
        close = (np.abs(geo_got - geo_ref) <= SAMPLE_RTOL * (1.0 + np.abs(geo_ref))).all(axis=1)
        uv_ref = rec[:, 7:9]; uv_got = got[:, 9:11]
        uv_set = (uv_got != 0.0).any(axis=1)
        uv_ok = ~uv_set | (np.abs(uv_got - uv_ref) <= SAMPLE_RTOL * (1.0 + np.abs(uv_ref))).all(axis=1)
    bad |= both & ~np.where(medium, close, exact)
    bad |= both & (got[:, 8] != rec[:, 9])                                      # front_face
    bad |= both & ~uv_ok
    # a miss is [0] = 0, [11..14] = -1 and the rest 0; [15] is always 0
    miss = ~g_hit
    bad |= miss & ((got[:, 0:11] != 0.0).any(axis=1) | (got[:, 11:15] != -1.0).any(axis=1))
    bad |= got[:, 15] != 0.0
    # a medium hit names no material and no primitive, but its object
    bad |= medium & ((got[:, 11] != -1.0) | (got[:, 13] != -1.0) | (got[:, 14] != -1.0) | (got[:, 12] < 0.0))
    bad |= both & ~medium & ((got[:, 11:15] < 0.0).any(axis=1))
    idx = np.nonzero(bad)[0]
    text = "; ".join(f"ray {k}: {rays[k].tolist()} got {got[k, :9].tolist()} ref hit={bool(hit[k])} {geo_ref[k].tolist()}" for k in idx[:3])
    print(f"{name}: {len(rays)} rays, {int(hit.sum())} hits, {int(medium.sum())} medium, {int(uv_set.sum())} with u/v, {len(idx)} differ")
    return len(idx), text


@pytest.mark.parametrize("name", SCENES)
def test_caller_rays_against_the_oracle(name):
    pb, ob, _ = _scene(name)
    rays = _rays(name)
    hit, rec = _oracle_hits(name)
    # the batch is not vacuous (the oracle's answer alone; the seeds were chosen on the CPU)
    assert hit.mean() > 0.25
    assert (hit & _zero_component(rays)).sum() > 100
    if name in MEDIA_SCENES:
        assert _certain_medium_hits(rays, hit, rec).sum() > 20
    got = R.query_hits(pb, rays, 1e-5, SEED)
    n_bad, text = _compare(name, got, rays, hit, rec)
    assert n_bad <= (MAX_BAD if name in MEDIA_SCENES else 0), text
    assert R.last_query_ms(pb) > 0.0


@pytest.mark.parametrize("name", ["cornell", "teapot"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_batches(name, n):
    """One ray, one lane short of a wave, a wave, one lane more, a workgroup and a lane: the first n rays of the batch (ray k's stream
    depends on k alone, so the reference is the batch's)."""
    pb, _, _ = _scene(name)
    rays = _rays(name)[:n]
    hit, rec = _oracle_hits(name)
    got = R.query_hits(pb, rays, 1e-5, SEED)
    n_bad, text = _compare(name, got, rays, hit[:n], rec[:n])
    assert n_bad == 0, text


STAGE_W, STAGE_H = 17, 16                      # 272 items: one whole workgroup and a second whose only wave is partial


def assert_staging_changes_no_word(pb, call, monkeypatch):
    """Every query kernel copies the filter tree into LDS once per workgroup when the whole tree fits (the random spheres' does) and walks
    it from global memory otherwise.  `call()` -> the output arrays of one query of STAGE_W * STAGE_H items on scene `pb`: as it is, with
    nothing staged (RT_NODE_CACHE_MAX=0) and with the limit one node short of the tree, which is a second way to nothing — the launch
    report does not say what was staged, so the staged call is held to both.  Equal word for word.  (Shared by the six families' files.)"""
    nodes = R.flatten(pb)["bvh_nodes"]
    # the tree fits the workgroup's share of LDS, so the first call does stage: 32 bytes a filter node; the random spheres' class is held to 3
    # waves per SIMD in every family (the *Waves tables), so at most 3 workgroups share a CU's 160 KB, and the host rounds down to 1 KB
    assert nodes > 8 and nodes * 32 <= (160 * 1024 // 3) & ~1023, nodes
    monkeypatch.delenv("RT_NODE_CACHE_MAX", raising=False)
    staged = [np.array(a, np.float64) for a in call()]
    assert any((a != 0.0).any() for a in staged)
    for limit in ("0", str(nodes - 1)):
        monkeypatch.setenv("RT_NODE_CACHE_MAX", limit)
        for a, b in zip(staged, call()):
            words, other = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64)
            assert int((words != other).sum()) == 0, f"RT_NODE_CACHE_MAX={limit}"
    monkeypatch.delenv("RT_NODE_CACHE_MAX")


@pytest.mark.parametrize("form", ["caller_rays", "camera"])
def test_the_staged_filter_tree_changes_no_word(form, monkeypatch):
    pb, _, cam = _scene("random")
    rays = _rays("random")[:STAGE_W * STAGE_H]
    if form == "camera":
        assert_staging_changes_no_word(pb, lambda: R.query_camera(pb, cam, STAGE_W, STAGE_H, 1, SEED, want_rays=True), monkeypatch)
    else:
        assert_staging_changes_no_word(pb, lambda: (R.query_hits(pb, rays, 1e-5, SEED),), monkeypatch)


def _material_scene(be):
    """Three spheres, four walls and a sphere of smoke, every one with a material of its own -> (scene, [(kind, geometry, material id)])."""
    b = SceneBuilder(be)
    world = b.HittableList()
    things = []
    b.Lambertian(b.ConstantTexture((0.1, 0.1, 0.1)))                              # (handle 0 is nobody's: a default would show)
    for k, (c, r) in enumerate([((0.0, 0.0, 0.0), 1.0), ((3.0, 0.5, 1.0), 1.5), ((-2.5, 1.0, -2.0), 0.75)]):
        m = b.Lambertian(b.ConstantTexture((0.2 + 0.1 * k, 0.5, 0.5))) if k != 1 else b.Metal((0.8, 0.8, 0.8), 0.1)
        world.push(b.Sphere(c, r, m)); things.append(("sphere", (np.array(c), r), m.id))
    for k, (plane, axis, kk) in enumerate([(Plane.XZ, 1, -3.0), (Plane.XY, 2, 8.0), (Plane.YZ, 0, -9.0), (Plane.YZ, 0, 9.0)]):
        m = b.Lambertian(b.ConstantTexture((0.9, 0.1 * k, 0.3)))
        world.push(b.AARect(plane, -10.0, 10.0, -10.0, 10.0, kk, m)); things.append(("rect", (axis, kk), m.id))
    fog = b.ConstantMedium(b.Sphere((0.0, 3.0, 3.0), 2.0, b.Dielectric(1.5)), 0.8, b.ConstantTexture((1.0, 1.0, 1.0)))
    world.push(fog)
    b.set_scene(world, [])
    return b, things


def test_material_and_primitive_of_a_hit():
    """[11] is the handle the builder returned for the object's material, [13] the primitive's kind: the object is identified from the
    ORACLE's hit position; a hit inside the smoke reports material -1 and kind -1."""
    pb, things = _material_scene(_lib.load())
    ob, _ = _material_scene(orc.load())
    rs = np.random.RandomState(3)
    n = 1500
    rays = np.zeros((n, 7))
    rays[:, 0:3] = rs.uniform(-8.0, 8.0, (n, 3)) * (1.0, 0.3, 1.0) + (0.0, 1.0, 0.0)
    rays[:, 3:6] = rs.normal(size=(n, 3))
    hit, rec = _oracle(ob, rays, SEED)
    got = R.query_hits(pb, rays, 1e-5, SEED)
    assert np.array_equal(got[:, 0] != 0.0, hit)
    seen = set(); n_fog = 0
    for k in np.nonzero(hit)[0]:
        p = rec[k, 0:3]
        if got[k, 13] == -1.0:                                                   # the device says: smoke.  The oracle's record agrees
            assert rec[k, 3:6].tolist() == [1.0, 0.0, 0.0] and rec[k, 9] == 0.0 and np.linalg.norm(p - (0.0, 3.0, 3.0)) < 2.0 + 1e-9
            assert got[k, 11] == -1.0 and got[k, 14] == -1.0 and got[k, 12] >= 0.0
            n_fog += 1
            continue
        who = [i for i, (kind, g, _) in enumerate(things)
               if (kind == "sphere" and abs(np.linalg.norm(p - g[0]) - g[1]) < 1e-9) or (kind == "rect" and abs(p[g[0]] - g[1]) < 1e-9)]
        assert len(who) == 1, (k, p.tolist(), who)
        kind, _, mat = things[who[0]]
        assert got[k, 11] == mat, (k, who, got[k].tolist())
        assert got[k, 13] == (1.0 if kind == "sphere" else 0.0)
        seen.add(who[0])
    assert seen == set(range(len(things))) and n_fog > 10


@pytest.mark.parametrize("name", ["cornell", "random", "teapot"])
@pytest.mark.parametrize("sample", [0, 5])
def test_camera_mode(name, sample):
    """The camera ray of one sample of every pixel of a 33 x 17 frame, generated on the device: the rays equal the oracle's camera rays
    bit for bit, the records the oracle's world.hit, and rt_query_hits on the same rays gives the same words.  (Scenes without media:
    see the module docstring.)"""
    W, H, seed = 33, 17, 0x5EED + 3
    pb, ob, cam = _scene(name)
    hits, rays = R.query_camera(pb, cam, W, H, sample, seed, want_rays=True)
    olib = orc.load().lib
    ref = np.zeros((H, W, 7))
    buf = (C.c_double * 7)()
    for row in range(H):
        for i in range(W):
            olib.orc_camera_ray(C.byref(cam), W, H, i, H - 1 - row, seed, sample, buf)
            ref[row, i] = buf[:]
    assert np.array_equal(rays.view(np.uint64), ref.view(np.uint64))
    flat_rays = rays.reshape(-1, 7); flat = hits.reshape(-1, 16)
    hit, rec = _oracle(ob, flat_rays, 0)
    n_bad, text = _compare(name, flat, flat_rays, hit, rec)
    assert n_bad == 0, text
    assert hit.mean() > 0.25
    again = R.query_hits(pb, flat_rays, 1e-5, 0)
    assert np.array_equal(again.view(np.uint64), flat.view(np.uint64))
    without_rays = R.query_camera(pb, cam, W, H, sample, seed)
    assert np.array_equal(without_rays.view(np.uint64), hits.view(np.uint64))


@pytest.mark.parametrize("name", ["cornell", "random"])
def test_device_forms(name):
    """Torch tensors on a stream of the caller's: word for word the host forms; the record behind the n-th is not touched; a second call
    gives the same words (no atomics, no order dependence)."""
    import torch
    pb, _, cam = _scene(name)
    rays = _rays(name)
    n = 1001
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(rays[:n].copy()).to(dev)
        d_hits = torch.full((n + 1, 16), canary, dtype=torch.float64, device=dev)
        d_hits2 = torch.full((n + 1, 16), canary, dtype=torch.float64, device=dev)
        R.query_hits_device(pb, n, d_rays, d_hits, 1e-5, SEED, stream=stream.cuda_stream)
        R.query_hits_device(pb, n, d_rays, d_hits2, 1e-5, SEED, stream=stream.cuda_stream)
    stream.synchronize()
    a, b = d_hits.cpu().numpy(), d_hits2.cpu().numpy()
    host = R.query_hits(pb, rays[:n], 1e-5, SEED)
    assert np.array_equal(a[:n].view(np.uint64), host.view(np.uint64))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.all(a[n] == canary)
    with pytest.raises(R.RenderError, match="hit buffer too small"):
        R.query_hits_device(pb, n + 2, d_rays, d_hits, stream=stream.cuda_stream)
    # camera mode
    W, H = 33, 17
    with torch.cuda.stream(stream):
        c_hits = torch.full((W * H + 1, 16), canary, dtype=torch.float64, device=dev)
        c_rays = torch.full((W * H + 1, 7), canary, dtype=torch.float64, device=dev)
        R.query_camera_device(pb, cam, W, H, c_hits, 5, 99, d_rays_out=c_rays, stream=stream.cuda_stream)
    stream.synchronize()
    h_hits, h_rays = R.query_camera(pb, cam, W, H, 5, 99, want_rays=True)
    ch, cr = c_hits.cpu().numpy(), c_rays.cpu().numpy()
    assert np.array_equal(ch[:-1].view(np.uint64), h_hits.reshape(-1, 16).view(np.uint64)) and np.all(ch[-1] == canary)
    assert np.array_equal(cr[:-1].view(np.uint64), h_rays.reshape(-1, 7).view(np.uint64)) and np.all(cr[-1] == canary)


def test_frames_are_untouched_by_a_query_and_a_changed_scene_is_seen():
    pbe = _lib.load()
    pb, cam, bg = scenes.cornell_box(pbe)
    _, before = R.render(pb, cam, bg, 16, 16, 4, 12, want_samples=True)
    ms = R.last_kernel_ms(pb); info = R.last_launch_info(pb)
    ray = np.array([[278.0, 278.0, -800.0, 0.05, 0.1, 1.0, 0.0]])
    first = R.query_hits(pb, ray)
    R.query_camera(pb, cam, 16, 16)
    assert R.last_kernel_ms(pb) == ms and R.last_launch_info(pb) == info        # what the frames report is the frames'
    _, after = R.render(pb, cam, bg, 16, 16, 4, 12, want_samples=True)
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    # one more sphere in the ray's way: the next query sees it
    assert first[0, 0] == 1.0 and first[0, 13] == 0.0
    glass = pb.Dielectric(1.5)
    pb.world.push(pb.Sphere((278.0 + 0.05 * 900.0, 278.0 + 0.1 * 900.0, 100.0), 30.0, glass))
    second = R.query_hits(pb, ray)
    assert second[0, 0] == 1.0 and second[0, 13] == 1.0 and second[0, 11] == glass.id and second[0, 1] < first[0, 1]


def test_rtrender_aov_normal(tmp_path):
    """`rtrender --aov normal FILE` on the Cornell box at 32 x 32 writes the image render.aov_image makes of query_camera's records."""
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    out = tmp_path / "normal.ppm"
    subprocess.run([exe, "--scene", "cornell", "--width", "32", "--height", "32", "--aov", "normal", str(out)], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", "32", "32", "255"]
    img = np.array(tok[4:], dtype=np.int64).reshape(32, 32, 3)
    pb, cam, _ = scenes.cornell_box(_lib.load())
    want = R.aov_image(R.query_camera(pb, cam, 32, 32, 0, 0x5EED), "normal")
    assert np.array_equal(img, want.astype(np.int64))
    assert len({tuple(p) for p in img.reshape(-1, 3).tolist()}) >= 4             # walls of several orientations are in view

"""Radiance queries on the GPU (rt_query_radiance and its _device form) against the oracle, sample by sample: ray_color (main.rs:41-120) along
rays the caller chooses, on every scene class — a list scene with a room (Cornell), a mesh scene (teapot room), one BVH with moving spheres
(random spheres), media / image texture / noise (final scene), a BVH with object leaves (medium_boundary_scene("bvh")) and a scene with the
principled material.

The oracle's stream for (ray k, sample s) is Rng(seed', s) with seed' = seed + 2 G (((k - 0xFFFFFFFF) << 32) mod 2^64) mod 2^64: then
for_stream(seed', s) == for_path(seed, k, s) (tests/test_radiance_query_host.py pins the identity).

Tolerances are the project's: per sample |d| <= 1e-9 (1 + |ref|), per ray sum |d| <= 1e-9 (spp + |ref|), non-finite patterns
identical, at most MAX_BAD = 2 diverged samples per case (a free-flight distance one ulp to the other side of a boundary)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import build_scene
from oracle import orc
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R
from raytracinginrust_amd import scenes
from raytracinginrust_amd.api import Camera, Plane, Rng, SceneBuilder

from test_ray_query_gpu import _world_box
from test_scene_forms_host import medium_boundary_scene

pytestmark = pytest.mark.gpu

SAMPLE_RTOL = 1e-9
MAX_BAD = 2
N_RAYS = 1093                                   # 17 waves and a partial one
SPP = 5
SEED = 2025
SCENES = ("cornell", "teapot", "random", "final", "medium_bvh", "pbr")
G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
U = 2.0 ** -53


# Where the random and the hostile third of a scene's rays start, where the world's own box would leave most samples black (the oracle's answer
# alone decides: at least a quarter of a scene's samples must be non-zero).  Random spheres: the ground sphere's box is 2000 across and mostly
# below the ground; final scene: the lit middle of the room, under the lamp; principled sphere: around the sphere, under the lamp.
ORIGINS = {"random": (np.array([-12.0, 0.1, -12.0]), np.array([12.0, 3.0, 12.0])),
           "final": (np.array([123.0, 380.0, 147.0]), np.array([423.0, 550.0, 412.0])),
           "pbr": (np.array([-20.0, 1.0, -20.0]), np.array([20.0, 45.0, 20.0]))}


def oracle_seed(seed, k):
    return (seed + 2 * G * (((k - 0xFFFFFFFF) << 32) & M64)) & M64


def gamma(n):
    return n * U / (1.0 - n * U)


def _depth(name):
    return 8 if name == "random" else 50


def _pbr_scene(be):
    """A sphere of the principled material on a grey floor under a rectangular light (tests/test_oracle_pbr.py's scene)."""
    b = SceneBuilder(be)
    pbr = b.PBR(b.ConstantTexture((0.8, 0.3, 0.2)), 0.2, 0.1, 0.5, 0.4, 0.3, 0.2, 0.3, 0.5, 0.6, 0.8)
    light = b.DiffuseLight(b.ConstantTexture((10.0, 10.0, 10.0)))
    rect_light = b.FlipNormal(b.AARect(Plane.XZ, -20.0, 20.0, -20.0, 20.0, 60.0, light))
    world = b.HittableList()
    world.push(b.Sphere((0.0, 10.0, 0.0), 10.0, pbr))
    world.push(b.AARect(Plane.XZ, -100.0, 100.0, -100.0, 100.0, 0.0, b.Lambertian(b.ConstantTexture((0.7, 0.7, 0.7)))))
    world.push(rect_light)
    b.set_scene(world, [rect_light])
    cam = Camera((0.0, 30.0, -80.0), (0.0, 10.0, 0.0), (0.0, 1.0, 0.0), 35.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    return b, cam, (0.0, 0.0, 0.0)


def _build(name, be):
    if name == "medium_bvh":
        return medium_boundary_scene(be, "bvh")
    if name == "pbr":
        return _pbr_scene(be)
    return build_scene(name, be, scenes.load_earthmap() if name == "final" else None)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(product scene, oracle scene, camera, background) of one of SCENES, built once."""
    pb, cam, bg = _build(name, _lib.load())
    ob, _, _ = _build(name, orc.load())
    return pb, ob, cam, tuple(float(x) for x in bg)


@functools.lru_cache(maxsize=None)
def _rays(name):
    """N_RAYS rays mixed as tests/test_ray_query_gpu.py mixes them: a third camera rays (the scene's own camera at 64 x 36), a third with
    random origins in the world's box and normal directions, a third hostile — direction components exactly zero, origins exactly on a
    face of the world's box (in the rooms: on a wall's plane), sometimes both."""
    _, ob, cam, _ = _scene(name)
    rs = np.random.RandomState(2000 + SCENES.index(name))
    n_cam = N_RAYS // 3
    rays = np.zeros((N_RAYS, 7))
    for k in range(n_cam):
        rays[k] = R.camera_ray(cam, 64, 36, int(rs.randint(0, 64)), int(rs.randint(0, 36)), 77, int(rs.randint(0, 16)))
    lo, hi = _world_box(ob)
    span_lo, span_hi = ORIGINS.get(name, (lo, hi))
    face_lo, face_hi = (lo, hi) if name in ("cornell", "teapot", "medium_bvh") else (span_lo, span_hi)      # the rooms: the walls' planes
    rest = N_RAYS - n_cam
    rays[n_cam:, 0:3] = rs.uniform(span_lo, span_hi, (rest, 3))
    rays[n_cam:, 3:6] = rs.normal(size=(rest, 3))
    rays[n_cam:, 6] = rs.uniform(0.0, 1.0, rest)
    for k in range(n_cam + rest // 2, N_RAYS):
        mode = rs.randint(0, 4)
        if mode in (0, 3):
            rays[k, 3 + rs.randint(0, 3)] = 0.0
        if mode == 1:
            a = rs.randint(0, 3)
            rays[k, 3 + a] = 0.0; rays[k, 3 + (a + 1 + rs.randint(0, 2)) % 3] = 0.0
        if mode in (2, 3):
            a = rs.randint(0, 3)
            rays[k, a] = (face_lo if rs.rand() < 0.5 else face_hi)[a]
    return rays


_memo = {}


def _oracle_samples(name, n, spp, ob=None, seed=SEED, depth=None):
    """The oracle's ray_color for samples [0, spp) of the first n rays of _rays(name) -> (n, spp, 3).  (k, s) alone decides a sample's
    stream, so every test of a scene shares what was computed before."""
    obe = orc.load()
    shared = ob is None
    if shared:
        ob = _scene(name)[1]
    bg = _scene(name)[3]
    depth = _depth(name) if depth is None else depth
    rays = _rays(name)
    out = np.zeros((n, spp, 3))
    for k in range(n):
        r = rays[k]
        for s in range(spp):
            key = (name, k, s, seed, depth)
            v = _memo.get(key) if shared else None
            if v is None:
                v = orc.ray_color(ob, r[0:3], r[3:6], r[6], bg, depth, Rng(obe, oracle_seed(seed, k), s))
                if shared:
                    _memo[key] = v
            out[k, s] = v
    return out


def _check_samples(name, got, ref, max_bad):
    """Samples against the oracle's, as tests/test_scene_forms_gpu.py compares frames; returns the mask of diverged samples."""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    assert np.array_equal(np.isinf(got), np.isinf(ref))
    fin = np.isfinite(ref)
    d = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, ref, 0.0)))).any(axis=-1)
    print(f"{name}: {bad.size} samples, {int((ref != 0.0).any(axis=-1).sum())} non-zero, {int((~fin).any(axis=-1).sum())} non-finite, "
          f"{int(bad.sum())} diverged, largest |d| / (1 + |ref|) = {float((d / (1.0 + np.abs(np.where(fin, ref, 0.0)))).max()):.3g}")
    assert bad.sum() <= max_bad, f"{int(bad.sum())} of {bad.size} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"
    return bad


def _exact_sum(samples):
    """Per ray and channel the sum of its samples in extended precision (its own error is 2^-11 of the bound's)."""
    return samples.astype(np.longdouble).sum(axis=1).astype(np.float64)


def _check_sums(sums, samples, ref, bad):
    """Per ray: the sum against the sum of the oracle's samples (rays with a diverged sample left out), and against the sum of the
    device's own samples within the order bound of N atomically added terms."""
    spp = ref.shape[1]
    ref_sum = ref.sum(axis=1)
    ok = ~bad.any(axis=1)
    fin = np.isfinite(ref_sum)
    assert np.array_equal(np.isnan(sums), np.isnan(samples.sum(axis=1)))
    rows = ok[:, None] & fin
    d = np.abs(np.where(rows, sums, 0.0) - np.where(rows, ref_sum, 0.0))
    assert (d <= SAMPLE_RTOL * (spp + np.abs(np.where(rows, ref_sum, 0.0)))).all()
    own = np.isfinite(samples).all(axis=1)
    d_own = np.abs(np.where(own, sums, 0.0) - np.where(own, _exact_sum(samples), 0.0))
    assert (d_own <= 2.0 * gamma(spp) * np.where(own, np.abs(samples).sum(axis=1), 0.0)).all()


@pytest.mark.parametrize("name", SCENES)
def test_every_scene_class_against_the_oracle(name):
    pb, _, _, bg = _scene(name)
    rays = _rays(name)
    ref = _oracle_samples(name, N_RAYS, SPP)
    # the case is not vacuous (the oracle's answer alone; the rays were chosen on the CPU)
    assert (ref != 0.0).any(axis=-1).mean() >= 0.25
    sums, samples, nonfinite = R.query_radiance(pb, rays, SPP, _depth(name), bg, SEED, want_samples=True)
    bad = _check_samples(name, samples, ref, MAX_BAD)
    _check_sums(sums, samples, ref, bad)
    assert nonfinite == int((~np.isfinite(ref)).any(axis=-1).sum()) or bad.any()
    assert R.last_query_ms(pb) > 0.0
    without = R.query_radiance(pb, rays, SPP, _depth(name), bg, SEED)
    assert without[1] == nonfinite and np.array_equal(np.isnan(without[0]), np.isnan(sums))


@pytest.mark.parametrize("name", ["cornell", "teapot"])
@pytest.mark.parametrize("n,spp", [(1, 1), (1, 65), (63, 1), (65, 3), (257, 2), (5, 129), (1, 1000)])
def test_small_shapes(name, n, spp):
    """One path; one ray in two waves; a lane short of a wave; a wave and a lane with the ray changing inside the wave; a workgroup and a
    lane; rays whose samples straddle chunks; one ray's samples from many waves and workgroups."""
    pb, _, _, bg = _scene(name)
    ref = _oracle_samples(name, n, spp)
    sums, samples, _ = R.query_radiance(pb, _rays(name)[:n], spp, _depth(name), bg, SEED, want_samples=True)
    bad = _check_samples(f"{name} {n} x {spp}", samples, ref, MAX_BAD)
    _check_sums(sums, samples, ref, bad)
    if (n, spp) == (1, 1000):
        fin = np.isfinite(samples).all(axis=1)
        exact = _exact_sum(samples)
        bound = 2.0 * gamma(spp) * np.abs(samples).sum(axis=1)
        print("(1, 1000): |sum - sum of samples| =", np.abs(sums - exact).tolist(), "bound", bound.tolist())
        assert (np.abs(sums - exact)[fin] <= bound[fin]).all()


def test_the_staged_filter_tree_changes_no_word(monkeypatch):
    """272 rays x 2 samples at max_depth 4 on the random spheres (a ray's two samples are two terms: their sum has one order)."""
    from test_ray_query_gpu import STAGE_H, STAGE_W, assert_staging_changes_no_word
    pb, _, _, bg = _scene("random")
    rays = _rays("random")[:STAGE_W * STAGE_H]
    assert_staging_changes_no_word(pb, lambda: R.query_radiance(pb, rays, 2, 4, bg, SEED, want_samples=True)[:2], monkeypatch)


def test_known_answers_without_the_oracle():
    pb, _, _, bg = _scene("cornell")
    rays = _rays("cornell")[:200]
    sums, samples, nonfinite = R.query_radiance(pb, rays, 3, 0, bg, SEED, want_samples=True)       # max_depth = 0: main.rs:42-45
    assert not sums.any() and not samples.any() and nonfinite == 0
    # rays that leave the random-spheres world: the background, bit for bit
    rb, _, _, sky = _scene("random")
    rs = np.random.RandomState(5)
    up = np.zeros((300, 7))
    up[:, 0:3] = rs.uniform((-10.0, 5.0, -10.0), (10.0, 9.0, 10.0), (300, 3))
    up[:, 3:6] = rs.normal(size=(300, 3)); up[:, 4] = np.abs(up[:, 4]) + 0.1
    sums, samples, _ = R.query_radiance(rb, up, 4, 8, sky, SEED, want_samples=True)
    want = np.array(sky)
    assert np.array_equal(samples.view(np.uint64), np.broadcast_to(want, samples.shape).copy().view(np.uint64))
    one, _ = R.query_radiance(rb, up, 1, 8, sky, SEED)
    assert np.array_equal(one.view(np.uint64), np.broadcast_to(want, one.shape).copy().view(np.uint64))
    # straight up from the middle of the Cornell box: the lamp's emission, exactly
    lamp = np.array([[278.0, 278.0, 278.0, 0.0, 1.0, 0.0, 0.0]])
    sums, samples, _ = R.query_radiance(pb, lamp, 7, 50, bg, SEED, want_samples=True)
    assert (samples == 15.0).all() and (sums == 7 * 15.0).all()


def _torch_buffers(n, spp, fill=0.0):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return (torch.full((n, 3), fill, dtype=torch.float64, device=dev), torch.full((n, spp, 3), fill, dtype=torch.float64, device=dev),
            torch.zeros(1, dtype=torch.int64, device=dev))


def test_passes():
    """(first_sample, accumulate) = (0, 0) for a samples, then (a, 1) for b: the samples of one call of a + b, bit for bit; the sums within
    the order bound; a further call with accumulate = 0 overwrites."""
    import torch
    name, a, b, n = "cornell", 3, 4, 301
    pb, _, _, bg = _scene(name)
    rays = _rays(name)[:n]
    depth = _depth(name)
    whole_sum, whole, whole_nf = R.query_radiance(pb, rays, a + b, depth, bg, SEED, want_samples=True)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_sum, d_sa, d_nf = _torch_buffers(n, a, 777.0)
    _, d_sb, _ = _torch_buffers(n, b, 777.0)
    R.query_radiance_device(pb, n, d_rays, d_sum, a, depth, bg, SEED, first_sample=0, accumulate=False, d_samples=d_sa, d_nonfinite=d_nf)
    R.query_radiance_device(pb, n, d_rays, d_sum, b, depth, bg, SEED, first_sample=a, accumulate=True, d_samples=d_sb, d_nonfinite=d_nf)
    torch.cuda.synchronize()
    passes = np.concatenate([d_sa.cpu().numpy(), d_sb.cpu().numpy()], axis=1)
    assert np.array_equal(passes.view(np.uint64), whole.view(np.uint64))
    assert int(d_nf.cpu()[0]) == whole_nf
    got = d_sum.cpu().numpy()
    fin = np.isfinite(whole).all(axis=(1, 2))
    bound = 2.0 * gamma(a + b) * np.abs(whole).sum(axis=1)
    assert (np.abs(got - _exact_sum(whole))[fin] <= bound[fin]).all()
    assert (np.abs(whole_sum - _exact_sum(whole))[fin] <= bound[fin]).all()
    assert (whole != 0.0).any(axis=-1).mean() > 0.25
    R.query_radiance_device(pb, n, d_rays, d_sum, a, depth, bg, SEED, first_sample=0, accumulate=False)
    torch.cuda.synchronize()
    first = passes[:, :a]
    over = d_sum.cpu().numpy()
    assert (np.abs(over - _exact_sum(first))[fin] <= 2.0 * gamma(a) * np.abs(first).sum(axis=1)[fin]).all()
    assert not np.array_equal(over[fin], got[fin])


@pytest.mark.parametrize("name", ["cornell", "random"])
def test_device_form(name):
    """Torch tensors on a stream of the caller's: the host form's samples word for word; two identical calls give identical samples; the
    words behind the last ray's are not touched."""
    import torch
    pb, _, _, bg = _scene(name)
    n, spp = 501, 3
    rays = _rays(name)[:n]
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(rays.copy()).to(dev)
        d_sum = torch.full((n + 1, 3), canary, dtype=torch.float64, device=dev)
        d_s1 = torch.full((n + 1, spp, 3), canary, dtype=torch.float64, device=dev)
        d_s2 = torch.full((n + 1, spp, 3), canary, dtype=torch.float64, device=dev)
        d_nf = torch.zeros(1, dtype=torch.int64, device=dev)
        R.query_radiance_device(pb, n, d_rays, d_sum, spp, _depth(name), bg, SEED, d_samples=d_s1, d_nonfinite=d_nf, stream=stream.cuda_stream)
        R.query_radiance_device(pb, n, d_rays, d_sum, spp, _depth(name), bg, SEED, d_samples=d_s2, stream=stream.cuda_stream)
    stream.synchronize()
    h_sum, h_samples, h_nf = R.query_radiance(pb, rays, spp, _depth(name), bg, SEED, want_samples=True)
    s1, s2, got = d_s1.cpu().numpy(), d_s2.cpu().numpy(), d_sum.cpu().numpy()
    assert np.array_equal(s1[:n].view(np.uint64), h_samples.view(np.uint64))
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
    assert np.all(s1[n] == canary) and np.all(got[n] == canary)
    assert int(d_nf.cpu()[0]) == h_nf
    fin = np.isfinite(h_samples).all(axis=(1, 2))
    assert (np.abs(got[:n] - _exact_sum(h_samples))[fin] <= 2.0 * gamma(spp) * np.abs(h_samples).sum(axis=1)[fin]).all()
    with pytest.raises(R.RenderError, match="sum buffer too small"):
        R.query_radiance_device(pb, n + 2, d_rays, d_sum, spp, 4, bg, stream=stream.cuda_stream)


def test_frames_are_untouched_by_a_query_and_a_changed_scene_is_seen():
    pbe = _lib.load()
    pb, cam, bg = scenes.cornell_box(pbe)
    _, before = R.render(pb, cam, bg, 16, 16, 4, 12, want_samples=True)
    ms = R.last_kernel_ms(pb); info = R.last_launch_info(pb); stats = R.last_stats(pb)
    ray = np.array([[278.0, 278.0, 100.0, -1.0, 0.1, 0.3, 0.0]])                # (towards the wall at x = 0)
    first, _ = R.query_radiance(pb, ray, 64, 12, bg, 9)
    assert R.last_kernel_ms(pb) == ms and R.last_launch_info(pb) == info and R.last_stats(pb) == stats      # what the frames report is the frames'
    _, after = R.render(pb, cam, bg, 16, 16, 4, 12, want_samples=True)
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    # a lamp in the ray's way: the next query sees it
    assert first.min() > 0.0 and first.max() < 64 * 14.0
    glow = pb.DiffuseLight(pb.ConstantTexture((20.0, 30.0, 40.0)))
    pb.world.push(pb.Sphere((178.0, 288.0, 130.0), 30.0, glow))
    second, _ = R.query_radiance(pb, ray, 64, 12, bg, 9)
    assert second.tolist() == [[64 * 20.0, 64 * 30.0, 64 * 40.0]]


def test_isotropic_scatter_flag():
    """RT_ISOTROPIC_SCATTER on the scene with media as BVH leaves, against the oracle with its Isotropic scattering too."""
    name, n, spp = "medium_bvh", 400, 3
    pb, _, _, bg = _scene(name)
    ob, _, _ = _build(name, orc.load())
    orc.set_isotropic_scatters(ob, True)
    ref = _oracle_samples(name, n, spp, ob=ob)
    plain = _oracle_samples(name, n, spp)
    assert (ref != plain).any(axis=-1).mean() > 0.02            # (the flag matters for these rays)
    _, samples, _ = R.query_radiance(pb, _rays(name)[:n], spp, _depth(name), bg, SEED, flags=R.RT_ISOTROPIC_SCATTER, want_samples=True)
    _check_samples(name + " isotropic", samples, ref, MAX_BAD)


def test_errors():
    import torch
    pb, _, _, bg = _scene("cornell")
    lib = R._rt()
    rays = np.ascontiguousarray(_rays("cornell")[:8])
    cbg = (C.c_double * 3)(*bg)
    poison = 4321.5
    sums = np.full((8, 3), poison)
    nf = C.c_uint64(99)

    def host(h=pb.h, n=8, r=rays.ctypes.data, b=cbg, spp=2, depth=4, flags=0, out=sums.ctypes.data):
        return lib.rt_query_radiance(h, n, r, b, spp, depth, 1, flags, out, None, C.byref(nf))

    for kw, text in [(dict(h=None), "null"), (dict(r=None), "null"), (dict(b=None), "null"), (dict(out=None), "null"),
                     (dict(spp=0), "samples_per_ray"), (dict(n=1 << 31), "2\\^31 - 1"), (dict(flags=R.RT_F32), "RT_F32"),
                     (dict(flags=R.RT_NEAR_FIRST_BVH), "RT_F32"), (dict(flags=1 << 20), "RT_F32")]:
        assert host(**kw) != 0, kw
        assert re.search(text, R._err()), (kw, R._err())
    assert (sums == poison).all() and nf.value == 99
    assert host(n=0) == 0 and (sums == poison).all() and nf.value == 99           # n = 0: nothing is touched
    assert host() == 0 and (sums != poison).all()

    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_sum = torch.full((8, 3), poison, dtype=torch.float64, device=d_rays.device)

    def dev(h=pb.h, n=8, r=d_rays.data_ptr(), b=cbg, spp=2, flags=0, first=0, out=d_sum.data_ptr(), nbytes=8 * 24):
        return lib.rt_query_radiance_device(h, n, C.c_void_p(r), b, spp, 4, 1, flags, first, 0, C.c_void_p(out), nbytes, None, None, None)

    for kw, text in [(dict(h=None), "null"), (dict(r=None), "null"), (dict(b=None), "null"), (dict(out=None), "null"),
                     (dict(spp=0), "samples_per_ray"), (dict(n=1 << 31), "2\\^31 - 1"), (dict(first=0xFFFFFFFF), "2\\^32 - 1"),
                     (dict(first=0xFFFFFFFE, spp=2), "2\\^32 - 1"), (dict(flags=R.RT_F32), "RT_F32"), (dict(nbytes=8 * 24 - 1), "too small"),
                     (dict(r=d_rays.data_ptr() + 8), "aligned")]:
        assert dev(**kw) != 0, kw
        assert re.search(text, R._err()), (kw, R._err())
    assert dev(n=0) == 0
    torch.cuda.synchronize()
    assert (d_sum.cpu().numpy() == poison).all()
    assert dev(first=0xFFFFFFFD, spp=2) == 0                                       # the largest legal sample index
    torch.cuda.synchronize()
    assert (d_sum.cpu().numpy() != poison).all()


def test_rtrender_panorama(tmp_path):
    """`rtrender --panorama FILE` at one sample per ray (a sum of one term is exact) writes, byte for byte, rt_write_ppm of
    query_radiance(equirect_rays(lookfrom, W, W / 2))."""
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    out = tmp_path / "pano.ppm"
    subprocess.run([exe, "--scene", "cornell", "--width", "64", "--spp", "1", "--depth", "10", "--panorama", str(out)], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    pb, cam, bg = scenes.cornell_box(_lib.load())
    W, H = 64, 32
    rays = R.equirect_rays(tuple(cam.lookfrom), W, H)
    sums, _ = R.query_radiance(pb, rays, 1, 10, bg, 0x5EED)
    want = tmp_path / "want.ppm"
    R.write_ppm(str(want), sums.reshape(H, W, 3), 1)
    assert out.read_bytes() == want.read_bytes()
    tok = out.read_text().split()
    assert tok[:4] == ["P3", "64", "32", "255"]
    assert len({tuple(p) for p in np.array(tok[4:], dtype=np.int64).reshape(-1, 3).tolist()}) >= 4        # the box is in view

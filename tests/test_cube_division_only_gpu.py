"""The list-scene kernels' Cube / room fast path keeps only the division for a clear lane (rt_kernel.hip: cube_fast, SITE 2): no range test,
no bounds test after it.  The fast path runs for a WAVE only when all 64 of its rays are clear, so a known-answer test whose rays are mostly
hostile (test_fuzz_gpu.test_list_search_ray_by_ray_on_hostile_rays) sends nearly every wave to the six exact tests.  Here the waves are
made of the rays a frame is made of — camera rays and bounces off the surfaces they hit — so that the division-only form is what answers,
and every answer is compared with the oracle's HittableList::hit bit for bit."""

import numpy as np
import pytest

from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Axis, Plane, SceneBuilder
from test_fuzz_gpu import _list_hits_gpu, _list_hits_oracle, _rand_box_room_scene, _same

pytestmark = pytest.mark.gpu


def _cornell(be):
    b = SceneBuilder(be)
    red, white, green = (b.Lambertian(b.ConstantTexture(c)) for c in ((0.65, 0.05, 0.05), (0.73, 0.73, 0.73), (0.12, 0.45, 0.15)))
    metal = b.Metal((0.8, 0.85, 0.88), 0.0)
    lamp = b.FlipNormal(b.AARect(Plane.XZ, 213.0, 343.0, 227.0, 332.0, 554.0, b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))))
    w = b.HittableList()                                                        # main.rs:291-309
    w.push(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 555.0, green)); w.push(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 0.0, red)); w.push(lamp)
    w.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white)); w.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white))
    w.push(b.AARect(Plane.XY, 0.0, 555.0, 0.0, 555.0, 555.0, white))
    w.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white), -18.0), (130.0, 0.0, 65.0)))
    w.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), metal), 15.0), (265.0, 0.0, 295.0)))
    b.set_scene(w, [lamp])
    b.world_handle, b.box = w, (np.zeros(3), np.full(3, 555.0))
    return b


def _room_clear(pbe, mn, mx, rays, t_min):
    """which rays the fast path calls clear against the box [mn, mx] with every face there (rt_debug_cube_hit)"""
    n = len(rays)
    boxes = np.tile(np.concatenate([mn, mx]), (n, 1))
    out = R.debug_cube_hit(boxes, rays, np.tile([t_min, np.inf], (n, 1)), float(np.abs(boxes).max()) * 1.0000002)
    return (out[:, 3].astype(int) & 8) != 0


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_list_search_on_waves_of_plain_rays(pbe, obe, seed):
    """Seeds 0-1: the Cornell box; 2-3: random box rooms.  First generation: rays from outside the open front into the box; second and third:
    from the very points the oracle says the previous generation hit (on walls, on the lamp, on the rotated boxes' faces — position as
    hit.rs computes it, so on the surface to within an ulp or on either side of it), in random directions.  The same hit-or-miss, t, position,
    normal and front_face as the oracle, bit for bit.  A quarter of the waves of 64 at least must be clear for the room (a plain ray is clear
    with probability > 0.99, test_parity_gpu: 0.99 ** 64 = 0.53 of such waves), or the test is not testing the division-only form."""
    rnd = np.random.default_rng(900 + seed)
    if seed < 2:
        pb, ob = _cornell(pbe), _cornell(obe)
    else:
        pb = _rand_box_room_scene(pbe, 60 + seed)[0]
        ob = _rand_box_room_scene(obe, 60 + seed)[0]
    mn, mx = (np.asarray(v, dtype=np.float64) for v in pb.box)
    ext = mx - mn
    n = 64 * 160
    eye = mn + ext * np.array([0.5, 0.5, -1.45]) + rnd.normal(size=(n, 3)) * ext * 0.01
    tgt = mn + rnd.uniform(0.0, 1.0, (n, 3)) * ext
    rays = np.ascontiguousarray(np.concatenate([eye, (tgt - eye) * 10.0 ** rnd.uniform(-1, 1, (n, 1))], axis=1))
    n_hits = 0
    clear_waves = []
    for generation in range(3):
        got = _list_hits_gpu(pbe, pb, rays, 1e-5)
        ref = _list_hits_oracle(ob, rays, 1e-5)
        hit_g, hit_r = got[:, 0] != 0.0, ref[:, 0] != 0.0
        assert np.array_equal(hit_g, hit_r), f"generation {generation}: hit-or-miss differs for {int((hit_g != hit_r).sum())} rays, e.g. ray {rays[np.flatnonzero(hit_g != hit_r)[0]].tolist()}"
        h = hit_r
        ok = _same(got[h, 1], ref[h, 1]) & _same(got[h, 2:5], ref[h, 2:5]).all(axis=1) & _same(got[h, 5:8], ref[h, 5:8]).all(axis=1) & (got[h, 8] == ref[h, 8])
        assert ok.all(), f"generation {generation}: {int((~ok).sum())} of {int(h.sum())} hits differ, e.g. ray {rays[np.flatnonzero(h)[np.flatnonzero(~ok)[0]]].tolist()}"
        n_hits += int(h.sum())
        clear_waves.append(_room_clear(pbe, mn, mx, rays, 1e-5).reshape(-1, 64).all(axis=1).mean())
        # the next generation: from the hit points (a miss starts again at a random point inside), random directions of random length
        o = np.where(h[:, None], ref[:, 2:5], mn + rnd.uniform(0.05, 0.95, (n, 3)) * ext)
        d = rnd.normal(size=(n, 3)) * 10.0 ** rnd.uniform(-1, 1, (n, 1))
        rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    assert n_hits > 1.5 * n, n_hits
    print(f"seed {seed}: share of waves whose 64 rays are all clear for the room, per generation: {[round(float(c), 3) for c in clear_waves]}")
    assert min(clear_waves) > 0.25, clear_waves


@pytest.mark.parametrize("seed", [0, 4, 5])
def test_samples_of_the_room_form_are_the_plain_lists(pbe, seed, monkeypatch):
    """rt_render_samples of the f64 list-scene kernel with the room (its walls through the fast path: the division only) and with the walls as
    bare rects (RT_NO_ROOM: each wall the exact rect test of rect.rs:49-60): 0 differing 64-bit words.  Seed 0: the Cornell box."""
    def mk():
        from raytracinginrust_amd import scenes
        return scenes.cornell_box(pbe) if seed == 0 else _rand_box_room_scene(pbe, 700 + seed)[:3]
    W, H, spp, depth = 64, 64, 16, 50
    b, cam, bg = mk()
    _, with_room = R.render(b, cam, bg, W, H, spp, depth, seed=11 + seed, want_samples=True)
    has_room = any(o["is_cube"] & 2 for o in R.debug_objects(b))
    monkeypatch.setenv("RT_NO_ROOM", "1")
    b0, cam0, bg0 = mk()
    assert not any(o["is_cube"] & 2 for o in R.debug_objects(b0))
    _, plain = R.render(b0, cam0, bg0, W, H, spp, depth, seed=11 + seed, want_samples=True)
    words = int((with_room.view(np.uint64) != plain.view(np.uint64)).sum())
    assert words == 0, f"{words} differing 64-bit words (room formed: {has_room})"
    assert seed != 0 or has_room

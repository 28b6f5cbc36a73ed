"""The lean f64 kernel's primary pass (rt_kernel.hip PrimaryPass, csrc/rt_primary.h) on the device.

The pass moves a path's first level to another iteration and skips objects the pixel's rays provably miss; per sample nothing may
change.  So: rt_render_samples with the pass against the same frame with RT_NO_PRIMARY_PASS — 0 differing 64-bit words, equal counts of
non-finite samples, frames equal to summation order — at the smallest shapes where the pass can go wrong: refills that straddle pixels,
frames of fewer than 64 samples, frames whose tail chunks are most of them, the narrowest frames, max_depth 0 / 1 / 2, padding pixels and
sharded tiles, lens and pinhole, the camera inside the room, the list without the room form, bare and flipped
rects, 33 objects (no mask), a sphere light (another kernel: no pass).  The NaN-guard route under a partial mask is
reached through rt_debug_list_hit_masked (no camera frame reaches it deterministically).  And the device classifier equals its host
twin mask for mask."""
import numpy as np
import pytest

from raytracinginrust_amd import dist as D, render as R, scenes
from raytracinginrust_amd.api import Axis, Camera, Plane, SceneBuilder

pytestmark = pytest.mark.gpu

LEAN = "rt::pathtrace_kernel<double, 0u>"
CORNELL_CAM = ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0)


def on_off(monkeypatch, b, cam, bg, W, H, spp, depth, seed=41, lean=True):
    """The frame with the pass and without it: samples word for word, the frames to summation order, the non-finite counts."""
    monkeypatch.delenv("RT_NO_PRIMARY_PASS", raising=False)
    f1, s1 = R.render(b, cam, bg, W, H, spp, depth, seed=seed, want_samples=True)
    n1 = R.last_stats(b)["nonfinite_samples"]
    if lean:
        assert R.last_loop_info(b)["kernel"] == LEAN
    monkeypatch.setenv("RT_NO_PRIMARY_PASS", "1")
    f0, s0 = R.render(b, cam, bg, W, H, spp, depth, seed=seed, want_samples=True)
    n0 = R.last_stats(b)["nonfinite_samples"]
    monkeypatch.delenv("RT_NO_PRIMARY_PASS")
    assert int((s1.view(np.uint64) != s0.view(np.uint64)).sum()) == 0
    assert n1 == n0
    fin = np.isfinite(f0)
    assert np.array_equal(fin, np.isfinite(f1))
    # a pixel's sum is spp terms added in some order: |difference| <= spp * 2^-52 * sum |terms|
    bound = spp * 2.0 ** -52 * np.abs(np.where(np.isfinite(s0), s0, 0.0)).sum(axis=2) + 1e-300
    assert np.all(np.abs(np.where(fin, f1 - f0, 0.0)) <= bound)
    return s1


@pytest.fixture(scope="module")
def cornell(pbe):
    return scenes.cornell_box(pbe)


@pytest.mark.parametrize("spp", [1, 5, 64, 65, 100])
def test_8x8_refills_that_straddle_pixels(cornell, monkeypatch, spp):
    b, cam, bg = cornell
    s = on_off(monkeypatch, b, cam, bg, 8, 8, spp, 50)
    assert (s != 0.0).any()


@pytest.mark.parametrize("W,H", [(2, 24), (24, 2)])
def test_narrowest_frames(cornell, monkeypatch, W, H):
    """The library renders no frame with W or H of 1 (u, v divide by W - 1 and H - 1): the narrowest frames it does render, and the refusal."""
    b, cam, bg = cornell
    on_off(monkeypatch, b, cam, bg, W, H, 70, 50)
    with pytest.raises(R.RenderError):
        R.render(b, cam, bg, 1 if W == 2 else W, 1 if H == 2 else H, 4, 50)


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_shallow_paths_end_in_the_pass(cornell, monkeypatch, depth):
    b, cam, bg = cornell
    on_off(monkeypatch, b, cam, bg, 24, 24, 96, depth)


def test_tail_chunks_are_most_of_the_frame(cornell, monkeypatch):
    b, cam, bg = cornell
    on_off(monkeypatch, b, cam, bg, 5, 3, 1024, 50)         # 15 pixels: every one of them is split into chunks of its samples


@pytest.mark.parametrize("aperture", [0.0, 0.05])
def test_lens_and_pinhole(cornell, monkeypatch, aperture):
    b, _, bg = cornell
    cam = Camera(*CORNELL_CAM, aperture, 10.0, 0.0, 1.0)
    on_off(monkeypatch, b, cam, bg, 31, 17, 128, 50)


def test_camera_inside_the_room(cornell, monkeypatch):
    b, _, bg = cornell
    cam = Camera((278.0, 300.0, 100.0), (200.0, 100.0, 500.0), (0.0, 1.0, 0.0), 70.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    on_off(monkeypatch, b, cam, bg, 32, 32, 128, 50)


def test_axis_aligned_pinhole_odd_width(cornell, monkeypatch):
    """A pinhole on the room's axis, an odd width.  (The jitter makes d.x of the centre column zero only when a 53-bit U01 is exactly 0:
    this frame does NOT reach the NaN-guard route; the test below does.)"""
    b, _, bg = cornell
    cam = Camera(*CORNELL_CAM, 0.0, 10.0, 0.0, 1.0)
    on_off(monkeypatch, b, cam, bg, 33, 33, 64, 50)


def test_a_masked_wave_on_the_nan_guard_route_searches_the_whole_list(cornell):
    """The pass's search (world_hit_list<double, true>, through rt_debug_list_hit_masked) with the mask "room alone" on rays aimed at the
    boxes.  A wave of ordinary rays leaves the boxes out: every ray reaches the room behind them.  The same wave with ONE ray whose
    d.x is exactly zero takes the NaN-guard route: it searches the list as the reference has it — other indices, which the mask's bits
    do not name — in full, so every ray of it gets what the unmasked search gives, word for word, boxes included."""
    b, _, _ = cornell
    objs = R.debug_objects(b)
    assert len(objs) == 4 and objs[1]["is_cube"] & 2                # [light] [room] [short box] [tall box]
    g = np.random.default_rng(3)
    o = np.array([278.0, 278.0, -800.0])
    targets = np.concatenate([g.uniform([290.0, 20.0, 320.0], [400.0, 300.0, 420.0], (32, 3)),      # inside the tall box
                              g.uniform([150.0, 20.0, 100.0], [250.0, 140.0, 200.0], (32, 3))])     # inside the short box
    plain = np.concatenate([np.tile(o, (64, 1)), targets - o], axis=1)
    assert (plain[:, 3:] != 0.0).all()
    risky = plain.copy()
    risky[0, 3:] = [0.0, -0.05, 1.0]                                # d.x = 0: risky_component fires for this wave
    room_only = 0b0010
    free_plain, free_risky = R.debug_list_hit(b, plain), R.debug_list_hit(b, risky)
    assert set(free_plain[:, 9].astype(int)) == {2, 3}              # unmasked: every ray hits a box
    masked_plain = R.debug_list_hit(b, plain, mask=room_only)
    assert (masked_plain[:, 0] == 1.0).all() and (masked_plain[:, 9] == 1.0).all()       # the boxes are left out: the room behind them
    masked_risky = R.debug_list_hit(b, risky, mask=room_only)
    assert np.array_equal(masked_risky.view(np.uint64), free_risky.view(np.uint64))
    assert np.array_equal(free_risky[1:, 1:9].view(np.uint64), free_plain[1:, 1:9].view(np.uint64))      # ... the box hits (t, point, normal) of the unmasked search
    assert not np.array_equal(masked_risky[1:, 1], masked_plain[1:, 1])


def test_without_the_room_form(pbe, monkeypatch):
    monkeypatch.setenv("RT_NO_ROOM", "1")
    b, cam, bg = scenes.cornell_box(pbe)
    assert len(R.debug_objects(b)) > 4
    on_off(monkeypatch, b, cam, bg, 32, 32, 128, 50)


def _rect_list(pbe, n_extra=0):
    b = SceneBuilder(pbe)
    grey = b.Lambertian(b.ConstantTexture((0.6, 0.6, 0.6)))
    light = b.FlipNormal(b.AARect(Plane.XZ, 113.0, 443.0, 127.0, 432.0, 554.0, b.DiffuseLight(b.ConstantTexture((7.0, 7.0, 7.0)))))
    world = b.HittableList()
    world.push(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 0.0, grey))
    world.push(b.FlipNormal(b.FlipNormal(b.AARect(Plane.XY, 100.0, 300.0, 50.0, 400.0, 300.0, grey))))
    world.push(light)
    world.push(b.FlipNormal(b.AARect(Plane.YZ, 0.0, 555.0, 0.0, 555.0, 555.0, grey)))
    world.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (120.0, 200.0, 120.0), grey), 25.0), (300.0, 0.0, 200.0)))
    for q in range(n_extra):
        world.push(b.FlipNormal(b.AARect(Plane.XY, 20.0 + 15.0 * q, 30.0 + 15.0 * q, 20.0, 60.0, 400.0 + q, grey)))
    b.set_scene(world, [light])
    return b, Camera(*CORNELL_CAM, 0.05, 10.0, 0.0, 1.0), (0.02, 0.03, 0.05)


def test_bare_and_flipped_rects(pbe, monkeypatch):
    b, cam, bg = _rect_list(pbe)
    on_off(monkeypatch, b, cam, bg, 32, 32, 128, 50)


def test_33_objects_no_mask(pbe, monkeypatch):
    b, cam, bg = _rect_list(pbe, n_extra=28)
    assert len(R.debug_objects(b)) == 33
    on_off(monkeypatch, b, cam, bg, 24, 24, 128, 50)
    assert (R.debug_primary_mask(b, cam, 24, 24, np.array([[0, 0], [12, 12]], np.uint32)) == 0xFFFFFFFF).all()


def test_sphere_light_scene(pbe, monkeypatch):
    """A sphere in the list: the classifier leaves it a candidate (host twin), and the frame — another kernel's — is the same either way."""
    b = SceneBuilder(pbe)
    grey = b.Lambertian(b.ConstantTexture((0.6, 0.6, 0.6)))
    light = b.Sphere((278.0, 400.0, 278.0), 60.0, b.DiffuseLight(b.ConstantTexture((9.0, 9.0, 9.0))))
    world = b.HittableList()
    world.push(b.FlipNormal(b.AARect(Plane.XZ, 0.0, 555.0, 0.0, 555.0, 0.0, grey)))
    world.push(light)
    b.set_scene(world, [light])
    cam = Camera(*CORNELL_CAM, 0.0, 10.0, 0.0, 1.0)
    m = R.debug_primary_mask(b, cam, 16, 16, np.array([[0, 0], [8, 15]], np.uint32))
    assert ((m >> 1) & 1).all()
    on_off(monkeypatch, b, cam, (0.0, 0.0, 0.0), 16, 16, 64, 50, lean=False)


def test_padding_pixels_and_sharded_tiles(cornell, monkeypatch):
    import torch
    b, cam, bg = cornell
    W, H, spp, depth, tile, world = 19, 11, 80, 50, 7, 3            # 209 pixels in tiles of 7: the last tile has padding pixels
    frames = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("RT_NO_PRIMARY_PASS", "1")
        parts = [D.TileRenderer(b, cam, bg, W, H, spp, depth, tile_px=tile, rank=r, world=world).render_local().clone() for r in range(world)]
        torch.cuda.synchronize()
        frames.append(D.assemble(torch.stack(parts, 0), W, H, tile).cpu().numpy())
    monkeypatch.delenv("RT_NO_PRIMARY_PASS")
    full = R.render(b, cam, bg, W, H, spp, depth)
    for f in frames:
        assert np.all(np.abs(f - full) <= 1e-12 * (spp + np.abs(full)))


def test_two_passes_of_32_equal_one_of_64(cornell):
    b, cam, bg = cornell
    W, H = 12, 9
    _, whole = R.render(b, cam, bg, W, H, 64, 50, want_samples=True)
    with R.Progressive(b, cam, bg, W, H, 50) as frame:
        a = frame.add(32, want_samples=True)
        c = frame.add(32, want_samples=True)
    got = np.concatenate([a, c], axis=2)
    assert int((got.view(np.uint64) != whole.view(np.uint64)).sum()) == 0


def test_device_masks_equal_the_host_twin(cornell, pbe):
    g = np.random.default_rng(5)
    for (b, cam, _), (W, H) in ((cornell, (800, 800)), (_rect_list(pbe), (64, 48))):
        px = np.stack([g.integers(0, W, 4096), g.integers(0, H, 4096)], 1).astype(np.uint32)
        px[:4] = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]
        dev = R.debug_primary_mask(b, cam, W, H, px)
        host = R.debug_primary_mask(b, cam, W, H, px, host=True)
        assert np.array_equal(dev, host)
        assert (host != (1 << len(R.debug_objects(b))) - 1).any()      # (the classifier does clear something here)

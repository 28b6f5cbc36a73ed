"""The lean f64 kernel's shade fill (rt_kernel.hip trace_shade_fill) on the device.

The primary pass queues first-hit records, and lanes whose path ended pop one between the hit record and the material section; a path's
arithmetic and draws are what they were.  So: rt_render_samples against the same frame with RT_NO_PRIMARY_PASS (camera paths through the
queue, the generic loop) — 0 differing 64-bit words, equal non-finite counts — and against the CPU oracle per sample, on the Cornell box,
a box room and a random list scene, at the shapes where the queue's edges lie: one pass per pixel with the queue drying every few
iterations (64 x 2 x 64), a frame smaller than one wave's appetite (2 x 2 x 64: refills that generate nothing), refills that span several
pixels so that popped lanes change pixel (16 x 16 x 4), a partial last refill (8 x 8 x 100), and max_depth 1, 2 and 50 (a path popped and
ended in the same iteration; depth_left of a popped record).  And the frame sums of rt_render_device equal the per-pixel sums of the
per-sample words to summation order, with the non-finite count attributed by pixel and sample as the samples say."""
import numpy as np
import pytest

from raytracinginrust_amd import dist as D, render as R, scenes
from raytracinginrust_amd.api import Camera, Plane, SceneBuilder

from test_fuzz_gpu import SAMPLE_RTOL, _rand_box_room_scene, _rand_list_scene
from test_primary_pass_gpu import LEAN, on_off

pytestmark = pytest.mark.gpu

SHAPES = [(64, 2, 64), (2, 2, 64), (16, 16, 4), (8, 8, 100)]
DEPTHS = [1, 2, 50]


def _cornell(be):
    return scenes.cornell_box(be)


def _box_room(be):
    return _rand_box_room_scene(be, 3)[:3]


def _list_scene(be):
    return _rand_list_scene(be, 5)


SCENES = {"cornell": _cornell, "box_room": _box_room, "list": _list_scene}
_BUILT = {}
_ORACLE = {}


def _built(name, be, side):
    if (name, side) not in _BUILT:
        _BUILT[(name, side)] = SCENES[name](be)
    return _BUILT[(name, side)]


def _oracle_samples(name, obe, W, H, spp, depth, seed):
    """The oracle's per-sample words and non-finite count of one case: computed once, shared, never written to."""
    key = (name, W, H, spp, depth, seed)
    if key not in _ORACLE:
        from oracle import orc
        ob, ocam, obg = _built(name, obe, "o")
        _, rs, cnt = orc.render(ob, ocam, obg, W, H, spp, depth, seed=seed, want_samples=True, want_counters=True)
        rs.setflags(write=False)
        _ORACLE[key] = (rs, cnt["nonfinite"])
    return _ORACLE[key]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,H,spp", SHAPES)
@pytest.mark.parametrize("name", list(SCENES))
def test_samples_word_for_word(pbe, obe, monkeypatch, name, W, H, spp, depth):
    b, cam, bg = _built(name, pbe, "p")
    seed = 41
    gs = on_off(monkeypatch, b, cam, bg, W, H, spp, depth, seed=seed)      # pass on against off: 0 differing words, counts, frames
    n_gpu = R.last_stats(b)["nonfinite_samples"]
    rs, n_ref = _oracle_samples(name, obe, W, H, spp, depth, seed)
    assert np.array_equal(np.isnan(gs), np.isnan(rs)) and np.array_equal(np.isinf(gs), np.isinf(rs))
    fin = np.isfinite(rs)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs, 0.0)))).any(axis=-1)
    assert bad.sum() <= 2, f"{int(bad.sum())} of {W * H * spp} samples diverged from the oracle; first at {np.argwhere(bad)[:3].tolist()}"
    assert n_gpu == n_ref


def _device_frame(b, cam, bg, W, H, spp, depth, seed):
    import torch
    tile = 64
    part = D.TileRenderer(b, cam, bg, W, H, spp, depth, seed=seed, tile_px=tile, rank=0, world=1).render_local().clone()
    torch.cuda.synchronize()
    n = R.last_stats(b)["nonfinite_samples"]
    return D.assemble(torch.stack([part], 0), W, H, tile).cpu().numpy(), n


def _sums_equal_samples(b, cam, bg, W, H, spp, depth, seed=7):
    frame, n_dev = _device_frame(b, cam, bg, W, H, spp, depth, seed)
    assert R.last_loop_info(b)["kernel"] == LEAN
    _, s = R.render(b, cam, bg, W, H, spp, depth, seed=seed, want_samples=True)
    n_smp = R.last_stats(b)["nonfinite_samples"]
    assert n_dev == n_smp == int((~np.isfinite(s)).any(axis=-1).sum())
    want = s.sum(axis=2)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(frame))          # a poisoned sample poisons its own pixel's sum, and no other
    assert np.array_equal(np.isnan(want), np.isnan(frame))
    err = np.abs(np.where(fin, frame - want, 0.0))
    print(f"max |frame - sum of samples| = {err.max():.3e}; non-finite samples {n_dev}")
    assert np.all(err <= 1e-12 * (spp + np.abs(np.where(fin, want, 0.0))))
    return n_dev


def test_frame_sums_equal_the_sums_of_the_samples(pbe):
    b, cam, bg = _built("cornell", pbe, "p")
    assert _sums_equal_samples(b, cam, bg, 64, 64, 128, 50) == 0


def test_nonfinite_samples_are_counted_in_their_own_pixel(pbe):
    """tests/test_parity_gpu.py's NaN scene (a `lights` entry with the trait-default pdf: the mixture pdf is 0 for grazing directions and
    the weight NaN) runs on the lean kernel: the poisoned samples must poison their own pixels' sums, the others none."""
    b = SceneBuilder(pbe)
    white = b.Lambertian(b.ConstantTexture((0.73, 0.73, 0.73)))
    floor = b.AARect(Plane.XZ, -100.0, 100.0, -100.0, 100.0, 0.0, white)
    cube = b.Cube((-10.0, 0.0, -10.0), (10.0, 20.0, 10.0), white)
    world = b.HittableList()
    world.push(floor)
    world.push(cube)
    b.set_scene(world, [cube])
    cam = Camera((0.0, 50.0, -120.0), (0.0, 5.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    assert _sums_equal_samples(b, cam, (0.5, 0.7, 1.0), 32, 32, 8, 10) > 100

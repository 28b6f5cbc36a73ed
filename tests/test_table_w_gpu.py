"""The compact lean f64 kernel's material section with the whole ONB from the table (rt_kernel.hip merged_arms_table_w, ring_w; rt_ir.h
DOnbW): w = normalized(n) is the rect's stored magnitudes with the sign bits of the rect word (Lemma W), v and u the slot those bits name,
and each lane runs one normalisation — Lambertian normalized(dir), Metal normalized(reflect(..)) — in one shared instruction run.  Per lane
the draws and the f64 operations are the parent's, so every sample must be the parent's 64-bit words.  The wide-ring kernel, which serves the
same scenes under RT_NO_ONB_TABLE, still runs the arithmetic path (normalise n, probe, fallback): it is the comparison.

1. Lemma W on the device (rt_debug_ring_w: world.hit + finalize_hit, then normalized(normal) by the kernel's normalisation beside ring_w's
   w) on 64 x 200 rays into each of four scenes — plain rays, their bounces, and tests/test_fuzz_gpu.py's hostile rays (zero, denormal, NaN
   and infinite components, origins on the planes), the families of tests/test_compact_ring_gpu.py.  0 differing words.
2. Samples (rt_render_samples) at 2 x 2 x 333, 8 x 8 x 100, 64 x 2 x 64 and 16 x 16 x 4 with max_depth 1, 2 and 50 against the same scene
   under RT_NO_ONB_TABLE and under RT_NO_PRIMARY_PASS: 0 differing words; against the CPU oracle: 0 differing words at max_depth 1, 0 diverged
   samples deeper (tests/test_hit_ring_gpu.py's rule).  Scenes: the Cornell box (Metal fuzz 0, the -18 degree box); a room whose Metal has
   fuzz 0.3 (the rejection loop runs across the moved normalisation); a room whose every surface is Metal (no Lambertian lane in any
   wave; at max_depth 1 the absorbed ray's `done` path through the per-lane flush); an all-Lambertian room without a light (n_lights == 0:
   the cosine arm only); a rect under the idiom at 7 degrees (w != n in bits: tests/test_table_w_host.py).
3. After each render: the compact kernel ran, with its LDS bytes and 5 workgroups per CU; a rect under RotateX still runs the wide kernel.
4. The NaN scene of tests/test_parity_gpu.py: the count of non-finite samples is the wide kernel's and the queue loop's, each sample in
   its own pixel's sum.
5. The frame sums of the Cornell box at 64 x 64 x 128 against the sums of its samples."""
import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes
from raytracinginrust_amd.api import Axis, Camera, Plane, SceneBuilder

from test_compact_ring_gpu import _assert_ring
from test_compact_ring_host import BOX_ROOM_SEEDS, COMPACT, QN_W, _one_rect_scene, rotate_x
from test_fuzz_gpu import SAMPLE_RTOL, _hostile_rays, _rand_box_room_scene
from test_onb_table_host import bounce_rays, plain_rays
from test_primary_pass_gpu import on_off
from test_shade_fill_gpu import _sums_equal_samples
from test_table_w_host import angle_idiom

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 333), (8, 8, 100), (64, 2, 64), (16, 16, 4)]
DEPTHS = [1, 2, 50]
SEED = 41
ROOM_CAM = Camera((50.0, 50.0, -140.0), (50.0, 50.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)


def _room(be, kind):
    """a 100^3 room open at the front — floor, ceiling, back and side walls —, a box under the idiom at -18 degrees and a bare Cube.
    fuzzy: Lambertian walls, a lamp, the boxes and one wall Metal with fuzz 0.3; metal: every surface Metal (fuzz 0, 0.3 and 1), a lamp;
    dark: every surface Lambertian, no lamp and no `lights` (n_lights == 0), lit by the background through the open front"""
    b = SceneBuilder(be)
    cols = ((0.65, 0.05, 0.05), (0.73, 0.73, 0.73), (0.12, 0.45, 0.15), (0.3, 0.4, 0.8), (0.8, 0.85, 0.88), (0.9, 0.6, 0.2), (0.5, 0.5, 0.5))
    fuzz = (0.0, 0.3, 1.0, 0.3, 0.0, 0.3, 0.0)
    if kind == "metal":
        mats = [b.Metal(c, f) for c, f in zip(cols, fuzz)]
    else:
        mats = [b.Lambertian(b.ConstantTexture(c)) for c in cols]
        if kind == "fuzzy":
            mats[4], mats[5], mats[6] = b.Metal(cols[4], 0.3), b.Metal(cols[5], 0.3), b.Metal(cols[6], 0.3)
    w = b.HittableList()
    w.push(b.AARect(Plane.YZ, 0.0, 100.0, 0.0, 100.0, 100.0, mats[2]))
    w.push(b.AARect(Plane.YZ, 0.0, 100.0, 0.0, 100.0, 0.0, mats[0]))
    lamp = b.FlipNormal(b.AARect(Plane.XZ, 35.0, 65.0, 35.0, 65.0, 99.5, b.DiffuseLight(b.ConstantTexture((15.0, 15.0, 15.0)))))
    if kind != "dark":
        w.push(lamp)
    w.push(b.AARect(Plane.XZ, 0.0, 100.0, 0.0, 100.0, 0.0, mats[1]))
    w.push(b.AARect(Plane.XZ, 0.0, 100.0, 0.0, 100.0, 100.0, mats[3]))
    w.push(b.AARect(Plane.XY, 0.0, 100.0, 0.0, 100.0, 100.0, mats[4]))
    w.push(b.Translate(b.Rotate(Axis.Y, b.Cube((0.0, 0.0, 0.0), (30.0, 30.0, 30.0), mats[5]), -18.0), (20.0, 0.0, 15.0)))
    w.push(b.Cube((55.0, 0.0, 50.0), (85.0, 60.0, 80.0), mats[6]))
    b.set_scene(w, [] if kind == "dark" else [lamp])
    b.box = (np.zeros(3), np.full(3, 100.0))
    return b, ROOM_CAM, (0.2, 0.3, 0.5) if kind == "dark" else (0.0, 0.0, 0.0)


def _idiom7(be):
    """a floor, a lamp above it and one rect under Translate(RotateY(.., 7 degrees)), seen from the side"""
    def more(b, w, m):
        w.push(b.FlipNormal(b.AARect(Plane.XZ, -10.0, 10.0, -10.0, 10.0, 30.0, b.DiffuseLight(b.ConstantTexture((8.0, 8.0, 8.0))))))
    b = _one_rect_scene(be, angle_idiom(7.0), more)
    b.box = (np.array([-50.0, 0.0, -50.0]), np.array([50.0, 30.0, 50.0]))
    return b, Camera((20.0, 15.0, -40.0), (3.0, 5.0, 5.0), (0.0, 1.0, 0.0), 50.0, 1.0, 0.0, 10.0, 0.0, 1.0), (0.2, 0.3, 0.5)


def _cornell(be):
    b, cam, bg = scenes.cornell_box(be)
    b.box = (np.zeros(3), np.full(3, 555.0))
    return b, cam, bg


SCENES = {"cornell": _cornell, "fuzzy_room": lambda be: _room(be, "fuzzy"), "metal_room": lambda be: _room(be, "metal"),
          "dark_room": lambda be: _room(be, "dark"), "idiom7": _idiom7}
RAY_SCENES = {"cornell": _cornell, "fuzzy_room": lambda be: _room(be, "fuzzy"), "idiom7": _idiom7,
              "box_room_62": lambda be: _rand_box_room_scene(be, BOX_ROOM_SEEDS[1])[:3]}
_BUILT, _ORACLE = {}, {}


def _built(name, be, side, monkeypatch=None):
    """the scene for the product library ("p"), for the oracle ("o"), or for the product library flattened without the table ("w": wide ring)"""
    if (name, side) not in _BUILT:
        make = SCENES.get(name) or RAY_SCENES[name]
        if side == "w":
            monkeypatch.setenv("RT_NO_ONB_TABLE", "1")                 # (read when the scene is flattened: the query below flattens it)
            s = make(be)
            assert R.debug_ring_form(s[0]) == {"compact": False, "entries": QN_W, "entry_bytes": 104}
            monkeypatch.delenv("RT_NO_ONB_TABLE")
        else:
            s = make(be)
            if side == "p":
                assert R.debug_ring_form(s[0]) == COMPACT, name
        _BUILT[(name, side)] = s
    return _BUILT[(name, side)]


def _oracle_samples(name, obe, W, H, spp, depth):
    key = (name, W, H, spp, depth)
    if key not in _ORACLE:
        from oracle import orc
        ob, ocam, obg = _built(name, obe, "o")
        _, rs, cnt = orc.render(ob, ocam, obg, W, H, spp, depth, seed=SEED, want_samples=True, want_counters=True)
        rs.setflags(write=False)
        _ORACLE[key] = (rs, cnt["nonfinite"])
    return _ORACLE[key]


# ---- 1. Lemma W
@pytest.mark.parametrize("name", list(RAY_SCENES))
def test_lemma_w_the_tables_w_is_the_normalised_normal(pbe, name):
    b = _built(name, pbe, "p")[0]
    mn, mx = b.box
    rnd = np.random.default_rng(1977)
    n = 64 * 50
    wmag = R.debug_onb_table_w(b)
    mag = R.debug_onb_table(b)[0]
    rays = plain_rays(rnd, mn, mx, n)
    batches = []
    for generation in range(2):                                                   # plain rays, then their bounces off the hit points
        batches.append(rays)
        out = np.zeros((n, 12)); tm = np.full(n, 1e-5)
        assert pbe.lib.rt_debug_list_hit(b.h, n, rays.ctypes.data, tm.ctypes.data, out.ctypes.data) == 0, pbe.lib.rt_last_error()
        rays = bounce_rays(rnd, mn, mx, out[:, 0] != 0.0, out[:, 2:5])
    batches.append(_hostile_rays(rnd, n, mn, mx, planes_y=(0.5 * (mn[1] + mx[1]),)))
    batches.append(_hostile_rays(rnd, n, mn, mx))
    assert sum(len(r) for r in batches) == 64 * 200
    total_hits, seen_signs, n_w_not_n = 0, set(), 0
    for rays in batches:
        hit, rect, wn, wt = R.debug_ring_w(b, rays, np.full(len(rays), 1e-5))
        a, t = np.ascontiguousarray(wn[hit]).view(np.uint64), np.ascontiguousarray(wt[hit]).view(np.uint64)
        differ = int((a != t).sum())
        wrong = (a != t).any(axis=1)
        assert differ == 0, f"{differ} words of {a.size} differ; first: rect {rect[hit][wrong][0]}, " \
                            f"normalized(n) {wn[hit][wrong][0].tolist()}, table {wt[hit][wrong][0].tolist()}"
        assert (rect[hit] >= 0).all() and (rect[hit] < len(wmag)).all()
        assert ((t & np.uint64(0x7FFFFFFFFFFFFFFF)) == wmag[rect[hit]]).all()
        total_hits += int(hit.sum())
        seen_signs |= set(((t >> np.uint64(63)) * np.array([1, 2, 4], np.uint64)).sum(axis=1).tolist())
        n_w_not_n += int((wmag[rect[hit]] != mag[rect[hit]]).any(axis=1).sum())
    print(f"{name}: {total_hits} hits of {64 * 200} rays, sign patterns seen {sorted(int(s) for s in seen_signs)}, hits with w != n in bits {n_w_not_n}")
    assert total_hits > 64 * 200 // 10 and len(seen_signs) >= 2
    if name != "box_room_62":
        assert n_w_not_n > 0, "no hit on a face whose w differs from its n: the scene would not tell the table's w from the normal"


# ---- 2., 3. samples
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,H,spp", SHAPES)
@pytest.mark.parametrize("name", list(SCENES))
def test_samples_word_for_word(pbe, obe, monkeypatch, name, W, H, spp, depth):
    b, cam, bg = _built(name, pbe, "p")
    gs = on_off(monkeypatch, b, cam, bg, W, H, spp, depth, seed=SEED)      # the table's w against the queue loop's arithmetic: 0 differing words, counts, frames
    _assert_ring(b, "wide")                                                # (its last render, RT_NO_PRIMARY_PASS, ran the wide kernel's queue loop)
    _, again = R.render(b, cam, bg, W, H, spp, depth, seed=SEED, want_samples=True)
    _assert_ring(b, "compact")
    n_gpu = R.last_stats(b)["nonfinite_samples"]
    assert int((again.view(np.uint64) != gs.view(np.uint64)).sum()) == 0
    bw, camw, bgw = _built(name, pbe, "w", monkeypatch)
    _, ws = R.render(bw, camw, bgw, W, H, spp, depth, seed=SEED, want_samples=True)
    _assert_ring(bw, "wide")
    n_diff = int((ws.view(np.uint64) != gs.view(np.uint64)).sum())
    assert n_diff == 0, f"{n_diff} of {gs.size} words differ between the table's w and the arithmetic path"
    assert R.last_stats(bw)["nonfinite_samples"] == n_gpu
    assert (gs != 0.0).any()
    rs, n_ref = _oracle_samples(name, obe, W, H, spp, depth)
    assert np.array_equal(np.isnan(gs), np.isnan(rs)) and np.array_equal(np.isinf(gs), np.isinf(rs))
    fin = np.isfinite(rs)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs, 0.0)))).any(axis=-1)
    n_words = int((gs.view(np.uint64) != rs.view(np.uint64)).sum())
    print(f"{name} {W}x{H}x{spp} depth {depth}: {n_words} of {gs.size} words differ from the oracle's, max |gpu - oracle| {d.max():.3e}, diverged {int(bad.sum())}")
    assert int(bad.sum()) == 0, f"{int(bad.sum())} of {W * H * spp} samples diverged from the oracle; first at {np.argwhere(bad)[:3].tolist()}"
    if depth == 1:
        assert n_words == 0, f"{n_words} of {gs.size} words differ from the oracle's at max_depth 1"
    assert n_gpu == n_ref


def test_a_rect_under_rotate_x_still_runs_the_wide_kernel(pbe, monkeypatch):
    b = _one_rect_scene(pbe, rotate_x)
    cam = Camera((20.0, 15.0, -40.0), (3.0, 5.0, 5.0), (0.0, 1.0, 0.0), 50.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s = on_off(monkeypatch, b, cam, (0.2, 0.3, 0.5), 8, 8, 100, 50)
    R.render(b, cam, (0.2, 0.3, 0.5), 8, 8, 100, 50)
    _assert_ring(b, "wide")
    assert (s != 0.0).any()


# ---- 4.
def test_nan_scene_counts_are_the_arithmetic_paths(pbe, monkeypatch):
    """tests/test_parity_gpu.py's NaN scene (a `lights` entry with the trait-default pdf poisons grazing samples; bare rects and a bare Cube:
    the compact ring).  The count of non-finite samples with the table's w equals the queue loop's (on_off) and the wide kernel's, the
    samples are the same words, and each poisoned sample poisons its own pixel's sum and no other (_sums_equal_samples)."""
    def make():
        b = SceneBuilder(pbe)
        white = b.Lambertian(b.ConstantTexture((0.73, 0.73, 0.73)))
        floor = b.AARect(Plane.XZ, -100.0, 100.0, -100.0, 100.0, 0.0, white)
        cube = b.Cube((-10.0, 0.0, -10.0), (10.0, 20.0, 10.0), white)
        world = b.HittableList()
        world.push(floor)
        world.push(cube)
        b.set_scene(world, [cube])
        return b
    b = make()
    assert R.debug_ring_form(b)["compact"]
    cam, bg = Camera((0.0, 50.0, -120.0), (0.0, 5.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0), (0.5, 0.7, 1.0)
    s = on_off(monkeypatch, b, cam, bg, 32, 32, 8, 10, seed=7)
    n = int((~np.isfinite(s)).any(axis=-1).sum())
    assert n > 100
    assert _sums_equal_samples(b, cam, bg, 32, 32, 8, 10, seed=7) == n
    _assert_ring(b, "compact")
    monkeypatch.setenv("RT_NO_ONB_TABLE", "1")
    bw = make()
    assert not R.debug_ring_form(bw)["compact"]
    monkeypatch.delenv("RT_NO_ONB_TABLE")
    _, sw = R.render(bw, cam, bg, 32, 32, 8, 10, seed=7, want_samples=True)
    _assert_ring(bw, "wide")
    assert R.last_stats(bw)["nonfinite_samples"] == n and int((sw.view(np.uint64) != s.view(np.uint64)).sum()) == 0


# ---- 5.
PARENT_MAX_FRAME_ERROR = 2.0 ** -41           # 4.547e-13: the parent build on these inputs, three runs, each time this value
FRAME_ERROR_BOUND = 4.0 * PARENT_MAX_FRAME_ERROR


def test_frame_sums_equal_the_sums_of_the_samples(pbe):
    """The Cornell box at 64 x 64 x 128, depth 50, seed 11: rt_render_device's per-pixel sums against the sums of rt_render_samples' words.
    The samples are the parent's words, so a pixel's sum can differ from the parent's by the order of its 128 additions alone (a lane adds
    its samples in its own order and hands partial sums in by atomics, whose order varies from run to run).
    Measured on these inputs, max |frame - sum of samples| over the frame: the parent build 4.547e-13 = 2^-41 in three runs of three; this
    build 4.547e-13 in three runs of three (printed).  That is one unit in the last place of a sum in [2048, 4096), two of one in [1024, 2048).
    Bound: 4 x the parent's measured value, 1.819e-12, absolute, on every pixel — room for the run-to-run order of the atomics to move the
    largest sums by a few units in the last place, and 70 to 1100 times below the 1e-12 (spp + |sum|) the older ring tests allow here."""
    from test_shade_fill_gpu import LEAN, _device_frame
    b, cam, bg = _built("cornell", pbe, "p")
    frame, n_dev = _device_frame(b, cam, bg, 64, 64, 128, 50, 11)
    assert R.last_loop_info(b)["kernel"] == LEAN
    _assert_ring(b, "compact")
    _, s = R.render(b, cam, bg, 64, 64, 128, 50, seed=11, want_samples=True)
    _assert_ring(b, "compact")
    assert n_dev == 0 and R.last_stats(b)["nonfinite_samples"] == 0 and np.isfinite(s).all() and np.isfinite(frame).all()
    want = s.sum(axis=2)
    err = float(np.abs(frame - want).max())
    print(f"max |frame - sum of samples| = {err:.3e} (parent {PARENT_MAX_FRAME_ERROR:.3e}, bound {FRAME_ERROR_BOUND:.3e}); largest sum {float(np.abs(want).max()):.1f}")
    assert err <= FRAME_ERROR_BOUND, f"max |frame - sum of samples| = {err:.3e} > {FRAME_ERROR_BOUND:.3e}"

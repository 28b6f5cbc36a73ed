"""The host side of tests/test_later_trips_gpu.py, without a GPU: the shapes of tests/later_trips_cases.py do take the device loops into
a later trip by the limits the library reports, and they are the smallest of their kind that do; at those shapes the host twins — the
references of the GPU tests — are held once to the NumPy restatements of tests/adaptive_cases.py, tests/denoise_frame_cases.py and their
neighbours, so that the big-shape reference is anchored on the specification and not only against itself; the oracle's batch entry point is
its one-path entry point; and the launch getter says that nothing was launched."""
import ctypes as C

import numpy as np
import pytest

from oracle import orc
from raytracinginrust_amd import render as R
from raytracinginrust_amd import scenes

import adaptive_cases as AC
import denoise_cases as DC
import denoise_frame_cases as FC
import denoise_variance_cases as VC
import later_trips_cases as LT
import moments_cases as MC
from moments_cases import differing_words


# ---------------------------------------------------------------- the hooks
def test_loop_limits_are_reported_by_name():
    lim = R.debug_loop_limits()
    assert tuple(lim) == R.LOOP_LIMITS and all(v > 0 for v in lim.values())
    lib = R._rt()
    assert lib.rt_debug_loop_limits(None, 0) == len(R.LOOP_LIMITS)
    assert lib.rt_debug_loop_limits(None, 3) < 0 and "null argument" in R._err()
    few = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.rt_debug_loop_limits(few, 3) == len(R.LOOP_LIMITS)                  # a short buffer gets its share and nothing behind it
    assert list(few) == [lim["denoise_frame_max_blocks"], lim["denoise_frame_threads"], lim["variance_max_blocks"], 7]
    # what the kernels' own code needs of them: whole waves, four pixels per lane of the compaction, one workgroup for the scan
    for name in ("denoise_frame_threads", "variance_threads", "adaptive_threads", "resolve_threads", "query_threads", "radiance_threads", "pixels_threads"):
        assert lim[name] % 64 == 0
    assert lim["compaction_block_px"] == 4 * lim["adaptive_threads"] and lim["scan_threads"] <= 1024


def test_the_launch_getter_without_a_launch(pbe):
    b, _, _ = scenes.cornell_box(pbe)
    lib = R._rt()
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.rt_last_query_launch(None, out) != 0 and "null argument" in R._err()
    assert lib.rt_last_query_launch(b.h, None) != 0 and "null argument" in R._err()
    assert lib.rt_last_query_launch(b.h, out) != 0 and "no ray query" in R._err() and list(out) == [7, 7, 7, 7]
    with pytest.raises(R.RenderError, match="no ray query"):
        R.last_query_launch(b)
    if R.device_count() == 0:                              # a query that cannot be launched leaves it so
        with pytest.raises(R.RenderError, match="no HIP device"):
            R.query_hits(b, np.zeros((4, 7)))
        with pytest.raises(R.RenderError, match="no ray query"):
            R.last_query_launch(b)


def test_the_shapes_cross_their_loops_and_are_the_smallest_that_do():
    lim = R.debug_loop_limits()
    # C: 1035 workgroup counts are two trips of the scan, 2050 three; neither frame is more than ten rows above its trip count
    two, three = LT.COMPACTION_SHAPES
    assert LT.scan_trips(two, lim) == 2 and LT.scan_trips(three, lim) == 3
    per_trip = lim["compaction_block_px"] * lim["scan_threads"]
    assert two[0] * two[1] - per_trip < 2 * two[1] * 5 and three[0] * three[1] - 2 * per_trip < 2 * three[1]
    assert (two[0] * two[1]) % 4 == 1 and (three[0] * three[1]) % 4 == 2           # neither is a whole number of four-pixel groups
    assert LT.adaptive_resolve_trips(two, lim) == 2 and LT.adaptive_resolve_trips(three, lim) == 3
    assert LT.scan_trips((600, 1024), lim) == 1                                    # the largest shape of tests/test_adaptive_gpu.py
    # D: above both caps by less than six rows, with an odd count of doubles; tests/denoise_cases.py's largest frame is one trip
    H, W = LT.DENOISE_SHAPE
    for which in ("denoise_frame", "variance"):
        assert LT.pair_trips(LT.DENOISE_SHAPE, lim, which) == 2 and LT.pair_trips((H - 6, W), lim, which) == 1 and LT.pair_trips((67, 130), lim, which) == 1
    assert (H * W * 3) % 2 == 1
    # E: one pixel more than a multiple of four, above the cap by less than two rows
    H, W = LT.RESOLVE_SHAPE
    assert LT.resolve_trips(LT.RESOLVE_SHAPE, lim) == 2 and LT.resolve_trips((H - 2, W), lim) == 1 and LT.resolve_trips((2160, 3840), lim) == 1
    assert (H * W) % lim["resolve_px_per_lane"] == 1
    # A: the rule the chunk cases raise their path counts by
    full = {"workgroups": 1280, "threads": 256, "waves": 5120, "chunk": 100, "chunks": 300}
    assert LT.paths_for_two_chunks(full, 30000) == 2 * 5120 * 100
    assert LT.paths_for_two_chunks(dict(full, chunks=10240), 1024000) == 1024000 and LT.paths_for_two_chunks(dict(full, chunks=10239), 1023900) == 1024000


def test_need_maps_are_what_they_are_called():
    for shape in LT.COMPACTION_SHAPES:
        n_px = shape[0] * shape[1]
        maps = LT.need_maps(shape)
        assert len(maps["empty"]) == 0 and np.array_equal(maps["full"], np.arange(n_px))
        assert len(maps["last_block"]) == 1 and maps["last_block"][0] // 1024 == (n_px - 1) // 1024
        assert len(maps["block_1024"]) == 1 and maps["block_1024"][0] // 1024 == 1024
        assert abs(len(maps["random_1pc"]) / n_px - 0.01) < 0.001 and abs(len(maps["random_50pc"]) / n_px - 0.5) < 0.005
        assert len(maps["random_50pc"]) > 2048 * 256                               # more than one sweep of the merge kernel's grid
        for pixels in maps.values():
            assert pixels.dtype == np.uint32 and (np.diff(pixels.astype(np.int64)) > 0).all()


# ---------------------------------------------------------------- the oracle's batch entry point
def test_ray_color_paths_is_ray_color_path(obe):
    ob, cam, bg = scenes.cornell_box(obe)
    rays = np.array([R.camera_ray(cam, 16, 16, i, j, 5, 0) for i, j in ((3, 4), (8, 8), (12, 2), (0, 15), (15, 0))])
    spp, depth, seed, first = 7, 12, 2025, 3
    got = orc.ray_color_paths(ob, rays, spp, bg, depth, seed, first_sample=first, nthreads=3)
    assert got.shape == (5, spp, 3) and (got != 0.0).any()
    for k in range(5):
        for s in range(spp):
            want = orc.ray_color_path(ob, rays[k, 0:3], rays[k, 3:6], rays[k, 6], bg, depth, seed, k, first + s)
            assert differing_words(got[k, s], np.array(want)) == 0, (k, s)
    assert differing_words(orc.ray_color_paths(ob, rays, spp, bg, depth, seed, first_sample=first, nthreads=1), got) == 0


# ---------------------------------------------------------------- the host twins at the big shapes are the specification
@pytest.mark.parametrize("shape", LT.COMPACTION_SHAPES, **LT.IDS)
def test_adaptive_twins_equal_the_numpy_restatement_at_the_big_shapes(shape):
    S, Q, n, b = LT.big_state(shape)
    want = AC.numpy_error(S, Q, n, b)
    e2, stats = R.adaptive_error_host(S, Q, n, b, tau=0.05)
    assert differing_words(e2, want) == 0
    f = MC.finite(want.reshape(-1))
    with np.errstate(all="ignore"):
        assert [stats["converged"], stats["unconverged"], stats["nonfinite"]] == [int((f & (want.reshape(-1) <= 0.05 * 0.05)).sum()),
                                                                                   int((f & (want.reshape(-1) > 0.05 * 0.05)).sum()), int((~f).sum())]
    sizes = set()
    for tau, spread, cap in ((1.0 / 256.0, 1, AC.MAX_SAMPLES), (0.05, 0, AC.CAP), (0.05, 1, 40)):
        got = R.adaptive_select_host(S, Q, n, b, AC.N_B, tau, cap, spread)
        assert np.array_equal(got, AC.numpy_select(S, Q, n, b, AC.N_B, tau, cap, spread)), (tau, spread, cap)
        sizes.add(len(got))
    assert len(sizes) == 3 and min(sizes) > 0
    for name, pixels in LT.need_maps(shape).items():
        fS, fQ, fn, fb = LT.flag_state(shape, pixels)
        assert np.array_equal(R.adaptive_select_host(fS, fQ, fn, fb, AC.N_B, 0.01, AC.MAX_SAMPLES, 0), pixels), name
    want_img, changed = AC.numpy_resolve(S, n)
    got_img, got_changed = R.adaptive_resolve_rgb8_host(S, n)
    assert np.array_equal(got_img, want_img) and got_changed == changed == shape[0] * shape[1]
    prev = want_img.copy(); prev.reshape(-1, 3)[::3, 1] ^= 1
    assert R.adaptive_resolve_rgb8_host(S, n, prev)[1] == AC.numpy_resolve(S, n, prev)[1] == len(prev.reshape(-1, 3)[::3])
    p = np.random.RandomState(5).uniform(0.0, 8.0, shape + (3,))
    pixels = LT.need_maps(shape)["random_50pc"]
    want = AC.numpy_merge(p, AC.N_B, S, Q, n, b, pixels)
    got = [a.copy() for a in (p, S, Q, n, b)]
    R.adaptive_merge_host(got[0], AC.N_B, got[1], got[2], got[3], got[4], pixels)
    for g, w in zip(got[:3], want[:3]):
        assert differing_words(g, w) == 0
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])


def test_variance_twins_equal_the_numpy_restatement_at_the_big_shape():
    shape = LT.DENOISE_SHAPE
    S, Q, N, B = MC.state(shape)
    assert differing_words(R.moments_variance_host(S, Q, N, B), VC.numpy_variance(S, Q, N, B)) == 0
    S, Q, n, b = FC.variance_state(shape)
    assert differing_words(R.adaptive_variance_host(S, Q, n, b), FC.numpy_adaptive_variance(S, Q, n, b)) == 0


@pytest.mark.parametrize("combo", [(False, False, False), (True, True, True)], ids=FC.combo_id)
def test_denoise_frame_twin_equals_the_numpy_restatement_at_the_big_shape(combo):
    shape = LT.DENOISE_SHAPE
    rgb, n, var, alb, hits = FC.frames(shape, combo)
    k, sigma, flags = 2, (VC.SIGMAS if combo[1] else DC.SIGMAS)[0], 1
    got = R.denoise_frame_host(rgb, hits, n, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, k, sigma, flags, want_var=combo[1])
    want, want_v = FC.numpy_denoise_frame(rgb, n, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, hits, k, sigma, flags)
    if combo[1]:
        assert differing_words(got[0], want) == 0 and differing_words(got[1], want_v) == 0
    else:
        assert differing_words(got, want) == 0


def test_filter_twins_equal_the_numpy_restatement_at_the_big_shape_with_three_iterations():
    shape = LT.DENOISE_SHAPE
    rgb, var, hits = VC.case(shape)
    assert differing_words(R.denoise_host(rgb, DC.SAMPLES, hits, 3, DC.SIGMAS[0], 1), DC.numpy_denoise(rgb, DC.SAMPLES, hits, 3, DC.SIGMAS[0], 1)) == 0
    got = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, 3, VC.SIGMAS[0], 1, want_var=True)
    want = VC.numpy_denoise_variance(rgb, VC.SAMPLES, var, hits, 3, VC.SIGMAS[0], 1)
    assert differing_words(got[0], want[0]) == 0 and differing_words(got[1], want[1]) == 0

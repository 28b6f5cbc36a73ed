"""Every frame and query kernel past the first trip of its loops (tests/later_trips_cases.py has the table: loop, what one trip covers, the
size that crosses it).  The other GPU test files hold these kernels to exact references at sizes where every device loop runs once; here
each loop is taken into its second or third trip at the smallest size that does so, against the same references with the same bounds —

  A. radiance_kernel, pixels_kernel: a wave's second chunk (`next_chunk += n_waves`, a refill that empties one chunk and goes on into the
     next, `(cur_k, cur_s)` of a chunk that starts in the middle of a ray) — the oracle sample by sample (SAMPLE_RTOL, MAX_BAD of
     tests/test_radiance_query_gpu.py), the frames' own sums (PARITY, MAX_BAD and the any-order bound of tests/test_adaptive_gpu.py), the
     same words with every chunk size, and rays and views whose radiance is known without any reference at the default chunk;
  B. query_kernel and the albedo kernels: the second batch of a lane — the oracle's records and the texture table, word for word;
  C. adaptive_scan_kernel's carry and the strides of the compaction's neighbours — the host twin;
  D. the grid-stride trips of rt_denoise_frame.hip and rt_denoise_var.hip and the filters on a frame of 38 x 37 tiles — the host twins, 0 words;
  E. resolve_rgb8_kernel's stride — rt_format_color

— and every test asserts, from what the library reports about its launches (render.last_query_launch, render.debug_loop_limits), that the
later trip was in fact taken: on a device with another CU count, or after a change of a cap, a test fails instead of testing nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import orc
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Camera

import adaptive_cases as AC
import denoise_cases as DC
import denoise_frame_cases as FC
import denoise_variance_cases as VC
import later_trips_cases as LT
import moments_cases as MC
from moments_cases import differing_words, gamma

import test_adaptive_gpu as AG
import test_albedo_query_gpu as AQ
import test_radiance_query_gpu as RD
import test_ray_query_gpu as RQ
from test_denoise_frame_gpu import CANARY, _shifted

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _lim():
    return R.debug_loop_limits()


def _words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ================================================================ A. chunks
CHUNK_SCENES = ("cornell", "random")                   # the lean list class, and one BVH
SHAPE_KINDS = ("one_ray", "5_samples", "70_samples")    # 1 ray x P samples; P / 5 rays x 5; P / 70 rays x 70 (a chunk of 100 or 64 starts inside a ray)


def _shape(kind, paths):
    spp = {"one_ray": paths, "5_samples": 5, "70_samples": 70}[kind]
    return (1 if kind == "one_ray" else -(-paths // spp)), spp


def _two_chunks_each(launch_of, paths):
    """The smallest path count >= paths at which launch_of(paths) reports two chunks for every wave (later_trips_cases.paths_for_two_chunks)."""
    for _ in range(40):                                    # (the launch grows with the work until the device is full: a doubling per step)
        want = LT.paths_for_two_chunks(launch_of(paths), paths)
        if want == paths:
            return paths
        paths = want
    raise AssertionError(f"no path count found at which every wave has two chunks (last tried: {paths})")


def _assert_second_chunk(launch, chunk, n_paths, threads):
    assert launch["chunk"] == chunk and launch["threads"] == threads and launch["chunks"] == -(-n_paths // chunk), launch
    assert launch["chunks"] >= 2 * launch["waves"], f"no wave was sure of a second chunk: {launch}"


def _radiance_rays(name, n):
    return np.resize(RD._rays(name), (n, 7)).copy()        # the file's 1093 rays, repeated (the ray's INDEX keys its samples)


@pytest.mark.parametrize("kind", SHAPE_KINDS)
@pytest.mark.parametrize("name", CHUNK_SCENES)
def test_radiance_chunks_against_the_oracle_and_each_other(name, kind, monkeypatch):
    pb, ob, _, bg = RD._scene(name)
    depth = RD._depth(name)

    def launch_of(paths):                                  # max_depth = 0: the launch of that many paths without their work
        n, spp = _shape(kind, paths)
        R.query_radiance(pb, np.zeros((n, 7)), spp, 0, bg, RD.SEED)
        return R.last_query_launch(pb)
    monkeypatch.setenv("RT_RADIANCE_CHUNK", str(max(LT.CHUNKS)))
    n, spp = _shape(kind, _two_chunks_each(launch_of, LT.PATHS))
    rays = _radiance_rays(name, n)
    ref = orc.ray_color_paths(ob, rays, spp, bg, depth, RD.SEED)
    assert (ref != 0.0).any(axis=-1).mean() >= (0.25 if n > 1 else 0.01)
    first = None
    for chunk in LT.CHUNKS:
        monkeypatch.setenv("RT_RADIANCE_CHUNK", str(chunk))
        sums, samples, _ = R.query_radiance(pb, rays, spp, depth, bg, RD.SEED, want_samples=True)
        _assert_second_chunk(R.last_query_launch(pb), chunk, n * spp, _lim()["radiance_threads"])
        bad = RD._check_samples(f"{name} {n} x {spp} chunk {chunk}", samples, ref, RD.MAX_BAD)
        RD._check_sums(sums, samples, ref, bad)
        if first is None:
            first = samples
        else:                                              # "same samples with any value" (rt_host.cpp, where the variable is read)
            assert int((_words(samples) != _words(first)).sum()) == 0, f"chunk {chunk}: the samples differ from chunk {LT.CHUNKS[0]}'s"
    assert kind != "70_samples" or (100 % spp and 64 % spp)


def test_radiance_default_chunk_on_rays_that_need_no_oracle(monkeypatch):
    monkeypatch.delenv("RT_RADIANCE_CHUNK", raising=False)
    chunk, threads = _lim()["radiance_chunk"], _lim()["radiance_threads"]
    rs = np.random.RandomState(5)
    # straight up at the Cornell lamp from above the boxes: the lamp's emission, exactly; any order of adding 15.0 is exact
    pb, _, _, bg = RD._scene("cornell")
    n = 4099
    lamp = np.zeros((n, 7))
    lamp[:, 0] = rs.uniform(250.0, 306.0, n); lamp[:, 1] = 450.0; lamp[:, 2] = rs.uniform(250.0, 306.0, n); lamp[:, 4] = 1.0

    def launch_of(paths):
        R.query_radiance(pb, lamp, -(-paths // n), 0, bg, RD.SEED)
        return R.last_query_launch(pb)
    spp = -(-_two_chunks_each(launch_of, 2 * chunk * 64) // n)
    sums, samples, nonfinite = R.query_radiance(pb, lamp, spp, 50, bg, RD.SEED, want_samples=True)
    _assert_second_chunk(R.last_query_launch(pb), chunk, n * spp, threads)
    assert (samples == 15.0).all() and (sums == spp * 15.0).all() and nonfinite == 0
    # rays that leave the random-spheres world: the background, bit for bit; their sum within the any-order bound of spp equal terms
    rb, _, _, sky = RD._scene("random")
    spp = 8
    paths = _two_chunks_each(lambda p: (R.query_radiance(rb, np.zeros((-(-p // spp), 7)), spp, 0, sky, RD.SEED), R.last_query_launch(rb))[1], 2 * chunk * 64)
    n = -(-paths // spp)
    up = np.zeros((n, 7))
    up[:, 0:3] = rs.uniform((-10.0, 5.0, -10.0), (10.0, 9.0, 10.0), (n, 3))
    up[:, 3:6] = rs.normal(size=(n, 3)); up[:, 4] = np.abs(up[:, 4]) + 0.1
    sums, samples, _ = R.query_radiance(rb, up, spp, 8, sky, RD.SEED, want_samples=True)
    _assert_second_chunk(R.last_query_launch(rb), chunk, n * spp, threads)
    want = np.array(sky)
    assert np.array_equal(_words(samples), _words(np.broadcast_to(want, samples.shape).copy()))
    assert (np.abs(sums - spp * want) <= 2.0 * gamma(spp) * spp * np.abs(want)).all()


# ---- the pixel-list kernel: lists of 1, 65 and 256 pixels of tests/test_adaptive_gpu.py's 16 x 16 frame
LISTS = {"1_pixel": np.array([200], np.uint32), "65_pixels": np.arange(90, 155, dtype=np.uint32), "256_pixels": np.arange(AG.N_PX, dtype=np.uint32)}


def _render_list(pb, cam, bg, pixels, n_b, depth):
    import torch
    d_out = torch.from_numpy(AG._sentinel().copy()).cuda()
    d_list = torch.from_numpy(np.ascontiguousarray(pixels, np.uint32).view(np.int32).copy()).cuda()
    R.render_pixels_device(pb, cam, bg, AG.W, AG.H, n_b, depth, d_list, len(pixels), d_out, None, seed=AG.SEED)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _samples_are_not_negative(name):
    """The frames' samples of this view are >= 0 where they are finite: then sum|x| of a pixel is its sum (the bound below needs it)."""
    pb, cam, bg = AG._scene(name)
    _, samples = R.render(pb, cam, bg, AG.W, AG.H, 64, AG.DEPTH, seed=AG.SEED, want_samples=True)
    return bool((samples[np.isfinite(samples)] >= 0.0).all())


@pytest.mark.parametrize("which", tuple(LISTS))
@pytest.mark.parametrize("name", CHUNK_SCENES)
def test_pixel_list_chunks_against_the_frames_own_sums(name, which, monkeypatch):
    """The reference is the frames' own kernel, as in tests/test_adaptive_gpu.py, by its per-pixel sums (one pixel x a million samples has
    no room for the samples of a whole frame): a listed pixel holds the sentinel plus the sum of samples [0, n_b) of the frame of the same
    view and seed, within that file's bound with sum|x| = the sum (no sample is negative) and the reference sum's own any-order error
    (gamma_{n_b} of it) allowed for; an unlisted pixel keeps every word."""
    pb, cam, bg = AG._scene(name)
    pixels = LISTS[which]                                  # ("1_pixel": see below)
    assert _samples_are_not_negative(name)

    def launch_of(paths):
        _render_list(pb, cam, bg, pixels, -(-paths // len(pixels)), 0)
        return R.last_query_launch(pb)
    monkeypatch.setenv("RT_PIXELS_CHUNK", str(max(LT.CHUNKS)))
    n_b = -(-_two_chunks_each(launch_of, LT.PATHS) // len(pixels))
    ref = R.render(pb, cam, bg, AG.W, AG.H, n_b, AG.DEPTH, seed=AG.SEED).reshape(-1, 3)
    sent = AG._sentinel().reshape(-1, 3)
    # a pixel whose reference sum holds a non-finite sample can only be compared by its NaN / inf pattern: by the reference alone, the one
    # pixel is the first from the list's on whose sum is finite, and of a longer list most pixels must be
    fin = np.isfinite(ref).all(axis=1)
    if len(pixels) == 1:
        pixels = np.array([int(pixels[0]) + int(np.argmax(fin[int(pixels[0]):]))], np.uint32)
    assert fin[pixels.astype(np.int64)].mean() > (0.5 if len(pixels) > 1 else 0.99), "too few listed pixels have a finite reference sum"
    listed = np.zeros(AG.N_PX, bool); listed[pixels.astype(np.int64)] = True
    for chunk in LT.CHUNKS:
        monkeypatch.setenv("RT_PIXELS_CHUNK", str(chunk))
        out = _render_list(pb, cam, bg, pixels, n_b, AG.DEPTH).reshape(-1, 3)
        _assert_second_chunk(R.last_query_launch(pb), chunk, len(pixels) * n_b, _lim()["pixels_threads"])
        assert differing_words(out[~listed], sent[~listed]) == 0, chunk
        bad = 0
        for p in np.flatnonzero(listed):
            if not np.isfinite(ref[p]).all():
                assert AG.MC_masks_equal(out[p], sent[p] + ref[p]), (chunk, p)
                continue
            terms = ref[p] / (1.0 - gamma(n_b)) + sent[p]
            bound = 2.0 * gamma(n_b + 1) * terms + gamma(n_b) * ref[p] + n_b * AG.PARITY
            bad += not (np.abs(out[p] - (sent[p] + ref[p])) <= bound).all()
        print(f"{name} {which} x {n_b} chunk {chunk}: {bad} pixels outside the bound")
        assert bad <= (0 if name == "cornell" else min(AG.MAX_BAD, len(pixels) // 32)), chunk        # (2 of 65 or 256 pixels; of one pixel, none)


def test_pixel_list_default_chunk_on_views_that_need_no_reference(monkeypatch):
    monkeypatch.delenv("RT_PIXELS_CHUNK", raising=False)
    chunk, threads = _lim()["pixels_chunk"], _lim()["pixels_threads"]
    pixels = LISTS["256_pixels"]
    sent = AG._sentinel()
    # every pixel sees the Cornell lamp from below: 15.0 per sample, and any order of adding it to the sentinel (a multiple of 1/8) is exact
    pb, _, bg = AG._scene("cornell")
    under_the_lamp = Camera((278.0, 450.0, 279.5), (278.0, 554.0, 279.5), (0.0, 0.0, 1.0), 20.0, 1.0, 0.0, 10.0, 0.0, 1.0)

    def launch_of(paths):                                  # max_depth = 0: main.rs:42-45, nothing is added — and the launch is the same
        out = _render_list(pb, under_the_lamp, bg, pixels, -(-paths // AG.N_PX), 0)
        assert differing_words(out, sent) == 0
        return R.last_query_launch(pb)
    n_b = -(-_two_chunks_each(launch_of, 2 * chunk * 64) // AG.N_PX)
    out = _render_list(pb, under_the_lamp, bg, pixels, n_b, 50)
    _assert_second_chunk(R.last_query_launch(pb), chunk, AG.N_PX * n_b, threads)
    assert np.array_equal(out, sent + n_b * 15.0)
    # every pixel sees the sky of the random spheres: n_b times the background, within the any-order bound of n_b + 1 terms
    rb, _, sky = AG._scene("random")
    at_the_sky = Camera((0.0, 5.0, 0.0), (0.0, 50.0, 0.0), (0.0, 0.0, 1.0), 20.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    n_b = -(-_two_chunks_each(lambda p: (_render_list(rb, at_the_sky, sky, pixels, -(-p // AG.N_PX), 0), R.last_query_launch(rb))[1], 2 * chunk * 64) // AG.N_PX)
    out = _render_list(rb, at_the_sky, sky, pixels, n_b, 8)
    _assert_second_chunk(R.last_query_launch(rb), chunk, AG.N_PX * n_b, threads)
    want = np.array(sky)
    assert (np.abs(out - (sent + n_b * want)) <= 2.0 * gamma(n_b + 1) * (sent + n_b * np.abs(want))).all()


# ================================================================ B. query batches
def _grid(pb, call):
    """(workgroups, threads) of the grid a query of at least one whole grid gets: `call(n)` runs one, n = every CU's eight resident
    workgroups of 256 (no query kernel can have more) and the batch of rays."""
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    call(cus * 8 * _lim()["query_threads"] + LT.QUERY_RAYS)
    launch = R.last_query_launch(pb)
    assert launch["chunk"] == 0 and launch["chunks"] == 0 and launch["threads"] == _lim()["query_threads"]
    return launch["workgroups"], launch["threads"]


def _assert_second_batch(pb, n, blocks, threads):
    launch = R.last_query_launch(pb)
    assert (launch["workgroups"], launch["threads"]) == (blocks, threads) and n > blocks * threads, (launch, n)


@pytest.mark.parametrize("name", ["cornell", "teapot"])
def test_caller_rays_in_the_second_batch(name):
    """The 4133 hostile rays of tests/test_ray_query_gpu.py repeated up to one grid and 4133 rays: the last 4133 records are second-batch
    work of the first 17 workgroups, partial last wave included.  (No media in these scenes: a record does not depend on the ray's index.)"""
    pb, _, _ = RQ._scene(name)
    rays, (hit, rec) = RQ._rays(name), RQ._oracle_hits(name)
    assert len(rays) == LT.QUERY_RAYS
    blocks, threads = _grid(pb, lambda n: R.query_hits(pb, np.resize(rays, (n, 7)), 1e-5, RQ.SEED))
    n = blocks * threads + LT.QUERY_RAYS
    tiled = np.resize(rays, (n, 7)).copy()
    got = R.query_hits(pb, tiled, 1e-5, RQ.SEED)
    _assert_second_batch(pb, n, blocks, threads)
    n_bad, text = RQ._compare(name, got, tiled, np.resize(hit, n), np.resize(rec, (n, 10)))
    assert n_bad == 0, text
    # the albedo kernels: the records are the query's words, the albedo is the table's on the batch's first and last 4133 rays (the second
    # batch) and the same words for every repetition of a ray
    ob = RQ._scene(name)[1]
    blocks_a, threads_a = _grid(pb, lambda m: R.query_albedo(pb, np.resize(rays, (m, 7)), 1e-5, RQ.SEED))
    n_a = blocks_a * threads_a + LT.QUERY_RAYS
    tiled_a = tiled if n_a == n else np.resize(rays, (n_a, 7)).copy()
    albedo, hits = R.query_albedo(pb, tiled_a, 1e-5, RQ.SEED, want_hits=True)
    _assert_second_batch(pb, n_a, blocks_a, threads_a)
    assert int((_words(hits) != _words(got if n_a == n else R.query_hits(pb, tiled_a, 1e-5, RQ.SEED))).sum()) == 0
    for part in (slice(0, LT.QUERY_RAYS), slice(n_a - LT.QUERY_RAYS, n_a)):
        counts = AQ._check_table(name, pb, ob, albedo[part], hits[part])
        assert counts["miss"] > 0 and counts["exact"] > 100
    assert int((_words(albedo) != _words(np.resize(albedo[:LT.QUERY_RAYS], albedo.shape))).sum()) == 0


@pytest.mark.parametrize("name", ["cornell", "teapot"])
def test_camera_mode_in_the_second_batch(name):
    """A frame 1031 pixels wide and just higher than one grid: every ray is rt_camera_ray's on the host, and the records are the oracle's on
    the first and last 300 pixels of the frame, the 300 on either side of the grid's end, and 20 000 others."""
    W, seed, sample = 1031, 0x5EED + 3, 2
    pb, ob, cam = RQ._scene(name)
    blocks, threads = _grid(pb, lambda n: R.query_camera(pb, cam, W, -(-n // W), sample, seed))
    H = blocks * threads // W + 2
    n = W * H
    assert blocks * threads + W < n <= blocks * threads + 2 * W and n < 2 * blocks * threads
    hits, rays = R.query_camera(pb, cam, W, H, sample, seed, want_rays=True)
    _assert_second_batch(pb, n, blocks, threads)
    flat_rays, flat = rays.reshape(-1, 7), hits.reshape(-1, 16)
    ref = (C.c_double * (7 * n))()
    base, fn, cam_p = C.addressof(ref), R._rt().rt_camera_ray, C.byref(cam)
    for k in range(n):
        row, i = divmod(k, W)
        if fn(cam_p, W, H, i, H - 1 - row, seed, sample, C.cast(base + 56 * k, C.POINTER(C.c_double))) != 0:
            raise AssertionError(R._err())
    assert np.array_equal(flat_rays.view(np.uint64), np.frombuffer(ref, np.uint64).reshape(n, 7))
    edge = blocks * threads
    picked = np.unique(np.concatenate([np.arange(300), np.arange(n - 300, n), np.arange(edge - 300, edge + 300),
                                       np.random.RandomState(3).randint(0, n, 20000)]))
    assert len(picked) >= 20000 and (picked >= edge).sum() >= 300 + 300
    hit, rec = RQ._oracle(ob, flat_rays[picked], 0)
    n_bad, text = RQ._compare(name, flat[picked], flat_rays[picked], hit, rec)
    assert n_bad == 0, text
    assert hit.mean() > 0.25


# ================================================================ C. the compaction's scan and its neighbours
def _dev(a, off, dtype=np.float64):
    return AG._shifted(a, off, dtype)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "off8"])
@pytest.mark.parametrize("shape", LT.COMPACTION_SHAPES, **LT.IDS)
def test_select_past_the_scans_first_trip(shape, off):
    lim = _lim()
    assert LT.scan_trips(shape, lim) == {LT.COMPACTION_SHAPES[0]: 2, LT.COMPACTION_SHAPES[1]: 3}[shape]
    n_px = shape[0] * shape[1]
    maps = LT.need_maps(shape, lim["compaction_block_px"], lim["scan_threads"])
    S, Q, n, _ = LT.flag_state(shape, maps["empty"])
    dS, dQ, dn = _dev(S, off), _dev(Q, off), _dev(n, off, np.uint32)
    for name, pixels in maps.items():
        b = LT.flag_state(shape, pixels)[3]
        got = AG._device_select(dS, dQ, dn, _dev(b, off, np.uint32), shape, AC.N_B, 0.01, AC.MAX_SAMPLES, 0)
        twin = R.adaptive_select_host(S, Q, n, b, AC.N_B, 0.01, AC.MAX_SAMPLES, 0)
        assert len(got) == len(pixels) and (np.diff(got.astype(np.int64)) > 0).all(), name
        assert np.array_equal(got, twin) and np.array_equal(got, pixels), name
    # adaptive_cases' state at this size, with the dilation and the cap
    S, Q, n, b = LT.big_state(shape)
    dS, dQ, dn, db = _dev(S, off), _dev(Q, off), _dev(n, off, np.uint32), _dev(b, off, np.uint32)
    sizes = set()
    for tau, spread, cap in ((1.0 / 256.0, 1, AC.MAX_SAMPLES), (0.05, 0, AC.CAP), (0.05, 1, 40)):
        got = AG._device_select(dS, dQ, dn, db, shape, AC.N_B, tau, cap, spread)
        assert np.array_equal(got, R.adaptive_select_host(S, Q, n, b, AC.N_B, tau, cap, spread)), (tau, spread, cap)
        sizes.add(len(got))
    assert len(sizes) == 3 and min(sizes) > 0


@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "off8"])
@pytest.mark.parametrize("shape", LT.COMPACTION_SHAPES, **LT.IDS)
def test_error_merge_and_resolve_with_counts_past_their_first_sweep(shape, off):
    import torch
    lim = _lim()
    n_px = shape[0] * shape[1]
    assert LT.adaptive_resolve_trips(shape, lim) >= 2 and LT.trips(n_px, lim["adaptive_max_blocks"] * lim["adaptive_threads"]) >= 2
    S, Q, n, b = LT.big_state(shape)
    dS, dQ, dn, db = _dev(S, off), _dev(Q, off), _dev(n, off, np.uint32), _dev(b, off, np.uint32)
    # (A)
    tau = 0.05
    want, want_stats = R.adaptive_error_host(S, Q, n, b, tau=tau)
    d_e2 = torch.full((n_px,), -1.0, dtype=torch.float64, device="cuda")
    d_st = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    R.adaptive_error_device(dS, dQ, dn, db, shape[1], shape[0], d_e2, tau, d_st)
    assert differing_words(d_e2.cpu().numpy().reshape(shape), want) == 0
    assert R.moments_stats(d_st.cpu().numpy().view(np.uint64), tau) == want_stats
    # (D): image bytes and changed count, without and with a previous image
    want_img, _ = R.adaptive_resolve_rgb8_host(S, n)
    prev = want_img.copy(); prev.reshape(-1, 3)[::3, 1] ^= 1
    for p_host in (None, prev):
        d_img = torch.full((n_px * 3 + 4,), 9, dtype=torch.uint8, device="cuda")
        d_chg = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_prev = None if p_host is None else torch.from_numpy(p_host.reshape(-1).copy()).cuda()
        R.adaptive_resolve_rgb8_device(dS, dn, shape[1], shape[0], d_img, d_prev, d_chg)
        out = d_img.cpu().numpy()
        assert np.array_equal(out[:n_px * 3].reshape(want_img.shape), want_img) and (out[n_px * 3:] == 9).all()
        assert int(d_chg.cpu()[0]) == R.adaptive_resolve_rgb8_host(S, n, p_host)[1]
    # (C): the merge over a list longer than one sweep of its grid
    p = np.random.RandomState(5).uniform(0.0, 8.0, shape + (3,))
    pixels = LT.need_maps(shape, lim["compaction_block_px"], lim["scan_threads"])["random_50pc"]
    assert LT.trips(len(pixels), lim["adaptive_max_blocks"] * lim["adaptive_threads"]) >= 2
    host = [a.copy() for a in (p, S, Q, n, b)]
    R.adaptive_merge_host(host[0], AC.N_B, host[1], host[2], host[3], host[4], pixels)
    dev = [_dev(p, off), _dev(S, off), _dev(Q, off), _dev(n, off, np.uint32), _dev(b, off, np.uint32)]
    R.adaptive_merge_device(dev[0], AC.N_B, dev[1], dev[2], dev[3], dev[4], _dev(pixels, 0, np.uint32), len(pixels))
    for g, w in zip(dev[:3], host[:3]):
        assert differing_words(g.cpu().numpy().reshape(w.shape), w) == 0
    assert np.array_equal(AG._u32(dev[3]).reshape(shape), host[3]) and np.array_equal(AG._u32(dev[4]).reshape(shape), host[4])


# ================================================================ D. the denoisers' element-wise kernels and filters
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned-16", "8-bytes-off"])
def test_variance_kernels_past_their_first_sweep(offset):
    import torch
    shape = LT.DENOISE_SHAPE
    H, W = shape
    assert LT.pair_trips(shape, _lim(), "variance") >= 2 and LT.pair_trips(shape, _lim(), "denoise_frame") >= 2 and (H * W * 3) % 2 == 1
    # rt_moments_variance_device (rt_denoise_var.hip)
    S, Q, N, B = MC.state(shape)
    want = R.moments_variance_host(S, Q, N, B)
    d_s, _ = _shifted(S, offset, torch.float64); d_q, _ = _shifted(Q, offset, torch.float64)
    d_v, v_buf = _shifted(np.full(S.shape, CANARY), offset, torch.float64)
    assert d_s.data_ptr() % 16 == 8 * offset
    R.moments_variance_device(d_s, d_q, N, B, W, H, d_v)
    torch.cuda.synchronize()
    out = v_buf.cpu().numpy()
    assert differing_words(out[offset:offset + S.size].reshape(S.shape), want) == 0
    assert np.all(out[:offset] == CANARY) and np.all(out[offset + S.size:] == CANARY)
    # rt_adaptive_variance_device (rt_denoise_frame.hip)
    S, Q, n, b = FC.variance_state(shape)
    want = R.adaptive_variance_host(S, Q, n, b)
    d_s, _ = _shifted(S, offset, torch.float64); d_q, _ = _shifted(Q, offset, torch.float64)
    d_n, _ = _shifted(n, offset, torch.int32); d_b, _ = _shifted(b, offset, torch.int32)
    d_v, v_buf = _shifted(np.full(S.shape, CANARY), offset, torch.float64)
    R.adaptive_variance_device(d_s, d_q, d_n, d_b, W, H, d_v)
    torch.cuda.synchronize()
    out = v_buf.cpu().numpy()
    assert differing_words(out[offset:offset + S.size].reshape(S.shape), want) == 0
    assert np.all(out[:offset] == CANARY) and np.all(out[offset + S.size:] == CANARY)


@pytest.mark.parametrize("combo", FC.COMBOS, ids=FC.combo_id)
def test_denoise_frame_past_the_first_sweep(combo):
    """K = 2: the LDS forms of the filters at steps 1 and 2 on 38 x 37 tiles, between element-wise kernels in their second trip; 16-byte
    aligned frames through the host form, and every frame 8 bytes off through the device form (the one-double tail kernels start at
    first != 0)."""
    import torch
    shape = LT.DENOISE_SHAPE
    H, W = shape
    assert LT.pair_trips(shape, _lim(), "denoise_frame") >= 2
    rgb, n, var, alb, hits = FC.frames(shape, combo)
    k, sigma, flags = 2, (VC.SIGMAS if combo[1] else DC.SIGMAS)[0], 1
    want = R.denoise_frame_host(rgb, hits, n, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, k, sigma, flags, want_var=combo[1])
    got = R.denoise_frame(rgb, hits, n, FC.SAMPLES, var, alb, FC.ALBEDO_SAMPLES, k, sigma, flags, want_var=combo[1])
    if combo[1]:
        assert differing_words(got[0], want[0]) == 0 and differing_words(got[1], want[1]) == 0
    else:
        assert differing_words(got, want) == 0
    d_hits = torch.from_numpy(hits.copy()).cuda()
    d_sum, _ = _shifted(rgb, 1, torch.float64)
    d_n = None if n is None else _shifted(n, 1, torch.int32)[0]
    d_var = None if var is None else _shifted(var, 1, torch.float64)[0]
    d_alb = None if alb is None else _shifted(alb, 1, torch.float64)[0]
    d_out, out_buf = _shifted(np.full(rgb.shape, CANARY), 1, torch.float64)
    d_vout, vout_buf = _shifted(np.full(shape, CANARY), 1, torch.float64)
    assert d_sum.data_ptr() % 16 == 8 and d_out.data_ptr() % 16 == 8
    R.denoise_frame_device(d_sum, d_hits, W, H, d_n, FC.SAMPLES, d_var, d_alb, FC.ALBEDO_SAMPLES, d_out, d_vout if combo[1] else None, None, k, sigma, flags)
    torch.cuda.synchronize()
    out = out_buf.cpu().numpy(); vout = vout_buf.cpu().numpy()
    assert differing_words(out[1:1 + rgb.size].reshape(rgb.shape), want[0] if combo[1] else want) == 0
    assert out[0] == CANARY and np.all(out[1 + rgb.size:] == CANARY)
    if combo[1]:
        assert differing_words(vout[1:1 + H * W].reshape(shape), want[1]) == 0 and vout[0] == CANARY and np.all(vout[1 + H * W:] == CANARY)
    assert differing_words(d_sum.cpu().numpy().reshape(rgb.shape), rgb) == 0


def test_the_filters_direct_form_at_this_size():
    """K = 3: step 4 runs the direct form (64 x 4 tiles) of both filters on the large frame too."""
    shape = LT.DENOISE_SHAPE
    rgb, var, hits = VC.case(shape)
    for flags in (0, 1):
        assert differing_words(R.denoise(rgb, DC.SAMPLES, hits, 3, DC.SIGMAS[0], flags), R.denoise_host(rgb, DC.SAMPLES, hits, 3, DC.SIGMAS[0], flags)) == 0
    got = R.denoise_variance(rgb, VC.SAMPLES, var, hits, 3, VC.SIGMAS[0], 1, want_var=True)
    want = R.denoise_variance_host(rgb, VC.SAMPLES, var, hits, 3, VC.SIGMAS[0], 1, want_var=True)
    assert differing_words(got[0], want[0]) == 0 and differing_words(got[1], want[1]) == 0


# ================================================================ E. the resolve
def _format_values(vals, n):
    """rt_format_color of every value of a 1-d array for n samples (a channel's byte depends on its own sum alone)."""
    padded = np.concatenate([vals, np.zeros(-len(vals) % 3)])
    return R.format_image(padded.reshape(-1, 1, 3), n).reshape(-1)[:len(vals)]


def test_resolve_past_its_grid(pbe):
    """A progressive frame of 2897 x 2897 pixels filled by load with tests/test_progressive_gpu.py's known-answer sums, repeated: the lanes
    of the first workgroups take a second group of four pixels, and the frame's last pixel is the byte-wise tail.  The reference is
    rt_format_color of the 22 k values, repeated like them.  A load makes the next resolve a first one (it reports W * H), so the pixels
    that change before the second resolve are changed the only way a frame offers without that: one pass of one sample at max_depth 0,
    which adds 0.0 to every sum and 1 to the sample count — the changed pixels are those whose bytes differ between 1000 and 1001 samples,
    a set known from rt_format_color alone, made to hold the frame's last pixel and the first pixel of the kernel's second trip."""
    from raytracinginrust_amd import scenes
    from test_progressive_gpu import _known_answer_sums
    lim = _lim()
    H, W = LT.RESOLVE_SHAPE
    n_px = H * W
    assert LT.resolve_trips(LT.RESOLVE_SHAPE, lim) == 2 and n_px % lim["resolve_px_per_lane"] == 1
    n = 1000
    vals = _known_answer_sums(n)
    flat = np.resize(vals, n_px * 3)
    second_trip = lim["resolve_max_blocks"] * lim["resolve_threads"] * lim["resolve_px_per_lane"]
    assert second_trip < n_px
    boundary = np.array([n * 0.25, n * 0.25, n * 0.25])                         # 128 at 1000 samples, 127 at 1001
    assert _format_values(boundary, n).tolist() == [128] * 3 and _format_values(boundary, n + 1).tolist() == [127] * 3
    for p in (second_trip, n_px - 1):
        flat[3 * p:3 * p + 3] = boundary
    want = {}
    for m in (n, n + 1):
        w = np.resize(_format_values(vals, m), n_px * 3)
        for p in (second_trip, n_px - 1):
            w[3 * p:3 * p + 3] = 128 if m == n else 127
        want[m] = w.reshape(H, W, 3)
    moved = (want[n] != want[n + 1]).any(axis=2)
    assert moved.reshape(-1)[second_trip] and moved.reshape(-1)[n_px - 1] and moved.reshape(-1)[second_trip:].sum() > 2 and 0 < moved.sum() < n_px // 2
    sums = flat.reshape(H, W, 3)
    b, cam, bg = scenes.cornell_box(pbe)
    with R.Progressive(b, cam, bg, W, H, 0) as frame:
        frame.load(sums, n)
        img, changed = frame.rgb8()
        assert int((img.astype(np.uint64) != want[n]).sum()) == 0 and changed == n_px and len(np.unique(want[n])) == 256
        frame.add(1)                                                           # max_depth = 0 (main.rs:42-45): every sample is (0, 0, 0)
        assert frame.samples == n + 1
        after = frame.sum()
        assert ((after == sums) | (np.isnan(after) & np.isnan(sums))).all()
        img2, changed2 = frame.rgb8()
        assert int((img2.astype(np.uint64) != want[n + 1]).sum()) == 0 and changed2 == int(moved.sum())
        assert frame.rgb8()[1] == 0

"""The averaged denoising guide on the GPU (rt_query_camera_guide and its _device form, csrc/rt_guide.hip; progressive frames with
guide_samples > 1) against the specification of csrc/rt_guide.h.

The reference for every comparison is the stack of single-sample rt_query_camera records — kernels this feature does not touch, held to
the oracle by tests/test_ray_query_gpu.py — reduced by the NumPy restatement of tests/guide_cases.py (a sequential loop over the samples).
The code under test is never its own reference.  What is required: 0 differing 64-bit words, a NaN matching any NaN, on one scene per
kernel class (list, one-BVH with a lens and moving spheres, mesh, media with an image texture, object leaves), for 1, 2 and 5 samples from
sample 0 and from sample 3, at 23 x 11 pixels (253: three whole waves and one of 61 lanes in a single batch); the fused albedo output is
rt_query_camera_albedo's words; a lane's second batch; the _device form on a stream of the caller's; and progressive frames whose four
denoised resolves equal, byte for byte, the host filters on the host-built guide."""
import functools

import numpy as np
import pytest

from raytracinginrust_amd import render as R

import guide_cases as G
import test_ray_query_gpu as RQ

pytestmark = pytest.mark.gpu

GW, GH, GSEED = 23, 11, 0x5EED + 11
SCENES = ("cornell", "random", "teapot", "final", "medium_bvh")     # list, one BVH (lens, moving spheres), mesh, media + image texture, object leaves
N_SAMPLES = (1, 2, 5)
FIRST = (0, 3)


@functools.lru_cache(maxsize=None)
def _single(name, sample, W=GW, H=GH, seed=GSEED):
    pb, _, cam = RQ._scene(name)
    out = R.query_camera(pb, cam, W, H, sample, seed)
    out.setflags(write=False)
    return out


def _reference(name, first, n, W=GW, H=GH, seed=GSEED):
    return G.numpy_guide(np.stack([_single(name, first + s, W, H, seed) for s in range(n)]))


# ---------------------------------------------------------------- 1. the kernel is the specification, per scene class
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("n", N_SAMPLES)
@pytest.mark.parametrize("name", SCENES)
def test_guide_equals_the_reduced_single_sample_records(name, n, first):
    pb, _, cam = RQ._scene(name)
    got = R.query_camera_guide(pb, cam, GW, GH, first, n, GSEED)
    want = _reference(name, first, n)
    assert got.shape == (GH, GW, 16)
    assert G.differing_words(got, want) == 0, np.argwhere(~RQ._same(got, want))[:5].tolist()
    assert R.last_query_ms(pb) > 0.0
    launch = R.last_query_launch(pb)
    assert launch["workgroups"] == 1 and launch["threads"] == 256 and launch["chunks"] == 0      # one batch: 253 lanes of one workgroup
    assert (want[..., 0] != 0.0).any()
    if n == 1:                                                                                  # words [0]-[8], [11], [12] are rt_query_camera's as values
        words = list(G.WORDS_OF_ONE_SAMPLE)
        a, b = got[..., words], _single(name, first)[..., words]
        assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()
    if name in ("final", "medium_bvh") and n == 5:                                              # the medium's draws come from the path's stream
        medium = np.stack([_single(name, first + s) for s in range(n)])
        assert ((medium[..., 0] != 0.0) & (medium[..., 11] == -1.0)).any()


def test_the_random_spheres_samples_really_differ():
    """Under the lens and the shutter a pixel's samples see other things: some pixel is covered partly, some pixel sees two materials."""
    for first in FIRST:
        want = _reference("random", first, 5)
        hits, material = want[..., 15], want[..., 11]
        assert ((hits > 0) & (hits < 5)).any(), first
        assert ((material == -1.0) & (hits >= 2)).any(), first
        stack = np.stack([_single("random", first + s) for s in range(5)])
        assert (stack[..., 11].max(axis=0) != stack[..., 11].min(axis=0)).sum() >= 5


# ---------------------------------------------------------------- 2. the fused albedo output
@pytest.mark.parametrize("name", SCENES)
def test_fused_albedo_is_the_albedo_querys_words(name):
    pb, _, cam = RQ._scene(name)
    for first, n in ((0, 1), (3, 5)):
        guide, alb = R.query_camera_guide(pb, cam, GW, GH, first, n, GSEED, want_albedo=True)
        want_alb = R.query_camera_albedo(pb, cam, GW, GH, first, n, GSEED)
        assert G.differing_words(alb, want_alb) == 0
        assert G.differing_words(guide, R.query_camera_guide(pb, cam, GW, GH, first, n, GSEED)) == 0
        assert G.differing_words(guide, _reference(name, first, n)) == 0
    assert (want_alb != 5.0).any()


# ---------------------------------------------------------------- 3. a lane's second batch
def test_guide_in_the_second_batch():
    """A Cornell-box frame 1031 pixels wide and a quarter higher than one grid of the guide kernel (less than a second whole batch: the
    bottom fifth of the picture, floor and box fronts, is second-trip work of the first workgroups), two samples.
    (tests/test_later_trips_gpu.py's pattern: the grid is read from what the library reports.)"""
    import torch
    W, seed, n_samples = 1031, 0x5EED + 3, 2
    pb, _, cam = RQ._scene("cornell")
    threads = R.debug_loop_limits()["query_threads"]
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    for albedo in (False, True):
        R.query_camera_guide(pb, cam, W, -(-(cus * 8 * threads + W) // W), 0, 1, seed, want_albedo=albedo)      # at least one whole grid
        launch = R.last_query_launch(pb)
        blocks = launch["workgroups"]
        assert launch["threads"] == threads and launch["chunk"] == 0 and launch["chunks"] == 0
        H = blocks * threads * 5 // (4 * W) + 1
        n = W * H
        assert blocks * threads + W < n < 2 * blocks * threads
        out = R.query_camera_guide(pb, cam, W, H, 0, n_samples, seed, want_albedo=albedo)
        launch = R.last_query_launch(pb)
        assert (launch["workgroups"], launch["threads"]) == (blocks, threads) and n > blocks * threads, (launch, n)      # a lane took a second trip
        guide = out[0] if albedo else out
        want = G.numpy_guide(np.stack([R.query_camera(pb, cam, W, H, s, seed) for s in range(n_samples)]))
        assert G.differing_words(guide, want) == 0
        second = want.reshape(-1, 16)[blocks * threads:]
        assert (second[:, 0] != 0.0).mean() > 0.25 and (second[:, 0] == 0.0).any()                  # the second trip's pixels see the box
        if albedo:
            assert G.differing_words(out[1], R.query_camera_albedo(pb, cam, W, H, 0, n_samples, seed)) == 0


@pytest.mark.parametrize("albedo", [False, True], ids=["guide", "guide_and_albedo"])
def test_the_staged_filter_tree_changes_no_word(albedo, monkeypatch):
    pb, _, cam = RQ._scene("random")

    def call():
        out = R.query_camera_guide(pb, cam, RQ.STAGE_W, RQ.STAGE_H, 1, 3, GSEED, want_albedo=albedo)
        return out if albedo else (out,)
    RQ.assert_staging_changes_no_word(pb, call, monkeypatch)


# ---------------------------------------------------------------- 4. the _device form
@pytest.mark.parametrize("name", ["cornell", "random"])
def test_device_form(name):
    """Torch tensors on a stream of the caller's: word for word the host form; nothing behind the last record is touched; a buffer that is
    too small is an error and writes nothing."""
    import torch
    pb, _, cam = RQ._scene(name)
    n = GW * GH
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    with torch.cuda.stream(stream):
        d_guide = torch.full((n + 1, 16), canary, dtype=torch.float64, device=dev)
        d_guide2 = torch.full((n + 1, 16), canary, dtype=torch.float64, device=dev)
        d_alb = torch.full((n + 1, 3), canary, dtype=torch.float64, device=dev)
        R.query_camera_guide_device(pb, cam, GW, GH, d_guide, None, 3, 5, GSEED, stream=stream.cuda_stream)
        R.query_camera_guide_device(pb, cam, GW, GH, d_guide2, d_alb, 3, 5, GSEED, stream=stream.cuda_stream)
    stream.synchronize()
    g, g2, a = d_guide.cpu().numpy(), d_guide2.cpu().numpy(), d_alb.cpu().numpy()
    want = _reference(name, 3, 5).reshape(-1, 16)
    assert G.differing_words(g[:n], want) == 0 and G.differing_words(g2[:n], want) == 0 and np.all(g[n] == canary) and np.all(g2[n] == canary)
    assert G.differing_words(a[:n], R.query_camera_albedo(pb, cam, GW, GH, 3, 5, GSEED).reshape(-1, 3)) == 0 and np.all(a[n] == canary)
    small = torch.full((n, 16), canary, dtype=torch.float64, device=dev)
    with pytest.raises(R.RenderError, match="guide buffer too small"):
        R.query_camera_guide_device(pb, cam, GW + 1, GH, small, None, 0, 2, GSEED, stream=stream.cuda_stream)
    with pytest.raises(R.RenderError, match="albedo buffer too small"):
        R.query_camera_guide_device(pb, cam, GW, GH, small, d_alb[:n - 1], 0, 2, GSEED, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.all(small.cpu().numpy() == canary)


# ---------------------------------------------------------------- 5. progressive frames
PW, PH, PDEPTH, PSEED, PGUIDE = 40, 24, 8, 0x5EED + 23, 4


def _host_guide(name, n):
    pb, _, cam = RQ._scene(name)
    return R.guide_from_hits(np.stack([R.query_camera(pb, cam, PW, PH, s, PSEED) for s in range(n)]))


def test_guide_samples_one_is_the_frame_as_it_was(pbe):
    from conftest import build_scene
    b, cam, bg = build_scene("random", pbe)
    k, sigma = 2, R.DENOISE_SIGMA
    with R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED) as plain, R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED, guide_samples=1) as one:
        plain.add(8); one.add(8)
        assert plain.guide_info() == (1, 0) and one.guide_info() == (1, 0)
        a, c = plain.rgb8_denoised(k, sigma), one.rgb8_denoised(k, sigma)
        assert np.array_equal(a, c) and plain.guide_info() == (1, 1) and one.guide_info() == (1, 1)
        want = R.format_image(R.denoise_host(plain.sum(), plain.samples, R.query_camera(b, cam, PW, PH, 0, PSEED), k, sigma, 0), plain.samples)
        assert np.array_equal(a.astype(np.uint64), want)
        one.set_guide_samples(1)                                                # the value in force: nothing is dropped
        assert np.array_equal(one.rgb8_denoised(k, sigma), a) and one.guide_info() == (1, 1)
        with pytest.raises(R.RenderError, match="guide_samples"):
            one.set_guide_samples(0)
        assert one.guide_info() == (1, 1)


def test_progressive_resolves_with_an_averaged_guide(pbe):
    """Each of the four denoised resolves equals format_color of its host filter on the frame's sums and guide_from_hits of the stacked
    single-sample records; another guide_samples rebuilds once; reset drops the guide; the frame resolves after its scene is gone."""
    from conftest import build_scene
    b, cam, bg = build_scene("random", pbe)
    k, sigma, sigma_v = 2, R.DENOISE_SIGMA, R.DENOISE_VARIANCE_SIGMA
    guide = _host_guide("random", PGUIDE)
    assert ((guide[..., 15] > 0) & (guide[..., 15] < PGUIDE)).any() and (guide[..., 0] != R.query_camera(b, cam, PW, PH, 0, PSEED)[..., 0]).any()
    alb = R.query_camera_albedo(b, cam, PW, PH, 0, 4, PSEED)
    with R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED, moments=True, guide_samples=PGUIDE) as frame:
        for _ in range(4):
            frame.add(2)
        assert frame.samples == 8 and frame.guide_info() == (PGUIDE, 0)
        s, N = frame.sum(), frame.samples
        V = R.moments_variance_host(s, frame.sq_sum(), N, frame.passes)
        got = frame.rgb8_denoised(k, sigma)
        assert frame.guide_info() == (PGUIDE, 1)
        assert np.array_equal(got.astype(np.uint64), R.format_image(R.denoise_host(s, N, guide, k, sigma, 0), N))
        assert np.array_equal(frame.rgb8_denoised_albedo(4, k, sigma).astype(np.uint64), R.format_image(R.denoise_albedo_host(s, N, alb, 4, guide, k, sigma, 0), N))
        assert np.array_equal(frame.rgb8_denoised_variance(k, sigma_v).astype(np.uint64), R.format_image(R.denoise_variance_host(s, N, V, guide, k, sigma_v, 0), N))
        assert np.array_equal(frame.rgb8_denoised_frame(k, sigma_v, variance=True, albedo_samples=4).astype(np.uint64),
                              R.format_image(R.denoise_frame_host(s, guide, None, N, V, alb, 4, k, sigma_v, 0), N))
        assert np.array_equal(frame.rgb8_denoised_frame(k, sigma).astype(np.uint64), R.format_image(R.denoise_frame_host(s, guide, None, N, None, None, 1, k, sigma, 0), N))
        assert frame.guide_info() == (PGUIDE, 1)                                # one guide served all of them
        sample0 = R.format_image(R.denoise_host(s, N, R.query_camera(b, cam, PW, PH, 0, PSEED), k, sigma, 0), N)
        assert (got.astype(np.uint64) != sample0).any()                         # ... and it is another guide than sample 0's
        # the key: another flags value re-packs the same records
        assert np.array_equal(frame.rgb8_denoised(k, sigma, R.RT_DENOISE_SAME_MATERIAL).astype(np.uint64),
                              R.format_image(R.denoise_host(s, N, guide, k, sigma, R.RT_DENOISE_SAME_MATERIAL), N))
        builds = frame.guide_info()[1]
        # another value rebuilds once
        frame.set_guide_samples(2)
        assert frame.guide_info() == (2, builds)
        two = frame.rgb8_denoised(k, sigma)
        assert frame.guide_info() == (2, builds + 1)
        assert np.array_equal(two.astype(np.uint64), R.format_image(R.denoise_host(s, N, _host_guide("random", 2), k, sigma, 0), N))
        assert np.array_equal(frame.rgb8_denoised(k, sigma), two) and frame.guide_info() == (2, builds + 1)
        frame.set_guide_samples(1)
        assert np.array_equal(frame.rgb8_denoised(k, sigma).astype(np.uint64), sample0) and frame.guide_info() == (1, builds + 2)
        # reset drops the guide and keeps the setting
        frame.set_guide_samples(PGUIDE)
        frame.rgb8_denoised(k, sigma)
        frame.reset()
        frame.add(2); frame.add(1)
        n_before = frame.guide_info()[1]
        again = frame.rgb8_denoised(k, sigma)
        assert frame.guide_info() == (PGUIDE, n_before + 1)
        assert np.array_equal(again.astype(np.uint64), R.format_image(R.denoise_host(frame.sum(), frame.samples, guide, k, sigma, 0), frame.samples))


def test_a_frame_with_a_guide_resolves_after_its_scene_is_gone(pbe):
    from conftest import build_scene
    b, cam, bg = build_scene("random", pbe)                                    # a scene of this test's own: it is destroyed below
    guide = R.guide_from_hits(np.stack([R.query_camera(b, cam, PW, PH, s, PSEED) for s in range(PGUIDE)]))
    k, sigma = 2, R.DENOISE_SIGMA
    frame = R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED, guide_samples=PGUIDE)
    try:
        frame.add(4)
        before = frame.rgb8_denoised(k, sigma)
        b.close()
        assert np.array_equal(frame.rgb8_denoised(k, sigma), before)
        assert np.array_equal(before.astype(np.uint64), R.format_image(R.denoise_host(frame.sum(), frame.samples, guide, k, sigma, 0), frame.samples))
        frame.set_guide_samples(2)
        with pytest.raises(R.RenderError, match="destroyed"):
            frame.rgb8_denoised(k, sigma)
    finally:
        frame.close()

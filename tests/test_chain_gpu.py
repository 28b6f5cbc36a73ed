"""Specular-chain guides on the GPU (rt_query_chain, rt_query_camera_chain_guide and their _device forms, csrc/rt_chain.hip; progressive
frames with set_guide_chain) against the specification of csrc/rt_chain.h.

The reference of every comparison is the NumPy restatement of tests/chain_cases.py composed with searches that are not under test: link l
of all items is one render.query_albedo(rays_l, t_min, seed_link, want_hits=True) call — the records are rt_query_hits' words
(tests/test_albedo_query_gpu.py, tests/test_ray_query_gpu.py pin both to the oracle) — and link 0 of the camera form is
render.query_camera(sample) with render.query_camera_albedo(sample, 1).  The code under test is never its own reference.  What is required:
0 differing 64-bit words, a NaN matching any NaN.  Views are 23 x 11 (253 items: three whole waves and one of 61 lanes); the caller-ray batches
add the 64 aimed rays (317: a partial last wave in a second workgroup)."""
import functools

import numpy as np
import pytest

from raytracinginrust_amd import render as R

import chain_cases as CC

pytestmark = pytest.mark.gpu

SEED = 0x5EED + 31
SCENES = ("chain", "cornell", "random", "teapot", "final")         # the test scene (media, textures), list, one BVH, mesh, object leaves
MAX_LINKS = (0, 1, 4, 64)
N_SAMPLES = ((1, 0), (5, 3))                                       # (n_samples, first_sample)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(scene, camera, Materials) in the library, built once."""
    from conftest import build_scene
    from raytracinginrust_amd import _lib, scenes
    pbe = _lib.load()
    if name == "chain":
        return CC.chain_scene(pbe)
    return CC.build_recorded(build_scene, name, pbe, scenes.load_earthmap() if name == "final" else None)


def _search(pb):
    def search(l, rays, seed):
        albedo, hits = R.query_albedo(pb, rays, CC.T_MIN, seed, want_hits=True)
        return hits, albedo
    return search


@functools.lru_cache(maxsize=None)
def _camera_sample(name, sample):
    """(rays, hits, albedo) of sample `sample` of the 23 x 11 view, flat: kernels this feature does not touch."""
    pb, cam, _ = _scene(name)
    hits, rays = R.query_camera(pb, cam, CC.W, CC.H, sample, SEED, want_rays=True)
    alb = R.query_camera_albedo(pb, cam, CC.W, CC.H, sample, 1, SEED)
    out = rays.reshape(-1, 7), hits.reshape(-1, 16), alb.reshape(-1, 3)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _caller_rays(name):
    rays = _camera_sample(name, 0)[0]
    if name == "chain":
        rays = np.concatenate([rays, CC.aimed_rays()])
    rays = np.ascontiguousarray(rays)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _caller_chain(name, max_links, max_fuzz):
    pb, _, mats = _scene(name)
    return CC.numpy_chain(_search(pb), _caller_rays(name), mats, max_links, max_fuzz, SEED)


@functools.lru_cache(maxsize=None)
def _camera_chain(name, sample, max_links, max_fuzz):
    pb, _, mats = _scene(name)
    rays, hits, alb = _camera_sample(name, sample)
    return CC.numpy_chain(_search(pb), rays, mats, max_links, max_fuzz, SEED, sample_index=sample, first=(hits, alb))


def _assert_words(got, want, what):
    bad = CC.differing_words(got, want)
    assert bad == 0, (what, bad, np.argwhere(np.asarray(got).view(np.uint64) != np.asarray(want).view(np.uint64))[:5].tolist())


# ---------------------------------------------------------------- 1. caller rays
@pytest.mark.parametrize("max_links", MAX_LINKS)
@pytest.mark.parametrize("name", SCENES)
def test_query_chain_equals_the_restatement(name, max_links):
    pb, _, _ = _scene(name)
    rays = _caller_rays(name)
    for max_fuzz in ((0.0, CC.INF) if name in ("chain", "random") else (0.0,)):
        want = _caller_chain(name, max_links, max_fuzz)
        hits, alb = R.query_chain(pb, rays, max_links, max_fuzz, CC.T_MIN, SEED, want_albedo=True)
        _assert_words(hits, want["hits"], "hits"); _assert_words(alb, want["albedo"], "albedo")
        _assert_words(R.query_chain(pb, rays, max_links, max_fuzz, CC.T_MIN, SEED), want["hits"], "hits without albedo")
        assert (hits[:, 15] == want["links"]).all() and (want["links"] <= max_links).all()
    assert R.last_query_ms(pb) > 0.0
    launch = R.last_query_launch(pb)
    assert launch["threads"] == R.debug_loop_limits()["query_threads"] and launch["workgroups"] == -(-len(rays) // launch["threads"]) and launch["chunks"] == 0
    if max_links == 0:                                           # the very words of the first-hit queries
        albedo0, hits0 = R.query_albedo(pb, rays, CC.T_MIN, SEED, want_hits=True)
        _assert_words(hits, R.query_hits(pb, rays, CC.T_MIN, SEED), "rt_query_hits"); _assert_words(hits, hits0, "hits"); _assert_words(alb, albedo0, "rt_query_albedo")
    elif name != "teapot":                                       # the comparison is about chains: some item follows a link
        assert (want["links"] >= 1).any(), name
    if name == "chain" and max_links == 64:                      # ... and on the test scene every kind of chain (tests/test_chain_host.py)
        c = _caller_chain(name, 64, 0.0)
        tail, end = c["links"][-64:], c["end"][-64:]
        assert {CC.END_SURFACE, CC.END_MISS, CC.END_ABSORBED, CC.END_FUZZ, CC.END_MAX_LINKS} <= set(end.tolist())
        assert (tail == 0).any() and (tail == 1).any() and (tail >= 3).any() and (tail >= 1).mean() >= 0.25
        assert c["seen"]["cannot_refract"][-64:].any() and c["seen"]["reflects_by_fresnel"][-64:].any()
        assert ((c["hits"][:, 0] != 0.0) & (c["hits"][:, 11] == -1.0)).any()                    # a medium ends a chain
        assert (c["albedo"] != 1.0).any() and (np.abs(c["albedo"] - c["weight"]) > 0).any()


# ---------------------------------------------------------------- 2. the camera form
@pytest.mark.parametrize("max_links", MAX_LINKS)
@pytest.mark.parametrize("n,first", N_SAMPLES)
@pytest.mark.parametrize("name", SCENES)
def test_camera_chain_guide_equals_the_restatement(name, n, first, max_links):
    pb, cam, _ = _scene(name)
    max_fuzz = CC.INF if (name == "random" and n == 5) else 0.0
    want_guide, want_alb, want_links = CC.numpy_camera_chain_guide([_camera_chain(name, first + s, max_links, max_fuzz) for s in range(n)])
    guide, alb, links = R.query_camera_chain_guide(pb, cam, CC.W, CC.H, max_links, max_fuzz, first, n, SEED, want_albedo=True, want_links=True)
    assert guide.shape == (CC.H, CC.W, 16) and alb.shape == (CC.H, CC.W, 3) and links.shape == (CC.H, CC.W) and links.dtype == np.uint32
    _assert_words(guide.reshape(-1, 16), want_guide, "guide"); _assert_words(alb.reshape(-1, 3), want_alb, "albedo sums")
    assert (links.reshape(-1) == want_links).all()
    _assert_words(R.query_camera_chain_guide(pb, cam, CC.W, CC.H, max_links, max_fuzz, first, n, SEED), guide, "guide alone")
    launch = R.last_query_launch(pb)
    assert launch["workgroups"] == 1 and launch["threads"] == 256 and launch["chunks"] == 0
    if max_links == 0:
        g0, a0 = R.query_camera_guide(pb, cam, CC.W, CC.H, first, n, SEED, want_albedo=True)
        _assert_words(guide, g0, "rt_query_camera_guide"); _assert_words(alb, a0, "its albedo sums"); assert (links == 0).all()
    elif name != "teapot":
        assert (links > 0).any(), name


# ---------------------------------------------------------------- 3. ended lanes keep their result
def test_ended_lanes_keep_their_result():
    """Five waves in which exactly one lane chains for 64 links between the mirrors while the other 63 end at link 0, and five waves whose
    lanes' chains have 0, 1, 2, ... links by lane: every record and albedo is the restatement's."""
    pb, _, mats = _scene("chain")
    aimed = CC.aimed_rays()
    c = _caller_chain("chain", 64, 0.0)
    pool, links = _caller_rays("chain"), c["links"]
    none = pool[links == 0]
    assert len(none) >= 63
    waves = 5
    lone = np.resize(none, (64 * waves, 7)).copy()
    where = [(7 * w + 3) % 64 + 64 * w for w in range(waves)]
    lone[where] = aimed[CC.NAMED["for_ever"]]
    # (rays that pass no medium: their chains do not depend on the index they are sent at)
    by_count = [aimed[CC.NAMED[k]] for k in ("no_link", "one_link", "two_links", "tir", "through", "for_ever")]
    mixed = np.array([by_count[j % 6] for j in range(64 * waves)])
    for rays, name in ((lone, "one long chain per wave"), (mixed, "mixed")):
        want = CC.numpy_chain(_search(pb), rays, mats, 64, 0.0, SEED)
        hits, alb = R.query_chain(pb, rays, 64, 0.0, CC.T_MIN, SEED, want_albedo=True)
        _assert_words(hits, want["hits"], name); _assert_words(alb, want["albedo"], name)
        if rays is lone:
            assert (want["links"][where] == 64).all() and want["links"].sum() == 64 * waves and len(want["live"]) == 65
        else:
            assert (want["links"] == np.array([(0, 1, 2, 3, 4, 64)[j % 6] for j in range(64 * waves)])).all()
            assert all(len(set(w.tolist())) == 6 for w in want["links"].reshape(waves, 64))     # every wave holds the whole mix


# ---------------------------------------------------------------- 4. a lane's second batch, partial waves, no rays
def test_caller_rays_in_the_second_batch():
    """One whole grid of the chain kernel (read from what the library reports after a sizing call) and one more batch of the Cornell box's
    camera rays, repeated: the last batch is second-trip work of the first workgroups and equals the first.  (No media in this scene: a
    record does not depend on the ray's index.)"""
    import torch
    pb, _, _ = _scene("cornell")
    rays = _caller_rays("cornell")
    m = len(rays)
    threads = R.debug_loop_limits()["query_threads"]
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    R.query_chain(pb, np.resize(rays, (cus * 8 * threads + m, 7)), 4, 0.0, CC.T_MIN, SEED, want_albedo=True)      # at least one whole grid
    launch = R.last_query_launch(pb)
    blocks = launch["workgroups"]
    assert launch["threads"] == threads and launch["chunk"] == 0 and launch["chunks"] == 0
    per_trip = -(-blocks * threads // m) * m                     # whole repetitions: record k of the last batch is ray k of the first
    n = per_trip + m
    tiled = np.resize(rays, (n, 7)).copy()
    hits, alb = R.query_chain(pb, tiled, 4, 0.0, CC.T_MIN, SEED, want_albedo=True)
    launch = R.last_query_launch(pb)
    assert (launch["workgroups"], launch["threads"]) == (blocks, threads) and n - m >= blocks * threads, (launch, n)     # a lane took a second trip
    want = _caller_chain("cornell", 4, 0.0)
    _assert_words(hits[:m], want["hits"], "first batch"); _assert_words(alb[:m], want["albedo"], "first batch")
    _assert_words(hits[n - m:], hits[:m], "last batch"); _assert_words(alb[n - m:], alb[:m], "last batch")
    _assert_words(hits, np.resize(hits[:m], hits.shape), "every repetition")
    assert (want["links"] >= 1).any()


@pytest.mark.parametrize("form", ["caller_rays", "camera", "camera_and_albedo"])
def test_the_staged_filter_tree_changes_no_word(form, monkeypatch):
    from test_ray_query_gpu import STAGE_H, STAGE_W, assert_staging_changes_no_word
    pb, cam, _ = _scene("random")
    rays = R.query_camera(pb, cam, STAGE_W, STAGE_H, 0, SEED, want_rays=True)[1].reshape(-1, 7)

    def call():
        if form == "caller_rays":
            return R.query_chain(pb, rays, 4, 1.0, CC.T_MIN, SEED, want_albedo=True)
        albedo = form == "camera_and_albedo"
        out = R.query_camera_chain_guide(pb, cam, STAGE_W, STAGE_H, 4, 1.0, 1, 3, SEED, want_albedo=albedo, want_links=True)
        return tuple(np.asarray(a, np.float64) for a in out)
    assert_staging_changes_no_word(pb, call, monkeypatch)
    assert form != "caller_rays" or (call()[0][:, 15] >= 1.0).any()              # some chain followed a link


def test_one_ray_and_no_rays():
    pb, _, mats = _scene("chain")
    ray = CC.aimed_rays()[CC.NAMED["many_links"]:CC.NAMED["many_links"] + 1]
    want = CC.numpy_chain(_search(pb), ray, mats, 64, 0.0, SEED)
    hits, alb = R.query_chain(pb, ray, 64, 0.0, CC.T_MIN, SEED, want_albedo=True)
    _assert_words(hits, want["hits"], "n = 1"); _assert_words(alb, want["albedo"], "n = 1")
    assert want["links"][0] >= 3
    hits, alb = R.query_chain(pb, np.zeros((0, 7)), 64, 0.0, CC.T_MIN, SEED, want_albedo=True)
    assert hits.shape == (0, 16) and alb.shape == (0, 3)


# ---------------------------------------------------------------- 5. the _device forms
def test_device_forms():
    """Torch tensors on a stream of the caller's: word for word the host forms; nothing behind the last record is touched; albedo and links
    may be left out; a buffer that is too small is an error and writes nothing."""
    import torch
    pb, cam, _ = _scene("chain")
    rays = _caller_rays("chain")
    n, px = len(rays), CC.W * CC.H
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream()
    canary = 12345.678
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(np.array(rays)).to(dev)
        d_hits = torch.full((n + 1, 16), canary, dtype=torch.float64, device=dev)
        d_hits2 = torch.full((n + 1, 16), canary, dtype=torch.float64, device=dev)
        d_alb = torch.full((n + 1, 3), canary, dtype=torch.float64, device=dev)
        R.query_chain_device(pb, n, d_rays, d_hits, 4, 0.0, None, CC.T_MIN, SEED, stream=stream.cuda_stream)
        R.query_chain_device(pb, n, d_rays, d_hits2, 4, 0.0, d_alb, CC.T_MIN, SEED, stream=stream.cuda_stream)
        d_guide = torch.full((px + 1, 16), canary, dtype=torch.float64, device=dev)
        d_guide2 = torch.full((px + 1, 16), canary, dtype=torch.float64, device=dev)
        d_sums = torch.full((px + 1, 3), canary, dtype=torch.float64, device=dev)
        d_links = torch.full((px + 1,), 77, dtype=torch.int32, device=dev)
        R.query_camera_chain_guide_device(pb, cam, CC.W, CC.H, d_guide, 4, 0.0, None, None, 3, 5, SEED, stream=stream.cuda_stream)
        R.query_camera_chain_guide_device(pb, cam, CC.W, CC.H, d_guide2, 4, 0.0, d_sums, d_links, 3, 5, SEED, stream=stream.cuda_stream)
    stream.synchronize()
    want = _caller_chain("chain", 4, 0.0)
    h, h2, a = d_hits.cpu().numpy(), d_hits2.cpu().numpy(), d_alb.cpu().numpy()
    _assert_words(h[:n], want["hits"], "hits"); _assert_words(h2[:n], want["hits"], "hits with albedo"); _assert_words(a[:n], want["albedo"], "albedo")
    assert np.all(h[n] == canary) and np.all(h2[n] == canary) and np.all(a[n] == canary)
    want_guide, want_alb, want_links = CC.numpy_camera_chain_guide([_camera_chain("chain", 3 + s, 4, 0.0) for s in range(5)])
    g, g2, s, l = d_guide.cpu().numpy(), d_guide2.cpu().numpy(), d_sums.cpu().numpy(), d_links.cpu().numpy()
    _assert_words(g[:px], want_guide, "guide"); _assert_words(g2[:px], want_guide, "guide with outputs"); _assert_words(s[:px], want_alb, "sums")
    assert (l[:px] == want_links.astype(np.int32)).all() and l[px] == 77
    assert np.all(g[px] == canary) and np.all(g2[px] == canary) and np.all(s[px] == canary)
    small = torch.full((n, 16), canary, dtype=torch.float64, device=dev)
    with pytest.raises(R.RenderError, match="hit buffer too small"):
        R.query_chain_device(pb, n + 1, d_rays, small, 4, 0.0, None, CC.T_MIN, SEED, stream=stream.cuda_stream)
    with pytest.raises(R.RenderError, match="albedo buffer too small"):
        R.query_chain_device(pb, n, d_rays, small, 4, 0.0, d_alb[:n - 1], CC.T_MIN, SEED, stream=stream.cuda_stream)
    with pytest.raises(R.RenderError, match="guide buffer too small"):
        R.query_camera_chain_guide_device(pb, cam, 2 * CC.W, CC.H, small, 4, 0.0, None, None, 0, 2, SEED, stream=stream.cuda_stream)
    with pytest.raises(R.RenderError, match="links buffer too small"):
        R.query_camera_chain_guide_device(pb, cam, CC.W, CC.H, small, 4, 0.0, None, d_links[:px - 1], 0, 2, SEED, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.all(small.cpu().numpy() == canary)


# ---------------------------------------------------------------- 6. progressive frames
PW, PH, PDEPTH, PSEED, PGUIDE = 40, 24, 8, 0x5EED + 23, 3


def test_progressive_resolves_with_a_chain_guide(pbe):
    """After set_guide_chain(4, 0.0) the denoised resolves equal, byte for byte, format_color of the host filters on the frame's sums with
    the guide and the albedo sums of query_camera_chain_guide; one launch serves all of them; the default setting is set_guide_chain(0, 0)."""
    b, cam, _ = CC.chain_scene(pbe)
    bg = (0.7, 0.8, 1.0)
    k, sigma, sigma_v = 2, R.DENOISE_SIGMA, R.DENOISE_VARIANCE_SIGMA
    guide, alb = R.query_camera_chain_guide(b, cam, PW, PH, 4, 0.0, 0, PGUIDE, PSEED, want_albedo=True)
    first = R.query_camera_guide(b, cam, PW, PH, 0, PGUIDE, PSEED)
    assert CC.differing_words(guide, first) != 0
    with R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED, moments=True, guide_samples=PGUIDE, guide_chain=(4, 0.0)) as frame, \
            R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED, guide_samples=PGUIDE) as plain:
        assert frame.guide_chain_info() == (4, 0.0) and plain.guide_chain_info() == (0, 0.0)
        for _ in range(2):
            frame.add(2)
        plain.add(4)
        ps, pN = plain.sum(), plain.samples
        s, N = frame.sum(), frame.samples
        V = R.moments_variance_host(s, frame.sq_sum(), N, frame.passes)
        assert frame.guide_info() == (PGUIDE, 0) and frame.albedo_info() == (0, 0)
        got = frame.rgb8_denoised(k, sigma)
        assert frame.guide_info() == (PGUIDE, 1) and frame.albedo_info() == (PGUIDE, 1)         # the guide and the sums, one launch
        assert np.array_equal(got.astype(np.uint64), R.format_image(R.denoise_host(s, N, guide, k, sigma, 0), N))
        assert np.array_equal(frame.rgb8_denoised_albedo(16, k, sigma).astype(np.uint64), R.format_image(R.denoise_albedo_host(s, N, alb, PGUIDE, guide, k, sigma, 0), N))
        assert np.array_equal(frame.rgb8_denoised_variance(k, sigma_v).astype(np.uint64), R.format_image(R.denoise_variance_host(s, N, V, guide, k, sigma_v, 0), N))
        assert np.array_equal(frame.rgb8_denoised_frame(k, sigma, albedo_samples=16).astype(np.uint64),
                              R.format_image(R.denoise_frame_host(s, guide, None, N, None, alb, PGUIDE, k, sigma, 0), N))
        assert np.array_equal(frame.rgb8_denoised_frame(k, sigma).astype(np.uint64), R.format_image(R.denoise_frame_host(s, guide, None, N, None, None, 1, k, sigma, 0), N))
        counts = np.full((PH, PW), N, np.uint32)                                                # without a history the blend is the frame with counts
        assert np.array_equal(frame.rgb8_temporal(k, sigma).astype(np.uint64), R.format_image(R.denoise_frame_host(s, guide, counts, 1, None, None, 1, k, sigma, 0), N))
        assert frame.guide_info() == (PGUIDE, 1) and frame.albedo_info() == (PGUIDE, 1)
        # the default setting is set_guide_chain(0, 0): first hits
        base = plain.rgb8_denoised(k, sigma)
        base_alb = plain.rgb8_denoised_albedo(4, k, sigma)
        assert np.array_equal(base.astype(np.uint64), R.format_image(R.denoise_host(plain.sum(), plain.samples, first, k, sigma, 0), plain.samples))
        assert (plain.rgb8_denoised(k, sigma).astype(np.uint64) != R.format_image(R.denoise_host(ps, pN, guide, k, sigma, 0), pN)).any()
        plain.set_guide_chain(0, 0.0)
        assert plain.guide_info() == (PGUIDE, 1)                                                # the value in force: nothing is dropped
        assert np.array_equal(plain.rgb8_denoised(k, sigma), base) and np.array_equal(plain.rgb8_denoised_albedo(4, k, sigma), base_alb)
        assert plain.guide_info() == (PGUIDE, 1) and plain.albedo_info() == (4, 1)
        # switching the chain on drops the guide and the sums, and off again gives the first bytes back
        plain.set_guide_chain(4, 0.0)
        assert plain.albedo_info()[0] == 0
        assert np.array_equal(plain.rgb8_denoised(k, sigma).astype(np.uint64), R.format_image(R.denoise_host(ps, pN, guide, k, sigma, 0), pN)) and plain.guide_info() == (PGUIDE, 2)
        plain.set_guide_chain(0, 0.0)
        assert np.array_equal(plain.rgb8_denoised(k, sigma), base) and np.array_equal(plain.rgb8_denoised_albedo(4, k, sigma), base_alb)
        for bad, word in (((65, 0.0), "max_links"), ((4, -1.0), "max_fuzz"), ((4, float("nan")), "max_fuzz")):
            with pytest.raises(R.RenderError, match=word):
                plain.set_guide_chain(*bad)
        assert plain.guide_chain_info() == (0, 0.0)


def test_set_view_reprojects_with_first_hits_whatever_the_setting(pbe):
    from raytracinginrust_amd.api import Camera
    b, cam, _ = CC.chain_scene(pbe)
    bg = (0.7, 0.8, 1.0)
    cam2 = Camera((5.6, 5.2, -14.0), (5.0, 5.0, 5.0), (0.0, 1.0, 0.0), 40.0, CC.W / CC.H, 0.1, 19.0, 0.0, 1.0)
    out = []
    for chain in (None, (4, 0.0)):
        with R.Progressive(b, cam, bg, PW, PH, PDEPTH, PSEED, guide_samples=PGUIDE, guide_chain=chain) as frame:
            frame.add(4)
            frame.rgb8_denoised(2, R.DENOISE_SIGMA)              # (the chain guide is in place when the view moves)
            frame.set_view(cam2, PSEED + 1)
            out.append(frame.history())
            assert frame.history_info()["pixels"] > 0 and frame.guide_chain_info() == (chain or (0, 0.0))
    assert CC.differing_words(out[0][0], out[1][0]) == 0 and np.array_equal(out[0][1], out[1][1])

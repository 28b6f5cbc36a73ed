"""Progressive frames on the GPU (rt_progressive_*, csrc/rt_resolve.hip): passes of samples that accumulate into a device-resident frame
and the reference's format_color resolved on the device.

What is compared with what:
  * per sample, the passes' samples against the CPU oracle's samples 0..63 under the rules of test_scene_forms_gpu._compare_with_oracle
    (NaN / inf patterns identical, at most 2 samples beyond 1e-9 relative), and against rt_render_samples of the same build BIT FOR BIT —
    the same kernel with the same key (the pass offset is folded into the seed: test_progressive_host.py), so there is nothing to tolerate;
  * per pixel, the accumulated sums against the one-shot sums within the bound that holds for ANY order of adding the same N terms in
    f64 (Higham, Accuracy and Stability of Numerical Algorithms, §4.2): |delta| <= 2 * gamma * sum|x_i|, gamma = (N-1)u / (1 - (N-1)u),
    u = 2^-53 — each of the two sums is within gamma * sum|x_i| of the exact one.  Derived, not measured;
  * the device resolve against the host's rt_format_color, which is its specification: zero mismatches."""
import os
import subprocess

import numpy as np
import pytest

from conftest import build_scene
from oracle import orc
from raytracinginrust_amd import _lib, render as R, scenes
from test_scene_forms_host import cornell_light_tree

pytestmark = pytest.mark.gpu

SAMPLE_RTOL = 1e-9
MAX_BAD = 2
PASSES = (1, 7, 24, 32)
SPP = sum(PASSES)
U = 2.0 ** -53

CASES = {   # name: (W, H, depth, seed) — sizes the oracle finishes in seconds at 64 spp
    "cornell": (40, 40, 20, 0x5EED),          # a list scene
    "random": (48, 27, 8, 11),                # a world that is one BVH
    "teapot": (48, 27, 20, 12),               # a mesh scene that takes the persistent loop
    "final": (32, 32, 20, 13),                # media, textures, moving spheres
    "light_tree": (40, 40, 12, 31),           # F_NESTED (lists inside `lights`)
}


def _make(name, be, earth):
    if name == "light_tree":
        return cornell_light_tree(be, False)
    return build_scene(name, be, earth)


def _words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _sum_bound(samples):
    """2 * gamma_N * sum|x_i| per pixel and channel for the N samples along axis 2, and the mask of pixels whose samples are all finite."""
    n = samples.shape[2]
    gamma = (n - 1) * U / (1.0 - (n - 1) * U)
    finite = np.isfinite(samples).all(axis=(2, 3))
    return 2.0 * gamma * np.abs(np.where(np.isfinite(samples), samples, 0.0)).sum(axis=2), finite


def _assert_sums_agree(a, b, samples, what=""):
    bound, finite = _sum_bound(samples)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.where(finite[..., None], a - b, 0.0))
    print(f"{what}: max |delta| {d.max():.3e}, max delta / bound {np.max(d / np.maximum(bound, 1e-300)):.3f}, pixels with a non-finite sample {int((~finite).sum())}")
    assert np.all(d <= bound), f"{what}: sums differ by more than any summation order allows"
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


def _assert_oracle_rule(gs, rs):
    assert np.array_equal(np.isnan(gs), np.isnan(rs)), "NaN pattern differs"
    assert np.array_equal(np.isinf(gs), np.isinf(rs))
    fin = np.isfinite(rs)
    d = np.abs(np.where(fin, gs, 0.0) - np.where(fin, rs, 0.0))
    bad = (d > SAMPLE_RTOL * (1.0 + np.abs(np.where(fin, rs, 0.0)))).any(axis=-1)
    assert bad.sum() <= MAX_BAD, f"{int(bad.sum())} of {bad.size} samples diverged; first at {np.argwhere(bad)[:3].tolist()}"


_RUNS = {}


def _run(name, pbe, earth, flags=R.RT_F64):
    """The four uneven passes of one scene, with everything the tests below look at (rendered once per module)."""
    key = (name, flags)
    if key in _RUNS:
        return _RUNS[key]
    W, H, depth, seed = CASES[name]
    pb, pcam, pbg = _make(name, pbe, earth)
    one_sum, one_samples = R.render(pb, pcam, pbg, W, H, SPP, depth, seed=seed, flags=flags, want_samples=True)
    r = {"pb": pb, "cam": pcam, "bg": pbg, "one_sum": one_sum, "one_samples": one_samples, "parts": [], "images": [], "sums": [], "stats": [], "loop": []}
    with R.Progressive(pb, pcam, pbg, W, H, depth, seed=seed, flags=flags) as frame:
        assert frame.samples == 0
        for n in PASSES:
            r["parts"].append(frame.add(n, want_samples=True))
            r["stats"].append(R.last_stats(pb)["nonfinite_samples"])
            r["loop"].append(R.last_loop_info(pb))
            r["images"].append(frame.rgb8())
            r["sums"].append((frame.sum(), frame.samples))
        assert frame.samples == SPP
        r["again"] = frame.rgb8()                     # a second resolve with no pass in between
    r["samples"] = np.concatenate(r["parts"], axis=2)
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_passes_are_the_one_shot_frames_samples(name, pbe, obe, earth):
    """Test 4 of the issue: uneven passes (1, 7, 24, 32), concatenated, are the oracle's samples 0..63 and rt_render_samples' bit for bit."""
    W, H, depth, seed = CASES[name]
    r = _run(name, pbe, earth)
    assert [p.shape[2] for p in r["parts"]] == list(PASSES) and r["samples"].shape == (H, W, SPP, 3)
    assert np.array_equal(_words(r["samples"]), _words(r["one_samples"])), "a pass rendered other samples than the one-shot frame holds at those indices"
    ob, ocam, obg = _make(name, obe, earth)
    _, rs, cnt = orc.render(ob, ocam, obg, W, H, SPP, depth, seed=seed, want_samples=True, want_counters=True)
    _assert_oracle_rule(r["samples"], rs)
    assert sum(r["stats"]) == cnt["nonfinite"]                     # rt_last_stats after a pass reports that pass
    assert np.nansum(np.abs(rs)) > 0.0
    if name == "teapot":
        assert all(li["shape"] == "persistent" for li in r["loop"])
    if name == "light_tree":
        assert all(li["feats"] == 639 for li in r["loop"])


@pytest.mark.parametrize("name,flags", [(n, R.RT_F64) for n in CASES] + [("cornell", R.RT_F32), ("random", R.RT_F32)])
def test_accumulated_sums_within_the_any_order_bound(name, flags, pbe, earth):
    """Test 5: read_sum after the passes against the one-shot sum, per channel within 2 * gamma_64 * sum|x_i| (RT_F32 frames too: their
    sums are f64).  The f32 passes' samples are the f32 one-shot frame's bit for bit as well."""
    r = _run(name, pbe, earth, flags)
    assert np.array_equal(_words(r["samples"]), _words(r["one_samples"]))
    total, done = r["sums"][-1]
    assert done == SPP
    _assert_sums_agree(total, r["one_sum"], r["samples"], f"{name} flags={flags}")
    done_so_far = 0
    for (s, d), n in zip(r["sums"], PASSES):                       # and after every pass, against the sum of the samples so far
        done_so_far += n
        assert d == done_so_far
        part = r["samples"][:, :, :done_so_far]
        _assert_sums_agree(s, np.where(np.isfinite(part).all(axis=(2, 3))[..., None], part.sum(axis=2), s), part, f"{name} after {d}")


def test_resolve_equals_format_image_after_every_pass(pbe, earth):
    """Test 6 (a): the device resolve is format_color of the accumulated sums, every pixel and channel; and test 7: the changed-pixel count
    is the count of differing triples between consecutive resolves, W*H at the first, 0 when nothing was added in between."""
    W, H, _, _ = CASES["cornell"]
    r = _run("cornell", pbe, earth)
    prev = None
    for (img, changed), (s, done) in zip(r["images"], r["sums"]):
        assert img.dtype == np.uint8 and img.shape == (H, W, 3)
        assert np.array_equal(img.astype(np.uint64), R.format_image(s, done))
        expect = W * H if prev is None else int((img != prev).any(axis=-1).sum())
        assert changed == expect
        prev = img
    assert r["images"][1][1] > 0                                    # (1 -> 8 samples does move the image: the count is not trivially 0)
    again, changed = r["again"]
    assert changed == 0 and np.array_equal(again, prev)


def _known_answer_sums(n):
    """Sums whose resolve sits on and around every rounding boundary of the cast for n samples, and the special values."""
    k = np.arange(257, dtype=np.float64)
    v = [float(n) * (k / 256.0) ** 2, float(n) * 0.999 ** 2 * np.ones(1)]
    base = np.concatenate(v)
    out = [base]
    up, down = base.copy(), base.copy()
    for _ in range(8):                                              # eight f64 neighbours on each side
        up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
        out += [up.copy(), down.copy()]
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, -1.0, -1e300, 1e300, 1.7976931348623157e308,
                     np.inf, -np.inf, np.nan, -np.nan, float(n), float(n) * 0.5, float(n) * 2.0])
    rng = np.random.default_rng(n % 1000003)
    bits = rng.integers(0, 1 << 64, size=12000, dtype=np.uint64).view(np.float64)                    # any bit pattern: NaN payloads, denormals, both signs
    unit = rng.random(6000) * float(n)                                                               # and the range a real frame lives in
    return np.concatenate(out + [tiny, bits, unit])


@pytest.mark.parametrize("n", [1, 3, 64, 1000, 2 ** 32 - 1])
def test_resolve_known_answers(n, pbe):
    """Test 6 (b): a known-answer frame pushed in with load_sum must resolve to rt_format_color on every value: n * (k/256)^2 for k = 0..256
    with eight f64 neighbours on each side (the rounding boundaries of the cast), 0.999^2 * n and its neighbours, +-0, denormals,
    negatives, 1e300, +-inf, NaN, 12000 random bit patterns — 22 k values for each of five sample counts (1.1e5 in all), in a frame whose
    width and pixel count are not multiples of the kernel's four pixels per lane."""
    vals = _known_answer_sums(n)
    assert len(vals) > 22000
    W = 203
    H = -(-len(vals) // (3 * W))
    while (W * H) % 4 == 0 or W * H * 3 < len(vals):
        H += 1
    frame_vals = np.zeros(W * H * 3)
    frame_vals[:len(vals)] = vals
    frame_vals[len(vals):] = vals[:W * H * 3 - len(vals)]           # (the tail pixels carry boundary values too)
    sums = frame_vals.reshape(H, W, 3)
    b, cam, bg = scenes.cornell_box(pbe)
    with R.Progressive(b, cam, bg, W, H, 4) as frame:
        frame.load(sums, n)
        assert frame.samples == n
        img, changed = frame.rgb8()
        assert np.array_equal(_words(frame.sum()), _words(sums))    # a checkpoint comes back as it went in, NaN payloads included
    want = R.format_image(sums, n)
    assert want.max() <= 255
    mismatches = int((img.astype(np.uint64) != want).sum())
    assert mismatches == 0, f"{mismatches} of {want.size} channels differ from rt_format_color; first at {np.argwhere(img != want)[:3].tolist()}"
    assert changed == W * H
    assert len(np.unique(want)) == 256                              # every output level occurs


def test_resume_from_a_checkpoint_and_reset(pbe, earth):
    """Test 8: read_sum + samples after 32 spp, destroy, a fresh frame, load_sum, 32 more — and reset() then 64 in one pass: the samples
    of an uninterrupted run bit for bit, sums within the any-order bound."""
    W, H, depth, seed = CASES["cornell"]
    r = _run("cornell", pbe, earth)
    pb, cam, bg = r["pb"], r["cam"], r["bg"]
    with R.Progressive(pb, cam, bg, W, H, depth, seed=seed) as frame:
        first = frame.add(32, want_samples=True)
        checkpoint, done = frame.sum(), frame.samples
    assert done == 32
    with R.Progressive(pb, cam, bg, W, H, depth, seed=seed) as frame:
        frame.load(checkpoint, done)
        _, changed = frame.rgb8()
        assert changed == W * H                                     # a loaded frame's first resolve is a first resolve
        second = frame.add(32, want_samples=True)
        assert frame.samples == 64
        resumed = frame.sum()
        both = np.concatenate([first, second], axis=2)
        assert np.array_equal(_words(both), _words(r["one_samples"]))
        _assert_sums_agree(resumed, r["one_sum"], both, "resumed")
        frame.reset()
        assert frame.samples == 0 and not frame.sum().any()
        with pytest.raises(R.RenderError, match="0 samples"):
            frame.rgb8()
        whole = frame.add(64, want_samples=True)
        assert np.array_equal(_words(whole), _words(r["one_samples"]))
        _assert_sums_agree(frame.sum(), r["one_sum"], whole, "after reset")
        _, changed = frame.rgb8()
        assert changed == W * H


def test_nothing_leaks_into_the_one_shot_path(pbe, earth):
    """Test 9: rt_render before, between and after progressive use of the same scene returns the same 64-bit words."""
    W, H, depth, seed = CASES["cornell"]
    pb, cam, bg = scenes.cornell_box(pbe)
    before = R.render(pb, cam, bg, W, H, 16, depth, seed=seed)
    with R.Progressive(pb, cam, bg, W, H, depth, seed=seed) as frame:
        frame.add(5)
        between = R.render(pb, cam, bg, W, H, 16, depth, seed=seed)
        frame.add(11)
        part = frame.sum()
        ms = R.last_kernel_ms(pb)
        assert ms > 0.0
    after = R.render(pb, cam, bg, W, H, 16, depth, seed=seed)
    assert np.array_equal(_words(before), _words(between)) and np.array_equal(_words(before), _words(after))
    _, samples = R.render(pb, cam, bg, W, H, 16, depth, seed=seed, want_samples=True)
    _assert_sums_agree(part, before, samples, "interleaved")


def test_async_passes_and_device_resolve(pbe, earth):
    """Test 10: add_async back to back on one stream, resolve_rgb8_device on that stream, ONE wait at the end."""
    import torch
    W, H, depth, seed = CASES["cornell"]
    r = _run("cornell", pbe, earth)
    stream = torch.cuda.Stream()
    with R.Progressive(r["pb"], r["cam"], r["bg"], W, H, depth, seed=seed) as frame:
        for n in PASSES:
            frame.add_async(n, stream.cuda_stream)
        ptr = frame.rgb8_device(stream.cuda_stream)
        assert ptr != 0 and frame.samples == SPP
        img, changed = frame.rgb8_copy()                            # the one wait
        total = frame.sum()
        ptr2 = frame.rgb8_device(stream.cuda_stream)
        assert ptr2 not in (0, ptr)                                 # resolves alternate between two images
        img2, changed2 = frame.rgb8_copy()
    _assert_sums_agree(total, r["sums"][-1][0], r["samples"], "async against synchronous")
    assert np.array_equal(img.astype(np.uint64), R.format_image(total, SPP)) and changed == W * H
    assert np.array_equal(img2, img) and changed2 == 0


def test_frame_and_scene_lifetimes(pbe):
    """A scene changed after create: the next add is an error until reset; sample-count limits; a frame outlives its scene."""
    W, H = 16, 16
    b, cam, bg = scenes.cornell_box(pbe)
    frame = R.Progressive(b, cam, bg, W, H, 8)
    frame.add(2)
    with pytest.raises(R.RenderError, match="n_samples must be >= 1"):
        frame.add(0)
    nonzero = np.zeros((H, W, 3)); nonzero[3, 4, 1] = 0.25
    with pytest.raises(R.RenderError, match="samples_done = 0"):
        frame.load(nonzero, 0)
    assert frame.samples == 2
    frame.load(nonzero, 2 ** 32 - 2)
    with pytest.raises(R.RenderError, match=r"2\^32 - 1"):
        frame.add(2)
    assert frame.samples == 2 ** 32 - 2                             # nothing was launched
    frame.add(1)                                                    # the last sample index there is
    assert frame.samples == 2 ** 32 - 1
    with pytest.raises(R.RenderError, match=r"2\^32 - 1"):
        frame.add_async(1)
    frame.reset()
    b.Lambertian(b.ConstantTexture((0.1, 0.2, 0.3)))                # any builder call changes the scene
    with pytest.raises(R.RenderError, match="scene changed"):
        frame.add(1)
    frame.reset()
    frame.add(3)
    assert frame.samples == 3
    kept = frame.sum()
    b.close()                                                       # the scene goes first
    with pytest.raises(R.RenderError, match="destroyed"):
        frame.add(1)
    assert np.array_equal(_words(frame.sum()), _words(kept))        # what was rendered can still be read and resolved
    img, changed = frame.rgb8()
    assert changed == W * H and np.array_equal(img.astype(np.uint64), R.format_image(kept, 3))
    frame.close()


def test_render_progressive_generator(pbe):
    W, H, spp, depth = 24, 24, 20, 8
    b, cam, bg = scenes.cornell_box(pbe)
    seen = list(R.render_progressive(b, cam, bg, W, H, spp, depth, passes=3))
    assert [s for s, _, _ in seen] == [7, 14, 20]
    ref = R.format_image(R.render(b, cam, bg, W, H, spp, depth), spp)
    last = seen[-1][1]
    assert last.shape == (H, W, 3) and (last != ref).sum() <= 3 and np.abs(last.astype(int) - ref.astype(int)).max() <= 1      # (two summation orders: quantisation ties)
    assert seen[0][2] == W * H and all(c == int((a != p).any(-1).sum()) for (_, p, _), (_, a, c) in zip(seen, seen[1:]))
    assert [s for s, _, _ in R.render_progressive(b, cam, bg, W, H, 130, depth)] == [64, 128, 130]


def test_rtrender_progressive_writes_the_resolved_image(pbe):
    """Test 11: `rtrender --progressive N` prints the progress on stderr and the PPM of the device-resolved image: byte for byte the P3 text
    of format_image over the sums the same passes accumulate."""
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, spp, depth, n = 48, 27, 8, 20, 3
    run = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth), "--progressive", str(n)],
                         check=True, capture_output=True)
    assert b"\rSamples: 3 / 8" in run.stderr and b"\rSamples: 6 / 8" in run.stderr and b"\rSamples: 8 / 8" in run.stderr and run.stderr.endswith(b"Done.\n")
    pb, cam, bg = scenes.cornell_box(pbe, aspect_ratio=W / H)
    with R.Progressive(pb, cam, bg, W, H, depth) as frame:
        for k in (3, 3, 2):
            frame.add(k)
        img = R.format_image(frame.sum(), frame.samples)
    text = f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in img.reshape(-1, 3))
    assert run.stdout == text.encode()
    one_shot = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth)],
                              check=True, capture_output=True).stdout.split(b"\n")
    got = run.stdout.split(b"\n")
    assert len(got) == len(one_shot) and sum(a != b for a, b in zip(got, one_shot)) <= 3      # the one-shot path's PPM up to quantisation ties

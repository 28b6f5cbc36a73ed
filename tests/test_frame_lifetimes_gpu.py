"""The lifetime rules of a progressive frame (csrc/rt_frames.cpp): what a frame still does once its scene is gone or has changed, what it
refuses and in which words, and that frames created and destroyed next to each other neither share nor keep anything.

A Cornell box at 8 x 8, passes of 2 samples, depth 4, one filter iteration; the plain resolve, the four denoised resolves and the temporal
resolve.  Every refusal here is decided on the host before any launch."""
import numpy as np
import pytest

from raytracinginrust_amd import render as R, scenes

pytestmark = pytest.mark.gpu

W = H = 8
DEPTH, SEED, N, K, ALB = 4, 0xF1A7, 2, 1, 3
SIG, VSIG = R.DENOISE_SIGMA, R.DENOISE_VARIANCE_SIGMA
OTHER_FLAGS, OTHER_ALB = R.RT_DENOISE_SAME_MATERIAL, ALB + 1

GONE = "the scene of this progressive frame has been destroyed"
NO_GUIDE = GONE + " and the frame holds no denoising guide for these flags: the guide is built from the scene (rt_query_camera_device)"
NO_ALBEDO = GONE + " and the frame holds no albedo sums for this albedo_samples: they are built from the scene (rt_query_camera_albedo_device)"
CHANGED = "the scene changed after this progressive frame was created: the frame is forgotten (rt_progressive_reset starts a new one)"

# every resolve of a frame with moments that is not adaptive: name -> call(frame, filter flags, albedo_samples)
RESOLVES = {
    "plain": lambda f, flags, alb: f.rgb8()[0],
    "denoised": lambda f, flags, alb: f.rgb8_denoised(K, SIG, flags),
    "variance": lambda f, flags, alb: f.rgb8_denoised_variance(K, VSIG, flags),
    "albedo": lambda f, flags, alb: f.rgb8_denoised_albedo(alb, K, SIG, flags),
    "frame": lambda f, flags, alb: f.rgb8_denoised_frame(K, VSIG, flags, variance=True, albedo_samples=alb),
    "temporal": lambda f, flags, alb: f.rgb8_temporal(K, SIG, flags),
}
USE_FLAGS = ("denoised", "variance", "albedo", "frame", "temporal")
USE_ALBEDO = ("albedo", "frame")


def _other_view():
    return scenes.Camera((248.0, 288.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.05, 10.0, 0.0, 1.0)


def _frame(b, cam, bg, passes=2, **kw):
    f = R.Progressive(b, cam, bg, W, H, DEPTH, SEED, moments=True, **kw)
    for _ in range(passes):
        f.add(N)
    return f


def _all(f, names=RESOLVES):
    return {name: RESOLVES[name](f, 0, ALB) for name in names}


def _same(got, want):
    assert got.keys() == want.keys()
    for name in want:
        assert np.array_equal(got[name], want[name]), name


def _refused(call, sentence):
    with pytest.raises(R.RenderError) as e:
        call()
    assert str(e.value) == sentence


def _table(f, cam, before, first, guide, albedo):
    """What a frame whose scene is gone or has changed still does and what it refuses: `first` is the whole sentence of a call that needs
    the scene outright, `guide` and `albedo` those of a resolve that would have to build a guide or albedo sums from it."""
    _same(_all(f), before)
    for name in USE_FLAGS:
        _refused(lambda: RESOLVES[name](f, OTHER_FLAGS, ALB), guide)
    for name in USE_ALBEDO:
        _refused(lambda: RESOLVES[name](f, 0, OTHER_ALB), albedo)
    _refused(lambda: f.add(N), first)
    _refused(lambda: f.add_async(N), first)
    _refused(lambda: f.set_view(_other_view(), SEED + 1), first)
    assert f.samples == 2 * N
    _same(_all(f), before)                                      # a refusal leaves what the frame holds as it was


def test_after_the_scene_is_destroyed(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    f = _frame(b, cam, bg)
    try:
        before = _all(f)
        b.close()
        _table(f, cam, before, GONE, NO_GUIDE, NO_ALBEDO)
    finally:
        f.close()


def test_after_the_scene_is_changed(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    f = _frame(b, cam, bg)
    try:
        before = _all(f)
        builds = (f.guide_info()[1], f.albedo_info()[1])
        b.Sphere((100.0, 100.0, 100.0), 10.0, b.Lambertian(b.ConstantTexture((0.1, 0.2, 0.3))))
        _table(f, cam, before, CHANGED, CHANGED, CHANGED)
        assert (f.guide_info()[1], f.albedo_info()[1]) == builds
        f.reset()
        f.add(N); f.add_async(N); f.add(N)
        assert f.samples == 3 * N
        f.reset()
        f.add(N); f.add(N)
        _same(_all(f), before)                                  # (the sphere is in no list: the world renders as it did)
        assert (f.guide_info()[1], f.albedo_info()[1]) == (builds[0] + 1, builds[1] + 1)
        f.set_view(_other_view(), SEED + 1)
        assert f.samples == 0 and f.history_info()["views"] == 1
    finally:
        f.close(); b.close()


def _round(b, cam, bg):
    """create -> moments and adaptive -> two passes -> every resolve once (the temporal one on a frame of its own with a history: an
    adaptive frame has none) -> an adaptive pass and the two resolves that take its counts -> destroy"""
    out = {}
    with _frame(b, cam, bg, adaptive=True) as f:
        out.update(_all(f, ("plain", "denoised", "variance", "albedo", "frame")))
        out["error"] = f.error_map()
        info = f.add_adaptive(N, 1.0 / 1024.0)
        out["listed"] = np.array([info["listed"], info["kernel"]])
        out["counts"] = f.counts()[0]
        out["plain after"] = RESOLVES["plain"](f, 0, ALB)
        out["frame after"] = RESOLVES["frame"](f, 0, ALB)
    with _frame(b, cam, bg) as t:
        t.set_view(_other_view(), SEED + 1)
        out["preview"] = t.rgb8_temporal(0)
        t.add(N)
        out["temporal"] = RESOLVES["temporal"](t, 0, ALB)
        out["history"] = t.history()[1]
    return out


def test_create_and_destroy_rounds(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    try:
        first = _round(b, cam, bg)
        assert first["history"].any() and first["listed"][0] > 0
        for _ in range(2):
            _same(_round(b, cam, bg), first)
    finally:
        b.close()


def test_two_frames_on_one_scene(pbe):
    b, cam, bg = scenes.cornell_box(pbe)
    lone_b, _, _ = scenes.cornell_box(pbe)
    a, f, lone = _frame(b, cam, bg), _frame(b, cam, bg), _frame(lone_b, cam, bg, passes=3)
    try:
        a.close()
        f.add(N)
        assert f.samples == lone.samples == 3 * N
        want = _all(lone)
        _same(_all(f), want)
        b.close()                                               # the scene tells the one frame it still has
        _refused(lambda: f.add(N), GONE)
        _same(_all(f), want)
    finally:
        a.close(); f.close(); lone.close(); lone_b.close()

"""Albedo-demodulated denoising without a GPU (rt_denoise_albedo_host, csrc/rt_albedo_cpu.cpp) and rt_material_info: the specification
(csrc/rt_albedo.h (2): six lines around the unchanged filter) restated in NumPy equals the host twin with 0 differing 64-bit words; known
answers pin what the words mean; every bad argument is an error with a message for all three C forms before a device is looked at; and the
twin runs clean under AddressSanitizer + UBSan as a stand-alone program.  tests/test_denoise_albedo_gpu.py holds the HIP kernels to the twin."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import SceneBuilder, SceneError

import albedo_cases as AC
import denoise_cases as DC
from denoise_cases import INF, differing_words, sigma3


# ---------------------------------------------------------------- 1. the host twin is the specification
@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_restatement(pbe, shape):
    rgb, hits = DC.case(shape)
    for albedo_samples in AC.ALBEDO_SAMPLES:
        alb = AC.albedo_case(shape, albedo_samples)
        for k, sigma, flags in DC.settings_for(shape):
            got = R.denoise_albedo_host(rgb, DC.SAMPLES, alb, albedo_samples, hits, k, sigma, flags)
            want = AC.numpy_denoise_albedo(rgb, DC.SAMPLES, alb, albedo_samples, hits, k, sigma, flags)
            assert differing_words(got, want) == 0, (shape, albedo_samples, k, sigma, flags)
        # the inputs do what they are for
        mean = alb / albedo_samples
        assert (mean == 0.0).any() and ((mean > 0.0) & (mean < AC.EPS)).any() and np.isnan(mean).any()
        if shape[0] * shape[1] >= 40:
            assert (mean == INF).any() and (mean == -INF).any() and (mean[np.isfinite(mean)] >= 1.0).any()
    if shape[0] * shape[1] > 1:
        assert (~np.isfinite(rgb)).sum() >= 3


# ---------------------------------------------------------------- 2. known answers
def test_an_albedo_of_ones_is_the_plain_filter():
    for shape in ((3, 5), (23, 37)):
        rgb, hits = DC.case(shape)
        ones = np.ones(shape + (3,))
        for k, sigma, flags in DC.settings_for(shape)[::5]:
            got = R.denoise_albedo_host(rgb, DC.SAMPLES, ones, 1, hits, k, sigma, flags)
            assert differing_words(got, R.denoise_host(rgb, DC.SAMPLES, hits, k, sigma, flags)) == 0


def test_a_black_channel_stays_black_whatever_its_neighbours_hold():
    H, W = 9, 12
    rs = np.random.RandomState(11)
    rgb = rs.uniform(0.5, 4.0, (H, W, 3)) * 4
    hits = np.zeros((H, W, 16)); hits[..., 0] = 1.0; hits[..., 1] = 1.0; hits[..., 5:8] = (0.0, 0.0, 1.0)
    alb = rs.uniform(0.2, 1.0, (H, W, 3)) * 3
    alb[4, 5, 1] = 0.0; alb[2, 8] = 0.0; alb[0, 0, 2] = 0.0
    out = R.denoise_albedo_host(rgb, 4, alb, 3, hits, 3, (INF, INF, INF), 0)
    assert out[4, 5, 1] == 0.0 and (out[2, 8] == 0.0).all() and out[0, 0, 2] == 0.0
    assert (out[alb != 0.0] > 0.0).all()
    # ... while the plain filter lights it from its neighbours
    assert R.denoise_host(np.where(alb == 0.0, 0.0, rgb), 4, hits, 3, (INF, INF, INF), 0)[4, 5, 1] > 0.0


def test_a_non_finite_albedo_demodulates_nothing():
    rgb, hits = DC.case((3, 5))
    for bad in (np.nan, INF, -INF):
        got = R.denoise_albedo_host(rgb, DC.SAMPLES, np.full((3, 5, 3), bad), 2, hits, 2, DC.SIGMAS[0], 0)
        assert differing_words(got, R.denoise_host(rgb, DC.SAMPLES, hits, 2, DC.SIGMAS[0], 0)) == 0


def test_output_may_alias_the_input(pbe):
    rgb, hits = DC.case((23, 37))
    alb = AC.albedo_case((23, 37), 5)
    before = rgb.copy()
    separate = R.denoise_albedo_host(rgb, DC.SAMPLES, alb, 5, hits, 4, DC.SIGMAS[0], 1)
    assert differing_words(rgb, before) == 0
    in_place = rgb.copy()
    assert pbe.lib.rt_denoise_albedo_host(in_place.ctypes.data, DC.SAMPLES, alb.ctypes.data, 5, hits.ctypes.data, 37, 23, 4, sigma3(DC.SIGMAS[0]), 1,
                                          in_place.ctypes.data) == 0
    assert differing_words(in_place, separate) == 0 and differing_words(in_place, before) != 0


# ---------------------------------------------------------------- 3. arguments
def _err(lib):
    return lib.rt_last_error().decode()


def test_bad_arguments_are_errors_with_a_message(pbe):
    lib = pbe.lib
    rgb = np.ones((3, 4, 3)); alb = np.ones((3, 4, 3)); hits = np.zeros((3, 4, 16)); out = np.full((3, 4, 3), 7.0)
    dev = C.c_void_p(0x1000)                                   # never dereferenced: every call below is refused before a device is looked at
    good = sigma3((1.0, 1.0, 1.0))
    host_forms = (lib.rt_denoise_albedo_host, lib.rt_denoise_albedo)
    # (samples, albedo_samples, W, H, iterations, flags) -> a piece of the message
    for (samples, n_alb, W, H, k, flags), text in (((5, 0, 4, 3, 2, 0), "albedo_samples"), ((5, 1, 4, 3, 2, 2), "flag"), ((0, 1, 4, 3, 2, 0), "samples"),
                                                   ((5, 1, 0, 3, 2, 0), "W and H"), ((5, 1, 4, 3, 9, 0), "iterations")):
        for fn in host_forms:
            assert fn(rgb.ctypes.data, samples, alb.ctypes.data, n_alb, hits.ctypes.data, W, H, k, good, flags, out.ctypes.data) != 0 and text in _err(lib), (fn, text)
        assert lib.rt_denoise_albedo_device(dev, samples, dev, n_alb, dev, W, H, k, good, flags, dev, dev, 1 << 20, None) != 0 and text in _err(lib), text
    for fn in host_forms:
        for hole in (0, 2, 4, 8, 10):                           # rgb_sum, albedo_sum, hits, sigma, rgb_sum_out
            args = [rgb.ctypes.data, 5, alb.ctypes.data, 1, hits.ctypes.data, 4, 3, 2, good, 0, out.ctypes.data]
            args[hole] = None
            assert fn(*args) != 0 and "null argument" in _err(lib), (fn, hole)
    for hole in (0, 2, 4, 8, 10, 11):
        args = [dev, 5, dev, 1, dev, 4, 3, 2, good, 0, dev, dev, 1 << 20, None]
        args[hole] = None
        assert lib.rt_denoise_albedo_device(*args) != 0 and "null argument" in _err(lib), hole
    assert (out == 7.0).all()
    # the workspace: the filter's 128 bytes per pixel and the demodulated frame's 24, refused one byte short before anything else is looked at
    assert lib.rt_denoise_albedo_workspace_bytes(4, 3) == 4 * 3 * 152 and lib.rt_denoise_albedo_workspace_bytes(3840, 2160) == 3840 * 2160 * 152
    assert lib.rt_denoise_albedo_device(dev, 5, dev, 1, dev, 4, 3, 2, good, 0, dev, dev, 4 * 3 * 152 - 1, None) != 0 and "workspace too small" in _err(lib)
    assert lib.rt_denoise_albedo_device(dev, 5, dev, 1, C.c_void_p(0x1008), 4, 3, 2, good, 0, dev, dev, 4 * 3 * 152, None) != 0 and "16-byte aligned" in _err(lib)
    assert lib.rt_denoise_albedo_device(dev, 5, C.c_void_p(0x1004), 1, dev, 4, 3, 2, good, 0, dev, dev, 4 * 3 * 152, None) != 0 and "8-byte aligned" in _err(lib)
    # the existing entry points keep refusing the bit this feature did not become
    assert lib.rt_denoise_host(rgb.ctypes.data, 5, hits.ctypes.data, 4, 3, 2, good, 2, out.ctypes.data) != 0 and "flag" in _err(lib)
    # the progressive call and the queries' own limits
    img = np.zeros(36, np.uint8)
    assert lib.rt_progressive_resolve_denoised_albedo_rgb8(None, 4, 3, good, 0, img.ctypes.data) != 0 and "null argument" in _err(lib)
    with pytest.raises(ValueError):
        R.denoise_albedo_host(np.ones((3, 4, 3)), 1, np.ones((3, 5, 3)), 1, np.zeros((3, 4, 16)))
    with pytest.raises(R.RenderError, match="albedo_samples"):
        R.denoise_albedo_host(np.ones((3, 4, 3)), 1, np.ones((3, 4, 3)), 0, np.zeros((3, 4, 16)))


def test_albedo_query_arguments(pbe):
    """What the albedo queries refuse before a device or the scene is looked at."""
    from raytracinginrust_amd import scenes
    lib = pbe.lib
    b, cam, _ = scenes.cornell_box(pbe)
    dev = C.c_void_p(0x1000)
    out = np.full((6, 6, 3), 7.0)
    ray = np.zeros((1, 7))
    assert lib.rt_query_camera_albedo(b.h, C.byref(cam), 6, 6, 0, 0, 1, 0, out.ctypes.data) != 0 and "n_samples" in _err(lib)
    assert lib.rt_query_camera_albedo(b.h, C.byref(cam), 6, 6, 0xFFFFFFFF, 1, 1, 0, out.ctypes.data) != 0 and "2^32 - 1" in _err(lib)
    assert lib.rt_query_camera_albedo(b.h, C.byref(cam), 6, 6, 0, 1, 1, 1, out.ctypes.data) != 0 and "flags" in _err(lib)
    assert lib.rt_query_camera_albedo(b.h, C.byref(cam), 1, 6, 0, 1, 1, 0, out.ctypes.data) != 0 and "W and H" in _err(lib)
    assert lib.rt_query_camera_albedo(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, None) != 0 and "null argument" in _err(lib)
    assert lib.rt_query_camera_albedo_device(b.h, C.byref(cam), 6, 6, 0, 0, 1, 0, dev, 6 * 6 * 24, None) != 0 and "n_samples" in _err(lib)
    assert lib.rt_query_camera_albedo_device(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, dev, 6 * 6 * 24 - 1, None) != 0 and "too small" in _err(lib)
    assert lib.rt_query_camera_albedo_device(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, C.c_void_p(0x1004), 6 * 6 * 24, None) != 0 and "8-byte aligned" in _err(lib)
    assert lib.rt_query_albedo(b.h, 1, ray.ctypes.data, 1e-5, 0, 1, out.ctypes.data, None) != 0 and "flags" in _err(lib)
    assert lib.rt_query_albedo(b.h, 1, None, 1e-5, 0, 0, out.ctypes.data, None) != 0 and "null argument" in _err(lib)
    assert lib.rt_query_albedo(b.h, 1, ray.ctypes.data, 1e-5, 0, 0, None, None) != 0 and "null argument" in _err(lib)
    assert lib.rt_query_albedo(b.h, 0, ray.ctypes.data, 1e-5, 0, 0, out.ctypes.data, None) == 0          # n = 0: nothing to do, nothing touched
    assert lib.rt_query_albedo_device(b.h, 0, dev, 1e-5, 0, 0, dev, 0, None, 0, None) == 0
    assert lib.rt_query_albedo_device(b.h, 2, dev, 1e-5, 0, 0, dev, 47, None, 0, None) != 0 and "too small" in _err(lib)
    assert lib.rt_query_albedo_device(b.h, 2, dev, 1e-5, 0, 0, dev, 48, dev, 255, None) != 0 and "too small" in _err(lib)
    assert lib.rt_query_albedo_device(b.h, 2, C.c_void_p(0x1008), 1e-5, 0, 0, dev, 48, None, 0, None) != 0 and "16-byte aligned" in _err(lib)
    assert lib.rt_query_albedo_device(b.h, 2, dev, 1e-5, 0, 0, dev, 48, C.c_void_p(0x1008), 256, None) != 0 and "16-byte aligned" in _err(lib)
    assert (out == 7.0).all()


# ---------------------------------------------------------------- 4. rt_material_info
def test_material_info_on_one_material_per_kind(pbe):
    b = SceneBuilder(pbe)
    t0 = b.ConstantTexture((0.1, 0.2, 0.3))
    t1 = b.ConstantTexture((0.9, 0.9, 0.9))
    t2 = b.CheckTexture(t0, t1)
    mats = [("lambertian", b.Lambertian(t2), t2.id, (0.0, 0.0, 0.0)), ("metal", b.Metal((0.8, 0.6, 0.25), 0.3), -1, (0.8, 0.6, 0.25)),
            ("dielectric", b.Dielectric(1.5), -1, (0.0, 0.0, 0.0)), ("diffuse_light", b.DiffuseLight(t1), t1.id, (0.0, 0.0, 0.0)),
            ("isotropic", b.Isotropic(t0), t0.id, (0.0, 0.0, 0.0)),
            ("pbr", b.PBR(t1, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0), t1.id, (0.0, 0.0, 0.0))]
    for kind, h, tex, albedo in mats:
        info = R.material_info(b, h.id)
        assert R.MATERIAL_KINDS[info["kind"]] == kind and info["texture"] == tex and tuple(info["albedo"]) == albedo, (kind, info)
    # the same after the scene has been flattened (the flattened table marks materials whose textures read u, v: not part of the kind)
    b.set_scene(b.Sphere((0.0, 0.0, 0.0), 1.0, mats[0][1]), [])
    R.flatten(b)
    assert R.MATERIAL_KINDS[R.material_info(b, mats[0][1].id)["kind"]] == "lambertian"
    for bad in (-1, len(mats), 1 << 20):
        with pytest.raises(R.RenderError, match="bad material handle"):
            R.material_info(b, bad)
    kt = (C.c_int32 * 2)(); alb = (C.c_double * 3)()
    assert pbe.lib.rt_material_info(None, 0, kt, alb) != 0 and "null argument" in _err(pbe.lib)
    assert pbe.lib.rt_material_info(b.h, 0, None, alb) != 0 and "null argument" in _err(pbe.lib)


def test_albedo_image():
    a = np.array([[[0.0, 4.0, 2.0], [np.nan, -1.0, 8.0]]])
    assert R.albedo_image(a, 4).tolist() == [[[0, 255, 127], [0, 0, 255]]]


# ---------------------------------------------------------------- 5. the host twin under AddressSanitizer + UBSan, stand-alone
def test_host_twin_under_sanitizers(tmp_path):
    """The runtimes are linked statically, so the program needs nothing from its environment (as tests/test_denoise_host.py's)."""
    if os.environ.get("RT_SANITIZER_RUN") == "1":
        return
    exe = str(tmp_path / "denoise_albedo_san")
    csrc = os.path.join(ROOT, "raytracinginrust_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(csrc, "rt_denoise_cpu.cpp"), os.path.join(csrc, "rt_albedo_cpu.cpp"),
                    os.path.join(ROOT, "tests", "denoise_albedo_san_main.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and run.stderr == "", run.stdout + run.stderr

"""The averaged denoising guide without a GPU (rt_guide_from_hits_host, csrc/rt_guide_cpu.cpp): the specification of csrc/rt_guide.h restated
in NumPy (tests/guide_cases.py: a sequential loop over the samples) equals the host twin with 0 differing 64-bit words, a NaN matching any
NaN; one sample gives the record back as values; the record is a drop-in for every `hits` parameter (rt_denoise_host on it equals the NumPy
filter on it); bad arguments are errors; and the twin runs clean under AddressSanitizer + UBSan as a stand-alone program.
tests/test_guide_gpu.py holds the HIP kernel to the same restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracinginrust_amd import render as R

import denoise_cases as DC
import guide_cases as G


# ---------------------------------------------------------------- 1. the host twin is the specification
@pytest.mark.parametrize("n_samples", G.N_SAMPLES)
def test_host_twin_equals_the_numpy_restatement(n_samples):
    hits, labels = G.stack(n_samples)
    got = R.guide_from_hits(hits)
    want = G.numpy_guide(hits)
    assert got.shape == (len(labels), 16)
    assert G.differing_words(got, want) == 0, [labels[k] for k in np.argwhere((got != want).any(axis=-1))[:5, 0]]
    # the stack holds what it is meant to hold
    h = want[:, 15]
    seen = {lab[0] for lab in labels}
    assert {"all", "none"} <= seen and (h == n_samples).any() and (h == 0).any()
    assert (n_samples % 2 != 0) == ("tie" not in seen)
    if n_samples % 2 == 0:
        tie = np.array([lab[0] == "tie" for lab in labels])
        assert (h[tie] * 2 == n_samples).all() and (want[tie, 0] == 1.0).all()                 # a tie counts as hit
    if n_samples >= 3:
        below = np.array([lab[0] == "below_half" for lab in labels])
        assert (want[below, 0] == 0.0).all() and (h[below] >= 1).all()                          # a miss to the filter that still carries what was seen
        assert (want[below & np.isfinite(want[:, 1]), 1] > 0.0).all()
    if n_samples >= 2:
        full = np.array([lab[0] == "all" for lab in labels])
        for mat, word, value in (("mixed_materials", 11, -1.0), ("medium", 11, -1.0), ("mixed_objects", 12, -1.0), ("same", 11, 3.0), ("same", 12, 7.0),
                                 ("medium", 12, 5.0), ("last_differs", 11, -1.0)):
            rows = full & np.array([lab[1] == mat for lab in labels])
            assert rows.any() and (want[rows, word] == value).all(), (mat, word)
        assert (want[full, 0] == 1.0).all()                                                     # mixed materials are never a miss
    assert np.isnan(want[:, 1]).any() and np.isinf(want[:, 2]).any() and np.isnan(want[:, 3]).any()
    assert (want[:, 9:11] == 0.0).all() and (want[:, 13:15] == -1.0).all()
    assert not np.signbit(want[np.isfinite(want).all(axis=-1)][:, 1:9]).all()


def test_image_shaped_stacks():
    hits, _ = G.stack(5)
    hits = hits[:, :6 * 9].reshape(5, 6, 9, 16)
    got = R.guide_from_hits(hits)
    assert got.shape == (6, 9, 16) and G.differing_words(got, G.numpy_guide(hits)) == 0
    with pytest.raises(ValueError):
        R.guide_from_hits(np.zeros((5, 6, 9, 15)))


def test_one_sample_gives_the_record_back_as_values():
    hits, labels = G.stack(1)
    got = R.guide_from_hits(hits)
    words = list(G.WORDS_OF_ONE_SAMPLE)
    a, b = got[:, words], hits[0][:, words]
    assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()
    neg = np.signbit(hits[0][:, 2:8]) & (hits[0][:, 2:8] == 0.0)
    assert neg.any() and not np.signbit(got[:, 2:8][neg]).any()                                # -0.0 comes back as +0.0
    assert (got[:, 15] == hits[0][:, 0]).all()


# ---------------------------------------------------------------- 2. the record is a drop-in for `hits`
@pytest.mark.parametrize("n_samples", (2, 5))
def test_the_filter_takes_the_record_unchanged(n_samples):
    H, W = 7, 9
    hits, _ = G.stack(n_samples, seed=3, hostile=False, repeat=3)
    assert hits.shape[1] >= H * W
    guide = R.guide_from_hits(hits[:, :H * W].reshape(n_samples, H, W, 16))
    assert (guide[..., 0] == 0.0).any() and (guide[..., 0] == 1.0).any() and (guide[..., 11] == -1.0).any() and (guide[..., 11] >= 0.0).any()
    rgb = np.random.RandomState(n_samples).uniform(0.0, 4.0, (H, W, 3)) * DC.SAMPLES
    for flags in (0, R.RT_DENOISE_SAME_MATERIAL):
        for k, sigma in ((2, DC.SIGMAS[0]), (3, DC.SIGMAS[1])):
            got = R.denoise_host(rgb, DC.SAMPLES, guide, k, sigma, flags)
            assert DC.differing_words(got, DC.numpy_denoise(rgb, DC.SAMPLES, guide, k, sigma, flags)) == 0, (flags, k)
    a = R.denoise_host(rgb, DC.SAMPLES, guide, 2, DC.SIGMAS[1], 0)
    b = R.denoise_host(rgb, DC.SAMPLES, guide, 2, DC.SIGMAS[1], R.RT_DENOISE_SAME_MATERIAL)
    assert DC.differing_words(a, b) != 0                                                        # the key is read from the record


# ---------------------------------------------------------------- 3. arguments
def test_bad_arguments_are_errors_with_a_message(pbe):
    lib = pbe.lib
    hits = np.zeros((2, 3, 16)); out = np.full((3, 16), 7.0)
    assert lib.rt_guide_from_hits_host(None, 2, 3, out.ctypes.data) != 0 and "null argument" in lib.rt_last_error().decode()
    assert lib.rt_guide_from_hits_host(hits.ctypes.data, 2, 3, None) != 0 and "null argument" in lib.rt_last_error().decode()
    assert lib.rt_guide_from_hits_host(hits.ctypes.data, 0, 3, out.ctypes.data) != 0 and "n_samples" in lib.rt_last_error().decode()
    assert (out == 7.0).all()
    assert lib.rt_guide_from_hits_host(hits.ctypes.data, 2, 0, out.ctypes.data) == 0 and (out == 7.0).all()         # no pixels: nothing to do
    assert lib.rt_progressive_set_guide_samples(None, 4) != 0 and "null argument" in lib.rt_last_error().decode()
    n, builds = C.c_uint32(), C.c_uint64()
    assert lib.rt_progressive_guide_info(None, C.byref(n), C.byref(builds)) != 0 and "null argument" in lib.rt_last_error().decode()


def test_guide_query_arguments(pbe):
    """What the guide queries refuse before a device or the scene is looked at."""
    from raytracinginrust_amd import scenes
    lib = pbe.lib
    b, cam, _ = scenes.cornell_box(pbe)
    dev = C.c_void_p(0x1000)
    out = np.full((6, 6, 16), 7.0)

    def err():
        return lib.rt_last_error().decode()
    assert lib.rt_query_camera_guide(b.h, C.byref(cam), 6, 6, 0, 0, 1, 0, out.ctypes.data, None) != 0 and "n_samples" in err()
    assert lib.rt_query_camera_guide(b.h, C.byref(cam), 6, 6, 0xFFFFFFFF, 1, 1, 0, out.ctypes.data, None) != 0 and "2^32 - 1" in err()
    assert lib.rt_query_camera_guide(b.h, C.byref(cam), 6, 6, 0, 1, 1, 1, out.ctypes.data, None) != 0 and "flags" in err()
    assert lib.rt_query_camera_guide(b.h, C.byref(cam), 1, 6, 0, 1, 1, 0, out.ctypes.data, None) != 0 and "W and H" in err()
    assert lib.rt_query_camera_guide(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, None, None) != 0 and "null argument" in err()
    assert lib.rt_query_camera_guide(None, C.byref(cam), 6, 6, 0, 1, 1, 0, out.ctypes.data, None) != 0 and "null argument" in err()
    assert lib.rt_query_camera_guide_device(b.h, C.byref(cam), 6, 6, 0, 0, 1, 0, dev, 6 * 6 * 128, None, 0, None) != 0 and "n_samples" in err()
    assert lib.rt_query_camera_guide_device(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, dev, 6 * 6 * 128 - 1, None, 0, None) != 0 and "guide buffer too small" in err()
    assert lib.rt_query_camera_guide_device(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, dev, 6 * 6 * 128, dev, 6 * 6 * 24 - 1, None) != 0 and "albedo buffer too small" in err()
    assert lib.rt_query_camera_guide_device(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, C.c_void_p(0x1008), 6 * 6 * 128, None, 0, None) != 0 and "16-byte aligned" in err()
    assert lib.rt_query_camera_guide_device(b.h, C.byref(cam), 6, 6, 0, 1, 1, 0, dev, 6 * 6 * 128, C.c_void_p(0x1004), 6 * 6 * 24, None) != 0 and "8-byte aligned" in err()
    assert (out == 7.0).all()


def test_guide_fields():
    assert R.GUIDE_FIELDS["hits"] == slice(15, 16) and all(R.GUIDE_FIELDS[k] == v for k, v in R.HIT_FIELDS.items())


# ---------------------------------------------------------------- 4. the host twin under AddressSanitizer + UBSan, stand-alone
def test_host_twin_under_sanitizers(tmp_path):
    """The runtimes are linked statically, so the program needs nothing from its environment (as tests/test_denoise_albedo_host.py's)."""
    if os.environ.get("RT_SANITIZER_RUN") == "1":
        return
    exe = str(tmp_path / "guide_san")
    csrc = os.path.join(ROOT, "raytracinginrust_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(csrc, "rt_guide_cpu.cpp"), os.path.join(ROOT, "tests", "guide_san_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and run.stderr == "", run.stdout + run.stderr

"""Temporal variance through the C++ mirror (include/raytracinginrust.hpp) and the command line (host/rtrender):
tests/reproject_var_mirror_main.cpp is compiled against the library and checks itself — rtr::temporal_blend_variance and
rtr::reproject_variance(host) against known answers without a device; on the GPU rtr::reproject_variance against its host form and a
progressive frame with moments through set_view — and `rtrender --progressive N --orbit FRAMES,DEGREES --denoise K --denoise-variance S`
writes what the Python path yields."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R


def _mirror(tmp_path, mode):
    if os.environ.get("RT_SANITIZER_RUN") == "1":      # (the library in use is the sanitizer build: a program without its runtime cannot load it)
        return
    exe = str(tmp_path / "reproject_var_mirror")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "reproject_var_mirror_main.cpp"), "-o", exe,
                    "-L" + libdir, "-lrt_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    run = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok " + mode), run.stdout + run.stderr


def test_cpp_reproject_variance_and_blend_on_the_host(tmp_path):
    _mirror(tmp_path, "host")


@pytest.mark.gpu
def test_cpp_reproject_variance_and_progressive_set_view(tmp_path):
    _mirror(tmp_path, "gpu")


def test_rtrender_orbit_variance_arguments(tmp_path):
    if os.environ.get("RT_SANITIZER_RUN") == "1":      # (rtrender loads the library beside it, not the sanitizer build)
        return
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    allowed = b"--orbit goes with --progressive N, and of the other options only with --denoise K, --denoise-guide N and --denoise-variance SIGMA_V [--denoise-albedo N]\n"
    for args, word in ((["--progressive", "4", "--orbit", "3,2", "--denoise-variance", "3"], b"--denoise-variance goes with --progressive N and --denoise K"),
                       (["--progressive", "4", "--orbit", "3,2", "--denoise", "2", "--denoise-albedo", "4"], allowed),      # albedo without the variance stop
                       (["--progressive", "4", "--orbit", "3,2", "--denoise", "2", "--denoise-variance", "3", "--adaptive", "--until-error", "0.01"], allowed)):
        bad = subprocess.run([exe] + args, capture_output=True, timeout=120)
        assert bad.returncode == 2 and word in bad.stderr, (args, bad.stderr)
    # what this message no longer covers: the variance stop, with and without albedo, gets past the argument checks (without a
    # device the run then ends with another status and another message; with one it writes three tiny views)
    for extra in ([], ["--denoise-albedo", "4"]):
        run = subprocess.run([exe, "--scene", "cornell", "--width", "16", "--height", "16", "--depth", "2", "--progressive", "4", "--orbit", "3,2", "--out", str(tmp_path / "o"),
                              "--denoise", "2", "--denoise-variance", "3"] + extra,
                             capture_output=True, timeout=120)
        assert b"--orbit goes with" not in run.stderr and b"--denoise-variance goes with" not in run.stderr, run.stderr
    help_text = subprocess.run([exe, "--help"], capture_output=True, timeout=120).stdout + subprocess.run([exe, "--help"], capture_output=True, timeout=120).stderr
    assert b"with --denoise-variance SIGMA_V [--denoise-albedo N] as well through its variance stop" in help_text


@pytest.mark.gpu
def test_rtrender_orbit_variance_writes_what_the_python_path_yields(pbe, tmp_path):
    from raytracinginrust_amd import scenes
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, n, depth, frames, degrees, cap, seed = 48, 27, 4, 8, 3, 3.0, 24, 77
    b, cam, bg = scenes.cornell_box(pbe, aspect_ratio=W / H)

    def ppm(img):
        return (f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in np.asarray(img).reshape(-1, 3))).encode()

    def view(f):
        # rtrender's rotation of lookfrom about the axis vup through lookat, operation for operation (as tests/test_reproject_mirrors.py)
        import math
        a = degrees * float(f) * 3.141592653589793 / 180.0
        ca, sa = math.cos(a), math.sin(a)
        al = math.sqrt(cam.vup[0] * cam.vup[0] + cam.vup[1] * cam.vup[1] + cam.vup[2] * cam.vup[2])
        k = [cam.vup[e] / al for e in range(3)]
        r = [cam.lookfrom[e] - cam.lookat[e] for e in range(3)]
        kr = k[0] * r[0] + k[1] * r[1] + k[2] * r[2]
        x = [k[1] * r[2] - k[2] * r[1], k[2] * r[0] - k[0] * r[2], k[0] * r[1] - k[1] * r[0]]
        c = type(cam).from_buffer_copy(cam)
        c.lookfrom[:] = [cam.lookat[e] + r[e] * ca + x[e] * sa + k[e] * kr * (1.0 - ca) for e in range(3)]
        return c
    for extra, albedo in (([], 0), (["--denoise-albedo", "4"], 4)):
        out = str(tmp_path / f"orbit{albedo}")
        run = subprocess.run([exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--depth", str(depth), "--seed", str(seed), "--progressive", str(n),
                              "--orbit", f"{frames},{degrees}", "--history", str(cap), "--out", out, "--denoise", "2", "--denoise-variance", "3"] + extra,
                             capture_output=True, timeout=120)
        assert run.returncode == 0 and run.stdout == b"", run.stderr
        sigma = (3.0,) + tuple(R.DENOISE_SIGMA[1:])
        with R.Progressive(b, cam, bg, W, H, depth, seed, moments=True) as frame:
            for f in range(frames):
                if f:
                    frame.set_view(view(f), seed + f, cap)
                frame.add((n + 1) // 2); frame.add(n // 2)                   # (rtrender's two passes per view under the variance stop)
                want = frame.rgb8_temporal(2, sigma, variance=True, albedo_samples=albedo)
                with open(f"{out}_{f:03d}.ppm", "rb") as fh:
                    assert fh.read() == ppm(want), (albedo, f)
            # (so that the later files were resolves WITH a history of known variance)
            hv, hn = frame.history_variance(), frame.history()[1]
            assert ((hn > 0) & np.isfinite(hv).all(axis=-1)).sum() > W * H // 10

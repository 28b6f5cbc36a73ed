"""The averaged guide through the C++ mirror (include/raytracinginrust.hpp) and the command line (host/rtrender): tests/guide_mirror_main.cpp
is compiled against the library and checks itself — rtr::guide_from_hits against known answers without a device; on the GPU
rtr::query_camera_guide against rtr::guide_from_hits of the stacked records and a progressive frame with set_guide_samples — and
`rtrender --denoise-guide N` / `--aov coverage FILE` write what the Python path yields."""
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
    exe = str(tmp_path / "guide_mirror")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "guide_mirror_main.cpp"), "-o", exe,
                    "-L" + libdir, "-lrt_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    run = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok " + mode), run.stdout + run.stderr


def test_cpp_guide_from_hits(tmp_path):
    _mirror(tmp_path, "host")


@pytest.mark.gpu
def test_cpp_query_camera_guide_and_progressive(tmp_path):
    _mirror(tmp_path, "gpu")


@pytest.mark.gpu
def test_rtrender_guide_options_write_what_the_python_path_yields(pbe):
    from raytracinginrust_amd import scenes
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, spp, depth, n = 48, 27, 8, 8, 4
    common = [exe, "--scene", "random", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth)]
    b, cam, bg = scenes.random_scene(pbe, aspect_ratio=W / H)

    def ppm(img):
        return (f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in np.asarray(img).reshape(-1, 3))).encode()
    guide = R.query_camera_guide(b, cam, W, H, 0, n)
    assert ((guide[..., 15] > 0) & (guide[..., 15] < n)).any()
    for extra, g, count in ((["--denoise-guide", str(n)], guide, n), ([], R.query_camera_guide(b, cam, W, H, 0, 1), 1)):
        run = subprocess.run(common + ["--aov", "coverage", "-"] + extra, check=True, capture_output=True, timeout=120)
        grey = np.clip(g[..., 15] / count * 255.999, 0.0, 255.0).astype(np.uint8)             # hits / N * 255.999, truncated
        assert run.stdout == ppm(np.repeat(grey[..., None], 3, axis=-1)), extra
    frame_sum = R.render(b, cam, bg, W, H, spp, depth)
    run = subprocess.run(common + ["--denoise", "2", "--denoise-guide", str(n)], check=True, capture_output=True, timeout=120)
    assert run.stdout == ppm(R.format_image(R.denoise(frame_sum, spp, guide, 2, R.DENOISE_SIGMA, 0), spp))
    run = subprocess.run(common + ["--denoise", "2", "--denoise-guide", str(n), "--denoise-albedo", "4"], check=True, capture_output=True, timeout=120)
    alb = R.query_camera_albedo(b, cam, W, H, 0, 4)
    assert run.stdout == ppm(R.format_image(R.denoise_albedo(frame_sum, spp, alb, 4, guide, 2, R.DENOISE_SIGMA, 0), spp))
    prog = subprocess.run(common + ["--progressive", "4", "--denoise", "2", "--denoise-guide", str(n)], check=True, capture_output=True, timeout=120)
    with R.Progressive(b, cam, bg, W, H, depth, guide_samples=n) as frame:
        frame.add(4); frame.add(4)
        assert prog.stdout == ppm(frame.rgb8_denoised(2, R.DENOISE_SIGMA))
    bad = subprocess.run(common + ["--denoise-guide", "4"], capture_output=True, timeout=120)
    assert bad.returncode == 2 and b"--denoise-guide goes with" in bad.stderr
    bad = subprocess.run(common + ["--denoise", "2", "--denoise-guide", "0"], capture_output=True, timeout=120)
    assert bad.returncode == 2

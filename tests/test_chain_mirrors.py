"""Specular-chain guides through the C++ mirror (include/raytracinginrust.hpp) and the command line (host/rtrender):
tests/chain_mirror_main.cpp is compiled against the library and checks itself — rt_chain_step_host against a known answer without a device;
on the GPU rtr::query_chain against the chain composed link by link, rtr::query_camera_chain_guide and a progressive frame with
set_guide_chain — and `rtrender --denoise K --denoise-chain LINKS` / `--aov links FILE` write what the Python path yields."""
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
    exe = str(tmp_path / "chain_mirror")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "chain_mirror_main.cpp"), "-o", exe,
                    "-L" + libdir, "-lrt_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=300)
    run = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("ok " + mode), run.stdout + run.stderr


def test_cpp_chain_step_host(tmp_path):
    _mirror(tmp_path, "host")


def test_rtrender_refuses_chain_options_it_cannot_use():
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    for args, text in ((["--denoise-chain", "4"], b"--denoise-chain goes with"), (["--denoise", "2", "--denoise-chain", "65"], b"--denoise-chain needs"),
                       (["--denoise", "2", "--denoise-chain", "4,-1"], b"--denoise-chain needs"), (["--aov", "links", "-"], b"--aov links goes with")):
        bad = subprocess.run([exe, "--scene", "random", "--width", "16", "--height", "9"] + args, capture_output=True, timeout=120)
        assert bad.returncode == 2 and text in bad.stderr, (args, bad.stderr)


@pytest.mark.gpu
def test_cpp_query_chain_and_progressive(tmp_path):
    _mirror(tmp_path, "gpu")


@pytest.mark.gpu
def test_rtrender_chain_options_write_what_the_python_path_yields(pbe):
    from raytracinginrust_amd import scenes
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "host", "rtrender")
    assert os.path.exists(exe), "host/rtrender missing: run make -C raytracinginrust_amd/csrc"
    W, H, spp, depth, n, L = 48, 27, 8, 8, 2, 4
    common = [exe, "--scene", "random", "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth)]
    b, cam, bg = scenes.random_scene(pbe, aspect_ratio=W / H)

    def ppm(img):
        return (f"P3\n{W} {H}\n255\n" + "".join(f"{p[0]} {p[1]} {p[2]}\n" for p in np.asarray(img).reshape(-1, 3))).encode()
    guide1, alb1, links1 = R.query_camera_chain_guide(b, cam, W, H, L, 0.0, 0, 1, want_albedo=True, want_links=True)
    guide, alb, links = R.query_camera_chain_guide(b, cam, W, H, L, 0.5, 0, n, want_albedo=True, want_links=True)
    assert (links1 > 0).any() and (links > links1).any()
    for extra, l, count in ((["--denoise-chain", f"{L}"], links1, 1), (["--denoise-chain", f"{L},0.5", "--denoise-guide", str(n)], links, n)):
        run = subprocess.run(common + ["--aov", "links", "-"] + extra, check=True, capture_output=True, timeout=120)
        grey = np.clip(l.astype(np.float64) / (float(count) * float(L)) * 255.999, 0.0, 255.0).astype(np.uint8)
        assert run.stdout == ppm(np.repeat(grey[..., None], 3, axis=-1)), extra
    frame_sum = R.render(b, cam, bg, W, H, spp, depth)
    run = subprocess.run(common + ["--denoise", "2", "--denoise-chain", str(L)], check=True, capture_output=True, timeout=120)
    assert run.stdout == ppm(R.format_image(R.denoise(frame_sum, spp, guide1, 2, R.DENOISE_SIGMA, 0), spp))
    assert run.stdout != ppm(R.format_image(R.denoise(frame_sum, spp, R.query_camera(b, cam, W, H, 0), 2, R.DENOISE_SIGMA, 0), spp))
    run = subprocess.run(common + ["--denoise", "2", "--denoise-chain", f"{L},0.5", "--denoise-guide", str(n), "--denoise-albedo", "4"], check=True, capture_output=True, timeout=120)
    assert run.stdout == ppm(R.format_image(R.denoise_albedo(frame_sum, spp, alb, n, guide, 2, R.DENOISE_SIGMA, 0), spp))
    prog = subprocess.run(common + ["--progressive", "4", "--denoise", "2", "--denoise-chain", str(L)], check=True, capture_output=True, timeout=120)
    with R.Progressive(b, cam, bg, W, H, depth, guide_chain=(L, 0.0)) as frame:
        frame.add(4); frame.add(4)
        assert prog.stdout == ppm(frame.rgb8_denoised(2, R.DENOISE_SIGMA))
        assert prog.stdout == ppm(R.format_image(R.denoise_host(frame.sum(), frame.samples, guide1, 2, R.DENOISE_SIGMA, 0), frame.samples))

"""Denoiser timing and error table.  Part 1: kernel times of the pack kernel and of every iteration of rt_denoise_device (K = 5)
at 800 x 800 and 3840 x 2160 — HIP events between the launches (rt_debug_denoise_ms), warm, best of REPS; once as shipped (steps 1 and 2
from LDS tiles) and once with RT_DENOISE_NO_LDS=1 (every step straight from global memory: the A/B behind that choice) — beside the traffic floor of
each launch (pack: 152 B in, 96 B out per pixel; an iteration: 96 B in, 32 B out, the last one 24 B out) as achieved bytes/s.  The frames are
synthetic (a smooth colour field plus noise over a guide of a few planes): the kernels' time depends on the frame's size and, through the
skipped taps, on how many neighbours share a key, not on what the scene is.  Part 2: the clipped mean squared error against a converged
frame (tests/denoise_cases.py clipped_mse) of raw and denoised frames at 16 and 64 samples per pixel for K = 1 .. 5 on the four preview
scenes at reduced size, with the Python defaults' sigmas: what render.DENOISE_ITERATIONS is chosen from — the plain filter and, beside it,
the albedo-demodulated one (rt_denoise_albedo, albedo of ALBEDO_SAMPLES samples).  Part 3: the albedo query's kernel time
(rt_query_camera_albedo_device, rt_last_query_ms) at 1, 16 and 64 samples per pixel on the Cornell box at 800 x 800 and the random spheres
at 1200 x 675, beside the time of a path-tracing pass of the same number of samples from the same run, and the two element-wise kernels of
rt_denoise_albedo_device (rt_debug_albedo_modulate_ms) at 800 x 800 and 3840 x 2160 beside the pack kernel.
Part 4, `variance`: the variance-guided filter (rt_denoise_variance*) — its kernels' times beside the plain filter's from the same
run, as shipped and with RT_DENOISE_NO_LDS=1, and the variance kernel's; the whole denoised resolves of a progressive frame of C2's view
beside one 64-sample pass; and the error table above with columns for the variance-guided filter, moments from 4 passes, plus the
three-texture scene of §15.
Part 5, `guide`: the averaged guide (rt_query_camera_guide*) — the error rows of parts 2 and of tools/denoise_frame_probe.py's
random spheres with a line per row for a guide of GUIDE_SAMPLES samples beside sample 0's; the 40 x 40 thin-lens scene of
tests/guide_cases.py on three seeds; and the kernel time of rt_query_camera_guide_device without and with its albedo output at 1, 16 and 64
samples beside rt_query_camera_albedo_device and, for one sample, rt_query_camera_device, from the same run.
usage: python tools/denoise_probe.py [timing] [errors] > profiles/denoise.log
       python tools/denoise_probe.py guide > profiles/denoise_guide.log      (guide-cost: the kernel times alone)
       python tools/denoise_probe.py albedo errors > profiles/denoise_albedo.log
       python tools/denoise_probe.py variance > profiles/denoise_variance.log"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib, scenes  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5
K = 5
HBM_ACHIEVABLE = 6.3e12
ALBEDO_SAMPLES = 16


def synthetic(W, H, dev):
    """A frame of sums (16 samples) and hit records on the device: three planes side by side, ~10 % misses along the top, noisy colours."""
    g = torch.Generator(device=dev); g.manual_seed(1)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    rgb = torch.stack([0.5 + 0.4 * torch.sin(x / 97.0), 0.5 + 0.4 * torch.cos(y / 61.0), 0.3 + 0.2 * torch.sin((x + y) / 131.0)], dim=2)
    rgb = (rgb + 0.3 * torch.rand((H, W, 3), generator=g, device=dev, dtype=torch.float64)) * 16.0
    hits = torch.zeros((H, W, 16), device=dev, dtype=torch.float64)
    third = (x * 3.0 / W).floor()
    hits[..., 0] = 1.0
    hits[..., 1] = 5.0 + 0.01 * y
    hits[..., 2] = x / W * 10.0; hits[..., 3] = y / H * 10.0; hits[..., 4] = third
    hits[..., 5] = torch.where(third == 1.0, 0.6, 0.0); hits[..., 7] = torch.where(third == 1.0, 0.8, 1.0)
    hits[..., 11] = third
    miss = y < H * 0.1
    hits[miss] = 0.0
    hits[..., 11:15] = torch.where(miss[..., None], -1.0, hits[..., 11:15])
    return rgb.contiguous(), hits.contiguous()


def timing():
    for no_lds in (False, True):
        if no_lds:
            os.environ["RT_DENOISE_NO_LDS"] = "1"
        else:
            os.environ.pop("RT_DENOISE_NO_LDS", None)
        print("# ---- " + ("RT_DENOISE_NO_LDS=1: every iteration reads its taps from global memory" if no_lds else "as shipped: steps 1 and 2 from LDS tiles"))
        _timing()
    os.environ.pop("RT_DENOISE_NO_LDS", None)


def _timing():
    lib = _lib.load().lib
    dev = torch.device("cuda", torch.cuda.current_device())
    sigma = (C.c_double * 3)(*R.DENOISE_SIGMA)
    print(f"# denoiser kernel times, K = {K}, sigma = {R.DENOISE_SIGMA}, flags 0; HIP events, warm, best of {REPS}")
    print("# frame  kernel  ms  floor bytes  achieved TB/s  share of the 6.3 TB/s achievable HBM rate")
    for W, H in ((800, 800), (3840, 2160)):
        rgb, hits = synthetic(W, H, dev)
        out = torch.empty_like(rgb)
        need = R.denoise_workspace_bytes(W, H)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        best = np.full(K + 1, 1e30)
        for _ in range(REPS):
            ms = (C.c_float * (K + 1))()
            rc = lib.rt_debug_denoise_ms(C.c_void_p(rgb.data_ptr()), 16, C.c_void_p(hits.data_ptr()), W, H, K, sigma, 0, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(ws.data_ptr()), need, ms)
            if rc != 0:
                raise RuntimeError(lib.rt_last_error().decode())
            best = np.minimum(best, np.array(ms[:]))
        n = W * H
        floors = [n * (152 + 96)] + [n * (96 + 32)] * (K - 1) + [n * (96 + 24)]
        for k in range(K + 1):
            name = "pack" if k == 0 else f"iteration {k - 1} (step {1 << (k - 1)})"
            rate = floors[k] / (best[k] * 1e-3)
            print(f"{W}x{H}  {name}  {best[k]:.4f}  {floors[k]}  {rate / 1e12:.3f}  {rate / HBM_ACHIEVABLE:.2f}", flush=True)
        print(f"{W}x{H}  all {K + 1} launches  {best.sum():.4f} ms; working set of an iteration {n * 96 / 1e6:.0f} MB read + {n * 32 / 1e6:.0f} MB written", flush=True)
        del rgb, hits, out, ws


def errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    from denoise_cases import clipped_mse
    be = _lib.load()
    earth = scenes.load_earthmap()
    depth, truth_spp = 20, 4096
    print(f"# clipped MSE against {truth_spp} spp (seed 99), depth {depth}, sigma = {R.DENOISE_SIGMA}, flags 0: raw, then K = 1 .. 5 (ratio to raw);")
    print(f"# 'plain' rt_denoise, 'demod' rt_denoise_albedo with the albedo of samples 0 .. {ALBEDO_SAMPLES - 1} of the noisy frame's seed")
    for name, (W, H) in (("cornell", (100, 100)), ("random", (160, 90)), ("final", (100, 100)), ("teapot", (160, 90))):
        b, cam, bg = build_scene(name, be, earth)
        truth = R.render(b, cam, bg, W, H, truth_spp, depth, 99)
        hits = R.query_camera(b, cam, W, H, 0, 7)
        alb = R.query_camera_albedo(b, cam, W, H, 0, ALBEDO_SAMPLES, 7)
        for spp in (16, 64):
            noisy = R.render(b, cam, bg, W, H, spp, depth, 7)
            raw = clipped_mse(noisy, spp, truth, truth_spp)
            row, row_demod = [], []
            for k in range(1, 6):
                e = clipped_mse(R.denoise(noisy, spp, hits, k, R.DENOISE_SIGMA, 0), spp, truth, truth_spp)
                row.append(f"{e:.5f} ({e / raw:.2f})")
                e = clipped_mse(R.denoise_albedo(noisy, spp, alb, ALBEDO_SAMPLES, hits, k, R.DENOISE_SIGMA, 0), spp, truth, truth_spp)
                row_demod.append(f"{e:.5f} ({e / raw:.2f})")
            print(f"{name} {W}x{H} {spp} spp  raw {raw:.5f}  plain  " + "  ".join(row), flush=True)
            print(f"{name} {W}x{H} {spp} spp  raw {raw:.5f}  demod  " + "  ".join(row_demod), flush=True)


def albedo():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    be = _lib.load()
    lib = be.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"# rt_query_camera_albedo_device: kernel ms (rt_last_query_ms), warm, best of {REPS}; beside it a path-tracing pass of the same number of")
    print("# samples per pixel of the same view (rt_progressive_add, rt_last_kernel_ms), depth 50, from the same run")
    print("# scene frame  n_samples  albedo ms  Mrays/s  pass ms  albedo / pass")
    for name, (W, H) in (("cornell", (800, 800)), ("random", (1200, 675))):
        b, cam, bg = build_scene(name, be, None)
        d_alb = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
        for n in (1, 16, 64):
            best = 1e30
            for rep in range(REPS + 1):                           # the first run warms up (upload, code object)
                R.query_camera_albedo_device(b, cam, W, H, d_alb, 0, n, 7)
                ms = R.last_query_ms(b)
                if rep:
                    best = min(best, ms)
            best_pass = 1e30
            with R.Progressive(b, cam, bg, W, H, 50, 7) as frame:
                for rep in range(REPS + 1):
                    frame.add(n)
                    if rep:
                        best_pass = min(best_pass, R.last_kernel_ms(b))
            print(f"{name} {W}x{H}  {n}  {best:.4f}  {W * H * n / best / 1e3:.0f}  {best_pass:.4f}  {best / best_pass:.3f}", flush=True)
        del d_alb
    print(f"# the two element-wise kernels of rt_denoise_albedo_device (rt_debug_albedo_modulate_ms), HIP events, warm, best of {REPS}; floors: demodulate")
    print("# 48 B in + 24 B out per pixel, remodulate 48 B in + 24 B out; the pack kernel of the same frame (152 B in, 96 B out) beside them")
    print("# frame  kernel  ms  floor bytes  achieved TB/s")
    sigma = (C.c_double * 3)(*R.DENOISE_SIGMA)
    for W, H in ((800, 800), (3840, 2160)):
        rgb, hits = synthetic(W, H, dev)
        alb = (torch.rand((H, W, 3), device=dev, dtype=torch.float64) * ALBEDO_SAMPLES).contiguous()
        x = torch.empty_like(rgb)
        need = R.denoise_workspace_bytes(W, H)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        best = np.full(2, 1e30); best_pack = 1e30
        for _ in range(REPS):
            ms = (C.c_float * 2)()
            if lib.rt_debug_albedo_modulate_ms(C.c_void_p(rgb.data_ptr()), C.c_void_p(alb.data_ptr()), ALBEDO_SAMPLES, C.c_void_p(x.data_ptr()), W * H * 3, ms) != 0:
                raise RuntimeError(lib.rt_last_error().decode())
            best = np.minimum(best, np.array(ms[:]))
            pk = (C.c_float * 2)()
            if lib.rt_debug_denoise_ms(C.c_void_p(rgb.data_ptr()), 16, C.c_void_p(hits.data_ptr()), W, H, 1, sigma, 0, C.c_void_p(x.data_ptr()), C.c_void_p(ws.data_ptr()), need, pk) != 0:
                raise RuntimeError(lib.rt_last_error().decode())
            best_pack = min(best_pack, pk[0])
        n = W * H
        for kname, ms, floor in (("demodulate", best[0], n * 72), ("remodulate", best[1], n * 72), ("pack", best_pack, n * 248)):
            print(f"{W}x{H}  {kname}  {ms:.4f}  {floor}  {floor / (ms * 1e-3) / 1e12:.3f}", flush=True)
        del rgb, hits, alb, x, ws


VARIANCE_SIGMA_VS = (2.0, 3.0, 4.0)


def _variance_timing():
    lib = _lib.load().lib
    dev = torch.device("cuda", torch.cuda.current_device())
    sigma = (C.c_double * 3)(*R.DENOISE_VARIANCE_SIGMA)
    print(f"# variance-guided denoiser kernel times, K = {K}, sigma = {R.DENOISE_VARIANCE_SIGMA}, flags 0; HIP events, warm, best of {REPS}")
    print("# frame  kernel  ms  floor bytes  achieved TB/s  share of the 6.3 TB/s achievable HBM rate")
    for W, H in ((800, 800), (3840, 2160)):
        rgb, hits = synthetic(W, H, dev)
        # a variance on the scale of the synthetic noise: 0.3 * uniform per sample mean has variance 0.0075 per channel
        var = (0.0075 * (0.5 + torch.rand((H, W, 3), device=dev, dtype=torch.float64))).contiguous()
        sq = (rgb * rgb / 16.0 + 16.0 * 3.0 * var).contiguous()
        out = torch.empty_like(rgb)
        need = R.denoise_variance_workspace_bytes(W, H)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        best = np.full(K + 2, 1e30)
        for _ in range(REPS):
            ms = (C.c_float * (K + 2))()
            rc = lib.rt_debug_denoise_variance_ms(C.c_void_p(rgb.data_ptr()), 16, C.c_void_p(var.data_ptr()), C.c_void_p(hits.data_ptr()), W, H, K, sigma, 0,
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), need, ms)
            if rc != 0:
                raise RuntimeError(lib.rt_last_error().decode())
            best = np.minimum(best, np.array(ms[:]))
        n = W * H
        floors = [n * (152 + 24 + 96)] + [n * (32 + 16 + 32)] + [n * (96 + 32)] * (K - 1) + [n * (96 + 24)]
        for k in range(K + 2):
            name = "guide pack + colour pack" if k == 0 else "prefilter of v" if k == 1 else f"iteration {k - 2} (step {1 << (k - 2)})"
            rate = floors[k] / (best[k] * 1e-3)
            print(f"{W}x{H}  {name}  {best[k]:.4f}  {floors[k]}  {rate / 1e12:.3f}  {rate / HBM_ACHIEVABLE:.2f}", flush=True)
        print(f"{W}x{H}  all {K + 3} launches  {best.sum():.4f} ms", flush=True)
        # the variance kernel: 48 B in, 24 B out per pixel
        v_out = torch.empty_like(rgb)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        best_v = 1e30
        for rep in range(REPS + 1):
            ev[0].record()
            R.moments_variance_device(rgb, sq, 16, 4, W, H, v_out, stream=torch.cuda.current_stream().cuda_stream)
            ev[1].record(); ev[1].synchronize()
            if rep:
                best_v = min(best_v, ev[0].elapsed_time(ev[1]))
        print(f"{W}x{H}  moments variance  {best_v:.4f}  {n * 72}  {n * 72 / (best_v * 1e-3) / 1e12:.3f}  {n * 72 / (best_v * 1e-3) / HBM_ACHIEVABLE:.2f}", flush=True)
        del rgb, hits, var, sq, out, ws, v_out


def _variance_resolve():
    import time
    from raytracinginrust_amd import workloads
    be = _lib.load()
    w = workloads.WORKLOADS["C2"]
    b, cam, bg = workloads.build(w, be, None)
    print(f"# a progressive frame of C2's view ({w.scene}, {w.W}x{w.H}, depth {w.max_depth}) with moments, two passes of 64 samples: host time of each resolve call")
    print(f"# (it ends with the copy of the image to the host), warm, best of {REPS}; the pass: rt_last_kernel_ms of a 64-sample pass plus its merge, host time")
    with R.Progressive(b, cam, bg, w.W, w.H, w.max_depth, 7, moments=True) as frame:
        best_pass = 1e30
        for _ in range(3):
            t0 = time.perf_counter(); frame.add(64); best_pass = min(best_pass, (time.perf_counter() - t0) * 1e3)
        print(f"pass of 64 samples (kernel {R.last_kernel_ms(b):.3f} ms)  {best_pass:.3f} ms")
        for name, fn in (("rgb8", lambda: frame.rgb8()), ("rgb8_denoised K = 2", lambda: frame.rgb8_denoised()), ("rgb8_denoised_variance K = 2", lambda: frame.rgb8_denoised_variance())):
            best = 1e30
            for rep in range(REPS + 1):
                t0 = time.perf_counter(); fn(); dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    best = min(best, dt)
            print(f"{name}  {best:.3f} ms  ({best / best_pass:.3f} of the pass)", flush=True)


def _variance_errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    from denoise_cases import clipped_mse
    from test_denoise_albedo_gpu import textured_scene
    be = _lib.load()
    earth = scenes.load_earthmap()
    depth, truth_spp, n_passes = 20, 4096, 4
    print(f"# clipped MSE against {truth_spp} spp (seed 99), depth {depth}, flags 0: raw, then K = 1 .. 5 (ratio to raw); the noisy frame is a progressive")
    print(f"# frame of {n_passes} equal passes (seed 7) with moments; 'plain' rt_denoise with sigma = {R.DENOISE_SIGMA}; 'var s' rt_denoise_variance with sigma_v = s and")
    print(f"# sigma_n, sigma_p = {R.DENOISE_VARIANCE_SIGMA[1:]}; the default sigma_v is {R.DENOISE_VARIANCE_SIGMA[0]:g}")
    cases = [(name, size, lambda name=name: build_scene(name, be, earth)) for name, size in (("cornell", (100, 100)), ("random", (160, 90)), ("final", (100, 100)), ("teapot", (160, 90)))]
    cases.append(("textured", (100, 100), lambda: textured_scene(be)))
    for name, (W, H), make in cases:
        b, cam, bg = make()
        truth = R.render(b, cam, bg, W, H, truth_spp, depth, 99)
        hits = R.query_camera(b, cam, W, H, 0, 7)
        for spp in (16, 64):
            with R.Progressive(b, cam, bg, W, H, depth, 7, moments=True) as frame:
                for _ in range(n_passes):
                    frame.add(spp // n_passes)
                noisy, var = frame.sum(), frame.variance()
            raw = clipped_mse(noisy, spp, truth, truth_spp)
            rows = {"plain": []}
            for k in range(1, 6):
                e = clipped_mse(R.denoise(noisy, spp, hits, k, R.DENOISE_SIGMA, 0), spp, truth, truth_spp)
                rows["plain"].append(f"{e:.5f} ({e / raw:.2f})")
                for sv in VARIANCE_SIGMA_VS:
                    e = clipped_mse(R.denoise_variance(noisy, spp, var, hits, k, (sv,) + tuple(R.DENOISE_VARIANCE_SIGMA[1:]), 0), spp, truth, truth_spp)
                    rows.setdefault(f"var {sv:g}", []).append(f"{e:.5f} ({e / raw:.2f})")
            for label, row in rows.items():
                print(f"{name} {W}x{H} {spp} spp  raw {raw:.5f}  {label}  " + "  ".join(row), flush=True)


def variance():
    for no_lds in (False, True):
        if no_lds:
            os.environ["RT_DENOISE_NO_LDS"] = "1"
        else:
            os.environ.pop("RT_DENOISE_NO_LDS", None)
        print("# ---- " + ("RT_DENOISE_NO_LDS=1: every iteration reads its taps from global memory" if no_lds else "as shipped: steps 1 and 2 from LDS tiles"))
        _timing()
        _variance_timing()
    os.environ.pop("RT_DENOISE_NO_LDS", None)
    _variance_resolve()
    _variance_errors()


GUIDE_SAMPLES = 16


def _guide_errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    from denoise_cases import clipped_mse
    be = _lib.load()
    earth = scenes.load_earthmap()
    depth, truth_spp = 20, 4096
    print(f"# clipped MSE against {truth_spp} spp (seed 99), depth {depth}, sigma = {R.DENOISE_SIGMA}, flags 0: raw, then K = 1 .. 5 (ratio to raw); part 2's rows,")
    print(f"# each with the guide of sample 0 (rt_query_camera) and with the averaged guide of samples 0 .. {GUIDE_SAMPLES - 1} (rt_query_camera_guide); the albedo")
    print(f"# of samples 0 .. {ALBEDO_SAMPLES - 1} comes from the same launch as the averaged guide")
    for name, (W, H) in (("cornell", (100, 100)), ("random", (160, 90)), ("final", (100, 100)), ("teapot", (160, 90))):
        b, cam, bg = build_scene(name, be, earth)
        truth = R.render(b, cam, bg, W, H, truth_spp, depth, 99)
        hits = R.query_camera(b, cam, W, H, 0, 7)
        guide, alb = R.query_camera_guide(b, cam, W, H, 0, GUIDE_SAMPLES, 7, want_albedo=True)
        cov = guide[..., 15]
        print(f"# {name} {W}x{H}: {int(((cov > 0) & (cov < GUIDE_SAMPLES)).sum())} pixels partly covered, {int(((guide[..., 11] == -1.0) & (cov >= 2) & (hits[..., 11] != -1.0)).sum())} "
              f"with mixed materials, {int((guide[..., 0] != hits[..., 0]).sum())} whose hit flag differs from sample 0's")
        for spp in (16, 64):
            noisy = R.render(b, cam, bg, W, H, spp, depth, 7)
            raw = clipped_mse(noisy, spp, truth, truth_spp)
            for label, fn in (("plain", lambda g, k: R.denoise(noisy, spp, g, k, R.DENOISE_SIGMA, 0)),
                              ("demod", lambda g, k: R.denoise_albedo(noisy, spp, alb, ALBEDO_SAMPLES, g, k, R.DENOISE_SIGMA, 0))):
                for gname, g in (("guide = sample 0", hits), (f"guide = {GUIDE_SAMPLES} samples", guide)):
                    row = []
                    for k in range(1, 6):
                        e = clipped_mse(fn(g, k), spp, truth, truth_spp)
                        row.append(f"{e:.5f} ({e / raw:.2f})")
                    print(f"{name} {W}x{H} {spp} spp  raw {raw:.5f}  {label}  {gname}  " + "  ".join(row), flush=True)


def _guide_frame_errors():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    be = _lib.load()
    W = H = 40
    truth_spp, depth = 2048, 20

    def mse(rgb_sum, n):
        mean = rgb_sum / (n if np.isscalar(n) else np.maximum(n, 1).astype(np.float64)[..., None])
        return float(np.mean((np.clip(mean, 0.0, 1.0) - np.clip(truth / truth_spp, 0.0, 1.0)) ** 2))
    print(f"# tools/denoise_frame_probe.py's random-spheres rows ({W}x{H}, depth {depth}, seed 7, truth {truth_spp} spp of seed 99, render.py's sigmas, albedo of 16")
    print("# samples), ratio to raw: uniform 4 x 4: albedo only / variance only / variance with albedo; adaptive: colour stop / variance stop / variance with albedo")
    b, cam, bg = build_scene("random", be, None)
    truth = R.render(b, cam, bg, W, H, truth_spp, depth, 99)
    hits = R.query_camera(b, cam, W, H, 0, 7)
    guide, alb = R.query_camera_guide(b, cam, W, H, 0, GUIDE_SAMPLES, 7, want_albedo=True)
    with R.Progressive(b, cam, bg, W, H, depth, 7, moments=True) as frame:
        for _ in range(4):
            frame.add(4)
        S, N, V = frame.sum(), frame.samples, frame.variance()
    raw = mse(S, N)
    for gname, g in (("guide = sample 0", hits), (f"guide = {GUIDE_SAMPLES} samples", guide)):
        for k in range(1, 6):
            a = mse(R.denoise_albedo(S, N, alb, 16, g, k, R.DENOISE_SIGMA), N)
            v = mse(R.denoise_variance(S, N, V, g, k, R.DENOISE_VARIANCE_SIGMA), N)
            both = mse(R.denoise_frame(S, g, None, N, V, alb, 16, k, R.DENOISE_VARIANCE_SIGMA), N)
            print(f"random  uniform 4 x 4  {gname}  raw {raw:.6f}  K = {k}  {a / raw:.3f}  {v / raw:.3f}  {both / raw:.3f}", flush=True)
    with R.Progressive(b, cam, bg, W, H, depth, 7, adaptive=True) as frame:
        while frame.add_adaptive(4, 1.0 / 64.0, 64)["listed"]:
            pass
        S, (n, _), V = frame.sum(), frame.counts(), frame.variance_counts()
    raw = mse(S, n)
    for gname, g in (("guide = sample 0", hits), (f"guide = {GUIDE_SAMPLES} samples", guide)):
        for k in range(1, 6):
            c = mse(R.denoise_frame(S, g, n, 1, None, None, 1, k, R.DENOISE_SIGMA), n)
            v = mse(R.denoise_frame(S, g, n, 1, V, None, 1, k, R.DENOISE_VARIANCE_SIGMA), n)
            both = mse(R.denoise_frame(S, g, n, 1, V, alb, 16, k, R.DENOISE_VARIANCE_SIGMA), n)
            print(f"random  adaptive tau 1/64 (mean {n.mean():.1f}, {n.min()} .. {n.max()} samples)  {gname}  raw {raw:.6f}  K = {k}  {c / raw:.3f}  {v / raw:.3f}  {both / raw:.3f}", flush=True)


def _guide_lens_scene():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import guide_cases as G
    from denoise_cases import clipped_mse
    b, cam, bg = G.lens_quality_scene(_lib.load())
    W, H = G.Q_W, G.Q_H
    print(f"# the thin-lens scene of tests/guide_cases.py, {W}x{H}, {G.Q_SPP} spp against {G.Q_TRUTH_SPP} spp of another seed, depth {G.Q_DEPTH}, K = {G.Q_ITERATIONS}, sigma = {G.Q_SIGMA},")
    print(f"# albedo of {G.Q_ALBEDO_SAMPLES} samples: clipped MSE raw / demodulated filter with sample 0's guide / with the guide of {G.Q_GUIDE_SAMPLES} samples, and the ratio of the last two")
    for seed, truth_seed in G.Q_SEEDS:
        noisy = R.render(b, cam, bg, W, H, G.Q_SPP, G.Q_DEPTH, seed)
        truth = R.render(b, cam, bg, W, H, G.Q_TRUTH_SPP, G.Q_DEPTH, truth_seed)
        hits = R.query_camera(b, cam, W, H, 0, seed)
        guide, alb = R.query_camera_guide(b, cam, W, H, 0, G.Q_GUIDE_SAMPLES, seed, want_albedo=True)
        raw = clipped_mse(noisy, G.Q_SPP, truth, G.Q_TRUTH_SPP)
        e0 = clipped_mse(R.denoise_albedo(noisy, G.Q_SPP, alb, G.Q_ALBEDO_SAMPLES, hits, G.Q_ITERATIONS, G.Q_SIGMA, 0), G.Q_SPP, truth, G.Q_TRUTH_SPP)
        e16 = clipped_mse(R.denoise_albedo(noisy, G.Q_SPP, alb, G.Q_ALBEDO_SAMPLES, guide, G.Q_ITERATIONS, G.Q_SIGMA, 0), G.Q_SPP, truth, G.Q_TRUTH_SPP)
        print(f"lens scene  seed {seed}  raw {raw:.6f}  sample 0 {e0:.6f} ({e0 / raw:.3f})  {G.Q_GUIDE_SAMPLES} samples {e16:.6f} ({e16 / raw:.3f})  ratio {e16 / e0:.3f}", flush=True)


def _guide_cost():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    be = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"# rt_query_camera_guide_device without and with its albedo output, rt_query_camera_albedo_device and (one sample) rt_query_camera_device: kernel ms")
    print(f"# (rt_last_query_ms: HIP events around the launch), warm, best of {REPS}, all from this run; Mrays/s = W H n_samples / ms; 'two launches' = guide + albedo query")
    print("# scene frame  n_samples  guide ms (Mrays/s)  guide+albedo ms (Mrays/s)  albedo query ms (Mrays/s)  two launches ms  fused / two launches  camera query ms")
    for name, (W, H) in (("cornell", (800, 800)), ("random", (1200, 675)), ("teapot", (1200, 675))):
        b, cam, bg = build_scene(name, be, None)
        d_guide = torch.empty((H, W, 16), dtype=torch.float64, device=dev)
        d_alb = torch.empty((H, W, 3), dtype=torch.float64, device=dev)

        def best_of(call):
            best = 1e30
            for rep in range(REPS + 1):                           # the first run warms up (upload, code object)
                call()
                ms = R.last_query_ms(b)
                if rep:
                    best = min(best, ms)
            return best
        for n in (1, 16, 64):
            g = best_of(lambda: R.query_camera_guide_device(b, cam, W, H, d_guide, None, 0, n, 7))
            ga = best_of(lambda: R.query_camera_guide_device(b, cam, W, H, d_guide, d_alb, 0, n, 7))
            a = best_of(lambda: R.query_camera_albedo_device(b, cam, W, H, d_alb, 0, n, 7))
            q = best_of(lambda: R.query_camera_device(b, cam, W, H, d_guide, 0, 7)) if n == 1 else None
            rate = lambda ms: W * H * n / ms / 1e3
            print(f"{name} {W}x{H}  {n}  {g:.4f} ({rate(g):.0f})  {ga:.4f} ({rate(ga):.0f})  {a:.4f} ({rate(a):.0f})  {g + a:.4f}  {ga / (g + a):.3f}  "
                  + (f"{q:.4f}" if q is not None else "-"), flush=True)
        del d_guide, d_alb


def guide():
    _guide_cost()
    _guide_lens_scene()
    _guide_frame_errors()
    _guide_errors()


if __name__ == "__main__":
    what = sys.argv[1:] or ["timing", "errors"]
    if "timing" in what:
        timing()
    if "albedo" in what:
        albedo()
    if "variance" in what:
        variance()
    if "errors" in what:
        errors()
    if "guide" in what:
        guide()
    if "guide-cost" in what:
        _guide_cost()

"""Radiance-query throughput on the BASELINE views (C1-C4): rt_query_radiance_device's kernel time (rt_last_query_ms, HIP events) for the
camera rays of sample 0 of every pixel (rt_query_camera's rays_out), SPP samples per ray at the workload's depth, beside the kernel time of a
frame of the same size, SPP samples per pixel and depth (rt_last_kernel_ms of rt_render: the same number of paths in the frame kernels) —
and the same query with the static dealing's chunks at 64 and at 1024 paths instead of 256 (RT_RADIANCE_CHUNK), which shows its tail.
Best of REPS launches each, after one warm-up.  usage: python tools/radiance_probe.py [C1 C2 ...] > profiles/radiance_queries.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib, scenes, workloads  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5
SPP = 64


def best_radiance_ms(b, n, d_rays, d_sum, depth, bg):
    best = 1e30
    for rep in range(REPS + 1):                                 # the first launch is the warm-up
        R.query_radiance_device(b, n, d_rays, d_sum, SPP, depth, bg)
        ms = R.last_query_ms(b)                                 # (waits for the kernel)
        if rep:
            best = min(best, ms)
    return best


def main(keys):
    be = _lib.load()
    earth = None
    print(f"# {SPP} samples per ray / pixel.  workload  paths  frame ms  Mpaths/s | query (chunks of 256) ms  Mpaths/s  query/frame | chunks of 64 ms | chunks of 1024 ms")
    for key in keys:
        w = workloads.WORKLOADS[key]
        if w.scene == "final" and earth is None:
            earth = scenes.load_earthmap()
        b, cam, bg = workloads.build(w, be, earth)
        n = w.W * w.H
        frame = 1e30
        for rep in range(REPS + 1):
            R.render(b, cam, bg, w.W, w.H, SPP, w.max_depth)
            if rep:
                frame = min(frame, R.last_kernel_ms(b))
        _, rays = R.query_camera(b, cam, w.W, w.H, 0, want_rays=True)
        d_rays = torch.from_numpy(rays.reshape(n, 7)).cuda()
        d_sum = torch.zeros((n, 3), dtype=torch.float64, device=d_rays.device)
        ms = {}
        for chunk in (256, 64, 1024):
            os.environ["RT_RADIANCE_CHUNK"] = str(chunk)
            ms[chunk] = best_radiance_ms(b, n, d_rays, d_sum, w.max_depth, bg)
        os.environ.pop("RT_RADIANCE_CHUNK", None)
        mp = lambda t: n * SPP / t / 1e3      # noqa: E731
        print(f"{key} {w.scene} {w.W}x{w.H} depth {w.max_depth}  {n * SPP}  {frame:.3f}  {mp(frame):.0f} | {ms[256]:.3f}  {mp(ms[256]):.0f}  {ms[256] / frame:.2f}x | "
              f"{ms[64]:.3f} | {ms[1024]:.3f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["C1", "C2", "C3", "C4"])

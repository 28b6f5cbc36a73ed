"""Ray-query throughput on the BASELINE views (C1-C4): rt_query_camera's kernel time (rt_last_query_ms) with the LDS node cache and
with it switched off (RT_NODE_CACHE_MAX=0: every filter node comes from global memory), beside the kernel time of a frame of one sample
and depth 1 on the same view (rt_last_kernel_ms of rt_render(spp = 1, max_depth = 1): the same primary search plus shading and
regeneration).  Best of REPS launches each, after one warm-up.  usage: python tools/query_probe.py [C1 C2 ...] > profiles/ray_queries.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib, scenes, workloads  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5


def best_query_ms(b, cam, W, H):
    R.query_camera(b, cam, W, H)
    best = 1e30
    for _ in range(REPS):
        R.query_camera(b, cam, W, H)
        best = min(best, R.last_query_ms(b))
    return best


def main(keys):
    be = _lib.load()
    earth = None
    print("# workload  rays  frame(spp=1,depth=1) ms  Mrays/s | query staged ms  Mrays/s | query unstaged ms  Mrays/s | nodes staged / in the scene")
    for key in keys:
        w = workloads.WORKLOADS[key]
        if w.scene == "final" and earth is None:
            earth = scenes.load_earthmap()
        b, cam, bg = workloads.build(w, be, earth)
        n = w.W * w.H
        R.render(b, cam, bg, w.W, w.H, 1, 1)
        frame = 1e30
        for _ in range(REPS):
            R.render(b, cam, bg, w.W, w.H, 1, 1)
            frame = min(frame, R.last_kernel_ms(b))
        info = R.last_launch_info(b)
        os.environ.pop("RT_NODE_CACHE_MAX", None)
        staged = best_query_ms(b, cam, w.W, w.H)
        os.environ["RT_NODE_CACHE_MAX"] = "0"
        unstaged = best_query_ms(b, cam, w.W, w.H)
        os.environ.pop("RT_NODE_CACHE_MAX", None)
        mr = lambda ms: n / ms / 1e3      # noqa: E731
        print(f"{key} {w.scene} {w.W}x{w.H}  {n}  {frame:.4f}  {mr(frame):.0f} | {staged:.4f}  {mr(staged):.0f} | {unstaged:.4f}  {mr(unstaged):.0f} | "
              f"frame kernel staged {info['bvh_nodes_in_lds']} / {info['bvh_nodes']}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["C1", "C2", "C3", "C4"])

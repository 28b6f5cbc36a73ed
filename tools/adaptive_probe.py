"""Adaptive frames: timing and error tables.  Part 1 (rate): the pixel-list kernel with the FULL list (rt_render_pixels_device,
every pixel listed, counts 0) against the frames' own kernel (a plain progressive pass) on the same view, one pass of n_b = 64 samples per
pixel: kernel ms between HIP events (rt_last_query_ms / rt_last_kernel_ms), warm, best of REPS, as Msamples/s, and their ratio — the active
share below which a list pass beats a full pass.  Views: the Cornell box at 800 x 800, depth 50 (workload C2's view), the teapot room
(a mesh) and the random spheres (one BVH) at 400 x 400.  Part 2 (kernels): the element-wise kernels of csrc/rt_adaptive.hip at 800 x 800
and 3840 x 2160 on synthetic frames — select + compaction (four launches), list merge over the full and over every other pixel,
error with counts (map + statistics), resolve with counts — beside rt_moments.hip's merge and error map from the same run; HIP events, warm,
best of REPS.  Part 3 (error): the Cornell box at 200 x 200, depth 50, seed 7, tau = 1/256, passes of 16: an adaptive frame run to its stop
or to 4096 samples per pixel, with spread 0 and 1, against a uniform frame with moments stopped by the same tau: total samples, kernel
time, and the RMS error of sqrt(mean) held to [0, 0.999] (display units) against 4096 samples of seed 99.
usage: python tools/adaptive_probe.py [rate] [kernels] [error] > profiles/adaptive.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5


def _scene(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    return build_scene(name, _lib.load(), None)


def _best_ms(launch):
    """Best of REPS of one launch between two HIP events on the current stream, after one warm run."""
    launch()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); launch(); b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def rate():
    n_b = 64
    print(f"# one pass of {n_b} samples per pixel over every pixel: the pixel-list kernel (full list) against the frames' kernel; kernel ms (HIP events), warm, best of {REPS}")
    print("# view  frames' kernel ms  Msamples/s  list kernel ms  Msamples/s  list / frames rate (the break-even active share)")
    for name, W, H, depth in (("cornell", 800, 800, 50), ("teapot", 400, 400, 50), ("random", 400, 400, 50)):
        b, cam, bg = _scene(name)
        n_px = W * H
        best = [1e30, 1e30]
        d_out = torch.zeros(n_px * 3, dtype=torch.float64, device="cuda")
        d_list = torch.arange(n_px, dtype=torch.int32, device="cuda")
        with R.Progressive(b, cam, bg, W, H, depth, 7) as frame:
            for rep in range(REPS + 1):
                frame.reset()
                frame.add(n_b)
                ms_frame = R.last_kernel_ms(b)
                R.render_pixels_device(b, cam, bg, W, H, n_b, depth, d_list, n_px, d_out, None, seed=7)
                torch.cuda.synchronize()
                ms_list = R.last_query_ms(b)
                if rep:
                    best = [min(best[0], ms_frame), min(best[1], ms_list)]
        msamples = n_px * n_b / 1e6
        r = [msamples / (ms * 1e-3) for ms in best]
        print(f"{name} {W}x{H} depth {depth}  {best[0]:.3f}  {r[0]:.0f}  {best[1]:.3f}  {r[1]:.0f}  {r[1] / r[0]:.3f}", flush=True)


def kernels():
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# element-wise kernels on synthetic frames, 16-byte aligned; HIP events, warm, best of {REPS}")
    print("# frame  kernel  ms")
    for W, H in ((800, 800), (3840, 2160)):
        n = W * H
        p, S, Q = [torch.rand(3 * n, device=dev, dtype=torch.float64) * 16.0 for _ in range(3)]
        Q.mul_(20.0)                                              # (Q >= S^2 / N: a plausible state, not one the clamp flattens)
        cnt = torch.full((n,), 64, dtype=torch.int32, device=dev); pas = torch.full((n,), 4, dtype=torch.int32, device=dev)
        e2 = torch.empty(n, device=dev, dtype=torch.float64)
        st = torch.zeros(4, device=dev, dtype=torch.int64)
        lst = torch.zeros(n, dtype=torch.int32, device=dev); n_list = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.zeros(R.adaptive_select_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
        img = torch.zeros(3 * n, dtype=torch.uint8, device=dev); chg = torch.zeros(1, dtype=torch.int64, device=dev)
        full = torch.arange(n, dtype=torch.int32, device=dev); half = torch.arange(0, n, 2, dtype=torch.int32, device=dev)
        tau = 1.0 / 256.0
        R.adaptive_select_device(S, Q, cnt, pas, W, H, 16, tau, lst, n_list, ws, stream=stream)
        torch.cuda.synchronize()
        listed = int(n_list.cpu()[0])

        def merge(pixels, k):
            cnt.fill_(64)                                         # (inside the timed window: 4 B per pixel beside the merge's 144)
            R.adaptive_merge_device(p, 16, S, Q, cnt, pas, pixels, k, stream=stream)

        rows = ((f"select + compaction (tau 1/256, spread 1: {listed} of {n} listed)", lambda: R.adaptive_select_device(S, Q, cnt, pas, W, H, 16, tau, lst, n_list, ws, stream=stream)),
                ("select + compaction (spread 0)", lambda: R.adaptive_select_device(S, Q, cnt, pas, W, H, 16, tau, lst, n_list, ws, spread=0, stream=stream)),
                ("count reset alone (part of the two list merge rows)", lambda: cnt.fill_(64)),
                ("list merge, every pixel", lambda: merge(full, n)),
                ("list merge, every other pixel", lambda: merge(half, (n + 1) // 2)),
                ("error with counts: map + statistics", lambda: R.adaptive_error_device(S, Q, cnt, pas, W, H, e2, tau, st, stream=stream)),
                ("error with counts: map", lambda: R.adaptive_error_device(S, Q, cnt, pas, W, H, e2, stream=stream)),
                ("resolve with counts", lambda: R.adaptive_resolve_rgb8_device(S, cnt, W, H, img, None, chg, stream=stream)),
                ("rt_moments: merge", lambda: R.moments_merge_device(p, 16, S, Q, stream=stream)),
                ("rt_moments: error map", lambda: R.moments_error_device(S, Q, 64, 4, W, H, e2, stream=stream)))
        for kname, launch in rows:
            print(f"{W}x{H}  {kname}  {_best_ms(launch):.4f}", flush=True)
        del p, S, Q, cnt, pas, e2, st, lst, ws, img, full, half


def _display(mean):
    return np.sqrt(np.clip(mean, 0.0, None)).clip(0.0, 0.999)


def error():
    b, cam, bg = _scene("cornell")
    W = H = 200
    depth, cap, n_b, tau = 50, 4096, 16, 1.0 / 256.0
    truth = _display(R.render(b, cam, bg, W, H, cap, depth, 99) / cap)
    print(f"# Cornell box {W}x{H}, depth {depth}, seed 7, tau = 1/256, passes of {n_b}, at most {cap} samples per pixel; RMS error in display units against {cap} spp of seed 99")
    print("# frame  passes  total samples  mean samples per pixel  largest count  kernel ms (sum over passes)  RMS error  pixels still above tau")

    def report(name, n_passes, total, most, ms, mean, stats):
        rms = float(np.sqrt(np.mean((_display(mean) - truth) ** 2)))
        print(f"{name}  {n_passes}  {total}  {total / (W * H):.1f}  {most}  {ms:.2f}  {rms:.5f}  {stats['unconverged']}", flush=True)

    with R.Progressive(b, cam, bg, W, H, depth, 7, moments=True) as frame:
        ms, n_passes = 0.0, 0
        while frame.samples < cap:
            frame.add(n_b); ms += R.last_kernel_ms(b); n_passes += 1
            if frame.passes >= 2 and frame.error_stats(tau)["unconverged"] == 0:
                break
        report("uniform, until_error", n_passes, frame.samples * W * H, frame.samples, ms, frame.sum() / frame.samples, frame.error_stats(tau))
    for spread in (0, 1):
        with R.Progressive(b, cam, bg, W, H, depth, 7, adaptive=True) as frame:
            ms, n_passes, shares = 0.0, 0, []
            while True:
                info = frame.add_adaptive(n_b, tau, cap, spread)
                if info["listed"] == 0:
                    break
                ms += R.last_query_ms(b) if info["kernel"] else R.last_kernel_ms(b)
                n_passes += 1
                shares.append(info["listed"] / (W * H))
            n, _ = frame.counts()
            report(f"adaptive, spread {spread}", n_passes, info["total"], int(n.max()), ms, frame.sum() / np.maximum(n, 1)[..., None], frame.error_stats(tau))
            marks = [shares[k] for k in (1, 3, 7, 15, 31, 63, 127) if k < len(shares)]
            print(f"#   active share after pass 2, 4, 8, ...: {' '.join(f'{s:.3f}' for s in marks)}; sample counts: median {int(np.median(n))}, 90th percentile {int(np.percentile(n, 90))}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["rate", "kernels", "error"]
    if "rate" in what:
        rate()
    if "kernels" in what:
        kernels()
    if "error" in what:
        error()

"""Moments timing and coverage table.  Part 1 (kernels): the merge kernel and the error kernel (map + statistics, and each
alone) of csrc/rt_moments.hip at 800 x 800 and 3840 x 2160 on synthetic frames — HIP events around the launch, warm, best of REPS — beside
their traffic floors (merge: 72 B in + 72 B out = 144 B per pixel; error: 48 B in + 8 B out, 48 B in for the statistics alone) as achieved
bytes/s, for 16-byte aligned buffers and for buffers 8 bytes off (the scalar merge kernel).  Part 2 (passes): the Cornell box at 800 x 800,
depth 50, 1024 samples per pixel (workload C2's view) as 16 passes of 64 and as 64 passes of 16, on a frame without and with moments: wall
time of the synchronous loop (frame.add) and of the passes enqueued back to back on one stream with one wait at the end (frame.add_async),
best of REPS_PASSES, and the difference per pass.  `passes --lib PATH` runs the plain frames of part 2 on another build of the library
(the parent commit's), which may lack the moments' entry points: the plain path is unchanged, so the two should agree within the
run-to-run spread.  Part 3 (coverage): the Cornell box at 200 x 200, depth 50, 16 passes of 16 samples with moments (seed 7) against 4096
samples of seed 99: the share of channels whose mean lies within 1, 2 and 3 estimated standard errors of the reference's (the reference's own
variance, the estimate scaled by N / 4096, is added), beside the normal distribution's 68.3 / 95.4 / 99.7 %; and the same after 4 passes of 64.
usage: python tools/moments_probe.py [kernels] [passes] [coverage] > profiles/progressive_moments.log
       python tools/moments_probe.py passes --lib path/to/parent/librt_amd.so"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5
REPS_PASSES = 3
HBM_ACHIEVABLE = 6.3e12


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


def kernels():
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# moments kernels on synthetic frames; HIP events, warm, best of {REPS}; floors: merge 144 B / pixel, error 56 B / pixel (48 B for the statistics alone)")
    print("# frame  alignment  kernel  ms  floor bytes  achieved TB/s  share of the 6.3 TB/s achievable HBM rate")
    for W, H in ((800, 800), (3840, 2160)):
        n = W * H
        for off, name in ((0, "16-byte"), (1, "8-byte")):
            bufs = [torch.rand(3 * n + off, device=dev, dtype=torch.float64)[off:] * 16.0 for _ in range(3)]
            p, S, Q = bufs
            Q.mul_(20.0)                                          # (Q >= S^2 / N: a plausible state, not one the clamp flattens)
            e2 = torch.empty(n, device=dev, dtype=torch.float64)
            st = torch.zeros(4, device=dev, dtype=torch.int64)
            rows = (("merge", lambda: R.moments_merge_device(p, 16, S, Q, stream=stream), n * 144),
                    ("error map + statistics", lambda: R.moments_error_device(S, Q, 64, 4, W, H, e2, 1.0 / 256.0, st, stream=stream), n * 56),
                    ("error map", lambda: R.moments_error_device(S, Q, 64, 4, W, H, e2, stream=stream), n * 56),
                    ("error statistics", lambda: R.moments_error_device(S, Q, 64, 4, W, H, None, 1.0 / 256.0, st, stream=stream), n * 48))
            for kname, launch, floor in rows:
                ms = _best_ms(launch)
                rate = floor / (ms * 1e-3)
                print(f"{W}x{H}  {name}  {kname}  {ms:.4f}  {floor}  {rate / 1e12:.3f}  {rate / HBM_ACHIEVABLE:.2f}", flush=True)
            del bufs, p, S, Q, e2, st


def _cornell():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    return build_scene("cornell", _lib.load(), None)


def passes(plain_only=False):
    b, cam, bg = _cornell()
    W = H = 800
    depth, spp = 50, 1024
    stream = torch.cuda.Stream()
    print(f"# Cornell box {W}x{H}, depth {depth}, {spp} samples per pixel in passes; wall ms, best of {REPS_PASSES} (a warm frame first)")
    print("# passes x size  frame  frame.add loop ms  add_async on one stream + one wait ms")
    table = {}
    for n_passes, size in ((16, 64), (64, 16)):
        for moments in ((False,) if plain_only else (False, True)):
            best = [1e30, 1e30]
            with R.Progressive(b, cam, bg, W, H, depth, 7, moments=moments) as frame:
                for rep in range(REPS_PASSES + 1):
                    frame.reset()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n_passes):
                        frame.add(size)
                    t1 = time.perf_counter()
                    frame.reset()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    for _ in range(n_passes):
                        frame.add_async(size, stream.cuda_stream)
                    stream.synchronize()
                    t3 = time.perf_counter()
                    if rep:
                        best = [min(best[0], (t1 - t0) * 1e3), min(best[1], (t3 - t2) * 1e3)]
            table[(n_passes, moments)] = best
            print(f"{n_passes} x {size}  {'moments' if moments else 'plain'}  {best[0]:.3f}  {best[1]:.3f}", flush=True)
        if not plain_only:
            d = [table[(n_passes, True)][k] - table[(n_passes, False)][k] for k in (0, 1)]
            print(f"{n_passes} x {size}  moments - plain: {d[0]:.3f} / {d[1]:.3f} ms = {d[0] / n_passes * 1e3:.1f} / {d[1] / n_passes * 1e3:.1f} us per pass", flush=True)


def coverage():
    b, cam, bg = _cornell()
    W = H = 200
    depth, truth_spp = 50, 4096
    truth = R.render(b, cam, bg, W, H, truth_spp, depth, 99) / truth_spp
    print(f"# coverage: Cornell box {W}x{H}, depth {depth}, seed 7 with moments against {truth_spp} spp of seed 99; channels with V > 0 and a mean < 1")
    print("# passes x size  channels  within 1 / 2 / 3 estimated standard errors (normal: 0.683 / 0.954 / 0.997)  unconverged at tau = 1/256  max standard error (display units)")
    for n_passes, size in ((16, 16), (4, 64), (64, 16)):
        with R.Progressive(b, cam, bg, W, H, depth, 7, moments=True) as frame:
            for _ in range(n_passes):
                frame.add(size)
            S, Q, N, B = frame.sum(), frame.sq_sum(), frame.samples, frame.passes
            st = frame.error_stats(1.0 / 256.0)
        with np.errstate(all="ignore"):
            m = S / N
            V = np.maximum(Q - S * S / N, 0.0) / (B - 1) / N
            z = np.abs(m - truth) / np.sqrt(V * (1.0 + N / truth_spp))
        use = np.isfinite(z) & (V > 0.0) & (m < 1.0)
        shares = [float((z[use] <= k).mean()) for k in (1, 2, 3)]
        print(f"{n_passes} x {size}  {int(use.sum())}  {shares[0]:.3f} / {shares[1]:.3f} / {shares[2]:.3f}  {st['unconverged']} of {W * H}  {st['max_error']:.4f}", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    plain_only = False
    if "--lib" in args:
        k = args.index("--lib")
        _lib._backend = _lib.load_path(args[k + 1], allow_missing=True)       # another build: only what it has is declared
        del args[k:k + 2]
        plain_only = True
    what = args or ["kernels", "passes", "coverage"]
    if "kernels" in what and not plain_only:
        kernels()
    if "passes" in what:
        passes(plain_only)
    if "coverage" in what and not plain_only:
        coverage()

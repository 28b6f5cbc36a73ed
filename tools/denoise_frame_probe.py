"""Denoising a frame as it is: cost and error tables.  Part 1 (kernels): rt_denoise_frame_device beside the device form it
reduces to — rt_denoise_device, rt_denoise_albedo_device, rt_denoise_variance_device — on synthetic frames at 800 x 800 and 3840 x 2160,
K = 2, the same buffers, the same run; the fourth mode (variance with albedo) and the forms with per-pixel counts beside them; and
rt_adaptive_variance_device beside rt_moments_variance_device.  The difference of a pair is what prepare and finish cost.  Part 2
(resolve): rt_progressive_resolve_denoised_frame_rgb8 against the existing denoised resolve of the same uniform Cornell-box frame in the
three modes that have a predecessor, and the resolve of an adaptive frame of the same view beside them.  HIP events, warm, best of REPS.
Part 3 (error): clipped MSE against 2048 samples of seed 99, as ratios to the raw frame, K = 1 .. 5: the Cornell box, the random spheres
and the textured scene of tests/test_denoise_albedo_gpu.py as uniform frames of 4 passes of 4 (albedo only, variance only, variance with
albedo), and the Cornell box as an adaptive frame (tau = 1/64, passes of 4, at most 64 samples per pixel; colour stop, variance stop).
usage: python tools/denoise_frame_probe.py [kernels] [resolve] [error] > profiles/denoise_frame.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5
K = 2
ALBEDO_SAMPLES = 4


def _scene(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if name == "textured":
        from test_denoise_albedo_gpu import textured_scene
        return textured_scene(_lib.load())
    from conftest import build_scene
    return build_scene(name, _lib.load(), None)


def _best_ms(launch):
    """Best of REPS of one call between two HIP events on the current stream, after one warm run."""
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
    b, cam, bg = _scene("cornell")
    print(f"# device forms, K = {K}, 16-byte aligned buffers, the Cornell box's guide records, synthetic sums; HIP events, warm, best of {REPS}")
    print("# frame  mode  predecessor ms  rt_denoise_frame_device ms (one count)  difference  rt_denoise_frame_device ms (per-pixel counts)")
    for W, H in ((800, 800), (3840, 2160)):
        n = W * H
        S = torch.rand(3 * n, device=dev, dtype=torch.float64) * 16.0
        V = torch.rand(3 * n, device=dev, dtype=torch.float64) * 0.01
        A = torch.rand(3 * n, device=dev, dtype=torch.float64) * ALBEDO_SAMPLES
        Q = S * S / 16.0 + torch.rand(3 * n, device=dev, dtype=torch.float64)
        cnt = torch.randint(8, 65, (n,), dtype=torch.int32, device=dev); pas = torch.full((n,), 4, dtype=torch.int32, device=dev)
        hits = torch.empty(16 * n, device=dev, dtype=torch.float64)
        R.query_camera_device(b, cam, W, H, hits, 0, 7)
        out = torch.empty(3 * n, device=dev, dtype=torch.float64)
        ws = torch.empty(R.denoise_frame_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sc, sv = R.DENOISE_SIGMA, R.DENOISE_VARIANCE_SIGMA

        def frame(counts, var, alb, sigma):
            return lambda: R.denoise_frame_device(S, hits, W, H, counts, 16, var, alb, ALBEDO_SAMPLES, out, None, ws, K, sigma, 0, stream)
        rows = (("colour stop", lambda: R.denoise_device(S, 16, hits, W, H, out, ws, K, sc, 0, stream), frame(None, None, None, sc), frame(cnt, None, None, sc)),
                ("colour stop, albedo", lambda: R.denoise_albedo_device(S, 16, A, ALBEDO_SAMPLES, hits, W, H, out, ws, K, sc, 0, stream), frame(None, None, A, sc), frame(cnt, None, A, sc)),
                ("variance stop", lambda: R.denoise_variance_device(S, 16, V, hits, W, H, out, None, ws, K, sv, 0, stream), frame(None, V, None, sv), frame(cnt, V, None, sv)),
                ("variance stop, albedo", None, frame(None, V, A, sv), frame(cnt, V, A, sv)))
        for mode, old, new, counted in rows:
            t_new, t_cnt = _best_ms(new), _best_ms(counted)
            if old is None:
                print(f"{W}x{H}  {mode}  -  {t_new:.4f}  -  {t_cnt:.4f}", flush=True)
            else:
                t_old = _best_ms(old)
                print(f"{W}x{H}  {mode}  {t_old:.4f}  {t_new:.4f}  {t_new - t_old:+.4f}  {t_cnt:.4f}", flush=True)
        t4 = _best_ms(lambda: R.moments_variance_device(S, Q, 64, 4, W, H, out, stream))
        tE = _best_ms(lambda: R.adaptive_variance_device(S, Q, cnt, pas, W, H, out, stream))
        print(f"{W}x{H}  variance frame: rt_moments_variance_device {t4:.4f}  rt_adaptive_variance_device {tE:.4f}", flush=True)
        del S, V, A, Q, cnt, pas, hits, out, ws


def resolve():
    b, cam, bg = _scene("cornell")
    depth = 8
    print(f"# denoised resolves of one Cornell-box frame (depth {depth}, 2 passes of 4; the adaptive frame: one more pass over the pixels above the median error), K = {K},")
    print(f"# guide and albedo sums built before the timed calls; the call includes its copy of the image to the host; HIP events on the null stream, warm, best of {REPS}")
    print("# frame  mode  existing resolve ms  rt_progressive_resolve_denoised_frame_rgb8 ms  difference  the same on the adaptive frame ms")
    for W, H in ((800, 800), (3840, 2160)):
        with R.Progressive(b, cam, bg, W, H, depth, 7, moments=True) as frame, R.Progressive(b, cam, bg, W, H, depth, 7, adaptive=True) as ada:
            for f in (frame, ada):
                f.add(4); f.add(4)
            tau = float(np.median(ada.error_map())) ** 0.5
            info = ada.add_adaptive(4, tau, None, 0)
            sc, sv = R.DENOISE_SIGMA, R.DENOISE_VARIANCE_SIGMA
            rows = (("colour stop", lambda: frame.rgb8_denoised(K, sc), (K, sc, 0, False, 0)),
                    (f"colour stop, albedo {ALBEDO_SAMPLES}", lambda: frame.rgb8_denoised_albedo(ALBEDO_SAMPLES, K, sc), (K, sc, 0, False, ALBEDO_SAMPLES)),
                    ("variance stop", lambda: frame.rgb8_denoised_variance(K, sv), (K, sv, 0, True, 0)),
                    (f"variance stop, albedo {ALBEDO_SAMPLES}", None, (K, sv, 0, True, ALBEDO_SAMPLES)))
            print(f"# {W}x{H}: the adaptive frame's third pass listed {info['listed']} of {W * H} pixels", flush=True)
            for mode, old, args in rows:
                t_new = _best_ms(lambda: frame.rgb8_denoised_frame(*args))
                t_ada = _best_ms(lambda: ada.rgb8_denoised_frame(*args))
                if old is None:
                    print(f"{W}x{H}  {mode}  -  {t_new:.3f}  -  {t_ada:.3f}", flush=True)
                else:
                    t_old = _best_ms(old)
                    same = np.array_equal(old(), frame.rgb8_denoised_frame(*args))
                    print(f"{W}x{H}  {mode}  {t_old:.3f}  {t_new:.3f}  {t_new - t_old:+.3f}  {t_ada:.3f}  (same bytes: {same})", flush=True)
            t_plain = _best_ms(lambda: frame.rgb8())
            print(f"{W}x{H}  the plain resolve (rgb8), for scale  {t_plain:.3f}", flush=True)


def _mse(rgb_sum, n, truth, truth_spp):
    mean = rgb_sum / (n if np.isscalar(n) else np.maximum(n, 1).astype(np.float64)[..., None])
    return float(np.mean((np.clip(mean, 0.0, 1.0) - np.clip(truth / truth_spp, 0.0, 1.0)) ** 2))


def error():
    W = H = 40
    truth_spp = 2048
    print(f"# clipped MSE against {truth_spp} samples of seed 99 as a ratio to the raw frame's; {W}x{H}, seed 7; sigmas: render.py's defaults; albedo sums of 16 samples")
    print("# scene  frame  raw MSE  K  albedo only  variance only  variance with albedo   (adaptive frames: colour stop  variance stop  variance with albedo)")
    for name, depth in (("textured", 12), ("cornell", 20), ("random", 20)):
        b, cam, bg = _scene(name)
        truth = R.render(b, cam, bg, W, H, truth_spp, depth, 99)
        hits = R.query_camera(b, cam, W, H, 0, 7)
        alb = R.query_camera_albedo(b, cam, W, H, 0, 16, 7)
        with R.Progressive(b, cam, bg, W, H, depth, 7, moments=True) as frame:
            for _ in range(4):
                frame.add(4)
            S, N, V = frame.sum(), frame.samples, frame.variance()
        raw = _mse(S, N, truth, truth_spp)
        for k in range(1, 6):
            a = _mse(R.denoise_albedo(S, N, alb, 16, hits, k, R.DENOISE_SIGMA), N, truth, truth_spp)
            v = _mse(R.denoise_variance(S, N, V, hits, k, R.DENOISE_VARIANCE_SIGMA), N, truth, truth_spp)
            both = _mse(R.denoise_frame(S, hits, None, N, V, alb, 16, k, R.DENOISE_VARIANCE_SIGMA), N, truth, truth_spp)
            print(f"{name}  uniform 4 x 4  {raw:.6f}  {k}  {a / raw:.3f}  {v / raw:.3f}  {both / raw:.3f}", flush=True)
        with R.Progressive(b, cam, bg, W, H, depth, 7, adaptive=True) as frame:
            while frame.add_adaptive(4, 1.0 / 64.0, 64)["listed"]:
                pass
            S, (n, _), V = frame.sum(), frame.counts(), frame.variance_counts()
        raw = _mse(S, n, truth, truth_spp)
        for k in range(1, 6):
            c = _mse(R.denoise_frame(S, hits, n, 1, None, None, 1, k, R.DENOISE_SIGMA), n, truth, truth_spp)
            v = _mse(R.denoise_frame(S, hits, n, 1, V, None, 1, k, R.DENOISE_VARIANCE_SIGMA), n, truth, truth_spp)
            both = _mse(R.denoise_frame(S, hits, n, 1, V, alb, 16, k, R.DENOISE_VARIANCE_SIGMA), n, truth, truth_spp)
            print(f"{name}  adaptive tau 1/64 (mean {n.mean():.1f}, {n.min()} .. {n.max()} samples)  {raw:.6f}  {k}  {c / raw:.3f}  {v / raw:.3f}  {both / raw:.3f}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "resolve", "error"]
    if "kernels" in what:
        kernels()
    if "resolve" in what:
        resolve()
    if "error" in what:
        error()

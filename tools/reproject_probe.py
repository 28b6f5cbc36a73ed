"""Temporal accumulation: cost and error tables.  Part 1 (kernels): rt_reproject_device (with and without per-pixel counts) and
rt_temporal_blend_device at 800 x 800 and 3840 x 2160 on the Cornell box's records of two views 2 degrees apart and synthetic sums, beside
the bytes each moves at the least; the reprojection also with the previous records packed first into the 8 words a tap reads (a torch
gather, only to see what the 128-byte records cost the taps).  Part 2 (set_view): rt_progressive_set_view on the C2 view (Cornell box,
800 x 800) beside a pass of 16 samples of it, host clock around synchronous calls.  Part 3 (error): an orbit of 2 degrees per view at 16
samples per view, 8 views, on the Cornell box (200 x 200) and the random spheres (256 x 144): RMS error of the display values (clipped to [0, 1], the
mean over the views after the first) against a 4096-spp frame of each view — raw, temporal, temporal + denoise (K = 2), denoise alone — with
the frame's records from sample 0 and from the averaged guide of 16 samples (rt_progressive_set_guide_samples).
Temporal variance (> profiles/reproject_variance.log).  vkernels: rt_reproject_variance_device beside rt_reproject_device on the same
inputs, and rt_temporal_blend_variance_device, at both sizes.  vsetview: rt_progressive_set_view on the C2 view with and without moments.
verror: the orbit table with 7 views, 16 samples per view as one pass and as 2 x 8, on the Cornell box, the random spheres and a three-texture
scene: raw, temporal, temporal + plain filter, temporal + variance stop without and with albedo_samples = 16, and the variance filter alone.
usage: python tools/reproject_probe.py [kernels] [setview] [error] [vkernels] [vsetview] [verror] > profiles/reproject.log"""
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
DEGREES = 2.0
SPP = 16
VIEWS = 8
REF_SPP = 4096
SIZES, DEPTH = {"cornell": (200, 200), "random": (256, 144)}, 50           # the scenes' own aspect ratios


def _scene(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import build_scene
    return build_scene(name, _lib.load(), None)


def _orbit(cam, degrees):
    a = np.radians(degrees)
    c = type(cam).from_buffer_copy(cam)
    r = np.array(cam.lookfrom[:]) - np.array(cam.lookat[:])
    c.lookfrom[:] = list(np.array(cam.lookat[:]) + np.array([np.cos(a) * r[0] + np.sin(a) * r[2], r[1], -np.sin(a) * r[0] + np.cos(a) * r[2]]))
    return c


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
    b, cam, _ = _scene("cornell")
    cam2 = _orbit(cam, DEGREES)
    print(f"# device forms on the Cornell box's records of two views {DEGREES} degrees apart, synthetic sums; HIP events, warm, best of {REPS}")
    print("# frame  kernel  ms  least bytes per pixel  GB/s at that count")
    for W, H in ((800, 800), (3840, 2160)):
        n = W * H
        S = torch.rand(3 * n, device=dev, dtype=torch.float64) * 16.0
        cnt = torch.randint(8, 65, (n,), dtype=torch.int32, device=dev)
        g0 = torch.empty(16 * n, device=dev, dtype=torch.float64); g1 = torch.empty(16 * n, device=dev, dtype=torch.float64)
        R.query_camera_device(b, cam, W, H, g0, 0, 7)
        R.query_camera_device(b, cam2, W, H, g1, 0, 8)
        hs = torch.empty(3 * n, device=dev, dtype=torch.float64); hn = torch.empty(n, device=dev, dtype=torch.int32)
        out = torch.empty(3 * n, device=dev, dtype=torch.float64); out_n = torch.empty(n, device=dev, dtype=torch.int32)
        torch.cuda.synchronize()
        # what must move at the least: the pixel's own record (128), one previous record's used words (64), sums and count of one tap (28), 28 out
        rows = (("reproject, counts", lambda: R.reproject_device(S, g0, cam, g1, W, H, hs, hn, d_prev_counts=cnt, stream=stream), 128 + 64 + 28 + 28),
                ("reproject, one count", lambda: R.reproject_device(S, g0, cam, g1, W, H, hs, hn, prev_samples=16, stream=stream), 128 + 64 + 24 + 28),
                ("blend, counts", lambda: R.temporal_blend_device(S, hs, hn, W, H, out, out_n, d_counts=cnt, stream=stream), 72 + 12),
                ("blend, one count", lambda: R.temporal_blend_device(S, hs, hn, W, H, out, out_n, samples=16, stream=stream), 72 + 8),
                ("(torch) pack previous records to 8 words", lambda: g0.view(n, 16)[:, [0, 2, 3, 4, 5, 6, 7, 12]].contiguous(), 128 + 64))
        for what, launch, bytes_px in rows:
            ms = _best_ms(launch)
            print(f"{W}x{H}  {what}  {ms:.4f}  {bytes_px}  {bytes_px * n / ms / 1e6:.0f}", flush=True)
        torch.cuda.synchronize()
        print(f"{W}x{H}  pixels with history: {int((hn != 0).sum())} of {n}", flush=True)


def setview():
    b, cam, bg = _scene("cornell")
    W = H = 800
    print(f"# rt_progressive_set_view on the C2 view (Cornell box, {W} x {H}) beside a pass of {SPP} samples; host clock around synchronous calls, best of {REPS}")
    with R.Progressive(b, cam, bg, W, H, DEPTH, 11) as fr:
        fr.add(SPP)
        fr.set_view(_orbit(cam, DEGREES), 12)                 # warm: buffers, the query kernels
        fr.add(SPP)
        t_pass, t_view, t_plain, t_res = [], [], [], []
        for k in range(REPS):
            t0 = time.perf_counter(); fr.add(SPP); t_pass.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); fr.set_view(_orbit(cam, DEGREES * (k + 2)), 13 + k); t_view.append(time.perf_counter() - t0)
            fr.add(SPP)
            t0 = time.perf_counter(); fr.rgb8_temporal(); t_res.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); fr.set_view(_orbit(cam, DEGREES * (k + 2)), 40 + k, 0); t_plain.append(time.perf_counter() - t0)
            fr.add(SPP)
        print(f"pass of {SPP} samples  {min(t_pass) * 1e3:.3f} ms")
        print(f"set_view with history  {min(t_view) * 1e3:.3f} ms  (blend, two record queries, reprojection, count read-back, the reset's memsets)")
        print(f"set_view, max_history = 0  {min(t_plain) * 1e3:.3f} ms")
        print(f"rgb8_temporal (iterations = 0, with the copy of {W * H * 3} bytes to the host)  {min(t_res) * 1e3:.3f} ms", flush=True)


def _rms(image8, ref):
    return float(np.sqrt(np.mean((image8.astype(np.float64) / 256.0 - ref) ** 2)))


def error():
    print(f"# orbit of {DEGREES} degrees per view, {SPP} samples per view, {VIEWS} views, max_history {R.REPROJECT_MAX_HISTORY}, sigma {R.REPROJECT_SIGMA}, K = 2,")
    print(f"# RMS error of the display values against {REF_SPP} spp of each view, the mean over views 1 .. {VIEWS - 1}; view 0 has no history")
    print("# scene  guide_samples  raw  temporal  temporal + denoise  denoise alone  pixels with history in the last view")
    for name, guide_samples in (("cornell", 1), ("cornell", 16), ("random", 1), ("random", 16)):
        b, cam, bg = _scene(name)
        EW, EH = SIZES[name]
        sums = {"raw": 0.0, "temporal": 0.0, "temporal+denoise": 0.0, "denoise": 0.0}
        with R.Progressive(b, cam, bg, EW, EH, DEPTH, 100, guide_samples=guide_samples) as fr:
            for v in range(VIEWS):
                view = _orbit(cam, DEGREES * v)
                if v:
                    fr.set_view(view, 100 + v)
                fr.add(SPP)
                if v == 0:
                    continue
                ref = np.clip(np.sqrt(R.render(b, view, bg, EW, EH, REF_SPP, DEPTH, 9000 + v) / REF_SPP), 0.0, 0.999)
                ref = np.floor(ref * 256.0) / 256.0
                sums["raw"] += _rms(fr.rgb8()[0], ref)
                sums["temporal"] += _rms(fr.rgb8_temporal(), ref)
                sums["temporal+denoise"] += _rms(fr.rgb8_temporal(2), ref)
                sums["denoise"] += _rms(fr.rgb8_denoised(2), ref)
            held = fr.history_info()["pixels"]
        k = VIEWS - 1
        print(f"{name} {EW}x{EH}  {guide_samples}  {sums['raw'] / k:.5f}  {sums['temporal'] / k:.5f}  {sums['temporal+denoise'] / k:.5f}  {sums['denoise'] / k:.5f}  {held} of {EW * EH}", flush=True)


def vkernels():
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    b, cam, _ = _scene("cornell")
    cam2 = _orbit(cam, DEGREES)
    print(f"# temporal variance, device forms on the Cornell box's records of two views {DEGREES} degrees apart, synthetic sums and variances; HIP events, warm, best of {REPS}")
    print("# frame  kernel  ms  least bytes per pixel  GB/s at that count")
    for W, H in ((800, 800), (3840, 2160)):
        n = W * H
        S = torch.rand(3 * n, device=dev, dtype=torch.float64) * 16.0
        V = torch.rand(3 * n, device=dev, dtype=torch.float64) / 16.0
        V[::97] = float("inf")
        cnt = torch.randint(8, 65, (n,), dtype=torch.int32, device=dev)
        g0 = torch.empty(16 * n, device=dev, dtype=torch.float64); g1 = torch.empty(16 * n, device=dev, dtype=torch.float64)
        R.query_camera_device(b, cam, W, H, g0, 0, 7)
        R.query_camera_device(b, cam2, W, H, g1, 0, 8)
        hs = torch.empty(3 * n, device=dev, dtype=torch.float64); hn = torch.empty(n, device=dev, dtype=torch.int32); hv = torch.empty(3 * n, device=dev, dtype=torch.float64)
        out = torch.empty(3 * n, device=dev, dtype=torch.float64)
        torch.cuda.synchronize()
        rows = (("reproject (parent kernel), counts", lambda: R.reproject_device(S, g0, cam, g1, W, H, hs, hn, d_prev_counts=cnt, stream=stream), 128 + 64 + 28 + 28),
                ("reproject_variance (fused), counts", lambda: R.reproject_variance_device(S, V, g0, cam, g1, W, H, hs, hn, hv, d_prev_counts=cnt, stream=stream), 128 + 64 + 52 + 52),
                ("reproject (parent kernel), one count", lambda: R.reproject_device(S, g0, cam, g1, W, H, hs, hn, prev_samples=16, stream=stream), 128 + 64 + 24 + 28),
                ("reproject_variance (fused), one count", lambda: R.reproject_variance_device(S, V, g0, cam, g1, W, H, hs, hn, hv, prev_samples=16, stream=stream), 128 + 64 + 48 + 52),
                ("blend_variance, counts", lambda: R.temporal_blend_variance_device(V, hv, hn, n, out, d_counts=cnt, stream=stream), 72 + 8),
                ("blend_variance, one count", lambda: R.temporal_blend_variance_device(V, hv, hn, n, out, samples=16, stream=stream), 72 + 4),
                ("blend_variance, no variance frame", lambda: R.temporal_blend_variance_device(None, hv, hn, n, out, samples=16, stream=stream), 48 + 4))
        ms_of = {}
        for what, launch, bytes_px in rows:
            ms = ms_of[what] = _best_ms(launch)
            print(f"{W}x{H}  {what}  {ms:.4f}  {bytes_px}  {bytes_px * n / ms / 1e6:.0f}", flush=True)
        torch.cuda.synchronize()
        print(f"{W}x{H}  fused / parent: counts {ms_of['reproject_variance (fused), counts'] / ms_of['reproject (parent kernel), counts']:.3f}, "
              f"one count {ms_of['reproject_variance (fused), one count'] / ms_of['reproject (parent kernel), one count']:.3f}", flush=True)


def vsetview():
    b, cam, bg = _scene("cornell")
    W = H = 800
    print(f"# rt_progressive_set_view on the C2 view (Cornell box, {W} x {H}), a frame without and with moments, 2 passes of {SPP // 2}; host clock around synchronous calls, best of {REPS}")
    for moments in (False, True, False, True):
        with R.Progressive(b, cam, bg, W, H, DEPTH, 11, moments=moments) as fr:
            fr.add(SPP // 2); fr.add(SPP // 2)
            fr.set_view(_orbit(cam, DEGREES), 12)                 # warm: buffers, the query kernels
            t_view, t_res, t_resv = [], [], []
            for k in range(REPS):
                fr.add(SPP // 2); fr.add(SPP // 2)
                t0 = time.perf_counter(); fr.set_view(_orbit(cam, DEGREES * (k + 2)), 13 + k); t_view.append(time.perf_counter() - t0)
                fr.add(SPP)
                fr.rgb8_temporal(2)
                t0 = time.perf_counter(); fr.rgb8_temporal(2); t_res.append(time.perf_counter() - t0)
                if moments:
                    fr.rgb8_temporal(2, variance=True)
                    t0 = time.perf_counter(); fr.rgb8_temporal(2, variance=True); t_resv.append(time.perf_counter() - t0)
            line = f"moments {int(moments)}  set_view with history  {min(t_view) * 1e3:.3f} ms  rgb8_temporal(2)  {min(t_res) * 1e3:.3f} ms"
            if moments:
                line += f"  rgb8_temporal(2, variance=True)  {min(t_resv) * 1e3:.3f} ms"
            print(line, flush=True)


def _textures():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_denoise_albedo_gpu import textured_scene
    return textured_scene(_lib.load())


def verror():
    views = 7
    print(f"# orbit of {DEGREES} degrees per view, {SPP} samples per view as one pass and as 2 x {SPP // 2}, {views} views, max_history {R.REPROJECT_MAX_HISTORY}, sigma {R.REPROJECT_SIGMA},")
    print(f"# K = 2, plain sigma {R.DENOISE_SIGMA}, variance sigma {R.DENOISE_VARIANCE_SIGMA}; RMS error of the display values against {REF_SPP} spp of each view, the mean over views 1 .. {views - 1}")
    print("# scene  passes  raw  temporal  temporal + plain filter  temporal + variance stop  ... + albedo 16  variance filter alone (no history)  history pixels with known variance in the last view")
    for name, (EW, EH) in (("cornell", SIZES["cornell"]), ("random", SIZES["random"]), ("textures", (200, 200))):
        b, cam, bg = _textures() if name == "textures" else _scene(name)
        refs = {}
        for passes in (1, 2):
            cols = ("raw", "temporal", "plain", "variance", "variance+albedo", "alone")
            sums = dict.fromkeys(cols, 0.0)
            with R.Progressive(b, cam, bg, EW, EH, DEPTH, 100, moments=True) as fr:
                for v in range(views):
                    view = _orbit(cam, DEGREES * v)
                    if v:
                        fr.set_view(view, 100 + v)
                    for _ in range(passes):
                        fr.add(SPP // passes)
                    if v == 0:
                        continue
                    if v not in refs:
                        ref = np.clip(np.sqrt(R.render(b, view, bg, EW, EH, REF_SPP, DEPTH, 9000 + v) / REF_SPP), 0.0, 0.999)
                        refs[v] = np.floor(ref * 256.0) / 256.0
                    ref = refs[v]
                    sums["raw"] += _rms(fr.rgb8()[0], ref)
                    sums["temporal"] += _rms(fr.rgb8_temporal(), ref)
                    sums["plain"] += _rms(fr.rgb8_temporal(2), ref)
                    sums["variance"] += _rms(fr.rgb8_temporal(2, variance=True), ref)
                    sums["variance+albedo"] += _rms(fr.rgb8_temporal(2, variance=True, albedo_samples=16), ref)
                    if passes == 2:
                        sums["alone"] += _rms(fr.rgb8_denoised_variance(2), ref)
                hv, hn = fr.history_variance(), fr.history()[1]
                held = int(((hn > 0) & np.isfinite(hv).all(axis=-1)).sum())
            k = views - 1
            alone = f"{sums['alone'] / k:.5f}" if passes == 2 else "-"
            print(f"{name} {EW}x{EH}  {passes}x{SPP // passes}  " + "  ".join(f"{sums[c] / k:.5f}" for c in cols[:5]) + f"  {alone}  {held} of {EW * EH}", flush=True)


if __name__ == "__main__":
    parts = sys.argv[1:] or ["kernels", "setview", "error"]
    torch.cuda.set_device(0)
    print(f"# {torch.cuda.get_device_name(0)}")
    for p in parts:
        {"kernels": kernels, "setview": setview, "error": error, "vkernels": vkernels, "vsetview": vsetview, "verror": verror}[p]()

"""Specular-chain guides: cost and error tables.  Part `baseline`: rt_query_camera_guide_device (first hits, with the albedo sums)
on C2's view (Cornell box, 800 x 800), the random spheres at 1200 x 675 and the final scene at 800 x 800, for 1 and 16 samples — the part that
also runs on a build without the chain entry points, so that the two builds can alternate.  Part `cost`: rt_query_camera_chain_guide_device
(with the albedo sums and the link counts) on the same views for max_links 0, 1, 4, 16, max_fuzz 0.  Part `share`: the share of items still
chaining at each link, counted by the NumPy restatement of tests/chain_cases.py over the library's own first-hit queries — what a scheme that
refills ended lanes could recover at most.  Part `quality`: RMS error of the display values against 4096 spp at 16 spp — raw and the four
filters of a progressive frame (plain, albedo, variance, frame with variance and albedo), each with the first-hit guide and with the chain guide
(max_links 4, max_fuzz 0), guide_samples 1 and 16, K = 1 .. 3 — on the random spheres (256 x 144), the final scene (200 x 200) and the test
scene of tests/chain_cases.py (253 x 121).  HIP events, warm, best of 5.
usage: python tools/chain_probe.py [baseline] [cost] [share] [quality] > profiles/chain.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: see _lib.load_path)

from raytracinginrust_amd import _lib  # noqa: E402
from raytracinginrust_amd import render as R  # noqa: E402

REPS = 5
VIEWS = (("cornell", 800, 800), ("random", 1200, 675), ("final", 800, 800))
LINKS = (0, 1, 4, 16)
SAMPLES = (1, 16)
SEED = 0x5EED
SPP, REF_SPP, DEPTH = 16, 4096, 50
QUALITY = (("random", 256, 144), ("final", 200, 200), ("chain", 253, 121))
Q_LINKS, Q_FUZZ = 4, 0.0


def _scene(name):
    from conftest import build_scene
    from raytracinginrust_amd import scenes
    if name == "chain":
        import chain_cases as CC
        b, cam, _ = CC.chain_scene(_lib.load())
        return b, cam, (0.7, 0.8, 1.0)
    return build_scene(name, _lib.load(), scenes.load_earthmap() if name == "final" else None)


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


def _buffers(W, H):
    dev = torch.device("cuda", torch.cuda.current_device())
    n = W * H
    return (torch.empty(16 * n, device=dev, dtype=torch.float64), torch.empty(3 * n, device=dev, dtype=torch.float64),
            torch.empty(n, device=dev, dtype=torch.int32))


def baseline():
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# rt_query_camera_guide_device with albedo sums (first hits); HIP events, warm, best of {REPS}")
    print("# view  n_samples  ms  Msearches/s")
    for name, W, H in VIEWS:
        b, cam, _ = _scene(name)
        g, a, _ = _buffers(W, H)
        for n in SAMPLES:
            ms = _best_ms(lambda: R.query_camera_guide_device(b, cam, W, H, g, a, 0, n, SEED, stream=stream))
            print(f"{name} {W}x{H}  {n}  {ms:.4f}  {W * H * n / ms / 1e3:.0f}", flush=True)


def cost():
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# rt_query_camera_chain_guide_device with albedo sums and link counts, max_fuzz 0; HIP events, warm, best of {REPS}")
    print("# view  n_samples  max_links  ms  links followed per sample  Msearches/s by the lanes' own chains")
    for name, W, H in VIEWS:
        b, cam, _ = _scene(name)
        g, a, l = _buffers(W, H)
        for n in SAMPLES:
            for L in LINKS:
                ms = _best_ms(lambda: R.query_camera_chain_guide_device(b, cam, W, H, g, L, 0.0, a, l, 0, n, SEED, stream=stream))
                torch.cuda.synchronize()
                followed = int(l.to(torch.int64).sum())
                print(f"{name} {W}x{H}  {n}  {L}  {ms:.4f}  {followed / (W * H * n):.4f}  {(W * H * n + followed) / ms / 1e3:.0f}", flush=True)


def share():
    import chain_cases as CC
    from conftest import build_scene
    from raytracinginrust_amd import scenes
    print("# share of items still chaining at link l (sample 0's camera rays, max_links 16, max_fuzz 0): the NumPy restatement over rt_query_albedo")
    print("# view  l = 0, 1, 2, ...")
    for name, W, H in (("cornell", 200, 200), ("random", 256, 144), ("final", 200, 200)):
        b, cam, mats = CC.build_recorded(build_scene, name, _lib.load(), scenes.load_earthmap() if name == "final" else None)
        hits, rays = R.query_camera(b, cam, W, H, 0, SEED, want_rays=True)

        def search(l, r, seed):
            albedo, h = R.query_albedo(b, r, CC.T_MIN, seed, want_hits=True)
            return h, albedo
        c = CC.numpy_chain(search, rays.reshape(-1, 7), mats, 16, 0.0, SEED, first=(hits.reshape(-1, 16), np.ones((W * H, 3))))
        print(f"{name} {W}x{H}  " + "  ".join(f"{v / (W * H):.4f}" for v in c["live"]), flush=True)


def _rms(image8, ref):
    return float(np.sqrt(np.mean((image8.astype(np.float64) / 256.0 - ref) ** 2)))


def quality():
    print(f"# RMS error of the display values against {REF_SPP} spp, frames of {SPP} spp (two passes of {SPP // 2}), depth {DEPTH}; chain: max_links {Q_LINKS}, max_fuzz {Q_FUZZ}")
    print(f"# albedo_samples 16 with the first-hit guide; with the chain guide the albedo sums are the chain's over guide_samples; default sigmas")
    print("# scene  guide  guide_samples  K  raw  plain  albedo  variance  frame (variance + albedo)")
    for name, W, H in QUALITY:
        b, cam, bg = _scene(name)
        ref = np.clip(np.sqrt(R.render(b, cam, bg, W, H, REF_SPP, DEPTH, 9001) / REF_SPP), 0.0, 0.999)
        ref = np.floor(ref * 256.0) / 256.0
        with R.Progressive(b, cam, bg, W, H, DEPTH, SEED, moments=True) as fr:
            fr.add(SPP // 2); fr.add(SPP // 2)
            raw = _rms(fr.rgb8()[0], ref)
            for chain in ((0, 0.0), (Q_LINKS, Q_FUZZ)):
                for gs in (1, 16):
                    fr.set_guide_samples(gs); fr.set_guide_chain(*chain)
                    for K in (1, 2, 3):
                        row = (_rms(fr.rgb8_denoised(K), ref), _rms(fr.rgb8_denoised_albedo(16, K), ref), _rms(fr.rgb8_denoised_variance(K), ref),
                               _rms(fr.rgb8_denoised_frame(K, variance=True, albedo_samples=16), ref))
                        print(f"{name} {W}x{H}  {'chain' if chain[0] else 'first hit'}  {gs}  {K}  {raw:.5f}  " + "  ".join(f"{x:.5f}" for x in row), flush=True)


if __name__ == "__main__":
    parts = sys.argv[1:] or ["baseline", "cost", "share", "quality"]
    torch.cuda.set_device(0)
    print(f"# {torch.cuda.get_device_name(0)}")
    for p in parts:
        {"baseline": baseline, "cost": cost, "share": share, "quality": quality}[p]()

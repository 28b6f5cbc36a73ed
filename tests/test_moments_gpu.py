"""The moments of a progressive frame on the GPU (csrc/rt_moments.hip, rt_progressive_enable_moments): the merge and error kernels against
the host twin with 0 differing 64-bit words, and frames with moments against what their own samples say.

What is compared with what:
  * the device forms on torch tensors against rt_moments_*_host (which tests/test_moments_host.py holds to the NumPy restatement): every
    word equal — sizes with an odd count, one pixel, buffers 8 bytes off 16-byte alignment (the scalar kernel), more pixels than one sweep
    of the grid;
  * a frame fed passes of ONE sample: a pass frame then holds exactly that sample (0.0 + x), so S and Q are the ascending sums of the samples
    and of their squares under ==, and the error map and statistics are the restatement's on those words;
  * a frame fed passes of several samples: S within the bound that holds for any order of adding the N samples, 2 gamma sum|x_i|
    (tests/test_progressive_gpu.py), and Q within the bound that follows from it (see _q_bound);
  * frames with and without moments, checkpoints, and passes on two streams, within the same bounds.
gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, §3.1); a sum of n terms commits n - 1 roundings."""

import numpy as np
import pytest

from conftest import build_scene
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Camera, SceneBuilder

import moments_cases as MC
from moments_cases import differing_words, gamma

pytestmark = pytest.mark.gpu

W = H = 16
DEPTH = 8
SEED = 0xBEEF
SIZES = (3, 5, 8, 16)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, copy=True)).cuda()


def _shifted(a, off):
    """A device copy of `a` whose address is `off` doubles behind a fresh allocation (torch allocations are at least 256-byte aligned)."""
    import torch
    flat = np.array(a, dtype=np.float64, copy=True).reshape(-1)
    buf = torch.zeros(flat.size + off, dtype=torch.float64, device="cuda")
    view = buf[off:]
    view.copy_(torch.from_numpy(flat))
    assert view.data_ptr() % 16 == (8 * off) % 16
    return view


# ---------------------------------------------------------------- 1. the kernels against the host twin
# (H, W): one pixel (3 doubles: one pair and the odd tail); 165 pixels (495 doubles, odd); 192; 90000 pixels; 614400 pixels = 1843200 doubles,
# more than one sweep of the merge's 2048 x 256 lanes over pairs and of the error kernel's 1024 x 256 over pixels
DEVICE_SHAPES = ((1, 1), (11, 15), (3, 64), (300, 300), (600, 1024))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned16", "off8"])
@pytest.mark.parametrize("shape", DEVICE_SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_device_forms_equal_the_host_twin(shape, off):
    import torch
    passes = MC.case(shape)
    n = passes[0].size
    hS = np.zeros(shape + (3,)); hQ = np.zeros(shape + (3,))
    dS = _shifted(hS, off); dQ = _shifted(hQ, off)
    for p, n_b in zip(passes, MC.PASS_SAMPLES):
        R.moments_merge_host(p, n_b, hS, hQ)
        dP = _shifted(p, off)
        R.moments_merge_device(dP, n_b, dS, dQ)
        assert int(np.count_nonzero(dP.cpu().numpy().view(np.uint64))) == 0          # the pass frame is all +0.0 afterwards
    gS = dS.cpu().numpy().reshape(hS.shape); gQ = dQ.cpu().numpy().reshape(hQ.shape)
    assert differing_words(gS, hS) == 0 and differing_words(gQ, hQ) == 0
    # the error map and the statistics, on the state with one infinite second moment
    S, Q, N, B = MC.state(shape)
    dS = _shifted(S, off); dQ = _shifted(Q, off)
    want = R.moments_error_host(S, Q, N, B)
    for tau in (1.0 / 256.0, 0.05):
        d_e2 = torch.full((shape[0] * shape[1],), -1.0, dtype=torch.float64, device="cuda")
        d_st = torch.full((4,), 77, dtype=torch.int64, device="cuda")              # the launcher zeroes the words
        R.moments_error_device(dS, dQ, N, B, shape[1], shape[0], d_e2, tau, d_st)
        assert differing_words(d_e2.cpu().numpy().reshape(shape), want) == 0
        st = R.moments_stats(d_st.cpu().numpy().view(np.uint64), tau)
        assert st == R.moments_stats_host(want, tau)
        assert st["converged"] + st["unconverged"] + st["nonfinite"] == shape[0] * shape[1]
        assert st["nonfinite"] == (1 if shape[0] * shape[1] >= 33 else 0)
        # each output alone
        d_st2 = torch.full((4,), 77, dtype=torch.int64, device="cuda")
        R.moments_error_device(dS, dQ, N, B, shape[1], shape[0], None, tau, d_st2)
        assert torch.equal(d_st2, d_st)
        d_e2b = torch.full_like(d_e2, -1.0)
        R.moments_error_device(dS, dQ, N, B, shape[1], shape[0], d_e2b)
        assert torch.equal(d_e2b.view(torch.int64), d_e2.view(torch.int64))
    assert n == 3 * shape[0] * shape[1]


def test_exact_threshold_on_the_device():
    import torch
    passes, sizes, tau = MC.exact_tau_case()
    dS = _t(np.zeros_like(passes[0])); dQ = _t(np.zeros_like(passes[0]))
    for p, n_b in zip(passes, sizes):
        R.moments_merge_device(_t(p), n_b, dS, dQ)
    d_e2 = torch.zeros(4, dtype=torch.float64, device="cuda"); d_st = torch.zeros(4, dtype=torch.int64, device="cuda")
    R.moments_error_device(dS, dQ, 2, 2, 4, 1, d_e2, tau, d_st)
    e2 = d_e2.cpu().numpy()
    st = R.moments_stats(d_st.cpu().numpy().view(np.uint64), tau)
    assert e2[0] == tau * tau and (st["converged"], st["unconverged"], st["nonfinite"]) == (3, 1, 0) and st["max_e2"] == e2[1]


# ---------------------------------------------------------------- 2. frames
def _cornell(pbe):
    return build_scene("cornell", pbe)


def _masks_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


def _sum_bound(samples):
    """2 gamma_{N-1} sum|x_i| per pixel and channel for the N samples along axis 2 — each of two sums of the same terms, in any order, is
    within gamma_{N-1} sum|x_i| of the exact one — and the mask of channels whose samples are all finite."""
    n = samples.shape[2]
    fin = np.isfinite(samples).all(axis=2)
    return 2.0 * gamma(n - 1) * np.abs(np.where(np.isfinite(samples), samples, 0.0)).sum(axis=2), fin


def _q_bound(parts):
    """Q of the NumPy pass sums in extended precision, and the bound on |Q_device - Q|: the device's pass frame differs from the NumPy pass
    sum P_b by at most beta_b = 2 gamma sum_b|x_i| (the any-order bound), so its square by at most 2 |P_b| beta_b + beta_b^2, and the
    B terms p * p / n_b are multiplied, divided and added in f64: gamma_B Q."""
    Q = np.zeros(parts[0].shape[:2] + (3,), np.longdouble); bound = np.zeros(Q.shape)
    fin = np.ones(Q.shape, bool)
    for part in parts:
        n_b = part.shape[2]
        beta, f = _sum_bound(part)
        P = np.where(f, part.sum(axis=2), 0.0)
        Q += P.astype(np.longdouble) ** 2 / n_b
        bound += (2.0 * np.abs(P) * beta + beta * beta) / n_b
        fin &= f
    Q = Q.astype(np.float64)
    return Q, bound + gamma(len(parts)) * Q, fin


def _run_passes(pbe, sizes, moments=True, seed=SEED):
    b, cam, bg = _cornell(pbe)
    with R.Progressive(b, cam, bg, W, H, DEPTH, seed=seed, moments=moments) as frame:
        parts = [frame.add(n, want_samples=True) for n in sizes]
        out = {"parts": parts, "S": frame.sum(), "samples": frame.samples, "passes": frame.passes, "rgb8": frame.rgb8()[0]}
        if moments:
            out.update(Q=frame.sq_sum(), e2=frame.error_map(), stats={tau: frame.error_stats(tau) for tau in (0.0, 1.0 / 256.0, 0.05, 1e30)})
    return out


_RUNS = {}


def _multi(pbe):
    if "multi" not in _RUNS:
        _RUNS["multi"] = _run_passes(pbe, SIZES)
    return _RUNS["multi"]


def test_passes_of_one_sample_are_exact(pbe):
    r = _run_passes(pbe, (1,) * 8)
    assert r["samples"] == 8 and r["passes"] == 8
    S = np.zeros((H, W, 3)); Q = np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        for part in r["parts"]:
            x = part[:, :, 0, :]
            S = S + x
            Q = Q + (x * x) / np.float64(1.0)
    fin = np.isfinite(S)
    assert _masks_equal(r["S"], S) and _masks_equal(r["Q"], Q)
    assert (r["S"][fin] == S[fin]).all(), "S is not the ascending sum of the samples"
    finq = np.isfinite(Q)
    assert (r["Q"][finq] == Q[finq]).all(), "Q is not the ascending sum of the samples' squares"
    assert np.abs(S[fin]).sum() > 0.0 and (Q[finq] > 0.0).any()
    want = MC.numpy_error(r["S"], r["Q"], 8, 8)
    assert differing_words(r["e2"], want) == 0
    for tau, st in r["stats"].items():
        assert MC.stats_words(st) == MC.numpy_stats(want, tau), tau
    assert r["stats"][1e30]["unconverged"] == 0 and r["stats"][0.0]["unconverged"] > 0 and r["stats"][0.0]["max_e2"] == np.nanmax(want[np.isfinite(want)])


def test_passes_of_several_samples_are_within_the_bounds(pbe):
    r = _multi(pbe)
    assert r["samples"] == sum(SIZES) and r["passes"] == len(SIZES)
    samples = np.concatenate(r["parts"], axis=2)
    bound, fin = _sum_bound(samples)
    S = samples.sum(axis=2)
    dS = np.abs(np.where(fin, r["S"] - S, 0.0))
    print(f"S: max |delta| {dS.max():.3e}, max delta / bound {np.max(dS / np.maximum(bound, 1e-300)):.3f}, channels with a non-finite sample {int((~fin).sum())}")
    assert (dS <= bound).all() and _masks_equal(r["S"], np.where(fin, S, r["S"]))
    Q, qbound, qfin = _q_bound(r["parts"])
    dQ = np.abs(np.where(qfin, r["Q"] - Q, 0.0))
    print(f"Q: max |delta| {dQ.max():.3e}, max delta / bound {np.max(dQ / np.maximum(qbound, 1e-300)):.3f}")
    assert (dQ <= qbound).all() and np.isfinite(r["Q"][qfin]).all() and (Q[qfin] > 0.0).any()
    # the map and the statistics are the restatement's on the frame's own words
    want = MC.numpy_error(r["S"], r["Q"], r["samples"], r["passes"])
    assert differing_words(r["e2"], want) == 0
    for tau, st in r["stats"].items():
        assert MC.stats_words(st) == MC.numpy_stats(want, tau), tau


def test_a_view_in_which_every_ray_misses(pbe):
    b = SceneBuilder(pbe)
    world = b.HittableList()
    world.push(b.Sphere((0.0, 0.0, 5.0), 0.5, b.Lambertian(b.ConstantTexture((0.5, 0.5, 0.5)))))       # behind the camera, which looks down -z
    b.set_scene(world, [])
    cam = Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    bg = (0.5, 0.25, 1.0)
    with R.Progressive(b, cam, bg, 13, 9, DEPTH, seed=3, moments=True) as frame:
        for _ in range(4):
            frame.add(4)
        S, e2, st = frame.sum(), frame.error_map(), frame.error_stats(1.0 / 256.0)
    assert (S == np.array(bg) * 16.0).all()
    assert differing_words(e2, np.zeros((9, 13))) == 0                     # every e2 is exactly +0.0
    assert (st["converged"], st["unconverged"], st["nonfinite"], st["max_e2"]) == (13 * 9, 0, 0, 0.0)


def test_parity_with_a_plain_frame(pbe):
    r = _multi(pbe)
    plain = _run_passes(pbe, SIZES, moments=False)
    assert plain["passes"] == 0
    samples = np.concatenate(r["parts"], axis=2)
    assert np.array_equal(np.concatenate(plain["parts"], axis=2).view(np.uint64), samples.view(np.uint64))      # the same samples, bit for bit
    bound, fin = _sum_bound(samples)
    d = np.abs(np.where(fin, r["S"] - plain["S"], 0.0))
    assert (d <= bound).all() and _masks_equal(r["S"], plain["S"])
    for run in (r, plain):                                                  # each image is the unchanged resolve of its own sums
        assert np.array_equal(run["rgb8"], R.format_image(run["S"], sum(SIZES)).astype(np.uint8))


def test_stopping(pbe):
    b, cam, bg = _cornell(pbe)
    items = list(R.render_progressive(b, cam, bg, W, H, 64, DEPTH, passes=8, seed=SEED, until_error=1e30))
    assert [it[0] for it in items] == [8, 16] and items[0][3] is None and items[1][3]["unconverged"] == 0
    items = list(R.render_progressive(b, cam, bg, W, H, 64, DEPTH, passes=8, seed=SEED, until_error=1e30, min_passes=3))
    assert [it[0] for it in items] == [8, 16, 24]
    items = list(R.render_progressive(b, cam, bg, W, H, 64, DEPTH, passes=6, seed=SEED, until_error=0.0, max_samples=24))
    assert [it[0] for it in items] == [4, 8, 12, 16, 20, 24] and items[-1][3]["unconverged"] > 0 and items[-1][3]["tau"] == 0.0
    assert items[-1][1].shape == (H, W, 3) and items[-1][3]["converged"] + items[-1][3]["unconverged"] + items[-1][3]["nonfinite"] == W * H
    plain = list(R.render_progressive(b, cam, bg, W, H, 16, DEPTH, passes=2, seed=SEED))      # without until_error: the items it always gave
    assert [len(it) for it in plain] == [3, 3]


def test_frame_calls(pbe):
    b, cam, bg = _cornell(pbe)
    with R.Progressive(b, cam, bg, W, H, DEPTH, seed=SEED) as frame:            # a frame without moments
        assert frame.passes == 0
        for call in (frame.error_map, frame.sq_sum, lambda: frame.error_stats(0.1), frame.error_map_device):
            with pytest.raises(R.RenderError, match="no moments"):
                call()
        frame.add(1)
        with pytest.raises(R.RenderError, match="0 samples"):
            frame.enable_moments()
        frame.reset()
        frame.enable_moments()                                                  # after a reset it may
        frame.enable_moments()                                                  # (twice is once)
        frame.add(2)
        assert frame.passes == 1
        for call in (frame.error_map, lambda: frame.error_stats(0.1), frame.error_map_device):
            with pytest.raises(R.RenderError, match="passes must be >= 2"):
                call()
        frame.add(3)
        S = frame.sum()
        assert frame.error_stats(0.1)["nonfinite"] == 0
        with pytest.raises(R.RenderError, match="tau"):
            frame.error_stats(-1.0)
        ptr = frame.error_map_device()
        assert ptr != 0 and frame.error_map_device() == ptr                     # one buffer, owned by the frame
        frame.load(S, 5)                                                        # sums alone: the second moments no longer describe them
        assert frame.samples == 5 and frame.passes == 0
        for call in (frame.error_map, lambda: frame.error_stats(0.1), frame.sq_sum):
            with pytest.raises(R.RenderError, match="invalid"):
                call()
        frame.add(1); frame.add(1)                                              # passes go on, the sums stay right
        assert frame.samples == 7
        with pytest.raises(R.RenderError, match="invalid"):
            frame.error_map()
        frame.reset()
        assert frame.samples == 0 and frame.passes == 0 and np.count_nonzero(frame.sq_sum()) == 0
        frame.add(2); frame.add(2)
        assert frame.passes == 2 and frame.error_map().shape == (H, W)          # moments stayed enabled
        z = np.zeros((H, W, 3))
        lib = pbe.lib
        for args, text in (((z, z, 1, 0), "go together"), ((z, z, 0, 1), "passes must be <= samples_done"), ((z, z, 3, 4), "passes must be <= samples_done"),
                           ((S, z, 0, 0), "non-zero frame"), ((z, z, 2 ** 32, 2), "2^32 - 1")):
            assert lib.rt_progressive_load_moments(frame._h, args[0].ctypes.data, args[1].ctypes.data, args[2], args[3]) != 0
            assert text in lib.rt_last_error().decode(), text
        assert frame.passes == 2


def test_checkpoint_and_resume(pbe):
    b, cam, bg = _cornell(pbe)
    tau = 0.05
    with R.Progressive(b, cam, bg, W, H, DEPTH, seed=SEED, moments=True) as first, R.Progressive(b, cam, bg, W, H, DEPTH, seed=SEED, moments=True) as second:
        first.add(3); first.add(5)
        ck = first.checkpoint()
        assert ck["samples"] == 8 and ck["passes"] == 2
        second.restore(ck)
        assert second.samples == 8 and second.passes == 2
        assert differing_words(second.sum(), ck["rgb_sum"]) == 0 and differing_words(second.sq_sum(), ck["sq_sum"]) == 0
        assert differing_words(second.error_map(), first.error_map()) == 0     # the same words give the same map
        part = first.add(8, want_samples=True)
        second.add(8)
        A = {"S": first.sum(), "Q": first.sq_sum(), "e2": first.error_map(), "st": first.error_stats(tau)}
        Bf = {"S": second.sum(), "Q": second.sq_sum(), "e2": second.error_map(), "st": second.error_stats(tau)}
    assert A["st"]["nonfinite"] == Bf["st"]["nonfinite"]
    # The two frames merged the same words with pass frames that differ by at most beta = 2 gamma sum|x_i| per channel.  What that allows
    # in e2 = (Q - S^2 / N) / ((B - 1) N 4 den), term by term, with a few u for the roundings of each quantity's own operations:
    N, B, n3, u = 16.0, 3.0, 8.0, 2.0 ** -53
    beta, fin = _sum_bound(part)
    P = np.where(fin, part.sum(axis=2), 0.0)
    cA, cB = MC.numpy_channels(A["S"], A["Q"], 16, 3), MC.numpy_channels(Bf["S"], Bf["Q"], 16, 3)
    assert np.array_equal(cA["saturated"], cB["saturated"])                  # (the rule is a step: a flip would need (m - 1)^2 = 9 V to 1e-15)
    S, Q = np.abs(A["S"]), np.abs(A["Q"])
    dS = beta + 2 * u * S
    dQ = (2 * np.abs(P) * beta + beta * beta) / n3 + 4 * u * P * P / n3 + 2 * u * Q
    dssb = dQ + (2 * S * dS + dS * dS) / N + 4 * u * (Q + S * S / N)
    de2 = dssb / ((B - 1) * N * 4 * cA["den"]) + cA["e2"] * (dS / N) / cA["den"] + 8 * u * cA["e2"]
    ok = fin & np.isfinite(A["S"]) & np.isfinite(Bf["S"])
    assert (np.abs(np.where(ok, A["S"] - Bf["S"], 0.0)) <= dS).all() and (np.abs(np.where(ok, A["Q"] - Bf["Q"], 0.0)) <= dQ).all()
    px_ok = ok.all(axis=2)
    d = np.abs(np.where(px_ok, A["e2"] - Bf["e2"], 0.0))
    lim = np.where(ok, de2, 0.0).max(axis=2)                                 # (the maximum over channels moves by at most the largest channel's change)
    print(f"e2 after resume: max |delta| {d.max():.3e}, max delta / bound {np.max(d / np.maximum(lim, 1e-300)):.3f}")
    assert (d <= lim).all() and px_ok.sum() > 0.9 * W * H


def test_async_passes_on_two_streams(pbe):
    import torch
    b, cam, bg = _cornell(pbe)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with R.Progressive(b, cam, bg, W, H, DEPTH, seed=SEED, moments=True) as ref:
        parts = [ref.add(n, want_samples=True) for n in (6, 10)]
    with R.Progressive(b, cam, bg, W, H, DEPTH, seed=SEED, moments=True) as frame:
        frame.add_async(6, s1.cuda_stream)
        frame.add_async(10, s2.cuda_stream)                                    # waits for the first pass's merge on the device, not on the host
        assert frame.passes == 2 and frame.samples == 16
        image, changed = frame.rgb8()                                          # waits for both
        S, Q, st = frame.sum(), frame.sq_sum(), frame.error_stats(0.05)
    assert changed == W * H and image.shape == (H, W, 3)
    samples = np.concatenate(parts, axis=2)
    bound, fin = _sum_bound(samples)
    assert (np.abs(np.where(fin, S - samples.sum(axis=2), 0.0)) <= bound).all()
    Qw, qbound, qfin = _q_bound(parts)
    assert (np.abs(np.where(qfin, Q - Qw, 0.0)) <= qbound).all()
    assert st["converged"] + st["unconverged"] + st["nonfinite"] == W * H

"""The kernels against closed-form radiometry (tests/closed_form_cases.py; the oracle's turn is tests/test_closed_form_host.py).

(a) f64 control: R.query_radiance on N copies of the case's ray (the radiance_kernel classes) and R.render through a pinhole camera
    that looks along the ray (the frame kernels; on the list scenes the lean kernel's primary pass and masks), in every family.
(b) RT_F32: R.render in every family, through render32 of test_f32_variant_gpu.py, which asserts the float instantiation ran.

N per case is the smallest power of two with 5 sigma / sqrt(N) <= 3e-4 E (1e-3 E for the cosine-only forms), in launches of at most
2^28 samples (128 x 128 pixels or 16384 rays, 16384 samples each; launch k under seed + k).  Asserted per channel:
    |mean - E| <= 5 sigma / sqrt(N) + r_T E,       sigma = sigma_rel * E from the case table (the oracle's, never the run's own),
and the spread of the per-pixel (per-ray) means is within 15 % of sigma / sqrt(samples per pixel): a wrong variance is a wrong
estimator too.  r_T is 0 for f64.

The camera.  vfov is chosen so small that the closed form varies by less than 2e-5 relative over the frame's footprint (asserted from
the four corner rays); the expectation is the centre's.

r_T for RT_F32, u = 2^-24: the rounded f32 operations between the draws and a sample's value, each at most u relative (a bound on
every sample, so on the mean).
  Direct light, rect lights (R1, R2, R3's rects, S2, T1), sample = L_e * rho * sc / pdf (rt_kernel.hip, the Lambertian arm):
    nd = normalized(dir): 3 products and 2 sums under a root (gamma_5 / 2 = 2.5 u), the root (0.5 u: halved by nothing, counted 1 u),
      one division per component (1 u): 4.5 u on every component, so on dot(n, nd) (n an axis: the dot itself is exact): 4.5 u
    sc = max(dot, 0) / pi: the division 1 u, pi as an f32 0.5 u: 1.5 u.  cpdf = cosine / pi is the same word where w = n.
    lpdf = t^2 |v|^2 / (cosine * area) (light_pdf_value): t = (k - o_k) / d_k 2 u, t * t 1 u, |v|^2 3 u, the product 1 u, cosine =
      |v_k| / length(v) 2.5 u + 1 u, area 3 u, cosine * area 1 u, the division 1 u, / n_lights 1 u: 16.5 u
    pdf = 0.5 lpdf + 0.5 cpdf: the halves exact, the sum 1 u; its error is at most the larger of its terms' plus 1 u: 17.5 u
    value: rho * sc 1 u, / pdf 1 u, L_e * beta 1 u: 3 u
    the hit point and the camera ray: p is off by at most 4 grid steps of its coordinates (u |p| each: o + t d, and the camera's
      corner and direction), and |grad ln E| is at most 1 / (distance to the light): 4 u |p| / h <= 8 u in every case here
    together 4.5 + 1.5 + 17.5 + 3 + 8 = 34.5 u: r_T = 35 u = 2.1e-6.
  Sphere lights (S1, R3's sphere) add the cancellation in 1 - cos_theta_max (sphere.rs:104-112): cos_theta_max carries 4 u (a
    squared length, a division, a difference, a root), which 1 - c magnifies by c / (1 - c) — 33 for S1, 121 for R3's sphere.  The
    pdf's cone and the sampled cone are the same rounded cone, so only its rim is weighted wrongly: at most that relative error times
    the sphere's share of E (1 for S1, 0.06 for R3).  r_T = 35 u + 4 u c / (1 - c) * share: 1.0e-5 for S1, 3.8e-6 for R3.
  The 0 / 1 cases: a sample is exact, the probability moves.  A draw is k 2^-24, so P(draw < x) is off by at most u absolute per
    decision; G1 has two decisions that matter (R1 at the top face, R2 below: the later ones carry R2^2 = 1.6e-3), and Schlick's value
    (normalize 4.5 u, a dot 3 u, 1 - c, five products, r0's 4, the sum: 16 u on R <= 0.07) moves p by 16 u * 0.07 / 0.93 = 1.2 u; the
    camera ray's direction (4 u) moves R1 by 0.26 * 4 u / 0.89 = 1.2 u: r_T = (2 / 0.89 + 1.2 + 1.2) u = 5 u.  M1: one decision
    (u / p absolute: 3.2 u at p = 0.32), and the chord (t1, t2 of the boundary, each about 4 u relative of 4, times |d| 1 u):
    density * 2 * 5 u * 4 = 20 u: r_T = 24 u.
These allowances are between 3e-7 and 1e-5 of E, a thirtieth of the statistical term at the most: they are the derivation's, not
a knob.  An f32 case that needs more is a finding (DESIGN.md D5 records what was found).

The colour check.  On the direct-light cases a sample is rho_c * X in every channel c with ONE random X (one scattering), so the
three means over rho_c agree up to rounding whatever X's noise is: |mean_c / E_c - mean_0 / E_0| <= 1e-12 in f64 (0.25 and 0.5
scale exactly, 0.75 X rounds: 2^-53 per sample) and <= r_T in f32.  A path that meets the receiver twice — a hit point behind its
own surface, re-hit by a grazing ray — carries rho_c^2 and breaks the proportion, so this check sees re-hits at 1e-6 where the mean
test resolves 3e-4.  (On the 0 / 1 cases the three channels are one number and the check is empty.)
  T1 in f32 is the one case that needs a derived term.  Its floor's vertices are 1000 away from the hit, and tri.rs's t =
  dot(s2, e2) / dot(s1, e1) cancels: s = o - v0 is ~1500 long, the products in cross(s, e1) . e2 reach 1500 * 2000 * 2000 = 6e9 and
  sum to |e1 x e2| h = 4e6, so t carries up to 6e9 * 2 u / 4e6 = 1.8e-4 relative, and the hit point lies up to d = 1.8e-4 off the
  plane.  From d below it, a cosine-sampled direction with cos < d / t_min (t_min = 0.001 in f32; probability (d / t_min)^2 = 0.032,
  and the cosine arm is taken half the time) meets the floor again: a share of up to 1.6e-2 of the paths, each of which may carry
  rho_c twice.  T1_REHIT = 1.6e-2 is that bound.  All the frame's rays are one ray up to the footprint, so the frame has ONE d:
  measured 6.7e-5 between the channels (share about 1.3e-4, d about 1.6e-5), within it.  f32 at that scale can give no more:
  the plane of three f32 vertices 1000 away is itself only defined to 6e-5."""
import math
import zlib

import numpy as np
import pytest

import closed_form_cases as CF
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Camera
from test_f32_variant_gpu import render32

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W = H = 128
SPP = 16384
LAUNCH = W * H * SPP                              # 2^28: the most one launch holds
LAUNCH_LIMIT_MS = 10000.0                         # a launch of 2^28 two-bounce paths takes tenths of a second; ten seconds is a fault
CASES = CF.cases()
PARAMS = [(name, family) for name, c in CASES.items() for family in c.families]


def r_t(case):
    """The rounding allowance of an RT_F32 frame of the case, relative to E (the module's docstring)."""
    def cone(spec, share):
        c = math.sqrt(1.0 - spec[1] ** 2 / sum((a - b) ** 2 for a, b in zip(spec[0], CF.R1_POINT)))
        return 4.0 * U * c / (1.0 - c) * share
    name = case.name
    if name == "G1":
        return 5.0 * U
    if name.startswith("M1"):
        return 24.0 * U
    if name.startswith("S1"):
        return 35.0 * U + cone(CF.S1_SPHERE, 1.0)
    if name.startswith("R3"):
        return 35.0 * U + cone(CF.R3_SPHERE, 0.06)
    return 35.0 * U


T1_REHIT = 1.6e-2


def colour_tol(case, f32):
    """The colour check's bound (the module's docstring)."""
    if not f32:
        return 1e-12
    return r_t(case) + (T1_REHIT if case.name == "T1" else 0.0)


def shape(case):
    """(launches, pixels a side, samples per pixel) for the case's N."""
    n = case.samples
    if n >= LAUNCH:
        return n // LAUNCH, W, SPP
    return 1, W, n // (W * H)


def seed_of(mode, name, family):
    """One fixed seed per assertion."""
    return zlib.crc32(f"{mode}/{name}/{family}".encode())


def camera(case):
    o, d = case.ray[0:3], case.ray[3:6] / np.linalg.norm(case.ray[3:6])
    t = float(case.ray[6])
    return Camera(tuple(o), tuple(o + case.focus * d), case.vup, case.vfov, 1.0, 0.0, case.focus, t, t)


def check(label, case, means, per_batch, allowance, kernel, ms, f32=False):
    """means (batches, 3): the assertions; the message carries z, the mean, E and the instantiation."""
    E, N = case.E, len(means) * per_batch
    sigma = case.sigma_rel * E
    mean = means.mean(axis=0)
    se = sigma / math.sqrt(N)
    z = (mean - E) / se
    spread = means.std(axis=0, ddof=1) / (sigma / math.sqrt(per_batch))
    colour = float(np.abs(mean / E - mean[0] / E[0]).max())
    text = (f"{label}: {kernel}, N = 2^{math.log2(N):.0f}, E = {E[0]:.10f}, mean = {mean[0]:.10f}, rel = {(mean[0] / E[0] - 1.0):+.2e}, "
            f"z = {z[0]:+.2f} / {z[1]:+.2f} / {z[2]:+.2f}, spread / sigma = {spread[0]:.4f}, r_T = {allowance:.1e}, colour = {colour:.1e}, "
            f"launches {len(ms)} x {np.mean(ms):.1f} ms (max {max(ms):.1f})")
    print(text)
    assert np.isfinite(means).all(), text
    assert (np.abs(mean - E) <= 5.0 * se + allowance * E).all(), text
    assert (np.abs(spread - 1.0) <= 0.15).all(), text
    assert colour <= colour_tol(case, f32), text
    assert max(ms) <= LAUNCH_LIMIT_MS, text


def test_footprints():
    """Over the frame's footprint the closed form varies by less than 2e-5 of the centre's value, which is the expectation."""
    for case in CASES.values():
        centre = case.value(case.ray)
        for ray in case.corner_rays(W):
            assert abs(float(case.value(ray) / centre - 1)) < 2e-5, case.name
        assert 0.0 < case.vfov < 0.01


@pytest.mark.parametrize("name,family", PARAMS)
def test_f64_radiance_query(pbe, name, family):
    """(a) rt_query_radiance: 16384 copies of the ray, 16384 samples of each, per launch."""
    case = CASES[name]
    launches, side, spp = shape(case)
    b, bg = case.make(pbe, family)
    rays = np.tile(case.ray, (side * side, 1))
    seed = seed_of("query", name, family)
    means, ms = [], []
    for k in range(launches):
        sums, nonfinite = R.query_radiance(b, rays, spp, CF.DEPTH, bg, seed + k)
        assert nonfinite == 0
        means.append(sums / spp)
        ms.append(R.last_query_ms(b))
    check(f"query f64 {name}/{family}", case, np.concatenate(means), spp, 0.0, f"radiance_kernel class {case.feats(family)}", ms)


def render64_sums(b, cam, bg, W, H, spp, depth, feats, seed):
    """render64 of test_f32_variant_gpu.py without the per-sample array (6 GB at these counts): the f64 frame, which must have run the
    instantiation named."""
    out = R.render(b, cam, bg, W, H, spp, depth, seed=seed)
    li = R.last_loop_info(b)
    assert li["kernel"] == f"rt::pathtrace_kernel<double, {feats}u>", li
    return out


def _frames(render, case, family, pbe, mode):
    """The case's launches through `render` -> (per-pixel means (pixels, 3), samples per pixel, the kernel that ran, kernel times)."""
    launches, side, spp = shape(case)
    b, bg = case.make(pbe, family)
    if case.base == CF.MESH:
        R.set_loop_shape(b, 0)                    # a mesh beside a list: the loop shape is otherwise measured per view (scheduling only)
    cam = camera(case)
    seed = seed_of(mode, case.name, family)
    means, ms = [], []
    for k in range(launches):
        out = render(b, cam, bg, side, side, spp, CF.DEPTH, case.feats(family), seed=seed + k)
        means.append(out.reshape(-1, 3) / spp)
        ms.append(R.last_kernel_ms(b))
    return np.concatenate(means), spp, R.last_loop_info(b)["kernel"], ms


@pytest.mark.parametrize("name,family", PARAMS)
def test_f64_frames(pbe, name, family):
    """(a) rt_render through the pinhole camera: the frame kernels, the double instantiation of the family."""
    case = CASES[name]
    means, spp, kernel, ms = _frames(render64_sums, case, family, pbe, "f64")
    check(f"frame f64 {name}/{family}", case, means, spp, 0.0, kernel, ms)


@pytest.mark.parametrize("name,family", PARAMS)
def test_f32_frames(pbe, name, family):
    """(b) RT_F32 through the same camera; render32 asserts that pathtrace_kernel<float, feats> of the family ran.

    R2_wall in the principled family is the case that found the f32 rect hit-point step (finalize_hit).  Before it,
    pathtrace_kernel<float, 127u> returned 155 ... 183 NaN samples of 2^28 on that scene under each of four seeds: a hit point that
    rounded to the far side of the wall at x = 555 (f32 grid 6e-5) was re-hit from behind by a grazing cosine-sampled ray, the path
    went on behind the wall and met the principled sphere that stands there, whose 0 / 0 cases give NaN.  The other families lost the
    same share of paths to a black background, which no mean can see."""
    case = CASES[name]
    means, spp, kernel, ms = _frames(lambda *a, **kw: render32(*a, want_samples=False, **kw), case, family, pbe, "f32")
    assert kernel == f"rt::pathtrace_kernel<float, {case.feats(family)}u>"
    check(f"frame f32 {name}/{family}", case, means, spp, r_t(case), kernel, ms, f32=True)

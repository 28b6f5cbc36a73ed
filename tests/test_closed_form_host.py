"""The CPU oracle against closed-form radiometry (tests/closed_form_cases.py): every case through orc.ray_color_paths at 2^24 samples, 1024
identical rays x 16384 samples.  Asserted per case and channel:
    |mean - E| <= 5 sigma / sqrt(N),    sigma = sigma_rel * E from the case table,
and the spread of the 1024 batch means is within 15 % of sigma / sqrt(N / 1024).  The second assertion is what pins sigma_rel, which the
GPU tests then take from the table (never from their own run).  The closed forms themselves are cross-checked here: Lambert's polygon
formula against the corner formula and against mpmath.quad, the sphere's against mpmath.quad.

The loose anchors of test_oracle_invariants.py stay as they are; these are the tight ones."""
import math
import time

import mpmath as mp
import numpy as np
import pytest

import closed_form_cases as CF
from oracle import orc

RAYS, SPP = 1024, 16384
CHUNK = 2048                                      # samples per call: (1024, 2048, 3) f64 = 48 MB
assert RAYS * SPP == CF.SIGMA_N


def oracle_batch_means(case, obe, family="none", seed=CF.SIGMA_SEED):
    """(1024, 3): the mean of the 16384 samples of each of 1024 copies of the case's ray (ray k, sample s on rng_path(seed, k, s))."""
    b, bg = case.make(obe, family)
    rays = np.tile(case.ray, (RAYS, 1))
    total = np.zeros((RAYS, 3))
    for first in range(0, SPP, CHUNK):
        s = orc.ray_color_paths(b, rays, CHUNK, bg, CF.DEPTH, seed, first_sample=first)
        if case.bernoulli:
            assert np.isin(s, (0.0, 1.0)).all(), f"{case.name}: a sample is neither 0 nor 1"
        total += s.sum(axis=1)
    return total / SPP


def check_mean_and_spread(name, batch_means, E, sigma_rel, n_per_batch):
    """The two assertions of the issue for an array of batch means (batches, 3) -> the text of the measured figures."""
    nb = len(batch_means)
    N = nb * n_per_batch
    mean = batch_means.mean(axis=0)
    sigma = sigma_rel * E
    z = (mean - E) / (sigma / math.sqrt(N))
    spread = batch_means.std(axis=0, ddof=1) / (sigma / math.sqrt(n_per_batch))
    text = (f"{name}: N = 2^{math.log2(N):.0f}, E = {E[0]:.10f}, mean = {mean[0]:.10f}, z = {z[0]:+.2f} / {z[1]:+.2f} / {z[2]:+.2f}, "
            f"sigma_rel = {sigma_rel:.4f}, measured / table = {spread[0]:.4f}")
    print(text)
    assert (np.abs(z) <= 5.0).all(), text
    assert (np.abs(spread - 1.0) <= 0.15).all(), text
    return text


@pytest.mark.parametrize("name", list(CF.cases()))
def test_oracle_against_the_closed_form(obe, name):
    case = CF.cases()[name]
    t = time.perf_counter()
    means = oracle_batch_means(case, obe)
    text = check_mean_and_spread(name, means, case.E, case.sigma_rel, SPP)
    print(f"  measured sigma_rel {means[:, 0].std(ddof=1) * math.sqrt(SPP) / case.E[0]:.4f}, {time.perf_counter() - t:.1f} s")
    assert text


def test_the_families_change_nothing(obe):
    """The family objects are out of every path's reach: with any of them the oracle gives the samples of the plain scene, word for word."""
    for name in ("R1", "R2", "S2", "G1"):
        case = CF.cases()[name]
        rays = np.tile(case.ray, (64, 1))
        want = None
        for family in case.families:
            b, bg = case.make(obe, family)
            got = orc.ray_color_paths(b, rays, 64, bg, CF.DEPTH, 3)
            if want is None:
                want = got
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, family)
        assert want.any()


def test_closed_forms_agree_with_each_other():
    """Lambert's formula = the corner formula = mpmath.quad for the rects; the sphere's formula = mpmath.quad; the values the issue states."""
    n = (0.0, 1.0, 0.0)
    for spec, p in ((CF.R1_LIGHT, CF.R1_POINT), (CF.R2_LIGHT, CF.R2_POINT), (CF.R3_LIGHT_B, CF.R1_POINT)):
        x0, x1, z0, z1, y, _ = spec
        lam = CF.polygon_cos_integral(p, n, CF._rect_verts(spec))
        px, py, pz = (mp.mpf(c) for c in p)          # (the differences in mpmath: x0 - p[0] in f64 is already rounded)
        corner = CF.rect_corner_integral(x0 - px, x1 - px, z0 - pz, z1 - pz, y - py)
        quad = CF.rect_quad_integral(p, n, x0, x1, z0, z1, y)
        assert abs(lam - corner) <= mp.mpf(10) ** -25 * lam and abs(quad - lam) <= mp.mpf(10) ** -12 * lam, (spec, lam, corner, quad)
    a, bh, h = 65.0, 52.5, 554.0                   # R2: 4 x the corner term
    assert abs(4 * CF.rect_corner_integral(0, a, 0, bh, h) - CF.polygon_cos_integral(CF.R2_POINT, n, CF._rect_verts(CF.R2_LIGHT))) < mp.mpf(10) ** -25
    assert float(CF.polygon_cos_integral(CF.R1_POINT, n, CF._rect_verts(CF.R1_LIGHT))) == pytest.approx(0.41083104137383, abs=1e-14)
    tilted = (0.1, 0.9, -0.2)                      # Lambert's formula under a normal that is not the rect's: against the plain integral
    lam = CF.polygon_cos_integral(CF.R1_POINT, tilted, CF._rect_verts(CF.R1_LIGHT))
    assert abs(CF.rect_quad_integral(CF.R1_POINT, tilted, *CF.R1_LIGHT[:5]) - lam) <= mp.mpf(10) ** -12 * lam
    for (c, r, _), nn in ((CF.S1_SPHERE, n), (CF.R3_SPHERE, n), (CF.S1_SPHERE, tilted)):
        s = CF.sphere_cos_integral(CF.R1_POINT, nn, c, r)
        assert abs(CF.sphere_quad_integral(CF.R1_POINT, nn, c, r) - s) <= mp.mpf(10) ** -12 * s
    cs = CF.cases()
    assert cs["R1"].E[0] == pytest.approx(0.13077158, abs=5e-9)
    assert cs["S1"].E[0] == pytest.approx(0.0569109, abs=5e-8)
    assert cs["G1"].E[0] == pytest.approx(0.8940590476, abs=5e-11)
    assert np.allclose(cs["S2"].E, cs["R1"].E, rtol=1e-12) and np.allclose(cs["T1"].E, cs["R1"].E, rtol=0, atol=0)
    assert cs["M1_sphere_d1"].E[0] == pytest.approx(math.exp(-0.5 * 2.0 * math.sqrt(0.95)), rel=1e-14)
    assert cs["M1_cube_d2"].E[0] == pytest.approx(math.exp(-0.5 * 2.0 / math.cos(math.radians(30.0))), rel=1e-14)
    assert cs["M1_sphere_d2"].E[0] == cs["M1_sphere_d1"].E[0]
    # R3: no light hides another — the sum of the irradiances is the expectation whatever the tree of `lights` looks like
    assert np.array_equal(cs["R3_flat"].E, cs["R3_nested"].E)


def test_sample_counts():
    """N per case: the smallest power of two with 5 sigma / sqrt(N) <= rel_tol * E; the figures the issue derives."""
    cs = CF.cases()
    for c in cs.values():
        n = c.samples
        assert 5.0 * c.sigma_rel / math.sqrt(n) <= c.rel_tol < 5.0 * c.sigma_rel / math.sqrt(n / 2), c.name
    assert cs["R1"].samples == 1 << 28 and cs["G1"].samples == 1 << 25

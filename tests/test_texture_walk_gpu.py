"""The texture walk on the device (rt_kernel.hip: tex_eval, perlin_noise, perlin_turb, sat_index, sat_u64) on hostile (u, v, p) of the
caller's, against the oracle's Texture::mapping (cases: tests/texture_cases.py; that they reach what they aim at, and that the oracle
obeys the same exact rules: tests/test_texture_walk_host.py).

A synthetic front-face record of a DiffuseLight goes through ONE call of shade_hit (rt_debug_shade, the all-features code shape) and
comes back with Texture::mapping(u, v, p) as its emitted colour.  What is required:
  * image lookups: 0 differing words — the texel index is integer arithmetic on identical inputs —, at u, v in {+-0, 1, 1 +- ulp, -ulp,
    2, -1, NaN, +-inf}, at every texel boundary +- 1 ulp, and on 2000 uniform (u, v) per image;
  * a checker's branch equals the one decided from the signs of the exact sines (mpmath, 160 bits) on EVERY case but those with a +-0
    argument or an underflowing product (at most 2 %, asserted on the host): a device sin within 1.3 ulp cannot flip a non-zero sine;
  * noise: everything before the final sin is + - x floor on identical inputs; for |scale p.z| <= 1e4 the sin's argument lies where
    DESIGN §6 measured both libms (device 0.754 ulp, glibc 0.56 ulp), so each channel is within 2^-52: 0.5 (0.754 + 0.56) ulp of a value
    in [0, 1], doubled for the rounding of 1 + sin.  Beyond that range the device's sin is measured here first (3000 log-uniform
    arguments in [1e4, 1e300] against mpmath, glibc beside it) and the bound is 0.5 (device max + glibc max) ulp(1), doubled.  NaN where
    the oracle has NaN;
  * a chain of 70 CheckTextures over an image on a sphere reads the image at the hit's own (u, v) (rt_query_albedo): the flattener's
    MAT_NEEDS_UV flag must see through a chain of any length."""
import functools

import numpy as np
import pytest

import texture_cases as T
from oracle import orc
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R

pytestmark = pytest.mark.gpu
SHADE_SEED = 1


@functools.lru_cache(None)
def _scenes():
    pb, ptex, pmats = T.build(_lib.load())
    ob, otex, omats = T.build(orc.load())
    assert {k: h.id for k, h in ptex.items()} == {k: h.id for k, h in otex.items()}
    assert {k: h.id for k, h in pmats.items()} == {k: h.id for k, h in omats.items()}
    return pb, ob, otex, omats


def _emitted(name, u, v, p):
    """(the device's emitted colour, the oracle's texture value) per case; orc_shade_batch's emitted colour must be the oracle's value too"""
    pb, ob, tex, mats = _scenes()
    rec, rays = T.records(mats[name].id, u, v, p)
    out = R.debug_shade(pb, rec, rays, seed=SHADE_SEED, shape="rest")
    assert (out[:, 13] == 1.0).all()
    want = T.oracle_values(ob, tex[name].id, u, v, p)
    ref, _ = orc.shade_batch(ob, rec, rays, seed=SHADE_SEED)
    assert T.same(ref[:, 10:13], want).all()
    return out[:, 10:13], want


@pytest.mark.parametrize("name", list(T.SMALL_IMAGES) + ["earth"])
def test_image_lookup_is_bit_identical(name):
    u, v, n_hostile = T.image_cases(name)
    p = np.random.RandomState(17).uniform(-3.0, 3.0, (len(u), 3))
    got, want = _emitted(name, u, v, p)
    bad = ~T.same(got, want).all(axis=1)
    print(f"{name}: {len(u)} lookups ({n_hostile} hostile), {int(bad.sum())} differ")
    assert not bad.any(), [(float(u[k]), float(v[k]), got[k].tolist(), want[k].tolist()) for k in np.flatnonzero(bad)[:5]]
    if name in T.SMALL_IMAGES:                                   # the device reached every texel itself
        w, h = T.SMALL_IMAGES[name]
        i, j = T.texel_of(got[:n_hostile])
        assert {(a, b) for a, b in zip(i, j)} == {(a, b) for a in range(w) for b in range(h)}


def test_checker_takes_the_branch_of_the_exact_sines():
    p = T.checker_points()
    odd, decided = T.checker_decisions()
    zero = np.zeros(len(p))
    got, want = _emitted("check2", zero, zero, p)
    took_odd = (got == np.array(T.CONSTS[0])).all(axis=1)
    assert (took_odd | (got == np.array(T.CONSTS[1])).all(axis=1)).all()
    wrong = decided & (took_odd != odd)
    print(f"checker: {len(p)} points, {int(decided.sum())} decided, {int(wrong.sum())} on the wrong branch, "
          f"{int((~decided & ~T.same(got, want).all(axis=1)).sum())} of the undecided differ from glibc's branch")
    assert not wrong.any(), p[np.flatnonzero(wrong)[:5]].tolist()
    # three deep: the same decision at every level; all leaves constants, so the oracle's words on every decided case
    got3, want3 = _emitted("check3", zero, zero, p)
    assert T.same(got3, want3).all(axis=1)[decided].all()
    assert {tuple(x) for x in got3[decided].tolist()} == {T.CONSTS[2], T.CONSTS[6]}


def _ulps_of_sin(shape):
    x = T.large_sin_arguments()
    dev = R.debug_math("sin", x, shape=shape)
    glibc = orc.libm("sin", x)
    assert np.isfinite(dev).all() and (np.abs(dev) <= 1.0).all()
    return float(T.sin_ulp_errors(dev, x).max()), float(T.sin_ulp_errors(glibc, x).max()), float((dev == glibc).mean())


@functools.lru_cache(None)
def _large_sin():
    """(device max ulp, glibc max ulp) of sin on [1e4, 1e300], the code shape rt_debug_shade's all-features form is compiled with"""
    d, g, _ = _ulps_of_sin("rest")
    return d, g


@pytest.mark.parametrize("shape", ["lean", "rest"])
def test_device_sin_on_large_arguments(shape):
    """The row DESIGN §6's table lacked: sin beyond the range of the kernels' other call sites, as a NoiseTexture far from the origin
    calls it.  The same requirement as tests/test_shade_kat_gpu.py::test_device_libm: within glibc's measured maximum + 2 ulp."""
    d, g, equal = _ulps_of_sin(shape)
    print(f"libm sin [1e4, 1e300] [{shape}]: device max {d:.3f} ulp, glibc max {g:.3f} ulp, {equal:.2%} of 3000 results bit-equal to glibc")
    assert d <= g + 2.0


def _noise_check(name, scale, got, want, p):
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all(), f"{name}: NaN / inf pattern differs"
    fin = np.isfinite(want).all(axis=1)
    small = T.in_measured_sin_range(scale, p) & fin
    large = ~T.in_measured_sin_range(scale, p) & fin
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want).max(axis=1)
    dev_max, glibc_max = _large_sin()
    bound_large = 0.5 * (dev_max + glibc_max) * np.spacing(1.0) * 2.0
    worst_small = float(d[small].max()) if small.any() else 0.0
    worst_large = float(d[large].max()) if large.any() else 0.0
    print(f"{name}: {int(small.sum())} cases in the measured range, max |d| = {worst_small * 2.0 ** 52:.3f} x 2^-52; {int(large.sum())} beyond it, "
          f"max |d| = {worst_large * 2.0 ** 52:.3f} x 2^-52 (bound {bound_large * 2.0 ** 52:.3f} x 2^-52); {int((~fin).sum())} non-finite; "
          f"{float(T.same(got, want).all(axis=1).mean()):.2%} bit-equal")
    assert worst_small <= 2.0 ** -52, p[small][np.argmax(d[small])].tolist()
    assert worst_large <= bound_large, p[large][np.argmax(d[large])].tolist()
    return int(small.sum()), int(large.sum())


@pytest.mark.parametrize("name", list(T.NOISE_SCALES))
def test_noise_on_lattice_points_saturating_indices_and_non_finite_points(name):
    scale = T.NOISE_SCALES[name]
    p = T.noise_points(scale)
    zero = np.zeros(len(p))
    got, want = _emitted(name, zero, zero, p)
    n_small, n_large = _noise_check(name, scale, got, want, p)
    assert n_small > 300 and (scale == 0.0 or n_large > 20)


def test_checker_over_an_image_and_a_noise_texture():
    """The mixed checker on the checker's own points, u and v uniform: the image's texel word for word where the exact sines say odd, the
    noise texture within its bounds where they say even (|4 p.z| reaches 1.3e5 here: both sin ranges)."""
    p = T.checker_points()
    odd, decided = T.checker_decisions()
    rs = np.random.RandomState(23)
    u, v = rs.uniform(0.0, 1.0, len(p)), rs.uniform(0.0, 1.0, len(p))
    got, want = _emitted("check_mixed", u, v, p)
    img = decided & odd
    assert img.sum() > 500 and T.same(got[img], want[img]).all()
    _, ob, tex, _ = _scenes()
    want_img = T.oracle_values(ob, tex["earth"].id, u[img], v[img], p[img])
    assert T.same(got[img], want_img).all()                      # and it IS the image's branch
    noise = decided & ~odd
    n_small, n_large = _noise_check("check_mixed (noise branch)", 4.0, got[noise], want[noise], p[noise])
    assert n_small > 100 and n_large > 100


def test_the_chain_walks_to_the_image_at_the_records_own_uv():
    u, v, _ = T.image_cases("img3x5")
    p = np.random.RandomState(5).uniform(-5.0, 5.0, (len(u), 3))
    got, want = _emitted("chain", u, v, p)
    assert T.same(got, want).all()
    assert len({tuple(x) for x in got.tolist()}) == 15


@pytest.mark.parametrize("n_checkers", [3, 64, 65, T.CHAIN])
def test_image_behind_a_chain_of_checkers_on_a_sphere(n_checkers):
    """Spheres whose Lambertian reads the earth map through a chain of CheckTextures (rt_query_albedo): the albedo is the oracle's texture
    value at the oracle's own record wherever u w and (1 - v) h are more than 2^-40 from an integer (sphere_uv goes through atan2 and
    acos, an ulp apart on the two sides), and at the device record's own u, v, p everywhere.  A flattener that does not see the image
    behind a long chain leaves (u, v) = (0, 0) in the record: one texel on every sphere."""
    pb, ptex, _ = T.chain_scene(_lib.load(), n_checkers)
    ob, tex, (w, h) = T.chain_scene(orc.load(), n_checkers)
    assert ptex == tex
    rays = T.chain_rays()
    albedo, hits = R.query_albedo(pb, rays, 1e-5, 3, want_hits=True)
    ref = orc.hit_records(ob, rays, 3)
    assert np.array_equal(hits[:, 0], ref[:, 0]) and (ref[:, 0] != 0.0).sum() > 1000
    hit = ref[:, 0] != 0.0
    own = T.oracle_values(ob, tex, hits[hit, 9], hits[hit, 10], hits[hit, 2:5])
    assert T.same(albedo[hit], own).all(), "the albedo is not the texture's value at the device record's own (u, v, p)"
    x, y = ref[hit, 9] * w, (1.0 - ref[hit, 10]) * h
    clear = (np.abs(x - np.rint(x)) > 2.0 ** -40) & (np.abs(y - np.rint(y)) > 2.0 ** -40)
    want = T.oracle_values(ob, tex, ref[hit, 9], ref[hit, 10], ref[hit, 2:5])
    bad = clear & ~T.same(albedo[hit], want).all(axis=1)
    print(f"chain of {n_checkers}: {int(hit.sum())} hits, {int(clear.sum())} clear of a texel boundary, {int(bad.sum())} differ from the oracle, "
          f"{len({tuple(a) for a in albedo[hit].tolist()})} distinct colours")
    assert clear.mean() > 0.99
    assert not bad.any(), f"{int(bad.sum())} albedos differ; device (u, v) of the first: {hits[hit][np.flatnonzero(bad)[0], 9:11].tolist()}"
    assert len({tuple(a) for a in want.tolist()}) > 100

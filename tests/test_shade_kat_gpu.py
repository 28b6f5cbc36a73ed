"""The shading side of rt_kernel.hip on the device, per function (csrc/rt_kat.hip: rt_debug_math, rt_debug_brdf, rt_debug_shade), under both
code shapes of the shared source — the lean list-scene unit's and the other unit's:

  * sincos_0_2pi and the device libm on the kernels' own argument ranges against mpmath (tests/shade_kat_cases.py; the host test measures
    glibc on the same sets): sincos_0_2pi within 1 ulp, each libm function within glibc's measured maximum + 2 ulp, special values of
    glibc's kind;
  * Vec3 / f64 in both forms against NumPy's `/`, onb_from_w against the oracle, the principled material's helpers against NumPy: 0
    differing words (GTR_1, which calls log2, within the bound its docstring derives);
  * pbr_brdf / brdf_pdf_value and ONE call of shade_hit against the oracle's one level of ray_color (orc_shade_batch): the stream's four
    words afterwards, done, depth_left and the NaN / inf pattern always exact; 0 differing words for the arms that call no libm function;
    the project's per-sample bound 1e-9 (1 + |ref|) on every output of the others, except for the inputs the oracle's margin marks
    (at most 1 % of a set: tests/test_shade_kat_host.py).

NaN: a quotient or a function value that is NaN is compared as NaN, not by its payload — x86 and the GPU produce different default NaNs."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import shade_kat_cases as K
from oracle import orc
from raytracinginrust_amd import render as R

pytestmark = pytest.mark.gpu
SHAPES = ("lean", "rest")


def differing(got, want):
    """words that differ, NaN compared as NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return int((~(K.same_words(got, want) | (np.isnan(got) & np.isnan(want)))).sum())


# ---------------------------------------------------------------- sincos_0_2pi
@pytest.mark.parametrize("shape", SHAPES)
def test_sincos_0_2pi(shape):
    r1, n_edge = K.r1_set()
    phi = 2.0 * K.PI * r1                                               # pdf.rs:12, as the kernel forms it
    got = R.debug_math("sincos_0_2pi", phi, shape=shape)
    with mpmath.workprec(K.MP_PREC):
        ex_s = [mpmath.sin(mpmath.mpf(float(x))) for x in phi]
        ex_c = [mpmath.cos(mpmath.mpf(float(x))) for x in phi]
    zs = [i for i, v in enumerate(ex_s) if v == 0]
    es = K.ulp_errors(got[:, 0], [v if v != 0 else None for v in ex_s])
    ec = K.ulp_errors(got[:, 1], ex_c)
    print(f"sincos_0_2pi [{shape}]: sin max {np.nanmax(es):.3f} ulp, cos max {np.nanmax(ec):.3f} ulp over {len(phi)} arguments")
    assert np.isfinite(got).all()
    assert np.nanmax(es) <= 1.0 and np.nanmax(ec) <= 1.0               # the bound the code's own comment claims (0.78)
    assert zs == [0] and K.words(got[0, 0]) == 0 and got[0, 1] == 1.0   # phi = 0: sin +0, cos 1
    sg = lambda v: -1 if v < 0 else 1
    for i in range(1, len(phi)):                                        # signs (the quadrant), everywhere: the boundaries are the first n_edge
        assert sg(got[i, 0]) == sg(ex_s[i]) and sg(got[i, 1]) == sg(ex_c[i]), (i, r1[i], got[i])
    lim = Fraction(4, 2 ** 53)
    worst = max(abs(Fraction(float(s)) ** 2 + Fraction(float(c)) ** 2 - 1) for s, c in got)
    print(f"sincos_0_2pi [{shape}]: max |sin^2 + cos^2 - 1| = {float(worst) * 2 ** 53:.3f} x 2^-53")
    assert worst <= lim
    assert n_edge == 52


# ---------------------------------------------------------------- the device libm
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(K.libm_sets()))
def test_device_libm(name, shape):
    fn, a, b = K.libm_sets()[name]
    exact = K.libm_exact(name)
    glibc = orc.libm(fn, a, b)
    dev = R.debug_math(fn, a, b, shape=shape)
    g, d = K.max_ulp(glibc, exact), K.max_ulp(dev, exact)
    equal = float((K.same_words(dev, glibc) | (np.isnan(dev) & np.isnan(glibc))).mean())
    print(f"libm {name} [{shape}]: device max {d:.3f} ulp, glibc max {g:.3f} ulp, {equal:.2%} of {len(a)} results bit-equal to glibc")
    bad = np.nonzero(K.kinds(dev) != K.kinds(glibc))[0]
    assert bad.size == 0, f"special values differ in kind at {a[bad[:5]].tolist()}: device {dev[bad[:5]].tolist()}, glibc {glibc[bad[:5]].tolist()}"
    assert d <= g + 2.0


# ---------------------------------------------------------------- Vec3 / f64
@pytest.mark.parametrize("shape", SHAPES)
def test_vector_division(shape):
    a, d, want_form = K.div_cases()
    out = R.debug_math("div3", a, d, shape=shape)
    with np.errstate(all="ignore"):
        want = a / d[:, None]
    assert differing(out[:, :3], want) == 0, f"{differing(out[:, :3], want)} quotients differ from NumPy's"
    form = out[:, 3]
    assert set(np.unique(form)) <= {0.0, 1.0}
    if shape == "lean":
        assert (form == 0.0).all()                                      # the lean unit divides three times
    else:
        assert (form[want_form == 1] == 1.0).all(), "ordinary operands must take the shared-denominator form"
        assert (form[want_form == 0] == 0.0).all(), "numerators whose v_div_scale disagree must take the plain divisions"
        print(f"div3 [rest]: {int(form.sum())} of {len(form)} lanes shared, {int((form[want_form == -1] == 0).sum())} of the extreme operands plain")


# ---------------------------------------------------------------- onb_from_w and the helpers
@pytest.mark.parametrize("shape", SHAPES)
def test_onb_from_w(shape):
    n = K.onb_normals()
    got = R.debug_math("onb_from_w", n, shape=shape)
    lib = orc.load().lib
    ref = np.zeros((len(n), 9))
    o9 = (orc.C.c_double * 9)()
    for i in range(len(n)):
        lib.orc_onb(orc._d(*n[i]), o9)
        ref[i] = list(o9)
    assert differing(got, ref) == 0
    w = ref[:, 6]
    assert (np.abs(w) > 0.9).any() and (np.abs(w) <= 0.9).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_brdf_helpers(shape):
    """+ - * / sqrt only: 0 differing words.  GTR_1 calls log2: with the oracle's log2 in the restatement, the device's value differs by
    log2's two errors — (D + G) ulp of log2 relative, D <= G + 2 by test_device_libm — carried through one multiplication and one
    division (1 ulp more): |got - want| <= (2 G + 3 + 1) ulp, G = glibc's measured maximum on these arguments."""
    cases = K.helper_cases()
    for name in ("GTR_2_aniso", "smithG_GGX", "smithG_GGX_aniso", "schlick_fresnel"):
        a, b = cases[name]
        got = R.debug_math(name, a, b, shape=shape)
        assert differing(got, K.np_helper(name, a, b)) == 0, name
    ndh, a = cases["GTR_1"]
    got = R.debug_math("GTR_1", ndh, a, shape=shape)
    a2 = a * a
    lg = orc.libm("log2", a2)
    with np.errstate(all="ignore"):
        want = np.where(a >= 1.0, 1.0 / K.PI, (a2 - 1.0) / (K.PI * lg * (1.0 + (a2 - 1.0) * ndh * ndh)))
    big = a >= 1.0
    assert big.sum() >= 3 and differing(got[big], want[big]) == 0      # a at 1, 1 + ulp, 2: the constant
    sm = ~big
    G = K.max_ulp(lg[sm], K._exact("log2", a2[sm], None))
    err = np.abs(got[sm] - want[sm]) / np.spacing(np.abs(want[sm]))
    print(f"GTR_1 [{shape}]: max {err.max():.2f} ulp from the restatement with glibc's log2 (glibc log2 max {G:.3f} ulp)")
    assert np.isfinite(got[sm]).all() and err.max() <= 2.0 * G + 4.0


# ---------------------------------------------------------------- pbr_brdf, brdf_pdf_value
@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(scene, lights):
        if (scene, lights) not in cache:
            pb, pm = K.make_scene(R._lib.load(), scene, lights)
            ob, om = K.make_scene(orc.load(), scene, lights)
            assert [h.id for h in pm["pbr"]] == [h.id for h in om["pbr"]] if scene == "full" else True
            cache[(scene, lights)] = (pb, ob, pm)
        return cache[(scene, lights)]
    return get


def _brdf_inputs(n, seed):
    """normals (axis-aligned, at the 0.9 boundary, random), r_in into the surface and r_out off it — or below the horizon — with
    |cosines| from 1e-6 up (no comparison of the BRDF within 1e-9 of its threshold), unnormalised"""
    r = np.random.default_rng(seed)
    rec, rays = K.synthetic_records([0], n, seed, graze=(1e-3, 1e-6))
    nrm, r_in = rec[:, 5:8], rays[:, 3:6]
    c = np.where(r.random(n) < 0.85, 1.0, -1.0) * np.where(r.random(n) < 0.2, 10.0 ** r.uniform(-6.0, -2.0, n), r.uniform(0.02, 1.0, n))
    t = np.cross(nrm, r.normal(size=(n, 3)))
    t /= np.sqrt((t * t).sum(1))[:, None]
    r_out = (np.sqrt(1.0 - c * c)[:, None] * t + c[:, None] * nrm) * 10.0 ** r.uniform(-3.0, 3.0, (n, 1))
    return r_in, r_out, nrm


@pytest.mark.parametrize("shape", SHAPES)
def test_brdf_against_the_oracle(scenes, shape):
    pb, ob, mats = scenes("full", "none")
    lib = orc.load().lib
    sets = K.pbr_sets()
    worst = 0.0
    n = 300
    for j, h in enumerate(mats["pbr"]):
        r_in, r_out, nrm = _brdf_inputs(n, 7600 + j)
        base = np.tile(np.array(sets[j][1]), (n, 1))
        got = R.debug_brdf(pb, h.id, r_in, r_out, nrm, base, shape=shape)
        ref = np.zeros((n, 4))
        o3 = orc._d(0, 0, 0)
        for i in range(n):
            lib.orc_brdf(ob.h, h.id, orc._d(*r_in[i]), orc._d(*r_out[i]), orc._d(*nrm[i]), o3)
            ref[i, :3] = list(o3)
            ref[i, 3] = lib.orc_brdf_pdf_value(ob.h, h.id, orc._d(*r_in[i]), orc._d(*r_out[i]), orc._d(*nrm[i]))
        ok = K.within(got, ref)
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.where(np.isfinite(ref), np.abs(got - ref) / (1.0 + np.abs(ref)), 0.0))
        worst = max(worst, float(rel))
        assert ok.all(), f"PBR set {j} {sets[j]}: {int((~ok).sum())} values beyond 1e-9 (1 + |ref|); first at record {np.nonzero(~ok.all(1))[0][:3].tolist()}"
        assert (ref[:, :3] == 0.0).all(1).any() and (ref[:, 3] > 0.0).any()          # below-horizon returns and ordinary values both occur
    print(f"brdf / brdf_pdf_value [{shape}]: max |got - ref| / (1 + |ref|) = {worst:.3e} over {len(sets)} parameter sets x {n}")


# ---------------------------------------------------------------- one bounce
def _classes(scene, lights, what, mats, rec, obe):
    """per record: True = an arm that calls no libm function (0 differing words), False = the per-sample bound"""
    ids = {k: v.id for k, v in mats.items() if k != "pbr"}
    exact_ids = [ids[k] for k in ("metal", "mirror", "light") + (("glass", "glass1", "iso") if scene == "full" else ())]
    exact = np.isin(rec[:, 11], exact_ids)
    if lights == "rect":                                                # Lambertian towards the rect light, with its whole mixture pdf
        lam = np.isin(rec[:, 11], [ids[k] for k in ("lam", "lam2") if k in ids])
        exact |= lam & K.first_draw_is_light(obe, K.SEED, len(rec))
    return exact


def _check(tag, got, ref, margin, exact):
    assert K.same_words(got[:, 15:19], ref[:, 15:19]).all(), f"{tag}: the stream afterwards differs on {int((~K.same_words(got[:, 15:19], ref[:, 15:19]).all(1)).sum())} records (the draw count)"
    assert (got[:, 13] == ref[:, 13]).all() and (got[:, 14] == ref[:, 14]).all(), f"{tag}: done / depth_left differ"
    assert (np.isnan(got) == np.isnan(ref)).all() and (np.isinf(got) == np.isinf(ref)).all(), f"{tag}: NaN / inf pattern differs"
    d = ~(K.same_words(got, ref) | (np.isnan(got) & np.isnan(ref)))
    assert not d[exact].any(), f"{tag}: {int(d[exact].sum())} words differ on arms that call no libm function; first record {np.nonzero(d.any(1) & exact)[0][:3].tolist()}"
    cmp_ = ~exact & (margin >= K.MARGIN)
    assert (~exact & ~cmp_).sum() <= K.MARGIN_CAP * len(got)
    ok = K.within(got[cmp_], ref[cmp_])
    with np.errstate(all="ignore"):
        rel = np.where(np.isfinite(ref[cmp_]), np.abs(got[cmp_] - ref[cmp_]) / (1.0 + np.abs(ref[cmp_])), 0.0)
    worst = float(rel.max()) if rel.size else 0.0
    assert ok.all(), f"{tag}: {int((~ok).sum())} values beyond 1e-9 (1 + |ref|), max {worst:.3e}; first record {np.nonzero(cmp_)[0][np.nonzero(~ok.all(1))[0][:3]].tolist()}"
    return worst, int(exact.sum()), int(cmp_.sum())


@pytest.mark.parametrize("name,scene,lights,what", K.bounce_sets())
def test_one_bounce_against_the_oracle(scenes, name, scene, lights, what):
    pb, ob, mats = scenes(scene, lights)
    rec, rays = K.set_records(what, mats, lambda r: R.query_hits(pb, r))
    assert len(rec) >= 500
    exact = _classes(scene, lights, what, mats, rec, orc.load())
    runs = [("rest", True)] + ([("lean", True), ("lean", False)] if scene == "list" else [])
    for flags in (0, R.RT_ISOTROPIC_SCATTER, R.RT_STOP_ON_ZERO):
        if flags == R.RT_ISOTROPIC_SCATTER and what not in ("exact",):
            continue
        ref, margin = orc.shade_batch(ob, rec, rays, seed=K.SEED, flags=flags)
        first = None
        for shape, table in runs:
            got = R.debug_shade(pb, rec, rays, seed=K.SEED, flags=flags, shape=shape, onb_table=table)
            worst, n_exact, n_cmp = _check(f"{name} flags {flags} {shape}{'' if table else ' no ONB table'}", got, ref, margin, exact)
            print(f"one bounce {name} flags {flags} [{shape}{'' if table else ', no ONB table'}]: {n_exact} records exact, {n_cmp} within the bound, max |got - ref| / (1 + |ref|) = {worst:.3e}")
            if first is None:
                first = got
            else:                                                       # the two code shapes, and the memo on and off: the same words on every input
                assert differing(got, first) == 0, f"{name}: {shape} (ONB table {table}) differs from {runs[0][0]}"
    assert exact.any() or what in ("lam", "pbr")


@pytest.mark.parametrize("scene,lights,what,shape", [("list", "rect", "real", "lean"), ("list", "rect", "listsyn", "rest"), ("full", "nested", "exact", "rest"),
                                                      ("full", "rect", "pbr", "rest")])
def test_beta_in_powers_of_two_scales_exactly(scenes, scene, lights, what, shape):
    pb, ob, mats = scenes(scene, lights)
    rec, rays = K.set_records(what, mats, lambda r: R.query_hits(pb, r))
    one = R.debug_shade(pb, rec, rays, seed=K.SEED, shape=shape)
    two = R.debug_shade(pb, rec, rays, beta=(2.0, 0.5, 4.0), seed=K.SEED, shape=shape)
    with np.errstate(all="ignore"):
        want = one.copy()
        want[:, 7:10] = one[:, 7:10] * np.array([2.0, 0.5, 4.0])
    tiny = (np.abs(want[:, 7:10]) < 2.0 ** -1000).any(1) & (want[:, 7:10] != 0.0).any(1)      # (a denormal product does not scale exactly)
    assert not tiny.any()
    assert differing(two, want) == 0

"""sphere_test, msphere_center, tri_test and the hit record finalize_hit builds for them (rt_kernel.hip) on the device, against the oracle
ray by ray, on the hostile rays of tests/primitive_cases.py (that those rays reach what they aim at, and that the oracle's own answers
are the exact ones wherever the case is clear: tests/test_primitive_hits_host.py).

Every scene form — the primitive alone in the world list, under Translate / Rotate / FlipNormal, as the leaves of a one-BVH world (16
and 300 spheres), as a BVH of triangles beside rect walls and beside triangles pushed into the list, as a ConstantMedium's boundary, as
BVHs inside a BVH — through rt_query_hits, which selects all three instantiations of rt_query.hip that can hold such primitives.
Required, on EVERY ray, clear or not: hit flag, t, position, normal, front_face and material handle identical to the oracle's record,
0 differing 64-bit words, any NaN matching any NaN (a ConstantMedium's hit goes through the device's log: there 1e-9 (1 + |ref|) and at
most 2 rays per batch, as tests/test_ray_query_gpu.py has it).  Every primitive has a material of its own, so the handle names the
primitive; object, primitive kind and primitive index must name one primitive each.  A triangle's u, v are the oracle's b1, b2 bit for
bit; a sphere's are within 2^-50 of the oracle's — DESIGN §6: the device's atan2 1.236 ulp, glibc's 0.501 ulp at |atan2| <= pi, one
rounding of + pi and the division: <= 3.8e-16, and 2^-50 is 2.3 times that — and exactly the oracle's 0 or 1 on the seam."""
import functools

import numpy as np
import pytest

import primitive_cases as P
import texture_cases as T
from oracle import orc
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Rng

from test_radiance_query_gpu import _check_samples, oracle_seed
from test_ray_query_gpu import MAX_BAD, SAMPLE_RTOL

pytestmark = pytest.mark.gpu

UV_BOUND = 2.0 ** -50
DEPTH, SPP, N_RADIANCE, RADIANCE_SEED = 3, 2, 1024, 2027


@functools.lru_cache(None)
def _product(name):
    S = P.build(name, _lib.load())
    assert S.things.keys() == P.oracle_scene(name).things.keys()
    return S


def _reads_uv(name, mats):
    things = P.oracle_scene(name).things
    return np.array([m >= 0 and things[int(m)][2] for m in mats])


def _differs(name, got, ref):
    """the mask of records that differ from the oracle's under the rules of the module docstring"""
    hit_g, hit_r = got[:, 0] != 0.0, ref[:, 0] != 0.0
    bad = hit_g != hit_r
    both = hit_g & hit_r
    medium = both & (got[:, 13] == -1.0)
    exact = P.same(got[:, 1:8], ref[:, 1:8]).all(axis=1)
    with np.errstate(invalid="ignore"):
        close = (np.abs(got[:, 1:8] - ref[:, 1:8]) <= SAMPLE_RTOL * (1.0 + np.abs(ref[:, 1:8]))).all(axis=1)
    bad |= both & ~np.where(medium, close, exact)
    bad |= both & (got[:, 8] != ref[:, 8])
    bad |= both & ~medium & (got[:, 11] != ref[:, 11])                  # the primitive, by its material
    bad |= medium & ((got[:, 11] != -1.0) | (got[:, 14] != -1.0) | (got[:, 12] < 0.0))
    bad |= ~hit_g & ((got[:, 0:11] != 0.0).any(axis=1) | (got[:, 11:15] != -1.0).any(axis=1))
    bad |= got[:, 15] != 0.0
    # u, v: 0 where the material reads none
    named = both & ~medium
    uv = named & _reads_uv(name, np.where(named, got[:, 11], -1.0))
    bad |= both & ~uv & (got[:, 9:11] != 0.0).any(axis=1)
    return bad, uv


@pytest.mark.parametrize("name", P.SCENES)
def test_hit_records_against_the_oracle(name, monkeypatch):
    S = _product(name)
    rays = np.ascontiguousarray(P.rays_of(name)[0])
    ref = P.oracle_hits(name)
    got = R.query_hits(S.b, rays, P.T_MIN, P.SEED)
    bad, _ = _differs(name, got, ref)
    hit = ref[:, 0] != 0.0
    print(f"{name}: {len(rays)} rays, {int(hit.sum())} hits, {int(np.isnan(ref[hit, 1]).sum())} with a NaN t, {int(bad.sum())} differ")
    assert bad.sum() <= (MAX_BAD if name in P.MEDIA_SCENES else 0), P.describe(name, bad)
    if name in P.BVH_SCENES:                                            # the tree in LDS whole, 8 nodes of it, none: where a node comes from changes no word
        assert R.flatten(S.b)["bvh_nodes"] > 8
        for limit in ("8", "0"):
            monkeypatch.setenv("RT_NODE_CACHE_MAX", limit)
            part = R.query_hits(S.b, rays, P.T_MIN, P.SEED)
            changed = (part.view(np.uint64) != got.view(np.uint64)).any(axis=1)
            assert not changed.any(), f"RT_NODE_CACHE_MAX={limit}: " + P.describe(name, changed)
        monkeypatch.delenv("RT_NODE_CACHE_MAX")


@pytest.mark.parametrize("name", [s for s in P.SCENES if s not in P.MEDIA_SCENES])
def test_object_and_primitive_index_name_one_primitive(name):
    """(object, primitive kind, primitive index) of a record and its material handle name each other: one triple per primitive, one
    primitive per triple, the kind that primitive's; a Mesh is one material over many triangles, so there only triple -> material."""
    S = _product(name)
    got = R.query_hits(S.b, np.ascontiguousarray(P.rays_of(name)[0]), P.T_MIN, P.SEED)
    hit = got[got[:, 0] != 0.0]
    by_triple, by_mat = {}, {}
    for rec in hit:
        triple, mat = tuple(rec[12:15].tolist()), int(rec[11])
        kind, what, _ = S.things[mat]
        assert rec[13] == P.KIND[kind], (triple, mat, kind)
        assert by_triple.setdefault(triple, mat) == mat, f"{name}: {triple} names materials {by_triple[triple]} and {mat}"
        if not (kind == "tri" and isinstance(what, str)):
            assert by_mat.setdefault(mat, triple) == triple, f"{name}: material {mat} is reported as {by_mat[mat]} and {triple}"
    print(f"{name}: {len(hit)} hits on {len(by_triple)} primitives of {len(S.things)}")
    assert len(by_triple) >= (1 if len(S.things) == 1 else 2)


def test_triangle_uv_are_the_barycentrics_bit_for_bit():
    name = "tri_alone"
    got = R.query_hits(_product(name).b, np.ascontiguousarray(P.rays_of(name)[0]), P.T_MIN, P.SEED)
    ref = P.oracle_hits(name)
    hit = ref[:, 0] != 0.0
    assert np.array_equal(got[:, 0] != 0.0, hit)
    assert P.same(got[hit, 9:11], ref[hit, 9:11]).all()
    assert np.isnan(ref[hit, 9:11]).any(axis=1).sum() >= 10 and (ref[hit, 9] == 0.0).sum() + (ref[hit, 10] == 0.0).sum() >= 1


def test_sphere_uv_at_the_poles_across_the_seam_and_everywhere_else():
    name = "sphere_origin"
    rays, fam, _, _ = P.rays_of(name)
    got = R.query_hits(_product(name).b, np.ascontiguousarray(rays), P.T_MIN, P.SEED)
    ref = P.oracle_hits(name)
    hit = ref[:, 0] != 0.0
    assert np.array_equal(got[:, 0] != 0.0, hit)
    g, r = got[hit, 9:11], ref[hit, 9:11]
    assert np.array_equal(np.isnan(g), np.isnan(r)), "NaN u, v where the oracle has none, or none where it has"
    fin = ~np.isnan(r)
    d = np.abs(np.where(fin, g, 0.0) - np.where(fin, r, 0.0))
    seam = fin[:, 0] & ((r[:, 0] == 0.0) | (r[:, 0] == 1.0))
    print(f"sphere u, v: {int(hit.sum())} hits, max |du| = {d[:, 0].max():.3e}, max |dv| = {d[:, 1].max():.3e} (bound {UV_BOUND:.3e}); "
          f"{int(np.isnan(r).any(axis=1).sum())} NaN; on the seam u = 0: {int((r[:, 0] == 0.0).sum())}, u = 1: {int((r[:, 0] == 1.0).sum())}; "
          f"{float(P.same(g, r).all(axis=1).mean()):.2%} bit-equal")
    assert d.max() <= UV_BOUND
    assert (g[seam, 0] == r[seam, 0]).all(), "u on the other side of the seam"
    assert (r[:, 0] == 0.0).sum() >= 10 and (r[:, 0] == 1.0).sum() >= 10 and np.isnan(r).any(axis=1).sum() >= 10


@pytest.mark.parametrize("name", ["sphere_origin", "tri_alone"])
def test_albedo_of_the_image_textured_primitives(name):
    """rt_query_albedo: the oracle's texture value at the DEVICE record's own (u, v, p), bit for bit; and at the ORACLE's own record
    wherever u w and (1 - v) h are more than 2^-40 from an integer (and u, v are numbers)."""
    S, O = _product(name), P.oracle_scene(name)
    rays = np.ascontiguousarray(P.rays_of(name)[0])
    albedo, hits = R.query_albedo(S.b, rays, P.T_MIN, P.SEED, want_hits=True)
    assert np.array_equal(hits.view(np.uint64), R.query_hits(S.b, rays, P.T_MIN, P.SEED).view(np.uint64))
    ref = P.oracle_hits(name)
    hit = ref[:, 0] != 0.0
    assert (albedo[~hit] == 1.0).all()
    tex = R.material_info(S.b, int(ref[hit, 11][0]))["texture"]
    own = T.oracle_values(O.b, tex, hits[hit, 9], hits[hit, 10], hits[hit, 2:5])
    assert T.same(albedo[hit], own).all()
    _, w, h = T.earth()
    with np.errstate(invalid="ignore"):
        x, y = ref[hit, 9] * w, (1.0 - ref[hit, 10]) * h
        clear = (np.abs(x - np.rint(x)) > 2.0 ** -40) & (np.abs(y - np.rint(y)) > 2.0 ** -40)
    want = T.oracle_values(O.b, tex, ref[hit, 9], ref[hit, 10], ref[hit, 2:5])
    bad = clear & ~T.same(albedo[hit], want).all(axis=1)
    print(f"{name}: {int(hit.sum())} hits, {int(clear.sum())} clear of a texel boundary, {int(bad.sum())} differ from the oracle's own record")
    assert clear.sum() >= 500 and not bad.any()


@functools.lru_cache(None)
def _oracle_radiance(name):
    obe = orc.load()
    ob = P.oracle_scene(name).b
    rays = P.rays_of(name)[0][:N_RADIANCE]
    out = np.zeros((len(rays), SPP, 3))
    for k, r in enumerate(rays):
        for s in range(SPP):
            out[k, s] = orc.ray_color(ob, r[0:3], r[3:6], r[6], P.BG, DEPTH, Rng(obe, oracle_seed(RADIANCE_SEED, k), s))
    return out


@pytest.mark.parametrize("name", P.RADIANCE_SCENES)
def test_paths_from_the_hostile_rays(name):
    """ray_color at depth 3, 2 samples of each of the first 1024 rays (rt_query_radiance), against the oracle's with the same streams:
    per sample |d| <= 1e-9 (1 + |ref|), NaN and inf where the oracle has them and nowhere else, at most 2 diverged samples."""
    rays = np.ascontiguousarray(P.rays_of(name)[0][:N_RADIANCE])
    ref = _oracle_radiance(name)
    _, samples, nonfinite = R.query_radiance(_product(name).b, rays, SPP, DEPTH, P.BG, RADIANCE_SEED, want_samples=True)
    _check_samples(name, samples, ref, MAX_BAD)
    assert nonfinite == int((~np.isfinite(samples)).any(axis=-1).sum())


@pytest.mark.parametrize("name", ["sphere_b", "mesh_room"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_batches(name, n):
    """one ray, a lane short of a wave, a wave, a lane more, a workgroup and a lane: n rays spread evenly over the batch, so that every
    family is among them (no media here: a ray's record depends on the ray alone)"""
    idx = np.linspace(0, len(P.rays_of(name)[0]) - 1, n).astype(int)
    rays = np.ascontiguousarray(P.rays_of(name)[0][idx])
    got = R.query_hits(_product(name).b, rays, P.T_MIN, P.SEED)
    bad, _ = _differs(name, got, P.oracle_hits(name)[idx])
    assert not bad.any(), f"{name}, {n} rays: {int(bad.sum())} differ, first {int(idx[np.flatnonzero(bad)[0]])}"

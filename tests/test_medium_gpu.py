"""ConstantMedium::hit on the device, ray by ray, against the restatement of tests/medium_cases.py fed with the DEVICE's own log.

A medium hit goes through m_log, which is not glibc's log: the older modules allow such records 1e-9 (1 + |ref|).  Here the log is taken
out of the comparison instead.  rt_debug_math("log") gives the device's m_log of every uniform a ray may draw — Rng(SEED, k)'s first
MAX_DRAWS numbers, under both code shapes, which must agree — and every other step of medium.rs:27-61 is + - x / sqrt and a comparison,
each rounded once.  So the restatement with that log must equal rt_query_hits' record on EVERY ray of every list scene, at every t_min of
T_MINS: hit flag, t, position, normal, front_face, u, v — 0 differing 64-bit words, any NaN matching any NaN; material and primitive
columns -1 on a medium hit and the object column the medium's item; an opaque item's record the oracle's, its handle the item's.  (That
the restatement is the reference's arithmetic, and that the rays reach what they aim at: tests/test_medium_host.py.)

BVH forms (media as BVH children, plain and under wrappers) are compared with the oracle's records: hit flag, the kind of thing hit and
which medium it is equal on all but MAX_BAD rays (tests/test_ray_query_gpu.py's rule), and on every other ray
|dt| <= 2^-50 |q| + 2^-52 |t|, q = hit_distance / len, and |dp_k| <= |dt| |d_k| + 2^-52 (|t d_k| + |p_k|) in the medium's frame: DESIGN §6 has the
device's log at 0.616 ulp and glibc's at 0.503, 1.12 ulp apart at the most; one rounding each of x, / and + makes 3.12 x 2^-52 |q| + 2^-52 |t|,
and the bound is 1.28 times that.  Under wrappers outside the medium the record's position is the medium's carried back up
(translate.rs:24-28, rotate.rs:88-104), which the issue's bound does not cover: there |dt| |d_k| is taken with the WORLD ray's d_k (dt
moves the point along the world ray; the direction through the rotation and back is the world's to 2^-51 |d|), and the rounding part,
2^-52 (|t d_k| + |p_k|) in the medium's frame, goes up through the wrappers with what each adds: a Rotate mixes two allowances with |c|, |s|
and adds 2^-52 (|c p_a| + |s p_b|), a Translate adds 2^-52 |p_k| (_carried).  The node cache (RT_NODE_CACHE_MAX 8 and 0) changes no word.

The stream after a medium: rt_query_radiance (depth 3, 2 samples of the first 1024 rays) and rt_render_samples (16 x 16 x 4) on
STREAM_SCENES with RT_ISOTROPIC_SCATTER, against the oracle with its Isotropic scattering, under the bounds of
tests/test_radiance_query_gpu.py and tests/test_shade_fill_gpu.py: a medium that draws when it should not shifts every later draw."""
import functools

import numpy as np
import pytest

import medium_cases as M
from oracle import orc
from raytracinginrust_amd import _lib
from raytracinginrust_amd import render as R
from raytracinginrust_amd.api import Camera, Rng

from test_radiance_query_gpu import _check_samples, oracle_seed
from test_ray_query_gpu import MAX_BAD

pytestmark = pytest.mark.gpu

DEPTH, SPP, N_RADIANCE, RADIANCE_SEED = 3, 2, 1024, 2029
FRAME = (16, 16, 4, 50, 43)                                            # W, H, spp, max_depth, seed


@functools.lru_cache(None)
def _product(name):
    return M.Scene(name, _lib.load())


@functools.lru_cache(None)
def _device_log(n):
    """m_log of uniforms(n) under both code shapes of rt_debug_math, which agree -> (n, MAX_DRAWS)"""
    u = M.uniforms(n).reshape(-1)
    lean, rest = R.debug_math("log", u, shape="lean"), R.debug_math("log", u, shape="rest")
    assert np.array_equal(lean.view(np.uint64), rest.view(np.uint64)), "the two code shapes of rt_debug_math give different logs"
    out = lean.reshape(n, M.MAX_DRAWS)
    out.setflags(write=False)
    return out


def _differs(got, want):
    """the mask of device records that are not the restated ones"""
    hit_g, hit_w = got[:, 0] != 0.0, want[:, 0] != 0.0
    bad = hit_g != hit_w
    both = hit_g & hit_w
    bad |= both & ~M.same(got[:, 1:9], want[:, 1:9]).all(axis=1)         # t, position, normal, front_face
    bad |= both & (got[:, 9:11] != 0.0).any(axis=1)                      # u, v: a medium's are 0, and no material here reads any
    bad |= both & (got[:, 11] != want[:, 11]) | both & (got[:, 12] != want[:, 12])
    medium = both & (want[:, 11] < 0.0)
    bad |= medium & ((got[:, 13] != -1.0) | (got[:, 14] != -1.0))
    bad |= both & ~medium & ((got[:, 13] < 0.0) | (got[:, 14] < 0.0))
    bad |= ~hit_g & ((got[:, 0:11] != 0.0).any(axis=1) | (got[:, 11:15] != -1.0).any(axis=1))
    bad |= got[:, 15] != 0.0
    return bad


def _carried(outer, p, e):
    """A rounding allowance e (n, 3) on a point p of the medium's frame, carried up through the wrappers outside the medium: a Rotate turns
    (e_a, e_b) into (|c| e_a + |s| e_b, |s| e_a + |c| e_b) and adds 2^-52 (|c p_a| + |s p_b|) for its two products and its sum on either
    side of the comparison (2^-53 each); a Translate adds 2^-52 |p + offset|."""
    for op in reversed(outer):
        if op[0] == "translate":
            p = p + np.array(op[1], np.float64)
            e = e + 2.0 ** -52 * np.abs(p)
        else:
            a, b = M._AB[op[1]]
            s, c = (abs(float(x)) for x in M._sin_cos(op[2]))
            e2 = e.copy()
            e2[:, a] = c * e[:, a] + s * e[:, b] + 2.0 ** -52 * (c * np.abs(p[:, a]) + s * np.abs(p[:, b]))
            e2[:, b] = s * e[:, a] + c * e[:, b] + 2.0 ** -52 * (s * np.abs(p[:, a]) + c * np.abs(p[:, b]))
            p, _, _ = M.op_back(op, p, p, p, None)
            e = e2
    return e


def _explain(name, t_min, got, res, bad):
    k = int(np.flatnonzero(bad)[0])
    lines = [M.describe(name, bad, t_min), f"  device   {got[k, :15].tolist()}", f"  restated {res['rec'][k, :15].tolist()}"]
    for i, I in res["info"].items():
        lines.append(f"  item {i}: t1 {I['t1'][k]!r} t2 {I['t2'][k]!r} closest {I['closest_in'][k]!r} drew {bool(I['drew'][k])} u {I['u'][k]!r} hd {I['hd'][k]!r} "
                     f"inside {I['inside'][k]!r} len {I['len'][k]!r}")
    return "\n".join(lines)


@pytest.mark.parametrize("name", M.LIST_SCENES)
def test_hit_records_word_for_word(name):
    S = _product(name)
    rays = np.ascontiguousarray(M.rays_of(name)[0])
    n = len(rays)
    log_u = _device_log(n)
    n_log = int((log_u.view(np.uint64) != M.glibc_log(n).view(np.uint64)).sum())
    for t_min in M.T_MINS:
        got = R.query_hits(S.b, rays, t_min, M.SEED)
        res = M.restate(name, t_min, log_u)
        bad = _differs(got, res["rec"])
        hit = got[:, 0] != 0.0
        print(f"{name}, t_min {t_min}: {n} rays, {int(res['drew'].sum())} draws, {int(hit.sum())} hits ({int((hit & (got[:, 11] < 0.0)).sum())} in a medium), "
              f"{n_log} of {log_u.size} logs differ from glibc's as words, {int(bad.sum())} records differ")
        assert not bad.any(), _explain(name, t_min, got, res, bad)


def test_the_comparison_resolves_the_log():
    """Fed glibc's log instead of the device's, the restatement does NOT equal the device's records: the logs differ in the last place on
    a few percent of the arguments, and that shows."""
    total = 0
    for name in ("sphere", "two_media", "in_out_rot"):
        rays = np.ascontiguousarray(M.rays_of(name)[0])
        got = R.query_hits(_product(name).b, rays, M.T_MINS[0], M.SEED)
        assert not _differs(got, M.restate(name, M.T_MINS[0], _device_log(len(rays)))["rec"]).any()
        n_bad = int(_differs(got, M.restate(name, M.T_MINS[0], M.glibc_log(len(rays)))["rec"]).sum())
        print(f"{name}: restated with glibc's log, {n_bad} of {len(rays)} records differ from the device's")
        total += n_bad
    assert total >= 10


@pytest.mark.parametrize("name", ["three_media_list", "opaque_between"])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_small_batches(name, n):
    """one ray, a lane short of a wave, a lane more, a workgroup and a lane: n rays spread over the batch — ray k of the SMALLER batch draws
    from Rng(SEED, k), so the restatement runs on that batch"""
    idx = np.linspace(0, len(M.rays_of(name)[0]) - 1, n).astype(int)
    rays = np.ascontiguousarray(M.rays_of(name)[0][idx])
    got = R.query_hits(_product(name).b, rays, M.T_MINS[0], M.SEED)
    res = M.restate(name, M.T_MINS[0], _device_log(len(M.rays_of(name)[0]))[:n], rays=rays)
    bad = _differs(got, res["rec"])
    assert not bad.any(), f"{name}, {n} rays: {int(bad.sum())} differ, first {int(np.flatnonzero(bad)[0])}"


# ---------------------------------------------------------------- BVH forms
@pytest.mark.parametrize("name", M.BVH_SCENES)
def test_bvh_forms_against_the_oracle(name, monkeypatch):
    S = _product(name)
    rays = np.ascontiguousarray(M.rays_of(name)[0])
    ref = M.oracle_world_hits(name, M.T_MINS[0])
    q = M.bvh_medium_terms(name)
    got = R.query_hits(S.b, rays, M.T_MINS[0], M.SEED)
    hit_g, hit_r = got[:, 0] != 0.0, ref[:, 0] != 0.0
    both = hit_g & hit_r
    med_g, med_r = both & (got[:, 11] < 0.0), both & (ref[:, 11] < 0.0)
    off = (hit_g != hit_r) | (med_g != med_r) | (both & ~med_r & (got[:, 11] != ref[:, 11]))
    # the object column names one medium, and the one the oracle's t belongs to
    obj_of = {}
    for k in np.flatnonzero(med_g & med_r & ~off):
        if obj_of.setdefault(int(got[k, 12]), int(q["item"][k])) != int(q["item"][k]):
            off[k] = True
    assert len(set(obj_of.values())) == len(obj_of) == 3, obj_of
    ok = both & ~off
    opaque = ok & ~med_r
    wrong = opaque & ~M.same(got[:, 1:9], ref[:, 1:9]).all(axis=1)
    m = ok & med_r
    wrong |= m & (~M.same(got[:, 5:9], ref[:, 5:9]).all(axis=1) | (got[:, 9:11] != 0.0).any(axis=1) | (got[:, 13] != -1.0) | (got[:, 14] != -1.0))
    sc = M.oracle_scene(name)
    with np.errstate(all="ignore"):
        dt = np.abs(got[:, 1] - ref[:, 1])
        t_bound = 2.0 ** -50 * np.abs(q["q"]) + 2.0 ** -52 * np.abs(ref[:, 1])
        wrong |= m & ~((dt <= t_bound) | M.same(got[:, 1], ref[:, 1]))                # (a NaN or an infinite t, or position: the same one)
        dp = np.abs(got[:, 2:5] - ref[:, 2:5])
        worst = 0.0
        for i in set(obj_of.values()):
            mi = m & (q["item"] == i)
            spec = sc.items[i]["spec"]
            o_recv, d_recv, _ = M.received(spec, rays)
            # the issue's bound with the WORLD ray's d_k (dt moves the point along the world ray) and, for the roundings, its 2^-52 (|t d_k| + |p_k|)
            # in the medium's frame carried up through the wrappers outside (_carried); no wrapper outside: the issue's bound as it stands
            p_bound = dt[:, None] * np.abs(rays[:, 3:6]) + _carried(spec[3], o_recv + ref[:, 1:2] * d_recv, 2.0 ** -52 * (np.abs(ref[:, 1:2] * d_recv) + np.abs(o_recv + ref[:, 1:2] * d_recv)))
            if spec[3]:
                p_bound = p_bound + dt[:, None] * 2.0 ** -51 * np.abs(d_recv).sum(axis=1, keepdims=True)      # (d through the rotation and back is the world's d to 2^-51 |d|)
            wrong |= mi & ~((dp <= p_bound) | M.same(got[:, 2:5], ref[:, 2:5])).all(axis=1)
            if mi.any():
                worst = max(worst, float(np.nanmax(np.where(mi[:, None] & (p_bound > 0.0) & np.isfinite(dp), dp / p_bound, 0.0))))
        rel = np.where(m & (t_bound > 0.0) & np.isfinite(dt), dt / t_bound, 0.0)
    print(f"{name}: {len(rays)} rays, {int(hit_r.sum())} hits, {int(med_r.sum())} in a medium (objects {obj_of}), {int(off.sum())} rays with another hit flag, kind or medium, "
          f"{int((m & M.same(got[:, 1], ref[:, 1])).sum())} medium t equal as words, largest |dt| / bound {float(np.nanmax(rel)):.3f}, largest |dp| / bound {worst:.3f}")
    assert off.sum() <= MAX_BAD, M.describe(name, off)
    assert not wrong.any(), M.describe(name, wrong)
    assert R.flatten(S.b)["bvh_nodes"] > 8
    for limit in ("8", "0"):
        monkeypatch.setenv("RT_NODE_CACHE_MAX", limit)
        part = R.query_hits(S.b, rays, M.T_MINS[0], M.SEED)
        changed = (part.view(np.uint64) != got.view(np.uint64)).any(axis=1)
        assert not changed.any(), f"RT_NODE_CACHE_MAX={limit}: " + M.describe(name, changed)
    monkeypatch.delenv("RT_NODE_CACHE_MAX")


# ---------------------------------------------------------------- the stream after a medium
@functools.lru_cache(None)
def _scattering_oracle(name):
    sc = M.Scene(name, orc.load())                                      # (a scene of its own: the flag is the scene's)
    orc.set_isotropic_scatters(sc.b, True)
    return sc


@functools.lru_cache(None)
def _oracle_radiance(name):
    obe = orc.load()
    ob = _scattering_oracle(name).b
    rays = M.rays_of(name)[0][:N_RADIANCE]
    out = np.zeros((len(rays), SPP, 3))
    for k, r in enumerate(rays):
        for s in range(SPP):
            out[k, s] = orc.ray_color(ob, r[0:3], r[3:6], r[6], M.BG, DEPTH, Rng(obe, oracle_seed(RADIANCE_SEED, k), s))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("name", M.STREAM_SCENES)
def test_paths_through_media(name):
    """ray_color at depth 3, 2 samples of each of the first 1024 rays (through and inside), Isotropic scattering on both sides"""
    rays = np.ascontiguousarray(M.rays_of(name)[0][:N_RADIANCE])
    ref = _oracle_radiance(name)
    assert ((ref != np.array(M.BG)).any(axis=-1)).mean() >= 0.25        # (paths that met something)
    _, samples, nonfinite = R.query_radiance(_product(name).b, rays, SPP, DEPTH, M.BG, RADIANCE_SEED, flags=R.RT_ISOTROPIC_SCATTER, want_samples=True)
    _check_samples(name, samples, ref, MAX_BAD)
    assert nonfinite == int((~np.isfinite(samples)).any(axis=-1).sum())


def _camera(name):
    c, radius = M.world_centre(M.SPECS[name][0])
    return Camera(tuple(c + np.array([0.3, 0.45, 1.5]) * radius), tuple(c), (0.0, 1.0, 0.0), 35.0, 1.0, 0.0, 10.0, 0.0, 1.0)


@functools.lru_cache(None)
def _oracle_frame(name):
    W, H, spp, depth, seed = FRAME
    _, rs, cnt = orc.render(_scattering_oracle(name).b, _camera(name), M.BG, W, H, spp, depth, seed=seed, want_samples=True, want_counters=True)
    rs.setflags(write=False)
    return rs, cnt


@pytest.mark.parametrize("name", M.STREAM_SCENES)
def test_frames_through_media(name):
    """rt_render_samples at 16 x 16 x 4: the frame kernels' media arms, per sample against the oracle"""
    W, H, spp, depth, seed = FRAME
    rs, cnt = _oracle_frame(name)
    assert cnt["medium_tests"] >= W * H * spp and ((rs != np.array(M.BG)).any(axis=-1)).mean() >= 0.25
    b = _product(name).b
    _, gs = R.render(b, _camera(name), M.BG, W, H, spp, depth, seed=seed, flags=R.RT_ISOTROPIC_SCATTER, want_samples=True)
    n_gpu = R.last_stats(b)["nonfinite_samples"]
    _check_samples(name + " frame", gs.reshape(-1, spp, 3), rs.reshape(-1, spp, 3), MAX_BAD)
    assert n_gpu == cnt["nonfinite"]

"""The oracle's side of the shading known-answer tests (tests/test_shade_kat_gpu.py runs the device's), no GPU:
the argument sets are deterministic; glibc — the libm the oracle is linked with — is measured on them against mpmath, max ulp per set;
orc_shade_batch, the one level of ray_color the device's shade_hit is compared with, is the code ray_color runs (depth 1: the emitted
term alone; depth 2 over a constant background the children miss into: e + w bg); and the inputs that the margin rule may take out of the
device comparison are at most 1 % of every set."""
import numpy as np
import pytest

import shade_kat_cases as K
from oracle import orc


def test_the_argument_sets_are_deterministic():
    first = {n: (v[1].copy(), None if v[2] is None else v[2].copy()) for n, v in K.libm_sets().items()}
    r1 = K.r1_set()[0].copy()
    div = [x.copy() for x in K.div_cases()]
    for f in (K.libm_sets, K.r1_set, K.div_cases):
        f.cache_clear()
    for n, v in K.libm_sets().items():
        assert K.same_words(first[n][0], v[1]).all() and (v[2] is None or K.same_words(first[n][1], v[2]).all()), n
    assert K.same_words(r1, K.r1_set()[0]).all()
    assert all(K.same_words(a, b).all() for a, b in zip(div, K.div_cases()))
    assert len(r1) == 3 + 49 + 8000 and len(K.pbr_sets()) >= 24


# glibc's own table of known maximum errors (the manual's "Errors in Math Functions", x86_64) has 1 or 2 ulp for each of these functions:
# a measurement above 2 would mean the measuring code is wrong, not glibc
GLIBC_CAP = 2.0


@pytest.mark.parametrize("name", list(K.libm_sets()))
def test_glibc_against_mpmath(name):
    fn, a, b = K.libm_sets()[name]
    got = orc.libm(fn, a, b)
    m = K.max_ulp(got, K.libm_exact(name))
    print(f"glibc {name}: max {m:.3f} ulp over {len(a)} arguments")
    assert m <= GLIBC_CAP


def _scene_cache():
    cache = {}

    def get(scene, lights):
        if (scene, lights) not in cache:
            cache[(scene, lights)] = K.make_scene(orc.load(), scene, lights)
        return cache[(scene, lights)]
    return get


@pytest.fixture(scope="module")
def scenes():
    return _scene_cache()


@pytest.mark.parametrize("name,scene,lights,what", K.bounce_sets())
def test_margin_share(scenes, name, scene, lights, what):
    """at most 1 % of any set has a libm-dependent comparison within 1e-9 of its threshold — by the oracle alone"""
    ob, mats = scenes(scene, lights)
    rec, rays = K.set_records(what, mats, lambda r: orc.hit_records(ob, r))
    assert len(rec) >= 500
    for flags in (0, 4):
        _, margin = orc.shade_batch(ob, rec, rays, seed=K.SEED, flags=flags)
        share = float((margin < K.MARGIN).mean())
        print(f"{name} flags {flags}: {len(rec)} records, margin < 1e-9 on {share:.4%}")
        assert share <= K.MARGIN_CAP


BG = (0.5, 2.0, 0.25)          # powers of two: (a / pdf) * bg is a * bg / pdf exactly


@pytest.mark.parametrize("scene,lights", [("list", "none"), ("list", "rect"), ("full", "none"), ("full", "rect"), ("full", "sphere"), ("full", "nested")])
def test_one_level_is_what_ray_color_runs_depth_1(scenes, scene, lights):
    """ray_color at depth 1 on a ray whose hit is the record: the emitted term only (the child call returns 0), bit for bit"""
    ob, mats = scenes(scene, lights)
    rays = K.real_rays(400, 7501)
    rec = orc.hit_records(ob, rays)
    keep = rec[:, 0] != 0.0
    rec, rays = rec[keep], rays[keep]
    out, _ = orc.shade_batch(ob, rec, rays, seed=K.SEED, depth_left=1)
    assert (out[:, 13] == 1.0).all()                                    # depth_left 1: every path ends here
    for k in range(len(rec)):
        c = np.array(orc.ray_color_path(ob, rays[k, 0:3], rays[k, 3:6], rays[k, 6], BG, 1, K.SEED, k))
        e = out[k, 10:13]
        scattered = out[k, 14] == 0.0
        want = np.zeros(3) + e if not scattered else e + out[k, 7:10] * 0.0          # emitted + w * 0 (inf * 0 = NaN where the reference has it)
        assert ((c == want) | (np.isnan(c) & np.isnan(want))).all(), (k, c, want)
    assert (out[:, 14] == 0.0).any() and (out[:, 10:13] != 0.0).any()


def _one_rect_scene(kind):
    """one big rect of one material in empty space, no lights: every child ray misses into the background"""
    from raytracinginrust_amd.api import SceneBuilder
    b = SceneBuilder(orc.load())
    tex = b.ConstantTexture((0.6, 0.7, 0.8))
    p, base = K.pbr_sets()[0]
    m = {"lam": lambda: b.Lambertian(tex), "metal": lambda: b.Metal((0.8, 0.85, 0.88), 0.3), "glass": lambda: b.Dielectric(1.5),
         "light": lambda: b.DiffuseLight(tex), "iso": lambda: b.Isotropic(tex), "pbr": lambda: b.PBR(b.ConstantTexture(base), *p)}[kind]()
    w = b.HittableList()
    w.push(b.AARect(1, -1000.0, 1000.0, -1000.0, 1000.0, 0.0, m))
    b.set_scene(w, [])
    return b


@pytest.mark.parametrize("kind", ["lam", "metal", "glass", "light", "iso", "pbr"])
def test_one_level_is_what_ray_color_runs_depth_2(kind):
    """ray_color at depth 2 where the child misses: e + w bg with orc_shade_batch's e and w"""
    ob = _one_rect_scene(kind)
    r = np.random.default_rng(7502)
    n = 150
    o = r.uniform(-300.0, 300.0, (n, 3)); o[:, 1] = r.uniform(1.0, 200.0, n) * r.choice([-1.0, 1.0], n)
    t = r.uniform(-400.0, 400.0, (n, 3)); t[:, 1] = 0.0
    rays = np.concatenate([o, t - o, np.zeros((n, 1))], 1)
    rec = orc.hit_records(ob, rays)
    assert (rec[:, 0] == 1.0).all()
    for flags in ((0, 4) if kind == "iso" else (0,)):
        orc.set_isotropic_scatters(ob, bool(flags & 4))
        out, _ = orc.shade_batch(ob, rec, rays, seed=K.SEED, depth_left=2, flags=flags)
        for k in range(n):
            c = np.array(orc.ray_color_path(ob, rays[k, 0:3], rays[k, 3:6], rays[k, 6], BG, 2, K.SEED, k))
            scattered = out[k, 14] == 1.0
            with np.errstate(all="ignore"):
                want = out[k, 10:13] + (out[k, 7:10] * np.array(BG) if scattered else 0.0)
            assert ((c == want) | (np.isnan(c) & np.isnan(want))).all(), (k, c, want)
        if kind in ("lam", "glass", "pbr") or (kind == "iso" and flags):
            assert (out[:, 14] == 1.0).all()
        if kind == "light" or (kind == "iso" and not flags):
            assert (out[:, 13] == 1.0).all() and (out[:, 14] == 2.0).all()

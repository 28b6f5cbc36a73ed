"""The loop that fills the oracle's libm table (oracle.cpp orc_lm, orc.libm_table_*), shared by tests/test_libm_replay_host.py (no GPU)
and tests/test_libm_replay_gpu.py.

The oracle routes every libm call that has a counterpart in the kernels through one hook, and each site names the device function the
kernel calls at the same place.  With a table set, the hook computes with the table's value for (op, operand words); an operand it does
not find goes to a miss list.  replay() runs an oracle batch, evaluates the misses with the caller's `device_math` — the device's own
libm through rt_debug_math on the GPU, glibc on the host — extends the table and runs again until a run misses nothing.  What the last
run returns is the reference's arithmetic on the device's libm values: a kernel that follows the reference's expression order equals it
word for word.

Later operands depend on earlier results (tan -> atan -> sin, cos; a checker's branch chooses the colour pow sees), so a set needs one
round per dependent generation, plus the one that finds nothing missing.  MAX_ROUNDS keeps a bug from looping forever; it is no tolerance."""
import numpy as np

import medium_cases as M
import primitive_cases as P
import shade_kat_cases as K
import texture_cases as T
from oracle import orc

MAX_ROUNDS = 8


class Counts(dict):
    """{op: (entries in the table, entries whose value differs from glibc's as words)}; .rounds: oracle runs made; .stats: the last
    run's {op: (lookups, matches)}; .operands: {op: (a, b) of the entries}"""
    rounds = 0
    stats = None
    operands = None


def same(a, b):
    """64-bit words, NaN equal to NaN"""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def differing_records(got, want):
    """rows with at least one differing word -> bool (n,)"""
    return ~same(got, want).reshape(len(got), -1).all(axis=1)


def host_math(op, a, b):
    """device_math of the host: the libm the oracle is linked with, per op as the product's rt_debug_math numbers them"""
    if op == "sincos_0_2pi":
        return np.stack(orc.sincos(a), 1)
    return orc.libm(op, a, b)


def glibc_of_site(op, a, b, g):
    """device_math that hands back what the oracle itself computed at the missing site (replay passes it as `g`): the hook then changes
    nothing.  (Where the kernel calls sin and cos of one operand, glibc's side is one sincos call, which host_math's sin / cos is not.)"""
    return g if op == "sincos_0_2pi" else g[:, 0]


def replay(run_oracle, device_math, label=None, wants_glibc=False):
    """-> (run_oracle()'s output under a table filled by device_math, Counts).  run_oracle(): one oracle batch (any of orc.shade_batch,
    orc.hit_records, orc.brdf ...; called once per round, its inputs must not change); device_math(op, a, b) -> values (n,), or (n, 2) for
    sincos_0_2pi; b is None where the op has one operand.  wants_glibc: device_math(op, a, b, g) also gets the oracle's own glibc values.
    The table is cleared before and after."""
    counts = Counts()
    held, operands = {}, {}
    orc.libm_table_clear()
    try:
        orc.libm_table_extend("sin", np.zeros(0), None, np.zeros(0))          # an empty table: everything misses
        for rnd in range(1, MAX_ROUNDS + 1):
            out = run_oracle()
            counts.stats, size = orc.libm_stats()
            misses = orc.libm_misses()
            if not misses:
                break
            for op, (a, b, g) in misses.items():
                two = op in orc.TABLE_TWO_OPERANDS
                v = np.asarray(device_math(op, a, b if two else None, g) if wants_glibc else device_math(op, a, b if two else None), np.float64)
                if op == "sincos_0_2pi":
                    assert v.shape == (len(a), 2), (op, v.shape)
                    orc.libm_table_extend(op, a, None, v[:, 0], v[:, 1])
                    diff = ~same(v, g).all(axis=1)
                else:
                    assert v.shape == (len(a),), (op, v.shape)
                    orc.libm_table_extend(op, a, b if two else None, v)
                    diff = ~same(v, g[:, 0])
                operands.setdefault(op, []).append((a, b))
                e, d = held.get(op, (0, 0))
                held[op] = (e + len(a), d + int(diff.sum()))
        else:
            raise AssertionError(f"{label}: the libm table still misses {sum(len(m[0]) for m in misses.values())} operands after {MAX_ROUNDS} rounds")
        counts.rounds = rnd
        counts.update(held)
        counts.operands = {op: (np.concatenate([x[0] for x in v]), np.concatenate([x[1] for x in v])) for op, v in operands.items()}
        assert size == sum(e for e, _ in held.values())                       # every miss was a new key
        assert all(l == m for l, m in counts.stats.values())                  # the last run found every operand
        if label is not None:
            print(f"libm replay {label}: {rnd} rounds; entries (differing from glibc) " + ", ".join(f"{op} {e} ({d})" for op, (e, d) in counts.items()))
        return out, counts
    finally:
        orc.libm_table_clear()


def merge(total, counts):
    """add one set's Counts into a running {op: [entries, differing]}"""
    for op, (e, d) in counts.items():
        t = total.setdefault(op, [0, 0])
        t[0] += e; t[1] += d
    return total


# ---------------------------------------------------------------- the sets both test files run (the oracle's side of each)
STOP_ON_ZERO, ISOTROPIC_SCATTER = 2, 4                           # the product's RT_STOP_ON_ZERO, RT_ISOTROPIC_SCATTER; orc_shade_batch's flags
HOSTILE_SETS = [("hostile sphere", "full", "sphere", "hostile"), ("hostile nested", "full", "nested", "hostile")]
TEXTURE_SHADE_SEED = 1
UV_SCENES = P.SPHERE_SETS + ("chain3",)                          # sphere scenes; chain3: four spheres under an image behind three checkers
MEDIA_SCENES = ("sphere", "cube", "tetra", "union")              # one per boundary family: a sphere, six rects, four triangles, a list of two shapes
BRDF_N = 300


def bounce_sets():
    """K.bounce_sets() and the sphere light on hostile shading points"""
    return K.bounce_sets() + HOSTILE_SETS


def bounce_flags(what):
    """as tests/test_shade_kat_gpu.py::test_one_bounce_against_the_oracle runs them"""
    return (0, ISOTROPIC_SCATTER, STOP_ON_ZERO) if what == "exact" else (0, STOP_ON_ZERO)


def bounce_records(what, mats, hits_fn):
    if what == "hostile":
        rec, rays, _ = K.sphere_light_records(mats)
        return rec, rays
    return K.set_records(what, mats, hits_fn)


def run_bounce(ob, rec, rays, what):
    """-> run_oracle: orc_shade_batch under every flag of the set, (flags, n, 19)"""
    return lambda: np.stack([orc.shade_batch(ob, rec, rays, seed=K.SEED, flags=f)[0] for f in bounce_flags(what)])


def texture_sets():
    """name -> (texture, u, v, p): the checker at the zeros of sin(10 p), three deep, over an image and a noise texture; the marble at
    the points of texture_cases.py"""
    p = T.checker_points()
    zero = np.zeros(len(p))
    rs = np.random.RandomState(23)
    sets = {"checker": ("check2", zero, zero, p), "checker three deep": ("check3", zero, zero, p),
            "checker over an image and a noise texture": ("check_mixed", rs.uniform(0.0, 1.0, len(p)), rs.uniform(0.0, 1.0, len(p)), p)}
    for name, scale in T.NOISE_SCALES.items():
        q = T.noise_points(scale)
        sets["marble " + name] = (name, np.zeros(len(q)), np.zeros(len(q)), q)
    return sets


def run_texture(ob, rec, rays):
    return lambda: orc.shade_batch(ob, rec, rays, seed=TEXTURE_SHADE_SEED)[0]


def uv_scene(name, be):
    """-> (builder, rays, seed) of a sphere scene whose records carry u, v"""
    if name == "chain3":
        return T.chain_scene(be, 3)[0], np.ascontiguousarray(T.chain_rays()), 3
    return P.build(name, be).b, np.ascontiguousarray(P.rays_of(name)[0]), P.SEED


def media_scene(name, be):
    return M.Scene(name, be).b, np.ascontiguousarray(M.rays_of(name)[0]), M.SEED


def run_hits(ob, rays, seed):
    return lambda: orc.hit_records(ob, rays, seed)


def brdf_inputs():
    """(r_in, r_out, normal) (sets, BRDF_N, 3) each: tests/test_shade_kat_gpu.py's _brdf_inputs for every parameter set"""
    from test_shade_kat_gpu import _brdf_inputs
    return [np.stack(x) for x in zip(*[_brdf_inputs(BRDF_N, 7600 + j) for j in range(len(K.pbr_sets()))])]


def run_brdf(ob, pbr_ids, r_in, r_out, nrm):
    """-> run_oracle: orc_brdf and orc_brdf_pdf_value of every parameter set, (sets, BRDF_N, 4)"""
    lib = orc.load().lib

    def run():
        ref = np.zeros(r_in.shape[:2] + (4,))
        o3 = orc._d(0, 0, 0)
        for j, mat in enumerate(pbr_ids):
            for i in range(r_in.shape[1]):
                a = (orc._d(*r_in[j, i]), orc._d(*r_out[j, i]), orc._d(*nrm[j, i]))
                lib.orc_brdf(ob.h, mat, a[0], a[1], a[2], o3)
                ref[j, i, :3] = o3[:]
                ref[j, i, 3] = lib.orc_brdf_pdf_value(ob.h, mat, a[0], a[1], a[2])
        return ref
    return run

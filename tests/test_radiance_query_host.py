"""Radiance queries, the parts that need no GPU: the panorama's rays, the identity that lets the oracle draw a path's stream, the two
symbols and their declarations, and the "no HIP device" error of both entry points."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import orc
from raytracinginrust_amd import _abi, _lib
from raytracinginrust_amd import render as R
from raytracinginrust_amd import scenes
from raytracinginrust_amd.api import Rng

G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def oracle_seed(seed, k):
    """seed' with for_stream(seed', s) == for_path(seed, k, s): the host streams' key is pixel 0xFFFFFFFF (csrc/rt_rng.h)."""
    return (seed + 2 * G * (((k - 0xFFFFFFFF) << 32) & M64)) & M64


def test_equirect_rays_known_values():
    W, H = 8, 4
    o = (1.0, 2.0, 3.0)
    rays = R.equirect_rays(o, W, H, time=0.25)
    assert rays.shape == (H * W, 7) and rays.dtype == np.float64
    assert (rays[:, 0:3] == o).all() and (rays[:, 6] == 0.25).all()
    assert np.allclose(np.linalg.norm(rays[:, 3:6], axis=1), 1.0, rtol=0, atol=4e-16)
    # output order: row 0 is the top row (looking up), rows run down; columns run from +x towards +z
    img = rays.reshape(H, W, 7)
    assert (img[0, :, 4] > 0.9).all() and (img[-1, :, 4] < -0.9).all() and (np.diff(img[:, 0, 4]) < 0.0).all()
    for r in range(H):
        for i in range(W):
            t, p = math.pi * (r + 0.5) / H, 2.0 * math.pi * (i + 0.5) / W
            assert img[r, i, 3:6].tolist() == [math.sin(t) * math.cos(p), math.cos(t), math.sin(t) * math.sin(p)]
    # towards the poles as H grows; the four cardinal directions at the equator of an odd-offset grid
    tall = R.equirect_rays(o, 4, 2000).reshape(2000, 4, 7)
    assert tall[0, 0, 4] > 1.0 - 1e-6 and tall[-1, 0, 4] < -1.0 + 1e-6
    eq = R.equirect_rays((0.0, 0.0, 0.0), 8, 1)                      # theta = pi / 2; phi = pi / 8 + k pi / 4
    assert np.allclose(eq[:, 4], 0.0, atol=1e-16)
    card = R.equirect_rays((0.0, 0.0, 0.0), 4, 1)[:, 3:6]            # phi = 45, 135, 225, 315 degrees
    h = math.sqrt(0.5)
    assert np.allclose(card, [[h, 0, h], [-h, 0, h], [-h, 0, -h], [h, 0, -h]], atol=1e-15)
    fine = R.equirect_rays((0.0, 0.0, 0.0), 4000, 1)[:, 3:6]         # the columns next to phi = 0, 90, 180, 270 degrees
    for col, want in [(0, (1, 0, 0)), (1000, (0, 0, 1)), (2000, (-1, 0, 0)), (3000, (0, 0, -1))]:
        assert np.allclose(fine[col], want, atol=1e-3) and np.allclose(fine[col - 1], want, atol=1e-3)


def test_seed_identity_against_the_oracles_streams(obe, pbe):
    """rt_rng_path(seed, k, s) — the stream sample s of ray k draws from — is the oracle's Rng(seed', s)."""
    rs = np.random.RandomState(11)
    ks = [0, 1, 2, 63, 64, 1092, 0x7FFFFFFE, 0x7FFFFFFD] + [int(x) for x in rs.randint(0, 0x7FFFFFFF, 20)]
    ss = [0, 1, 4, 999, 0xFFFFFFFE, 0xFFFFFFFD] + [int(x) for x in rs.randint(0, 0xFFFFFFFF, 6, dtype=np.int64)]
    words = (C.c_uint32 * 4)()
    for seed in (0, 2025, M64, int(rs.randint(0, 1 << 62))):
        for k in ks:
            for s in ss:
                pbe.fn("rng_path")(seed, k, s, words)
                state = list(words)
                # the oracle's host stream Rng(seed', s) is keyed as the path (seed', pixel 0xFFFFFFFF, sample s)
                obe.fn("rng_path")(oracle_seed(seed, k), 0xFFFFFFFF, s, words)
                assert list(words) == state, (seed, k, s)
    a, b = Rng(obe, oracle_seed(2025, 77), 5), Rng(pbe, oracle_seed(2025, 77), 5)
    assert [a.gen_f64() for _ in range(8)] == [b.gen_f64() for _ in range(8)]


def test_symbols_are_exported_and_declared():
    lib = _lib.load().lib
    for name in ("query_radiance", "query_radiance_device"):
        assert name in _abi.SIGNATURES
        fn = getattr(lib, "rt_" + name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(_abi.SIGNATURES[name][1])
    assert len(_abi.SIGNATURES["query_radiance"][1]) == 11 and len(_abi.SIGNATURES["query_radiance_device"][1]) == 15
    assert callable(R.query_radiance) and callable(R.query_radiance_device) and callable(R.equirect_rays)


def test_no_device_error():
    if R.device_count() > 0:
        pytest.skip("a HIP device is present: the GPU tests cover the entry points")
    pb, _, bg = scenes.cornell_box(_lib.load())
    rays = np.array([[278.0, 278.0, -800.0, 0.0, 0.0, 1.0, 0.0]])
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.query_radiance(pb, rays, 2, 4, bg)
    buf = np.zeros(16)                                               # (never dereferenced: the device check comes first)
    base = (buf.ctypes.data + 15) & ~15
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.query_radiance_device(pb, 1, base, base, 2, 4, bg, d_rgb_sum_bytes=24)
    # the argument checks come before the device's, as for every entry point
    with pytest.raises(R.RenderError, match="samples_per_ray"):
        R.query_radiance(pb, rays, 0, 4, bg)

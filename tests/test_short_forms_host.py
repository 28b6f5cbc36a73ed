"""The exact short forms of the lean f64 kernel (csrc/rt_short.h) on the host: the header is compiled into a stand-alone program
(tests/short_forms_main.cpp) with -ffp-contract=off, and everything is compared bit for bit with the expression each form stands for —
`/`, the U01 of rt_rng.h, the reference's |dot(v, n)|.  The kernel calls these very functions (tests/test_short_forms_gpu.py runs them
on the device)."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("short_forms") / "short_forms_main"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "short_forms_main.cpp")])
    out = subprocess.check_output([str(exe)], text=True)
    return {k: float(v) for k, v in (line.split() for line in out.splitlines())}


def test_enable_rule(report):
    """on for pi, 799, 2159, 3839, 1079; off for 1919, 399, 63 and a divisor of 0 (and for negative, non-finite and out-of-range divisors);
    2^53 rho as the rule computes it — one fma — for four of them"""
    assert report["rule_on"] == 5 and report["rule_off"] == 4 and report["rule_rejects_hostile"] == 1
    assert report["pi_reciprocal_is_the_literal"] == 1
    assert (report["rho_pi"], report["rho_799"], report["rho_1919"], report["rho_63"]) == (0.206, 0.240, 0.778, 0.500)


def test_enabled_divisors_are_pinned(report):
    """W - 1 for W in [3, 8192] with 2^53 |RN(1/C) C - 1| < 1/2: 5739 of the 8190 (222 more sit at exactly 1/2 and 2229 above it, counted
    with exact rationals)"""
    assert report["enabled_wm1_up_to_8192"] == 5739


def test_division_equals_the_quotient(report):
    """pi and every enabled W - 1 <= 8191; numerators in [0, 1), i + U01 with i < 2^15, exponents down to 2^-63, and within +-3 ulp of
    quotient midpoints: at least 10^8 operands, 0 differing — while x * zh alone differs on a good share of them"""
    assert report["div_operands"] >= 1e8 and report["div_operands_pi"] >= 3.9e6
    assert report["div_differing"] == 0
    assert report["div_product_alone_differing"] > 0.1 * report["div_operands"]


def test_division_guard_cases(report):
    """+0, -0, numerators below 2^-900, denormals, NaN, +-inf (and negative or huge numbers): each is outside the served range — the plain
    path — or equals `/`; none of them is served; the range's two ends are served and exact, and -0 is a trap indeed"""
    assert report["guard_ok"] == report["guard_cases"] == 16 and report["guard_served"] == 0
    assert report["range_ends_ok"] == 1 and report["minus_zero_is_the_trap"] == 1


def test_u01_without_conversions(report):
    assert report["u01_words"] == 1e7 and report["u01_differing"] == 0 and report["u01_spec_copy_differing"] == 0
    assert report["u01_edges_ok"] == report["u01_edges"] >= 4 and report["u01_of_all_ones_below_one"] == 1


def test_rect_light_absdot(report):
    """short against full on random finite v, every pattern of +-0 components among them; for v with a NaN or infinite component (or an
    overflowing length) the guard selects the full form — and the forms do differ there"""
    assert report["lpdf_vectors"] == 2e6 and report["lpdf_differing"] == 0
    assert report["lpdf_guard_cases"] == 45 and report["lpdf_guard_missed"] == 0 and report["lpdf_forms_differ_without_guard"] > 0

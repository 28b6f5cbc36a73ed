// tests/short_forms_main.cpp — stand-alone host program over csrc/rt_short.h (tests/test_short_forms_host.py compiles and runs it with
// -ffp-contract=off): the very functions the lean f64 kernel calls, compared bit for bit with the expressions they stand for.  Prints
// `name value` lines; the test asserts on them.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>
#include "../raytracinginrust_amd/csrc/rt_rng.h"
#include "../raytracinginrust_amd/csrc/rt_short.h"

using namespace rt;

static bool same(double a, double b) { return sf_bits(a) == sf_bits(b); }
static double pow2(int e) { return std::ldexp(1.0, e); }

// ---- division: numerators of four kinds against `/`, for one enabled divisor.  Returns the number of differing quotients.
static uint64_t g_operands = 0, g_product_alone_differs = 0;
static uint64_t check_divisor(double C, double zh, Rng& g, uint32_t per_kind) {
    uint64_t bad = 0;
    auto one = [&](double x) {
        if (!(x == 0.0 || sf_in_range(x)) || std::signbit(x)) return;       // (a midpoint walk may leave the served range: not an operand)
        g_operands++;
        const double want = x / C;
        if (!same(sf_div3(x, C, zh), want)) bad++;
        if (!same(x * zh, want)) g_product_alone_differs++;
    };
    for (uint32_t i = 0; i < per_kind; i++) {
        one(rng_u01(g, 0.0));                                                   // [0, 1)
        one((double)(rng_u32(g) >> 17) + rng_u01(g, 0.0));                      // i + U01, i < 2^15: the camera's numerators
        one(rng_range(g, 1.0, 2.0) * pow2(-(int)(rng_u32(g) >> 26)));           // exponents down to 2^-63
        // within +-3 ulp of a quotient's rounding midpoint: q a random quotient, x ~ C (q + ulp(q) / 2)
        const double q = rng_range(g, 1.0, 2.0) * pow2((int)(rng_u32(g) >> 27) - 16);
        const double half_ulp = (std::nextafter(q, std::numeric_limits<double>::infinity()) - q) * 0.5;
        const double xm = std::fma(C, q, C * half_ulp);
        uint64_t w = sf_bits(xm) - 3u;
        for (int k = 0; k < 7; k++) one(sf_from_bits(w + (uint64_t)k));
    }
    return bad;
}

int main() {
    // ---- the host's enable rule
    const double on_list[] = {SF_PI, 799.0, 2159.0, 3839.0, 1079.0}, off_list[] = {1919.0, 399.0, 63.0, 0.0};
    int rule_on = 0, rule_off = 0;
    for (double C : on_list) { const double zh = sf_recip_for(C); rule_on += (zh != 0.0 && same(zh, 1.0 / C)) ? 1 : 0; }
    for (double C : off_list) rule_off += sf_recip_for(C) == 0.0 ? 1 : 0;
    std::printf("rule_on %d\nrule_off %d\n", rule_on, rule_off);
    std::printf("rule_rejects_hostile %d\n", (int)(sf_recip_for(-3.0) == 0.0 && sf_recip_for(std::nan("")) == 0.0 && sf_recip_for(INFINITY) == 0.0 &&
                                                    sf_recip_for(pow2(-40)) == 0.0 && sf_recip_for(pow2(40)) == 0.0 && sf_recip_for(5e-324) == 0.0));
    std::printf("pi_reciprocal_is_the_literal %d\n", (int)same(sf_recip_for(SF_PI), SF_RCP_PI));
    std::printf("rho_pi %.3f\nrho_799 %.3f\nrho_1919 %.3f\nrho_63 %.3f\n", 0x1.0p53 * std::fabs(std::fma(1.0 / SF_PI, SF_PI, -1.0)),
                0x1.0p53 * std::fabs(std::fma(1.0 / 799.0, 799.0, -1.0)), 0x1.0p53 * std::fabs(std::fma(1.0 / 1919.0, 1919.0, -1.0)),
                0x1.0p53 * std::fabs(std::fma(1.0 / 63.0, 63.0, -1.0)));
    int enabled = 0;
    for (uint32_t W = 3; W <= 8192; W++) enabled += sf_recip_for((double)(W - 1u)) != 0.0 ? 1 : 0;
    std::printf("enabled_wm1_up_to_8192 %d\n", enabled);

    // ---- division: pi and every enabled W - 1 <= 8191
    Rng g = rng_for_stream(0x5F0A5ull, 1u);
    uint64_t bad = check_divisor(SF_PI, SF_RCP_PI, g, 400000u);
    const uint64_t pi_operands = g_operands;
    for (uint32_t W = 2; W <= 8192; W++) {
        const double C = (double)(W - 1u), zh = sf_recip_for(C);
        if (zh != 0.0) bad += check_divisor(C, zh, g, 1800u);
    }
    std::printf("div_operands %llu\ndiv_operands_pi %llu\ndiv_differing %llu\ndiv_product_alone_differing %llu\n", (unsigned long long)g_operands,
                (unsigned long long)pi_operands, (unsigned long long)bad, (unsigned long long)g_product_alone_differs);

    // ---- division, guard cases: each must be outside sf_in_range (the plain path) or equal `/`
    const double guards[] = {0.0, -0.0, pow2(-901), pow2(-900) * 0.999, 5e-324, 2.2250738585072014e-308 * 0.5, pow2(-1022), std::nan(""), -std::nan(""),
                             INFINITY, -INFINITY, -1.0, -pow2(-900), pow2(900), pow2(1000), 1.7976931348623157e308};
    int guard_ok = 0, guard_n = 0, guard_served = 0;
    for (double x : guards) {
        guard_n++;
        const bool served = sf_in_range(x);
        guard_served += served ? 1 : 0;
        const double q = sf_div3(x, SF_PI, SF_RCP_PI), want = x / SF_PI;
        guard_ok += (!served || same(q, want)) ? 1 : 0;
    }
    // the range's own ends are served and exact; +0 is not in the range, yet the three instructions are exact on it (the camera's numerators)
    const bool ends = sf_in_range(pow2(-900)) && sf_in_range(std::nextafter(pow2(900), 0.0)) && !sf_in_range(std::nextafter(pow2(-900), 0.0)) &&
                      same(sf_div3(pow2(-900), SF_PI, SF_RCP_PI), pow2(-900) / SF_PI) && same(sf_div3(std::nextafter(pow2(900), 0.0), SF_PI, SF_RCP_PI), std::nextafter(pow2(900), 0.0) / SF_PI) &&
                      same(sf_div3(pow2(-900), 0x1.0p32, sf_recip_for(0x1.0p32)), pow2(-932)) && same(sf_div3(0.0, 799.0, sf_recip_for(799.0)), 0.0);
    // -0 is the trap: the three instructions give +0 where `/` gives -0 — the reason it must not be served
    const bool minus_zero_trap = !same(sf_div3(-0.0, SF_PI, SF_RCP_PI), -0.0 / SF_PI) && !sf_in_range(-0.0);
    std::printf("guard_cases %d\nguard_ok %d\nguard_served %d\nrange_ends_ok %d\nminus_zero_is_the_trap %d\n", guard_n, guard_ok, guard_served, (int)ends, (int)minus_zero_trap);

    // ---- U01: the three additions against rt_rng.h's rng_u01 on the same words
    uint64_t u01_bad = 0, u01_spec_bad = 0; const uint32_t u01_n = 10000000u;
    for (uint32_t i = 0; i < u01_n; i++) {
        Rng g2 = g;
        const double spec = rng_u01(g, 0.0);
        const uint64_t u = rng_u64(g2);
        if (!same(sf_u01(u), spec)) u01_bad++;
        if (!same(sf_u01_spec(u), spec)) u01_spec_bad++;
    }
    const uint64_t edges[] = {0ull, ~0ull, 0x7FFull, ~0x7FFull, 0x800ull, 0xFFFFF80000000000ull, 0x000007FFFFFFF800ull, 0x0000080000000000ull, 1ull << 63};
    int edge_ok = 0, edge_n = 0;
    for (uint64_t u : edges) { edge_n++; edge_ok += same(sf_u01(u), sf_u01_spec(u)) ? 1 : 0; }
    std::printf("u01_words %u\nu01_differing %llu\nu01_spec_copy_differing %llu\nu01_edges %d\nu01_edges_ok %d\nu01_of_all_ones_below_one %d\n", u01_n, (unsigned long long)u01_bad,
                (unsigned long long)u01_spec_bad, edge_n, edge_ok, (int)(sf_u01(~0ull) < 1.0 && sf_u01(0ull) == 0.0));

    // ---- the rect light's |dot(v, n)|: short against full on finite v, every pattern of +-0 components included; the whole pdf too
    uint64_t lp_bad = 0, lp_n = 0, lp_guard_bad = 0, lp_guard_n = 0, lp_differs_unguarded = 0;
    for (uint32_t i = 0; i < 2000000u; i++) {
        double v[3];
        for (int a = 0; a < 3; a++) v[a] = rng_range(g, -1.0, 1.0) * pow2((int)(rng_u32(g) >> 27) - 16);
        const uint32_t pat = i % 64u;                   // bits 0-2: which components are zero, bits 3-5: their signs (as all signs flip)
        if (i < 1000000u) for (int a = 0; a < 3; a++) { if ((pat >> a) & 1u) v[a] = 0.0; if ((pat >> (3 + a)) & 1u) v[a] = -v[a]; }
        const uint32_t k = rng_index(g, 3u);
        const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double t = rng_range(g, 0.001, 1000.0), area = rng_range(g, 0.5, 20000.0);
        lp_n++;
        if (!sf_finite(len)) { lp_bad++; continue; }
        const double s = sf_rect_absdot_short(v[0], v[1], v[2], k), f = sf_rect_absdot_full(v[0], v[1], v[2], k);
        if (!same(s, f) || !same(sf_rect_pdf_tail(s, len, t, area), sf_rect_pdf_tail(f, len, t, area))) lp_bad++;
    }
    const double nonfinite[] = {std::nan(""), INFINITY, -INFINITY, 1e200, -1e200};       // (1e200: finite components, an infinite length: full form too)
    for (int a = 0; a < 3; a++)
        for (double x : nonfinite)
            for (uint32_t k = 0; k < 3; k++) {
                double v[3] = {0.25, -0.5, 0.125}; v[a] = x;
                const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                lp_guard_n++;
                if (sf_finite(len)) lp_guard_bad++;                                       // the guard must select the full form
                if (!same(sf_rect_absdot_short(v[0], v[1], v[2], k), sf_rect_absdot_full(v[0], v[1], v[2], k))) lp_differs_unguarded++;
            }
    std::printf("lpdf_vectors %llu\nlpdf_differing %llu\nlpdf_guard_cases %llu\nlpdf_guard_missed %llu\nlpdf_forms_differ_without_guard %llu\n", (unsigned long long)lp_n,
                (unsigned long long)lp_bad, (unsigned long long)lp_guard_n, (unsigned long long)lp_guard_bad, (unsigned long long)lp_differs_unguarded);
    return 0;
}

// csrc/rt_short.h — exact short forms for f64 arithmetic whose second operand is a constant of the scene or the frame (host + device).
//
// The lean f64 list-scene kernel (rt_kernel.hip, SHORT_FORMS) uses them in place of the compiler's 11-instruction IEEE divide, of two
// int -> f64 conversions and of two dot products with a 0/1 axis vector.  Every form returns the very bits of the expression it stands
// for whenever its stated conditions hold; the callers test the conditions (wave-uniformly) and run the plain expression otherwise.
// rt_rng.h stays the spec of U01.  tests/test_short_forms_host.py compiles this header into a stand-alone program and compares bit for
// bit; everything here must be compiled without contraction (-ffp-contract=off): the fma calls are the only fused operations.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_SF __host__ __device__ __forceinline__
#else
#define RT_SF inline
#endif

namespace rt {

RT_SF double sf_from_bits(uint64_t b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
RT_SF uint64_t sf_bits(double d) { uint64_t b; __builtin_memcpy(&b, &d, 8); return b; }

// ------------------------------------------------------------------ x / C in three instructions, C a constant
// With zh = RN(1/C) (one IEEE division, done once on the host):
//     q  = RN(x * zh)
//     r  = fma(-C, q, x)          (exact, see below)
//     q' = fma(r, zh, q)
// q' = RN(x / C).  This is Markstein's correction step (P. Markstein, "Computation of elementary functions on the IBM RISC System/6000
// processor", 1990; Muller et al., Handbook of Floating-Point Arithmetic, "division by a constant"): in binary round-to-nearest, if
//   (a) zh is within half an ulp of 1/C,
//   (b) q is a FAITHFUL rounding of x/C (one of the two neighbours of x/C, or x/C itself), and
//   (c) nothing underflows or overflows,
// then r = x - C q is representable (so the fma delivers it exactly) and RN(q + r zh) is the correctly rounded quotient.
// (a) holds because zh is a correctly rounded division.  (b): x zh - x/C = (x/C)(zh C - 1), so with rho = |zh C - 1| the product x zh
// is off by less than 2^53 rho ulp of x/C (|x/C| < 2^53 ulp), and its rounding adds at most half an ulp: q is faithful whenever
//     2^53 rho < 1/2.
// rho itself is computed exactly by ONE fma(zh, C, -1.0): zh C is within 2^-53 of 1, so the integer zC - 2^k behind it is below 2^53 and
// representable.  sf_recip_for enables the short form for a divisor only under that condition (pi: 0.206; 799: 0.240; 1919: 0.778 and
// 399, 63: exactly 0.5 are refused) and returns 0 otherwise — the callers branch on the zero, wave-uniformly, to the plain division.
// (c): the divisor is held to [2^-32, 2^32] and the numerator to +0 or [2^-900, 2^900): q is then a normal number above 2^-933, r —
// a multiple of ulp(C) ulp(q) >= 2^-1069 — is representable, and nothing reaches 2^1024.  A numerator of +0 gives q = r = q' = +0 = 0 / C.
// The traps the callers own: -0 (the three instructions give +0, `/` gives -0), negative numbers, denormals, NaN, infinities and anything
// below 2^-900 are NOT served: sf_in_range is the test, one unsigned comparison on the high dword.
RT_SF double sf_recip_for(double C) {
    if (!(C >= 0x1.0p-32 && C <= 0x1.0p32)) return 0.0;          // 0, negative, NaN, infinite or out of the range of (c): plain division
    const double zh = 1.0 / C;
    const double rho = __builtin_fabs(__builtin_fma(zh, C, -1.0));
    return (0x1.0p53 * rho < 0.5) ? zh : 0.0;
}
RT_SF double sf_div3(double x, double C, double zh) {
    const double q = x * zh;
    const double r = __builtin_fma(-C, q, x);
    return __builtin_fma(r, zh, q);
}
// 2^-900 <= x < 2^900 (positive, normal): the high dword of x in [0x07B00000, 0x78300000).  A set sign bit (negative numbers, -0), +0,
// denormals, infinities and NaNs all fall outside.
RT_SF bool sf_in_range(double x) { return (uint32_t)(sf_bits(x) >> 32) - 0x07B00000u < 0x78300000u - 0x07B00000u; }
static constexpr double SF_PI = 3.14159265358979323846264338327950288;      // the kernels' PI_T in f64
static constexpr double SF_RCP_PI = 0x1.45f306dc9c883p-2;                    // RN(1 / SF_PI); sf_recip_for(SF_PI) returns it (2^53 rho = 0.206)

// ------------------------------------------------------------------ U01 of rt_rng.h without conversions
// rt_rng.h: U01 = ((double)hi21 * 2^32 + (double)lo32) * 2^-53 with v = u >> 11, hi21 = v >> 32, lo32 = (uint32_t)v — two conversions,
// a product, a sum, a product: five f64-rate instructions, every one exact.  The same value from three additions, every one exact:
//     lo  = bits(0x3FE00000_00000000 | lo32) - 0.5      bits(..) = 1/2 + lo32 2^-53 (one ulp in [1/2, 1) is 2^-53)
//     hi  = bits(0x41E00000_00000000 | hi21) - 2^31     bits(..) = 2^31 + hi21 2^-21 (one ulp in [2^31, 2^32) is 2^-21; hi21 < 2^21)
//     U01 = hi + lo                                     = (hi21 2^32 + lo32) 2^-53, a 53-bit integer times 2^-53
RT_SF double sf_u01(uint64_t u) {
    const uint64_t v = u >> 11;
    const double lo = sf_from_bits(0x3FE0000000000000ULL | (uint64_t)(uint32_t)v) - 0.5;
    const double hi = sf_from_bits(0x41E0000000000000ULL | (v >> 32)) - 2147483648.0;
    return hi + lo;
}
// the rt_rng.h expression, on a u64 drawn earlier (what rng_u01 computes from rng_u64)
RT_SF double sf_u01_spec(uint64_t u) {
    const uint64_t v = u >> 11;
    return ((double)(uint32_t)(v >> 32) * 4294967296.0 + (double)(uint32_t)v) * 0x1.0p-53;
}

// ------------------------------------------------------------------ AARect::pdf_value (rect.rs:91-101) after its hit test
// The reference builds the rect's axis vector a (a 0/1 vector, 1 at k), the normal n = a if dot(v, a) < 0 else -a, and takes
// |dot(v, n)|.  sf_rect_absdot_full is that, operation by operation.  For a v whose components are all FINITE each product with a 0 or
// a 1 is exact — v_k, or a zero of some sign — and a zero added to x != 0 leaves x: dot(v, a) = v_k and dot(v, n) = -+v_k, except that
// for v_k = +-0 the sums are zeros whose SIGN depends on the other components' signs.  That sign is read by nothing: `< 0` is false for
// either zero (n = -a for both), and |.| of either zero is +0 = |v_k|.  So |dot(v, n)| = |v_k|, bit for bit, for every finite v.
// With a NaN or an infinity among the components 0 * inf = NaN enters the full form and the two differ: the caller tests length(v),
// which it holds anyway — a finite length implies finite components (an infinite or NaN component makes dot(v, v), and so its square
// root, infinite or NaN) — and runs the full form for the wave otherwise (sf_finite, one class test).
RT_SF bool sf_finite(double x) { return __builtin_isfinite(x); }
RT_SF double sf_rect_absdot_full(double vx, double vy, double vz, uint32_t k) {
    const double ax = k == 0u ? 1.0 : 0.0, ay = k == 1u ? 1.0 : 0.0, az = k == 2u ? 1.0 : 0.0;
    const bool neg = vx * ax + vy * ay + vz * az < 0.0;
    const double nx = neg ? ax : -1.0 * ax, ny = neg ? ay : -1.0 * ay, nz = neg ? az : -1.0 * az;
    return __builtin_fabs(vx * nx + vy * ny + vz * nz);
}
RT_SF double sf_rect_absdot_short(double vx, double vy, double vz, uint32_t k) { return __builtin_fabs(k == 0u ? vx : (k == 1u ? vy : vz)); }
// the rest of pdf_value, shared by both forms: distance_squared / (cosine * area), 0 for a cosine of 0
RT_SF double sf_rect_pdf_tail(double absdot, double len, double t, double area) {
    const double distance_squared = (t * t) * (len * len);
    const double cosine = absdot / len;
    return (cosine != 0.0) ? distance_squared / (cosine * area) : 0.0;
}

} // namespace rt

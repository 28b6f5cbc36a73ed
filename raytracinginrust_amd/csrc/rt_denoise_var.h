// csrc/rt_denoise_var.h — the variance-guided form of the denoiser of rt_denoise.h: the specification, the host twin's seams
// (rt_denoise_var_cpu.cpp, plain C++) and the launches of the HIP kernels (rt_denoise_var.hip) as the host library (rt_frames.cpp) sees them.
// No HIP include, as in rt_denoise.h: a stream travels as a void* and a HIP status as an int (0 = hipSuccess).
//
// rt_denoise.h stops colour bleeding with one sigma_c for the whole frame, tightened fourfold per iteration by hand.  Here the stop is
// measured in standard deviations of the two pixels it compares (the variance-guided a-trous filter of SVGF, Schied et al. 2017): the
// caller brings the variance of the mean of every pixel and channel — rt_moments.h (4), from the batch means of a progressive frame — and
// |c_q - c_p|^2, whose expectation is V_p + V_q when both pixels show the same thing, is compared with sigma_v^2 (V_p + V_q).  The variance
// is filtered along with the colour, so the stop tightens as fast as the picture gets cleaner: there is no 4^i.
//
// Only + - * / and comparisons, every operation rounded once (-ffp-contract=off), in this order.  "Finite" is v - v == 0.  The HIP kernels,
// denoise_variance_host and the NumPy restatement of tests/denoise_variance_cases.py give the same 64-bit words.
//
// (B) PACK, per pixel, once:  c = rgb_sum / samples (per channel);  the guide and the key exactly as in rt_denoise.h;
//         v = (V_0 + V_1) + V_2;   v = (v > 0 and v finite) ? v : 0
//     One scalar per pixel: it travels in the fourth slot of the packed colour {r, g, b, v}, which rt_denoise.h leaves 0, so an iteration
//     moves the bytes it moved before.  A NaN, a +inf, a negative or a zero sum of variances all count as 0: no information, and the EPS below
//     is then all the stop has.
//
// (C) PREFILTER of v, once, 3 x 3 (batch means of few passes give V very few degrees of freedom; this is SVGF's remedy):
//         b = (1/4, 1/2, 1/4);  acc = 0; wsum = 0
//         for dy = -1..1, for dx = -1..1 (this order): q = (y + dy, x + dx); outside the frame: skip;  key_q != key_p: skip
//           acc += (b[dy+1]*b[dx+1]) * v_q;   wsum += b[dy+1]*b[dx+1]
//         vs = acc / wsum                     (the centre always counts: wsum > 0)
//     vs replaces v from here on.
//
// (D) ITERATION i = 0 .. K-1, step s = 2^i: the iteration of rt_denoise.h — the taps, their order, the key test, the finite test, k, wn and
//     wp are its own — with another colour stop and with v filtered beside c.  On the host, once: kv = sigma_v * sigma_v; in and ip as in
//     rt_denoise.h.  EPS = 2^-16 = MOMENTS_DELTA^2: two variance-free pixels tolerate sigma_v output codes of linear difference.  Per tap:
//         den = kv * ((v_p + v_q) + EPS)
//         t   = 1 - d / den;   wc = t > 0 ? t*t : 0;   if !c_p_finite: wc = 1           (d as in rt_denoise.h)
//         w   = ((k*wc)*wn)*wp
//         acc += w*c_q (per channel);   vacc += (w*w)*v_q;   wsum += w
//     out:  c = wsum > 0 ? acc / wsum : c_p;   v = wsum > 0 ? vacc / (wsum*wsum) : v_p
//     sigma = (sigma_v, sigma_n, sigma_p); sigma_v is dimensionless.  +inf switches a stop off: with kv = +inf, d / den is 0 for a finite d and
//     NaN for an infinite one, so wc is 1 or 0 exactly where rt_denoise.h's is with sigma_c = +inf — the colour words of the two filters are
//     then the same.
// The result is c_K * samples, in sum units as in rt_denoise.h, and — for callers who want an error estimate of what they display — v_K, one
// double per pixel: the variance of the filtered mean under the assumption that the taps are independent.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "rt_denoise.h"

#if defined(__HIPCC__)
#define RT_DNV_FN __host__ __device__ inline
#else
#define RT_DNV_FN inline
#endif

namespace rt {

// the element-wise variance kernels' launch (rt_denoise_var.hip; here for rt_debug_loop_limits): one pair of doubles per lane and trip
static const uint32_t DNV_THREADS = 256u;
static const uint32_t DNV_MAX_BLOCKS = 2048u;                   // the element-wise variance kernel: grid-stride beyond that (rt_moments.hip)

static const double DENOISE_VAR_EPS = 0.0000152587890625;       // 2^-16
// the workspace of one run is rt_denoise.h's: two packed colour frames {r, g, b, v} and the packed guide, 128 bytes per pixel

// (B): the scalar variance of a pixel from its three channels'
RT_DNV_FN double denoise_var_scalar(double V0, double V1, double V2) {
    const double v = (V0 + V1) + V2;
    return (v > 0.0 && v - v == 0.0) ? v : 0.0;
}
// (D): the colour stop of one tap
RT_DNV_FN double denoise_var_stop(double d, double vp, double vq, double kv) {
    const double den = kv * ((vp + vq) + DENOISE_VAR_EPS);
    const double t = 1.0 - d / den;
    return t > 0.0 ? t * t : 0.0;
}

// What every entry point checks before it touches a pixel: "" or the message
std::string denoise_variance_check(uint64_t samples, uint32_t W, uint32_t H, uint32_t iterations, const double* sigma, uint32_t flags);
// The specification as code (arguments already checked).  rgb_sum_out may alias rgb_sum; var_out (W*H doubles) may be null.
void denoise_variance_host(const double* rgb_sum, uint64_t samples, const double* var, const double* hits, uint32_t W, uint32_t H,
                           uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out, double* var_out);

// ---- the kernels (rt_denoise_var.hip).  DEVICE pointers; d_color* and d_guide 16-byte aligned; asynchronous on `stream` (a hipStream_t);
// the return value is the hipError_t of the launch.  The guide is packed by launch_denoise_pack (rt_denoise.h).
// (B): d_rgb_sum and d_var (24 B / pixel each) -> d_color {r, g, b, v}
int launch_denoise_var_pack(const double* d_rgb_sum, uint64_t samples, const double* d_var, double* d_color, uint32_t n_px, void* stream);
// (C): d_color_in -> d_color_out, the colour copied and v replaced by vs
int launch_denoise_var_prefilter(const double* d_color_in, const double* d_guide, double* d_color_out, uint32_t W, uint32_t H, void* stream);
// (D), one iteration with step `step`, from d_color_in to d_color_out (packed) — or, the last one, to d_rgb_sum_out (24 B / pixel, multiplied
// by samples) and, when given, d_var_out (8 B / pixel) instead.  Steps 1 and 2 run from LDS tiles unless RT_DENOISE_NO_LDS is set.
int launch_denoise_var_filter(const double* d_color_in, const double* d_guide, double* d_color_out, double* d_rgb_sum_out, double* d_var_out,
                              uint32_t W, uint32_t H, uint32_t step, double kv, double in, double ip, uint64_t samples, void* stream);

} // namespace rt

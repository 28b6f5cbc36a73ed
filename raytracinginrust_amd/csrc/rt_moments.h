// csrc/rt_moments.h — the second moment of a progressive frame and its per-pixel error estimate: the specification, the host twin's
// seams (rt_moments_cpu.cpp, plain C++) and the launches of the HIP kernels (rt_moments.hip) as the host library (rt_frames.cpp) sees them.
// No HIP include: a stream travels as a void* and a HIP status as an int (0 = hipSuccess), as in rt_denoise.h, so that the host twin and its
// stand-alone sanitizer program compile with any C++ compiler.
//
// The path-tracing kernels gather no second moment (they are at their register limits).  It is taken BETWEEN passes, from the
// pass frames themselves (batch means): a pass of n_b samples renders into a pass frame p of its own, which is then merged.
//
// Only + - * / and comparisons, every operation rounded once (-ffp-contract=off), in this order.  "Finite" is v - v == 0.
//
// STATE, per pixel and channel: S the sum (the frame's sums), Q the second moment of the pass sums; per frame: N the samples done, B the
// passes merged.
//
// (1) MERGE of pass b (n_b samples, pass frame p), nb = (double)n_b, converted once:
//         S = S + p
//         Q = Q + (p * p) / nb
//     and, on the device only, p = +0.0: the merge leaves the pass frame ready for the next pass.
//
// (2) ERROR, for B >= 2.  Nd = (double)N, Bm1 = (double)(B - 1), both converted once.  Per channel:
//         m   = S / Nd
//         ssb = Q - (S * S) / Nd;   ssb = ssb > 0 ? ssb : 0        the between-batch sum of squares; E[ssb] = (B - 1) sigma^2 (one-way
//                                                                   ANOVA), for unequal n_b too
//         V   = (ssb / Bm1) / Nd                                    the variance of the mean
//         den = m >= delta ? m : delta,  delta = 2^-8               one output code, the role eps plays in rt_albedo.h
//         e2  = V / (4 * den)                                       the squared standard error in display space: format_color shows
//                                                                   sqrt(m) (src/vec.rs:125-131) and d sqrt(m) = dm / (2 sqrt(m))
//         if m >= 1 and (m - 1) * (m - 1) >= 9 * V:  e2 = 0         saturated beyond doubt: the mean lies three standard errors above the
//                                                                   clamp at 0.999
//     The pixel's e2: e = the first channel's; then for the second and the third channel's value x, in this order:
//         e not finite: e stays;  else x not finite: e = x;  else x > e: e = x
//     — the maximum of the three taken with >, first channel first, and the first non-finite value when there is one.
//     What the clamp does with a non-finite state: every comparison with a NaN is false, so a channel whose ssb is NaN — S is NaN or
//     +-inf, or Q is NaN, or a pass value so large that p * p and S * S both overflow — has ssb = 0, V = 0 and e2 = 0: what
//     format_color shows of such a channel (0 for a NaN, the clamp for an infinity) does not move with more samples either.  The one
//     non-finite e2 is +inf, from a +inf in Q beside a finite S * S / N, which no merge produces (a loaded checkpoint or a caller's own
//     frames can hold it).  The error map estimates the noise of finite pixels; a non-finite pixel is found in the sums.
//
// (3) STATISTICS for a threshold tau in display units (1/256 is one code value): tau2 = tau * tau, once, on the host.  Four 64-bit words:
//         [0] converged    the pixels with e2 finite and e2 <= tau2
//         [1] unconverged  the pixels with e2 finite and e2 > tau2
//         [2] nonfinite    the rest
//         [3] max_e2       the bit pattern of the largest finite e2: starts at +0.0 and is replaced by a finite e2 that is > it
//     Positive doubles order as their bit patterns do, so all four words are independent of the order in which pixels are visited: exact.
//
// (4) VARIANCE, for B >= 2: the intermediate V of (2) as a frame of its own, three doubles per pixel — the variance of the mean of every
//     channel, which the variance-guided denoiser (rt_denoise_var.h) takes as its input:
//         ssb = Q - (S * S) / Nd;   ssb = ssb > 0 ? ssb : 0;   V = (ssb / Bm1) / Nd
//     (2) computes its V with this very function, so e2 = V / (4 * den) holds word for word.  A non-finite state gives what (2) says: 0, or
//     +inf from a +inf in Q.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define RT_MOMENTS_FN __host__ __device__ inline
#else
#define RT_MOMENTS_FN inline
#endif

namespace rt {

static const double MOMENTS_DELTA = 0.00390625;                  // 2^-8
enum { MOMENTS_CONVERGED = 0, MOMENTS_UNCONVERGED = 1, MOMENTS_NONFINITE = 2, MOMENTS_MAX_E2 = 3, MOMENTS_STATS_WORDS = 4 };

// (1), one double: the arithmetic the kernels and the host twin share word for word
RT_MOMENTS_FN void moments_merge(double p, double nb, double& S, double& Q) {
    S = S + p;
    const double pp = p * p;
    Q = Q + pp / nb;
}
RT_MOMENTS_FN bool moments_finite(double v) { return v - v == 0.0; }
// (4), one channel: the variance of the mean
RT_MOMENTS_FN double moments_channel_variance(double S, double Q, double Nd, double Bm1) {
    const double ss = S * S;
    double ssb = Q - ss / Nd;
    ssb = ssb > 0.0 ? ssb : 0.0;
    return (ssb / Bm1) / Nd;
}
// (2), one channel
RT_MOMENTS_FN double moments_channel_e2(double S, double Q, double Nd, double Bm1) {
    const double m = S / Nd;
    const double V = moments_channel_variance(S, Q, Nd, Bm1);
    const double den = m >= MOMENTS_DELTA ? m : MOMENTS_DELTA;
    double e2 = V / (4.0 * den);
    if (m >= 1.0) {
        const double over = m - 1.0;
        if (over * over >= 9.0 * V) e2 = 0.0;
    }
    return e2;
}
// (2), one pixel: S and Q point at its three channels
RT_MOMENTS_FN double moments_pixel_e2(const double* S, const double* Q, double Nd, double Bm1) {
    double e = moments_channel_e2(S[0], Q[0], Nd, Bm1);
    for (int c = 1; c < 3; c++) {
        const double x = moments_channel_e2(S[c], Q[c], Nd, Bm1);
        if (!moments_finite(e)) continue;
        if (!moments_finite(x)) e = x;
        else if (x > e) e = x;
    }
    return e;
}

// What the entry points check before they touch a pixel: "" or the message
std::string moments_merge_check(uint64_t n_samples);
std::string moments_error_check(uint64_t samples, uint64_t passes, uint32_t W, uint32_t H);
std::string moments_tau_check(double tau);
// The specification as code (arguments already checked).  The host merge leaves pass_sum as it is.
void moments_merge_host(const double* pass_sum, uint64_t n_samples, double* rgb_sum, double* sq_sum, uint64_t n_doubles);
void moments_error_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint64_t n_px, double* e2_out);
void moments_stats_host(const double* e2, uint64_t n_px, double tau, uint64_t stats_out[4]);
void moments_variance_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint64_t n_doubles, double* var_out);

// ---- the kernels (rt_moments.hip).  DEVICE pointers, 8-byte aligned, the three of a merge distinct buffers; asynchronous on `stream` (a
// hipStream_t); the return value is the hipError_t of the launch.
// (1) over n doubles; d_pass_sum is all +0.0 afterwards.  16-byte accesses when all three buffers are 16-byte aligned.
int launch_moments_merge(double* d_pass_sum, uint64_t n_samples, double* d_rgb_sum, double* d_sq_sum, uint64_t n, void* stream);
// (2) and (3) over n_px pixels: d_e2_out (n_px doubles) and d_stats (four 64-bit words, ZEROED by the caller in stream order; tau2 = tau * tau)
// are each written when given.
int launch_moments_error(const double* d_rgb_sum, const double* d_sq_sum, uint64_t samples, uint64_t passes, uint32_t n_px, double* d_e2_out,
                         double tau2, unsigned long long* d_stats, void* stream);
// (4) over n doubles (rt_denoise_var.hip: a unit of its own, so that rt_moments.hip's code object does not change).  16-byte accesses when all
// three buffers are 16-byte aligned; d_var_out may be neither input.
int launch_moments_variance(const double* d_rgb_sum, const double* d_sq_sum, uint64_t samples, uint64_t passes, uint64_t n, double* d_var_out, void* stream);

} // namespace rt

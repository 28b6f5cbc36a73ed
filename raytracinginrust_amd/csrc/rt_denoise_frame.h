// csrc/rt_denoise_frame.h — denoising a frame as it is: one sample count for the frame or a count per pixel (an adaptive frame, rt_adaptive.h),
// with or without a variance frame (rt_denoise_var.h), with or without albedo sums (rt_albedo.h (2)).  The specification, the host twin's
// seams (rt_denoise_frame_cpu.cpp, plain C++) and the launches of the HIP kernels (rt_denoise_frame.hip) as the host library (rt_frames.cpp)
// sees them.  No HIP include: a stream travels as a void* and a HIP status as an int (0 = hipSuccess), as in rt_denoise.h.
//
// The filters themselves do not change: they compute c = rgb_sum / samples at their start and c_K * samples at their end, so a frame of
// per-pixel MEANS goes through them with samples = 1 (x / 1 and x * 1 are exact), an element-wise step in front and one behind — the shape
// of rt_albedo.h (2).  With equal counts every word is the one rt_denoise*, rt_denoise_albedo* and rt_denoise_variance* give.
//
// Only + - * / and comparisons, every operation rounded once (-ffp-contract=off), in this order.  The HIP kernels, denoise_frame_host and
// the NumPy restatement of tests/denoise_frame_cases.py give the same 64-bit words.
//
// (E) VARIANCE with counts, per pixel p and channel — rt_moments.h (4) with the pixel's own n and b:
//         V = b[p] >= 2 ? moments_channel_variance(S, Q, (double)n[p], (double)(b[p] - 1)) : +inf
//     +inf is rt_adaptive.h (A)'s e2 for such a pixel, and rt_denoise_var.h (B) counts it as "no information".  For b >= 2, (A)'s e2 is what
//     rt_moments.h (2) makes of this V; with all counts equal the frame is rt_moments.h (4)'s word for word.
//
// (F) FRAME DENOISE, per pixel p and channel:
//         N  = counts ? (double)n[p] : (double)samples
//         m  = albedo_modulation(albedo_sum, albedo_samples),  d = m >= eps ? m : eps      rt_albedo.h (2) steps 1-3;  no albedo: m = d = 1
//         x  = S / d
//         c  = x / N                   a pixel with N = 0 is non-finite here: the filters leave it out as a neighbour and repair it as a centre
//         Vd = (V / d) / d             only with a variance frame; without albedo Vd = V
//         y  = rt_denoise.h (c, samples = 1, hits, K, sigma, flags)                without a variance frame (sigma[0] = sigma_c)
//            | rt_denoise_var.h (c, samples = 1, Vd, hits, K, sigma, flags)        with one (sigma[0] = sigma_v); v_K as in that header, in the
//                                                                                  demodulated domain when albedo is given
//         s  = N > 0 ? y * N : +0.0
//         out = s * m
//     The order (y * N) * m is what makes the albedo form equal rt_denoise_albedo* for equal counts.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include "rt_denoise.h"
#include "rt_albedo.h"
#include "rt_moments.h"
#include "rt_denoise_var.h"

namespace rt {

// the element-wise kernels' launch (rt_denoise_frame.hip; here for rt_debug_loop_limits): one pair of doubles per lane and trip
static const uint32_t DNF_THREADS = 256u;
static const uint32_t DNF_MAX_BLOCKS = 2048u;                   // 8 resident workgroups' worth per CU; grid-stride beyond that (rt_moments.hip)

// the workspace of one run: the filter's own, then the frames c and Vd (3 doubles per pixel each, each padded to a multiple of 16 bytes so
// that both start 16-byte aligned in a 16-byte aligned workspace)
inline size_t denoise_frame_plane_bytes(uint64_t n_px) { return (size_t)((n_px * 3u * sizeof(double) + 15u) & ~(uint64_t)15u); }
inline size_t denoise_frame_workspace_bytes(uint64_t n_px) { return (size_t)n_px * DENOISE_WORKSPACE_BYTES_PER_PX + 2u * denoise_frame_plane_bytes(n_px); }

// (E), one channel
RT_MOMENTS_FN double frame_channel_variance(double S, double Q, uint32_t n, uint32_t b) {
    if (b < 2u) return HUGE_VAL;
    return moments_channel_variance(S, Q, (double)n, (double)(b - 1u));
}
// (F), one channel: m (1 without albedo sums), then what stands in front of the filter and behind it
RT_MOMENTS_FN double frame_modulation(bool has_albedo, double albedo_sum, double albedo_samples) {
    return has_albedo ? albedo_modulation(albedo_sum, albedo_samples) : 1.0;
}
RT_MOMENTS_FN double frame_mean(double S, double m, double N) {
    const double x = albedo_demodulate(S, m);
    return x / N;
}
RT_MOMENTS_FN double frame_variance(double V, double m) {
    const double d = (m >= ALBEDO_EPS) ? m : ALBEDO_EPS;
    return (V / d) / d;
}
RT_MOMENTS_FN double frame_sum(double y, double m, double N) {
    const double s = N > 0.0 ? y * N : 0.0;
    return s * m;
}

// What the entry points check before they touch a pixel: "" or the message.  The flags say which optional frames are given.
std::string denoise_frame_check(bool has_counts, uint64_t samples, bool has_var, bool has_albedo, uint64_t albedo_samples, uint32_t W, uint32_t H,
                                uint32_t iterations, const double* sigma, uint32_t flags, bool wants_var_out);
// The specifications as code (arguments already checked).  counts, var and albedo_sum may each be null; rgb_sum_out may alias rgb_sum;
// var_out (W*H doubles) may be null.
void adaptive_variance_host(const double* S, const double* Q, const uint32_t* n, const uint32_t* b, uint64_t n_px, double* var_out);
void denoise_frame_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* var, const double* albedo_sum, uint64_t albedo_samples,
                        const double* hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out,
                        double* var_out);

// ---- the element-wise kernels (rt_denoise_frame.hip).  DEVICE pointers: doubles 8-byte aligned, counts 4-byte aligned (16-byte accesses are
// used when all the doubles' buffers of a launch are 16-byte aligned); n_px pixels; asynchronous on `stream`; the return value is the
// hipError_t of the launch.
// (E): d_var_out (3 n_px doubles) may be neither input
int launch_frame_variance(const double* d_S, const double* d_Q, const uint32_t* d_n, const uint32_t* d_b, uint32_t n_px, double* d_var_out, void* stream);
// (F) in front of the filter: d_c = c;  d_vd = Vd when d_var AND d_albedo_sum are given (else it is not touched: Vd is V).  d_counts, d_var and
// d_albedo_sum may each be null.
int launch_frame_prepare(const double* d_rgb_sum, const uint32_t* d_counts, uint64_t samples, const double* d_var, const double* d_albedo_sum,
                         uint64_t albedo_samples, double* d_c, double* d_vd, uint32_t n_px, void* stream);
// (F) behind it: d_io = (d_io * N) * m, in place
int launch_frame_finish(double* d_io, const uint32_t* d_counts, uint64_t samples, const double* d_albedo_sum, uint64_t albedo_samples, uint32_t n_px, void* stream);

} // namespace rt

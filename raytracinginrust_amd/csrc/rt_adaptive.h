// csrc/rt_adaptive.h — adaptive progressive frames: per-pixel sample counts through error, selection, merge and resolve.  The specification,
// the host twin's seams (rt_adaptive_cpu.cpp, plain C++) and the launches of the HIP kernels (rt_adaptive.hip) as the host library
// (rt_frames.cpp) sees them.  No HIP include: a stream travels as a void* and a HIP status as an int (0 = hipSuccess), as in rt_moments.h.
//
// THE INVARIANT: pixel p of an adaptive frame with count n[p] holds exactly samples 0 .. n[p] - 1 of the streams rng_for_path(seed, p, s) —
// the very samples a one-shot frame of the same view and seed holds at those indices.  A pass has ONE size n_b for every listed pixel: a
// listed pixel receives samples [n[p], n[p] + n_b).
//
// STATE, per pixel: S and Q (three doubles each, rt_moments.h), n (uint32) the samples done, b (uint32) the passes the pixel took part in.
//
// Only + - * / (and format_color's sqrt in (D)), comparisons and integer operations, every floating-point operation rounded once, in this order.
//
// (A) ERROR with counts:
//         b[p] >= 2:  e2[p] = moments_pixel_e2(S[p], Q[p], (double)n[p], (double)(b[p] - 1))        rt_moments.h (2), unchanged
//         b[p] <  2:  e2[p] = +inf
//     The statistics are rt_moments.h (3)'s four words over this map (a pixel with b < 2 counts as nonfinite).
//
// (B) SELECTION for a pass of n_b samples, tau2 = tau * tau (once, on the host), spread in {0, 1}, max_samples <= 2^32 - 1:
//         need[p]   = b[p] < 2  or  (e2[p] finite and e2[p] > tau2)
//         needed[p] = need[p]  or  (spread = 1 and need[q] for one of the up to 8 neighbours q of p inside the frame)
//         active[p] = needed[p] and n[p] + n_b <= max_samples                                         (the sum in 64 bits)
//     The LIST is the output-order indices of the active pixels in ASCENDING order, and their count: np.flatnonzero(active).
//
// (C) LIST MERGE of a pass of n_b samples, nb = (double)n_b: for every listed p, per channel
//         moments_merge(pass[p], nb, S[p], Q[p]);   pass[p] = +0.0;          then   n[p] += n_b;  b[p] += 1
//     Unlisted pixels are neither read nor written.
//
// (D) RESOLVE with counts: format_color (src/vec.rs:125-131) with n[p] in the frame's sample count's place,
//         c = (256 * clamp(sqrt(S / (double)n[p]), 0, 0.999)) as u64         per channel;  n[p] = 0 gives 0
//     and the number of pixels whose triple differs from a previous image's (every pixel when there is none).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include "rt_moments.h"

namespace rt {

static const uint64_t ADAPTIVE_MAX_SAMPLES = 0xFFFFFFFFull;      // the sample field of a path's RNG key is 32 bits (rt_rng.h)

// (A), one pixel
RT_MOMENTS_FN double adaptive_pixel_e2(const double* S, const double* Q, uint32_t n, uint32_t b) {
    if (b < 2u) return HUGE_VAL;
    return moments_pixel_e2(S, Q, (double)n, (double)(b - 1u));
}
// (B), one pixel: need from its e2, and the cap
RT_MOMENTS_FN bool adaptive_need(double e2, uint32_t b, double tau2) {
    if (b < 2u) return true;
    return moments_finite(e2) && e2 > tau2;
}
RT_MOMENTS_FN bool adaptive_room(uint32_t n, uint32_t n_b, uint64_t max_samples) { return (uint64_t)n + (uint64_t)n_b <= max_samples; }
// (D), one channel
RT_MOMENTS_FN uint32_t adaptive_format_channel(double sum, uint32_t n) {
    if (n == 0u) return 0u;
    double x = sqrt(sum / (double)n);
    if (x < 0.0) x = 0.0; else if (x > 0.999) x = 0.999;          // f64::clamp: NaN stays NaN
    const double y = 256.0 * x;
    return (y > 0.0) ? (uint32_t)y : 0u;                          // `as u64`: NaN -> 0, negative -> 0; y <= 255.744 here
}

// What the entry points check before they touch a pixel: "" or the message
std::string adaptive_frame_check(uint32_t W, uint32_t H);
std::string adaptive_select_check(uint32_t W, uint32_t H, uint32_t n_b, double tau, uint64_t max_samples, uint32_t spread);
// The specification as code (arguments already checked)
void adaptive_error_host(const double* S, const double* Q, const uint32_t* n, const uint32_t* b, uint64_t n_px, double* e2_out);
uint32_t adaptive_select_host(const double* S, const double* Q, const uint32_t* n, const uint32_t* b, uint32_t W, uint32_t H, uint32_t n_b, double tau,
                              uint64_t max_samples, uint32_t spread, uint32_t* list_out);
void adaptive_merge_host(double* pass, uint32_t n_b, double* S, double* Q, uint32_t* n, uint32_t* b, const uint32_t* list, uint32_t n_list);
uint64_t adaptive_resolve_host(const double* S, const uint32_t* n, const uint8_t* rgb8_prev, uint8_t* rgb8_out, uint64_t n_px);

// ---- the element-wise kernels (rt_adaptive.hip).  DEVICE pointers: doubles 8-byte aligned, counts and lists 4-byte aligned; asynchronous on
// `stream` (a hipStream_t); the return value is the hipError_t of the launch.  No scratch; 16-byte accesses where the buffers' alignment allows.
// (A): d_e2_out (n_px doubles) and d_stats (four 64-bit words, ZEROED by the caller in stream order) are each written when given.
int launch_adaptive_error(const double* d_S, const double* d_Q, const uint32_t* d_n, const uint32_t* d_b, uint32_t n_px, double* d_e2_out, double tau2,
                          unsigned long long* d_stats, void* stream);
// (B): count, scan, scatter.  The workspace (16-byte aligned, adaptive_select_workspace_bytes) holds the need and active flags and the per-block counts.
static const uint32_t ADAPTIVE_BLOCK_PX = 1024u;                 // pixels one workgroup of the compaction covers: 256 lanes x 4 consecutive pixels
// the element-wise kernels' launch (rt_adaptive.hip; here for rt_debug_loop_limits): the scan is ONE workgroup of ADAPTIVE_SCAN_THREADS lanes that
// walks the workgroup counts that many at a time; the error and resolve kernels launch at most ADAPTIVE_ERROR_MAX_BLOCKS workgroups
static const uint32_t ADAPTIVE_THREADS = 256u;
static const uint32_t ADAPTIVE_MAX_BLOCKS = 2048u;            // 8 resident workgroups' worth per CU; grid-stride beyond that
static const uint32_t ADAPTIVE_ERROR_MAX_BLOCKS = 1024u;      // every workgroup ends with up to four atomics on one cache line (rt_moments.hip)
static const uint32_t ADAPTIVE_SCAN_THREADS = 1024u;
inline size_t adaptive_select_workspace_bytes(uint64_t n_px) {
    const uint64_t flags = (n_px + 15u) & ~(uint64_t)15u, blocks = (n_px + ADAPTIVE_BLOCK_PX - 1u) / ADAPTIVE_BLOCK_PX;
    return (size_t)(2u * flags + ((blocks * 4u + 15u) & ~(uint64_t)15u));
}
int launch_adaptive_select(const double* d_S, const double* d_Q, const uint32_t* d_n, const uint32_t* d_b, uint32_t W, uint32_t H, uint32_t n_b, double tau2,
                           uint64_t max_samples, uint32_t spread, uint32_t* d_list_out, uint32_t* d_count_out, void* d_workspace, void* stream);
// (C); d_max_out (nullptr, or one uint32 the caller initialised in stream order) is raised to the largest n[p] the merge wrote
int launch_adaptive_merge(double* d_pass, uint32_t n_b, double* d_S, double* d_Q, uint32_t* d_n, uint32_t* d_b, const uint32_t* d_list, uint32_t n_list,
                          uint32_t* d_max_out, void* stream);
// (C)'s counts over ALL pixels, n += n_b and b += 1 (a uniform pass: the frames' own kernel rendered it and launch_moments_merge, which is (C)'s
// arithmetic over every double, merged it)
int launch_adaptive_bump(uint32_t* d_n, uint32_t* d_b, uint32_t n_b, uint32_t n_px, void* stream);
// (D): *d_changed += the changed pixels (zeroed by the caller in stream order)
int launch_adaptive_resolve(const double* d_S, const uint32_t* d_n, const uint8_t* d_rgb8_prev, uint8_t* d_rgb8_out, unsigned long long* d_changed, uint32_t n_px, void* stream);

} // namespace rt

// csrc/rt_reproject_var.hip — the two kernels of temporal variance (rt_reproject_var.h): the reprojection of a frame's history WITH the
// variance of its mean (V) and the blend of a frame's variance with a history's (BV), for rt_reproject_variance, rt_reproject_variance_device,
// rt_temporal_blend_variance_device, rt_progressive_set_view on a frame with moments and rt_progressive_resolve_temporal_variance_rgb8
// (include/rt_amd.h).  A translation unit of its own: rt_reproject.o and every other unit's code object stay what they were.
//
// Exactness: the build's -ffp-contract=off -fno-fast-math make `/` the IEEE-correct f64 division and keep every operation one rounding, and
// reproject_variance_pixel / blend_variance are the host twin's own functions (rt_reproject_var_cpu.cpp).
//
// REPROJECT WITH VARIANCE: rt_reproject.hip's kernel with one more gather and one more output — one new-view pixel per lane, no loop, no
// LDS, no atomics, the R0 constants by value in the kernel's arguments.  ONE launch writes the sums, the counts and the variances: a second
// launch over the same records would repeat the gathers of 64 of every 128-byte record per tap, which are what the kernel costs.  Per tap
// that passes (R4) 24 more bytes are read (the tap's three variances, next to nothing else in their line unless the neighbouring lanes' taps
// are neighbours, as they are wherever the two views are close), and 24 more are written per pixel: 52 bytes out.
// BLEND: a flat stream, one pixel's three channels per lane and no loop: 48 B in (24 without a variance frame), 8 B of counts (4 without
// counts) and 24 B out per pixel.  A lane's three doubles are consecutive, so a wave reads and writes whole lines; the count is read once
// for the three channels, which is why the lane is a pixel and not a double.
#include <hip/hip_runtime.h>
#include "rt_reproject_var.h"

namespace rt {

__global__ __launch_bounds__(256) void reproject_variance_kernel(const ReprojectConsts K, const double* __restrict__ prev_sum, const uint32_t* __restrict__ prev_counts,
                                                                 const double* __restrict__ prev_var, const double* __restrict__ prev_hits,
                                                                 const double* __restrict__ cur_hits, double* __restrict__ hist_sum,
                                                                 uint32_t* __restrict__ hist_counts, double* __restrict__ hist_var, uint32_t n_px) {
    const uint64_t p = (uint64_t)blockIdx.x * REPROJECT_THREADS + threadIdx.x;
    if (p >= n_px) return;
    const double* ph = (const double*)__builtin_assume_aligned(prev_hits, 16);
    const double* ch = (const double*)__builtin_assume_aligned(cur_hits, 16);
    double out3[3], var3[3];
    const uint32_t Nh = reproject_variance_pixel(K, prev_sum, prev_counts, prev_var, ph, ch, p, out3, var3);
    double* o = hist_sum + 3u * p;
    o[0] = out3[0]; o[1] = out3[1]; o[2] = out3[2];
    double* v = hist_var + 3u * p;
    v[0] = var3[0]; v[1] = var3[1]; v[2] = var3[2];
    hist_counts[p] = Nh;
}

// (BV): pixel p's three channels (var_out may be var: neither is __restrict__; a lane reads its own three words before it writes them)
__global__ __launch_bounds__(256) void temporal_blend_variance_kernel(const double* var, const uint32_t* __restrict__ cnt, uint64_t Ns, const double* __restrict__ hvar,
                                                                      const uint32_t* __restrict__ hcnt, double* var_out, uint32_t n_px) {
    const uint64_t p = (uint64_t)blockIdx.x * REPROJECT_THREADS + threadIdx.x;
    if (p >= n_px) return;
    const uint64_t N = cnt ? (uint64_t)cnt[p] : Ns;
    const uint32_t h = hcnt[p];
    const double* vh = hvar + 3u * p;
    const double h0 = vh[0], h1 = vh[1], h2 = vh[2];
    double v0 = variance_unknown(), v1 = variance_unknown(), v2 = variance_unknown();
    if (var) { const double* v = var + 3u * p; v0 = v[0]; v1 = v[1]; v2 = v[2]; }
    double* o = var_out + 3u * p;
    o[0] = blend_variance(N, h, v0, h0); o[1] = blend_variance(N, h, v1, h1); o[2] = blend_variance(N, h, v2, h2);
}

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + REPROJECT_THREADS - 1u) / REPROJECT_THREADS); }     // n <= 2^31 - 1: fits

int launch_reproject_variance(const ReprojectConsts& K, const double* d_prev_sum, const uint32_t* d_prev_counts, const double* d_prev_var, const double* d_prev_hits,
                              const double* d_cur_hits, double* d_hist_sum_out, uint32_t* d_hist_counts_out, double* d_hist_var_out, void* stream) {
    const uint32_t n_px = K.W * K.H;
    if (n_px == 0u) return 0;
    hipLaunchKernelGGL(reproject_variance_kernel, dim3(blocks_for(n_px)), dim3(REPROJECT_THREADS), 0, (hipStream_t)stream, K, d_prev_sum, d_prev_counts, d_prev_var,
                       d_prev_hits, d_cur_hits, d_hist_sum_out, d_hist_counts_out, d_hist_var_out, n_px);
    return (int)hipGetLastError();
}

int launch_temporal_blend_variance(const double* d_var, const uint32_t* d_counts, uint64_t samples, const double* d_hist_var, const uint32_t* d_hist_counts,
                                   uint32_t n_px, double* d_var_out, void* stream) {
    if (n_px == 0u) return 0;
    hipLaunchKernelGGL(temporal_blend_variance_kernel, dim3(blocks_for(n_px)), dim3(REPROJECT_THREADS), 0, (hipStream_t)stream, d_var, d_counts, samples, d_hist_var,
                       d_hist_counts, d_var_out, n_px);
    return (int)hipGetLastError();
}

} // namespace rt

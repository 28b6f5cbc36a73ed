// csrc/rt_denoise_frame.hip — the three element-wise kernels of rt_denoise_frame.h: the variance frame of a frame with per-pixel counts (E),
// and what stands in front of the unchanged filters and behind them when a frame is denoised as it is (F), for rt_adaptive_variance_device,
// rt_denoise_frame*, rt_progressive_variance_counts and rt_progressive_resolve_denoised_frame_rgb8 (include/rt_amd.h).  A translation unit
// of its own: no other unit's code object changes when this file does.
//
// Exactness: the build's -ffp-contract=off -fno-fast-math make `/` the IEEE-correct f64 division and keep every operation one rounding, and
// frame_channel_variance / frame_mean / frame_variance / frame_sum are the host twin's own functions (rt_denoise_frame_cpu.cpp).
//
// Shape: rt_moments.hip's merge — pure streams over the 3 n_px doubles of a frame, grid-stride, no LDS, no atomics.  The frames are walked as
// flat arrays of doubles, so consecutive lanes touch consecutive addresses whatever 3 doubles per pixel do to a pixel's alignment: the PAIR
// form moves 16 bytes per access and serves buffers that are all 16-byte aligned, the tail (an odd count) and any other buffer go through
// the scalar form.  Double i belongs to pixel i / 3; its count is a 4-byte load that three (or, in a pair's case, up to six) neighbouring
// lanes share from the same cache line: 4 bytes per pixel beside the 24 of every frame read or written.
//     variance  48 B in + 8 B of counts, 24 B out
//     prepare   24 B in (+ 4 counts, + 24 variance, + 24 albedo), 24 B out (+ 24: Vd, only with variance AND albedo)
//     finish    24 B in and out, in place (+ 4 counts, + 24 albedo)
// Which optional frames exist is a kernel argument (a null pointer): uniform branches, one kernel per step and form.
#include <hip/hip_runtime.h>
#include "rt_denoise_frame.h"

namespace rt {

typedef double d2 __attribute__((ext_vector_type(2)));

// the pixels of doubles 2 i and 2 i + 1
__device__ __forceinline__ void pair_pixels(uint64_t i, uint64_t& p0, uint64_t& p1) {
    const uint64_t i0 = 2u * i;
    p0 = i0 / 3u;
    p1 = p0 + ((i0 - 3u * p0) == 2u ? 1u : 0u);
}

// ---- (E)
__global__ __launch_bounds__(256) void frame_variance2_kernel(const d2* __restrict__ sum, const d2* __restrict__ sq, const uint32_t* __restrict__ cnt,
                                                              const uint32_t* __restrict__ pas, d2* __restrict__ var, uint64_t n_pairs) {
    const uint64_t stride = (uint64_t)gridDim.x * DNF_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DNF_THREADS + threadIdx.x; i < n_pairs; i += stride) {
        uint64_t p0, p1;
        pair_pixels(i, p0, p1);
        const d2 s = sum[i], q = sq[i];
        d2 v;
        v.x = frame_channel_variance(s.x, q.x, cnt[p0], pas[p0]);
        v.y = frame_channel_variance(s.y, q.y, cnt[p1], pas[p1]);
        var[i] = v;
    }
}
__global__ __launch_bounds__(256) void frame_variance1_kernel(const double* __restrict__ sum, const double* __restrict__ sq, const uint32_t* __restrict__ cnt,
                                                              const uint32_t* __restrict__ pas, double* __restrict__ var, uint64_t first, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * DNF_THREADS;
    for (uint64_t i = first + (uint64_t)blockIdx.x * DNF_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t p = i / 3u;
        var[i] = frame_channel_variance(sum[i], sq[i], cnt[p], pas[p]);
    }
}

// ---- (F) in front of the filter.  Ns = (double)samples, used where cnt is null; na = (double)albedo_samples
__global__ __launch_bounds__(256) void frame_prepare2_kernel(const d2* __restrict__ sum, const uint32_t* __restrict__ cnt, double Ns, const d2* __restrict__ var,
                                                             const d2* __restrict__ alb, double na, d2* __restrict__ c, d2* __restrict__ vd, uint64_t n_pairs) {
    const uint64_t stride = (uint64_t)gridDim.x * DNF_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DNF_THREADS + threadIdx.x; i < n_pairs; i += stride) {
        double N0 = Ns, N1 = Ns;
        if (cnt) { uint64_t p0, p1; pair_pixels(i, p0, p1); N0 = (double)cnt[p0]; N1 = (double)cnt[p1]; }
        d2 a; a.x = 0.0; a.y = 0.0;
        if (alb) a = alb[i];
        const double m0 = frame_modulation(alb != nullptr, a.x, na), m1 = frame_modulation(alb != nullptr, a.y, na);
        const d2 s = sum[i];
        d2 r;
        r.x = frame_mean(s.x, m0, N0);
        r.y = frame_mean(s.y, m1, N1);
        c[i] = r;
        if (vd) {
            const d2 v = var[i];
            d2 w;
            w.x = frame_variance(v.x, m0);
            w.y = frame_variance(v.y, m1);
            vd[i] = w;
        }
    }
}
__global__ __launch_bounds__(256) void frame_prepare1_kernel(const double* __restrict__ sum, const uint32_t* __restrict__ cnt, double Ns, const double* __restrict__ var,
                                                             const double* __restrict__ alb, double na, double* __restrict__ c, double* __restrict__ vd,
                                                             uint64_t first, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * DNF_THREADS;
    for (uint64_t i = first + (uint64_t)blockIdx.x * DNF_THREADS + threadIdx.x; i < n; i += stride) {
        const double N = cnt ? (double)cnt[i / 3u] : Ns;
        const double m = frame_modulation(alb != nullptr, alb ? alb[i] : 0.0, na);
        c[i] = frame_mean(sum[i], m, N);
        if (vd) vd[i] = frame_variance(var[i], m);
    }
}

// ---- (F) behind it, in place
__global__ __launch_bounds__(256) void frame_finish2_kernel(d2* __restrict__ io, const uint32_t* __restrict__ cnt, double Ns, const d2* __restrict__ alb, double na,
                                                            uint64_t n_pairs) {
    const uint64_t stride = (uint64_t)gridDim.x * DNF_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DNF_THREADS + threadIdx.x; i < n_pairs; i += stride) {
        double N0 = Ns, N1 = Ns;
        if (cnt) { uint64_t p0, p1; pair_pixels(i, p0, p1); N0 = (double)cnt[p0]; N1 = (double)cnt[p1]; }
        d2 a; a.x = 0.0; a.y = 0.0;
        if (alb) a = alb[i];
        const d2 y = io[i];
        d2 r;
        r.x = frame_sum(y.x, frame_modulation(alb != nullptr, a.x, na), N0);
        r.y = frame_sum(y.y, frame_modulation(alb != nullptr, a.y, na), N1);
        io[i] = r;
    }
}
__global__ __launch_bounds__(256) void frame_finish1_kernel(double* __restrict__ io, const uint32_t* __restrict__ cnt, double Ns, const double* __restrict__ alb, double na,
                                                            uint64_t first, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * DNF_THREADS;
    for (uint64_t i = first + (uint64_t)blockIdx.x * DNF_THREADS + threadIdx.x; i < n; i += stride) {
        const double N = cnt ? (double)cnt[i / 3u] : Ns;
        io[i] = frame_sum(io[i], frame_modulation(alb != nullptr, alb ? alb[i] : 0.0, na), N);
    }
}

// (null pointers count as aligned: an absent frame forbids nothing)
static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e)) & 15u) == 0u;
}
static uint32_t blocks_for(uint64_t n) {
    const uint64_t b = (n + DNF_THREADS - 1u) / DNF_THREADS;
    return (uint32_t)(b > DNF_MAX_BLOCKS ? DNF_MAX_BLOCKS : b);
}

int launch_frame_variance(const double* d_S, const double* d_Q, const uint32_t* d_n, const uint32_t* d_b, uint32_t n_px, double* d_var_out, void* stream) {
    const uint64_t n = (uint64_t)n_px * 3u;
    if (n == 0u) return 0;
    const uint64_t n_pairs = aligned16(d_S, d_Q, d_var_out) ? n / 2u : 0u;
    if (n_pairs) hipLaunchKernelGGL(frame_variance2_kernel, dim3(blocks_for(n_pairs)), dim3(DNF_THREADS), 0, (hipStream_t)stream, (const d2*)d_S, (const d2*)d_Q, d_n, d_b, (d2*)d_var_out, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(frame_variance1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(DNF_THREADS), 0, (hipStream_t)stream, d_S, d_Q, d_n, d_b, d_var_out, 2u * n_pairs, n);
    return (int)hipGetLastError();
}

int launch_frame_prepare(const double* d_rgb_sum, const uint32_t* d_counts, uint64_t samples, const double* d_var, const double* d_albedo_sum,
                         uint64_t albedo_samples, double* d_c, double* d_vd, uint32_t n_px, void* stream) {
    const uint64_t n = (uint64_t)n_px * 3u;
    if (n == 0u) return 0;
    if (!d_var || !d_albedo_sum) d_vd = nullptr;                 // Vd is V itself
    const double Ns = (double)samples, na = (double)albedo_samples;
    const uint64_t n_pairs = aligned16(d_rgb_sum, d_vd ? d_var : nullptr, d_albedo_sum, d_c, d_vd) ? n / 2u : 0u;
    if (n_pairs) hipLaunchKernelGGL(frame_prepare2_kernel, dim3(blocks_for(n_pairs)), dim3(DNF_THREADS), 0, (hipStream_t)stream, (const d2*)d_rgb_sum, d_counts, Ns,
                                    (const d2*)d_var, (const d2*)d_albedo_sum, na, (d2*)d_c, (d2*)d_vd, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(frame_prepare1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(DNF_THREADS), 0, (hipStream_t)stream, d_rgb_sum, d_counts, Ns,
                                             d_var, d_albedo_sum, na, d_c, d_vd, 2u * n_pairs, n);
    return (int)hipGetLastError();
}

int launch_frame_finish(double* d_io, const uint32_t* d_counts, uint64_t samples, const double* d_albedo_sum, uint64_t albedo_samples, uint32_t n_px, void* stream) {
    const uint64_t n = (uint64_t)n_px * 3u;
    if (n == 0u) return 0;
    const double Ns = (double)samples, na = (double)albedo_samples;
    const uint64_t n_pairs = aligned16(d_io, d_albedo_sum) ? n / 2u : 0u;
    if (n_pairs) hipLaunchKernelGGL(frame_finish2_kernel, dim3(blocks_for(n_pairs)), dim3(DNF_THREADS), 0, (hipStream_t)stream, (d2*)d_io, d_counts, Ns, (const d2*)d_albedo_sum, na, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(frame_finish1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(DNF_THREADS), 0, (hipStream_t)stream, d_io, d_counts, Ns, d_albedo_sum, na, 2u * n_pairs, n);
    return (int)hipGetLastError();
}

} // namespace rt

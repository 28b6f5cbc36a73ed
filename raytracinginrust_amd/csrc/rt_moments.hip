// csrc/rt_moments.hip — the two kernels of a progressive frame's moments (rt_moments_*, rt_progressive_enable_moments, include/rt_amd.h);
// the specification is in rt_moments.h.  A translation unit of its own: rt_kernel.hip and every other unit's code object do not change
// when this file does.
//
// Exactness: the build's -ffp-contract=off -fno-fast-math make `/` the IEEE-correct f64 division and keep a * b + c two roundings, so every
// word equals the host twin's (rt_moments_cpu.cpp), which shares moments_merge / moments_pixel_e2 with this file.
//
// MERGE: a pure stream, 24 B in and 24 B out per double (S, Q, p read; S, Q and the zeroed p written) = 144 B per pixel.  Grid-stride, no
// LDS.  The PAIR form moves 16 bytes per access and serves buffers that are all 16-byte aligned; the tail (an odd count) and any other
// buffer go through the scalar form, as in rt_albedo.hip.
// ERROR: one pixel per lane, grid-stride: 48 B in, 8 B out when the map is asked for.  The statistics are summed per lane over the
// grid-stride loop, reduced across the wave with shuffles (the shape of rt_resolve.hip's changed-pixel count), then across the workgroup's
// four waves through 128 bytes of LDS, and added with ONE atomic per word and WORKGROUP; the maximum is an integer maximum of bit
// patterns, so no word depends on the order of arrival.  One atomic per word and wave was *measured* first: the four words share a cache
// line, atomics on one line are served one after another (about 150 per microsecond), and the 10 000 waves of an 800 x 800 frame made
// the kernel 0.20 ms at every frame size — 35 times its traffic floor.  Hence also the smaller grid: at most 1024 workgroups.
#include <hip/hip_runtime.h>
#include "rt_moments.h"

namespace rt {

typedef double d2 __attribute__((ext_vector_type(2)));

static const uint32_t MOMENTS_THREADS = 256u;
static const uint32_t MOMENTS_MAX_BLOCKS = 2048u;             // 8 resident workgroups' worth per CU; grid-stride beyond that
static const uint32_t MOMENTS_ERROR_MAX_BLOCKS = 1024u;       // the error kernel: every workgroup ends with up to four atomics on one cache line

__global__ __launch_bounds__(256) void moments_merge2_kernel(d2* __restrict__ pass, double nb, d2* __restrict__ sum, d2* __restrict__ sq, uint64_t n_pairs) {
    const uint64_t stride = (uint64_t)gridDim.x * MOMENTS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * MOMENTS_THREADS + threadIdx.x; i < n_pairs; i += stride) {
        const d2 p = pass[i];
        const d2 s = sum[i], q = sq[i];
        double s0 = s.x, s1 = s.y, q0 = q.x, q1 = q.y;
        moments_merge(p.x, nb, s0, q0);
        moments_merge(p.y, nb, s1, q1);
        d2 so, qo;
        so.x = s0; so.y = s1; qo.x = q0; qo.y = q1;
        sum[i] = so; sq[i] = qo;
        d2 z; z.x = 0.0; z.y = 0.0;
        pass[i] = z;
    }
}
__global__ __launch_bounds__(256) void moments_merge1_kernel(double* __restrict__ pass, double nb, double* __restrict__ sum, double* __restrict__ sq, uint64_t first, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * MOMENTS_THREADS;
    for (uint64_t i = first + (uint64_t)blockIdx.x * MOMENTS_THREADS + threadIdx.x; i < n; i += stride) {
        double s = sum[i], q = sq[i];
        moments_merge(pass[i], nb, s, q);
        sum[i] = s; sq[i] = q;
        pass[i] = 0.0;
    }
}

__global__ __launch_bounds__(256) void moments_error_kernel(const double* __restrict__ sum, const double* __restrict__ sq, double Nd, double Bm1, uint32_t n_px,
                                                            double* __restrict__ e2_out, double tau2, unsigned long long* stats) {
    const uint32_t stride = gridDim.x * MOMENTS_THREADS;
    uint32_t conv = 0u, unconv = 0u, nonfinite = 0u;          // (a lane sees at most n_px / stride + 1 pixels, a wave 64 times that: n_px < 2^31)
    double mx = 0.0;
    for (uint64_t p = (uint64_t)blockIdx.x * MOMENTS_THREADS + threadIdx.x; p < n_px; p += stride) {
        const double* s = sum + 3u * p;
        const double* q = sq + 3u * p;
        const double S[3] = {s[0], s[1], s[2]}, Q[3] = {q[0], q[1], q[2]};
        const double e = moments_pixel_e2(S, Q, Nd, Bm1);
        if (e2_out) e2_out[p] = e;
        if (!moments_finite(e)) nonfinite++;
        else {
            if (e <= tau2) conv++; else unconv++;
            if (e > mx) mx = e;
        }
    }
    if (!stats) return;                                        // (uniform: a kernel argument)
    unsigned long long mbits = (unsigned long long)__double_as_longlong(mx);      // mx >= +0.0: its bit pattern orders as it does
    for (int off = 32; off > 0; off >>= 1) {
        conv += __shfl_xor(conv, off, 64);
        unconv += __shfl_xor(unconv, off, 64);
        nonfinite += __shfl_xor(nonfinite, off, 64);
        const unsigned long long other = __shfl_xor(mbits, off, 64);
        mbits = other > mbits ? other : mbits;
    }
    __shared__ unsigned long long part[MOMENTS_THREADS / 64u][MOMENTS_STATS_WORDS];
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* w = part[threadIdx.x >> 6];
        w[MOMENTS_CONVERGED] = conv; w[MOMENTS_UNCONVERGED] = unconv; w[MOMENTS_NONFINITE] = nonfinite; w[MOMENTS_MAX_E2] = mbits;
    }
    __syncthreads();                                           // (every lane of the workgroup is here: `stats` is uniform)
    if (threadIdx.x == 0u) {
        unsigned long long c = 0ull, u = 0ull, nf = 0ull, mb = 0ull;
        for (uint32_t k = 0; k < MOMENTS_THREADS / 64u; k++) {
            c += part[k][MOMENTS_CONVERGED]; u += part[k][MOMENTS_UNCONVERGED]; nf += part[k][MOMENTS_NONFINITE];
            mb = part[k][MOMENTS_MAX_E2] > mb ? part[k][MOMENTS_MAX_E2] : mb;
        }
        if (c) atomicAdd(&stats[MOMENTS_CONVERGED], c);
        if (u) atomicAdd(&stats[MOMENTS_UNCONVERGED], u);
        if (nf) atomicAdd(&stats[MOMENTS_NONFINITE], nf);
        if (mb) atomicMax(&stats[MOMENTS_MAX_E2], mb);
    }
}

static uint32_t blocks_for(uint64_t n, uint32_t most = MOMENTS_MAX_BLOCKS) {
    const uint64_t b = (n + MOMENTS_THREADS - 1u) / MOMENTS_THREADS;
    return (uint32_t)(b > most ? most : b);
}

int launch_moments_merge(double* d_pass_sum, uint64_t n_samples, double* d_rgb_sum, double* d_sq_sum, uint64_t n, void* stream) {
    if (n == 0u) return 0;
    const bool aligned16 = ((((uintptr_t)d_pass_sum) | ((uintptr_t)d_rgb_sum) | ((uintptr_t)d_sq_sum)) & 15u) == 0u;
    const uint64_t n_pairs = aligned16 ? n / 2u : 0u;
    const double nb = (double)n_samples;
    if (n_pairs) hipLaunchKernelGGL(moments_merge2_kernel, dim3(blocks_for(n_pairs)), dim3(MOMENTS_THREADS), 0, (hipStream_t)stream, (d2*)d_pass_sum, nb, (d2*)d_rgb_sum, (d2*)d_sq_sum, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(moments_merge1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(MOMENTS_THREADS), 0, (hipStream_t)stream, d_pass_sum, nb, d_rgb_sum, d_sq_sum, 2u * n_pairs, n);
    return (int)hipGetLastError();
}

int launch_moments_error(const double* d_rgb_sum, const double* d_sq_sum, uint64_t samples, uint64_t passes, uint32_t n_px, double* d_e2_out,
                         double tau2, unsigned long long* d_stats, void* stream) {
    if (n_px == 0u) return 0;
    hipLaunchKernelGGL(moments_error_kernel, dim3(blocks_for(n_px, MOMENTS_ERROR_MAX_BLOCKS)), dim3(MOMENTS_THREADS), 0, (hipStream_t)stream, d_rgb_sum, d_sq_sum, (double)samples,
                       (double)(passes - 1u), n_px, d_e2_out, tau2, d_stats);
    return (int)hipGetLastError();
}

} // namespace rt

// csrc/rt_reproject.hip — the two kernels of temporal accumulation (rt_reproject.h): the reprojection of a frame's history into a new view
// (R) and the blend of a frame with a history (B), for rt_reproject, rt_reproject_device, rt_temporal_blend_device, rt_progressive_set_view
// and rt_progressive_resolve_temporal_rgb8 (include/rt_amd.h).  A translation unit of its own: no other unit's code object changes when this
// file does.
//
// Exactness: the build's -ffp-contract=off -fno-fast-math make `/` the IEEE-correct f64 division and keep every operation one rounding, and
// reproject_pixel / blend_count are the host twin's own functions (rt_reproject_cpu.cpp).
//
// REPROJECT: one new-view pixel per lane, no loop, no LDS, no atomics.  A lane reads its own 128-byte record (consecutive lanes, consecutive
// records: every byte of every line fetched belongs to the wave, though only words [0], [2..7] and [12] are used), and per tap 64 of the 128
// bytes of a previous record, 24 bytes of sums and a 4-byte count.  The taps of neighbouring lanes are neighbouring or the same previous
// pixels wherever the two views are close, so the gather hits in L2; under a large camera move it degrades to one line per tap.  The R0
// constants travel by value in the kernel's arguments (scalar registers).  28 bytes out per pixel.  The records are 16-byte aligned, which
// the kernel tells the compiler so that pairs of words move as one 16-byte access.
// BLEND: a flat stream over the 3 n_px doubles (16-byte PAIR form when every sums buffer is 16-byte aligned, else the scalar form, as in
// rt_moments.hip's merge), one element per lane and no loop; the lanes of the first n_px elements also blend one count each, so the counts
// are a second flat stream in the same launch: 48 B in and 24 out per pixel for the sums, 8 in (4 without counts) and 4 out for the counts.
#include <hip/hip_runtime.h>
#include "rt_reproject.h"

namespace rt {

typedef double d2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void reproject_kernel(const ReprojectConsts K, const double* __restrict__ prev_sum, const uint32_t* __restrict__ prev_counts,
                                                        const double* __restrict__ prev_hits, const double* __restrict__ cur_hits,
                                                        double* __restrict__ hist_sum, uint32_t* __restrict__ hist_counts, uint32_t n_px) {
    const uint64_t p = (uint64_t)blockIdx.x * REPROJECT_THREADS + threadIdx.x;
    if (p >= n_px) return;
    const double* ph = (const double*)__builtin_assume_aligned(prev_hits, 16);
    const double* ch = (const double*)__builtin_assume_aligned(cur_hits, 16);
    double out3[3];
    const uint32_t Nh = reproject_pixel(K, prev_sum, prev_counts, ph, ch, p, out3);
    double* o = hist_sum + 3u * p;
    o[0] = out3[0]; o[1] = out3[1]; o[2] = out3[2];
    hist_counts[p] = Nh;
}

// (B): doubles 2 i and 2 i + 1, and count i when i < n_cnt
__global__ __launch_bounds__(256) void temporal_blend2_kernel(const d2* sum, const uint32_t* cnt, uint64_t Ns, const d2* __restrict__ hsum,
                                                              const uint32_t* __restrict__ hcnt, d2* sum_out, uint32_t* cnt_out, uint64_t n_pairs, uint64_t n_cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * REPROJECT_THREADS + threadIdx.x;
    if (i >= n_pairs) return;
    const d2 a = sum[i], b = hsum[i];
    d2 r;
    r.x = a.x + b.x; r.y = a.y + b.y;
    sum_out[i] = r;
    if (i < n_cnt) cnt_out[i] = blend_count(cnt ? (uint64_t)cnt[i] : Ns, hcnt[i]);
}
// (sum_out may be sum and cnt_out may be cnt: neither pair is __restrict__)
__global__ __launch_bounds__(256) void temporal_blend1_kernel(const double* sum, const uint32_t* cnt, uint64_t Ns, const double* __restrict__ hsum,
                                                              const uint32_t* __restrict__ hcnt, double* sum_out, uint32_t* cnt_out, uint64_t first, uint64_t n,
                                                              uint64_t n_cnt) {
    const uint64_t i = first + (uint64_t)blockIdx.x * REPROJECT_THREADS + threadIdx.x;
    if (i >= n) return;
    sum_out[i] = sum[i] + hsum[i];
    if (i < n_cnt) cnt_out[i] = blend_count(cnt ? (uint64_t)cnt[i] : Ns, hcnt[i]);
}

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + REPROJECT_THREADS - 1u) / REPROJECT_THREADS); }     // n <= 3 (2^31 - 1): fits

int launch_reproject(const ReprojectConsts& K, const double* d_prev_sum, const uint32_t* d_prev_counts, const double* d_prev_hits, const double* d_cur_hits,
                     double* d_hist_sum_out, uint32_t* d_hist_counts_out, void* stream) {
    const uint32_t n_px = K.W * K.H;
    if (n_px == 0u) return 0;
    hipLaunchKernelGGL(reproject_kernel, dim3(blocks_for(n_px)), dim3(REPROJECT_THREADS), 0, (hipStream_t)stream, K, d_prev_sum, d_prev_counts, d_prev_hits, d_cur_hits,
                       d_hist_sum_out, d_hist_counts_out, n_px);
    return (int)hipGetLastError();
}

int launch_temporal_blend(const double* d_rgb_sum, const uint32_t* d_counts, uint64_t samples, const double* d_hist_sum, const uint32_t* d_hist_counts,
                          uint32_t n_px, double* d_sum_out, uint32_t* d_counts_out, void* stream) {
    const uint64_t n = (uint64_t)n_px * 3u;
    if (n == 0u) return 0;
    const bool aligned16 = ((((uintptr_t)d_rgb_sum) | ((uintptr_t)d_hist_sum) | ((uintptr_t)d_sum_out)) & 15u) == 0u;
    // the pair form blends the counts only when its n / 2 lanes cover all n_px of them (n_px >= 2); else everything goes through the scalar form
    const uint64_t n_pairs = (aligned16 && n_px >= 2u) ? n / 2u : 0u;
    if (n_pairs) hipLaunchKernelGGL(temporal_blend2_kernel, dim3(blocks_for(n_pairs)), dim3(REPROJECT_THREADS), 0, (hipStream_t)stream, (const d2*)d_rgb_sum, d_counts, samples,
                                    (const d2*)d_hist_sum, d_hist_counts, (d2*)d_sum_out, d_counts_out, n_pairs, (uint64_t)n_px);
    // the tail of the pair form (one double, first >= n_px: no count), or the whole frame
    if (2u * n_pairs < n) hipLaunchKernelGGL(temporal_blend1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(REPROJECT_THREADS), 0, (hipStream_t)stream, d_rgb_sum, d_counts,
                                             samples, d_hist_sum, d_hist_counts, d_sum_out, d_counts_out, 2u * n_pairs, n, (uint64_t)n_px);
    return (int)hipGetLastError();
}

} // namespace rt

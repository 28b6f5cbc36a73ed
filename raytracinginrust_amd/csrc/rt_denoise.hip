// csrc/rt_denoise.hip — the edge-avoiding a-trous filter of rt_denoise.h on the device, for rt_denoise* and
// rt_progressive_resolve_denoised_rgb8 (include/rt_amd.h).  A translation unit of its own: no path-tracing, query or resolve object
// changes when this file does.
//
// Exactness: the specification (rt_denoise.h) uses + - * / and comparisons only, and the build's -ffp-contract=off -fno-fast-math keep
// every one of them a single IEEE f64 operation here (no fused multiply-add, `/` is the correctly rounded v_div_scale / v_div_fmas /
// v_div_fixup sequence), in the order the host twin (rt_denoise_cpu.cpp) runs them: the two give the same words.
//
// Shape: a pack kernel turns the 24-byte sums and the 128-byte hit records into what the iterations read — a mean padded to {r, g, b, 0}
// (32 B) and a guide {n0, n1, n2, inv_t | x0, x1, x2, key} (64 B), both for 16-byte loads — and each iteration is one launch, one pixel per
// lane, the 25 taps unrolled.  Steps 1 and 2 stage a 16 x 16 tile and its halo in LDS (denoise_filter_lds_kernel); from step 4 on the halo
// no longer fits and the taps are read straight from global memory (denoise_filter_kernel): a wave covers 64 consecutive pixels of a row,
// so a tap row is 2 KB of colour and 4 KB of guide in whole cache lines.  A tap's key half (x, key) is read first; its colour and its
// normal half only if the keys agree.  The last iteration multiplies by the sample count and writes 24-byte sums — the only write that
// may land on the caller's input, which the pack kernel has finished reading by then (stream order).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "rt_denoise.h"

namespace rt {

static const uint32_t DN_BLOCK_X = 64u, DN_BLOCK_Y = 4u;         // one wave per row segment, four rows per workgroup
static const uint32_t DN_LDS_TILE = 16u;                        // the LDS form: 16 x 16 pixels per workgroup

__device__ __forceinline__ bool dn_finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ double dn_stop(double t) { return t > 0.0 ? t * t : 0.0; }

__global__ __launch_bounds__(256) void denoise_pack_kernel(const double* __restrict__ sum, double samples, const double2* __restrict__ hits,
                                                           uint32_t flags, double2* __restrict__ color, double2* __restrict__ guide, uint32_t n_px) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_px) return;
    if (color) {
        const double* s = sum + (size_t)p * 3u;
        const double r = s[0] / samples, g = s[1] / samples, b = s[2] / samples;
        double2* c = color + (size_t)p * 2u;
        c[0] = make_double2(r, g); c[1] = make_double2(b, 0.0);
    }
    if (guide) {
        const double2* h = hits + (size_t)p * 8u;                 // a record: 16 doubles
        const double2 ht = h[0], x01 = h[1], x2n0 = h[2], n12 = h[3], vm = h[5];      // {hit, t} {x0, x1} {x2, n0} {n1, n2} {v, material}
        const double key = ht.x != 0.0 ? ((flags & 1u) ? vm.y + 2.0 : 1.0) : 0.0;
        double2* g = guide + (size_t)p * 4u;
        g[0] = make_double2(x2n0.y, n12.x); g[1] = make_double2(n12.y, 1.0 / ht.y);
        g[2] = x01;                         g[3] = make_double2(x2n0.x, key);
    }
}

// LAST: write c * samples as 24-byte sums to `out` instead of a packed colour
template <bool LAST>
__global__ __launch_bounds__(256) void denoise_filter_kernel(const double2* __restrict__ color_in, const double2* __restrict__ guide, double* out,
                                                             uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t step, double ic_i, double in, double ip,
                                                             double samples) {
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int64_t x = (int64_t)tile_x * DN_BLOCK_X + threadIdx.x, y = (int64_t)tile_y * DN_BLOCK_Y + threadIdx.y;
    if (x >= (int64_t)W || y >= (int64_t)H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const double2 c01 = color_in[p * 2u], c2_ = color_in[p * 2u + 1u];
    const double2 g0 = guide[p * 4u], g1 = guide[p * 4u + 1u], g2 = guide[p * 4u + 2u], g3 = guide[p * 4u + 3u];
    const double cp0 = c01.x, cp1 = c01.y, cp2 = c2_.x;
    const double np0 = g0.x, np1 = g0.y, np2 = g1.x, inv_t = g1.y, xp0 = g2.x, xp1 = g2.y, xp2 = g3.x, key = g3.y;
    const bool cp_finite = dn_finite(cp0) && dn_finite(cp1) && dn_finite(cp2);
    const bool guided = key != 0.0;
    constexpr double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wsum = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = y + (int64_t)dy * step;
        if (qy < 0 || qy >= (int64_t)H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = x + (int64_t)dx * step;
            if (qx < 0 || qx >= (int64_t)W) continue;
            const size_t q = (size_t)qy * W + (size_t)qx;
            const double2 q2 = guide[q * 4u + 2u], q3 = guide[q * 4u + 3u];
            if (q3.y != key) continue;
            const double2 d01 = color_in[q * 2u], d2_ = color_in[q * 2u + 1u];
            const double cq0 = d01.x, cq1 = d01.y, cq2 = d2_.x;
            if (!(dn_finite(cq0) && dn_finite(cq1) && dn_finite(cq2))) continue;
            const double k = h[dy + 2] * h[dx + 2];
            const double e0 = cq0 - cp0, e1 = cq1 - cp1, e2 = cq2 - cp2;
            double d = (e0 * e0 + e1 * e1) + e2 * e2;
            double wc = dn_stop(1.0 - d * ic_i);
            if (!cp_finite) wc = 1.0;
            double wn = 1.0, wp = 1.0;
            if (guided) {
                const double2 q0 = guide[q * 4u], q1 = guide[q * 4u + 1u];
                const double m0 = q0.x - np0, m1 = q0.y - np1, m2 = q1.x - np2;
                d = (m0 * m0 + m1 * m1) + m2 * m2;
                wn = dn_stop(1.0 - d * in);
                const double r0 = q2.x - xp0, r1 = q2.y - xp1, r2 = q3.x - xp2;
                const double g = ((np0 * r0 + np1 * r1) + np2 * r2) * inv_t;
                wp = dn_stop(1.0 - (g * g) * ip);
            }
            const double w = ((k * wc) * wn) * wp;
            acc0 += w * cq0; acc1 += w * cq1; acc2 += w * cq2;
            wsum += w;
        }
    }
    const bool any = wsum > 0.0;
    const double o0 = any ? acc0 / wsum : cp0, o1 = any ? acc1 / wsum : cp1, o2 = any ? acc2 / wsum : cp2;
    if (LAST) {
        double* o = out + p * 3u;
        o[0] = o0 * samples; o[1] = o1 * samples; o[2] = o2 * samples;
    } else {
        double2* o = reinterpret_cast<double2*>(out) + p * 2u;
        o[0] = make_double2(o0, o1); o[1] = make_double2(o2, 0.0);
    }
}

// The same iteration for the small steps with the taps' data staged in LDS: a workgroup takes a 16 x 16 tile, loads the tile plus its halo of
// 2 * STEP pixels once — colour and guide as six planes of 16-byte words, so that consecutive lanes read consecutive words — and its lanes
// read their 25 taps from there.  (16 + 4 STEP)^2 x 96 bytes: 38 KB at step 1, 55 KB at step 2.  Entries outside the frame are never read.
template <bool LAST, int STEP>
__global__ __launch_bounds__(256) void denoise_filter_lds_kernel(const double2* __restrict__ color_in, const double2* __restrict__ guide, double* out,
                                                                 uint32_t W, uint32_t H, uint32_t tiles_x, double ic_i, double in, double ip, double samples) {
    constexpr int T = (int)DN_LDS_TILE + 4 * STEP, N = T * T;
    __shared__ double2 tile[6 * N];                               // planes: c01, c2_, g0, g1, g2, g3
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int64_t x0 = (int64_t)tile_x * DN_LDS_TILE - 2 * STEP, y0 = (int64_t)tile_y * DN_LDS_TILE - 2 * STEP;
    for (int i = (int)threadIdx.x; i < N; i += 256) {
        const int64_t gy = y0 + i / T, gx = x0 + i % T;
        if (gy < 0 || gy >= (int64_t)H || gx < 0 || gx >= (int64_t)W) continue;
        const size_t q = (size_t)gy * W + (size_t)gx;
        tile[i] = color_in[q * 2u]; tile[N + i] = color_in[q * 2u + 1u];
        tile[2 * N + i] = guide[q * 4u]; tile[3 * N + i] = guide[q * 4u + 1u]; tile[4 * N + i] = guide[q * 4u + 2u]; tile[5 * N + i] = guide[q * 4u + 3u];
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x % DN_LDS_TILE), ly = (int)(threadIdx.x / DN_LDS_TILE);
    const int64_t x = (int64_t)tile_x * DN_LDS_TILE + lx, y = (int64_t)tile_y * DN_LDS_TILE + ly;
    if (x >= (int64_t)W || y >= (int64_t)H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const int c = (ly + 2 * STEP) * T + (lx + 2 * STEP);
    const double2 c01 = tile[c], c2_ = tile[N + c], g0 = tile[2 * N + c], g1 = tile[3 * N + c], g2 = tile[4 * N + c], g3 = tile[5 * N + c];
    const double cp0 = c01.x, cp1 = c01.y, cp2 = c2_.x;
    const double np0 = g0.x, np1 = g0.y, np2 = g1.x, inv_t = g1.y, xp0 = g2.x, xp1 = g2.y, xp2 = g3.x, key = g3.y;
    const bool cp_finite = dn_finite(cp0) && dn_finite(cp1) && dn_finite(cp2);
    const bool guided = key != 0.0;
    constexpr double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wsum = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = y + dy * STEP;
        if (qy < 0 || qy >= (int64_t)H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = x + dx * STEP;
            if (qx < 0 || qx >= (int64_t)W) continue;
            const int q = c + dy * STEP * T + dx * STEP;
            const double2 q2 = tile[4 * N + q], q3 = tile[5 * N + q];
            if (q3.y != key) continue;
            const double2 d01 = tile[q], d2_ = tile[N + q];
            const double cq0 = d01.x, cq1 = d01.y, cq2 = d2_.x;
            if (!(dn_finite(cq0) && dn_finite(cq1) && dn_finite(cq2))) continue;
            const double k = h[dy + 2] * h[dx + 2];
            const double e0 = cq0 - cp0, e1 = cq1 - cp1, e2 = cq2 - cp2;
            double d = (e0 * e0 + e1 * e1) + e2 * e2;
            double wc = dn_stop(1.0 - d * ic_i);
            if (!cp_finite) wc = 1.0;
            double wn = 1.0, wp = 1.0;
            if (guided) {
                const double2 q0 = tile[2 * N + q], q1 = tile[3 * N + q];
                const double m0 = q0.x - np0, m1 = q0.y - np1, m2 = q1.x - np2;
                d = (m0 * m0 + m1 * m1) + m2 * m2;
                wn = dn_stop(1.0 - d * in);
                const double r0 = q2.x - xp0, r1 = q2.y - xp1, r2 = q3.x - xp2;
                const double g = ((np0 * r0 + np1 * r1) + np2 * r2) * inv_t;
                wp = dn_stop(1.0 - (g * g) * ip);
            }
            const double w = ((k * wc) * wn) * wp;
            acc0 += w * cq0; acc1 += w * cq1; acc2 += w * cq2;
            wsum += w;
        }
    }
    const bool any = wsum > 0.0;
    const double o0 = any ? acc0 / wsum : cp0, o1 = any ? acc1 / wsum : cp1, o2 = any ? acc2 / wsum : cp2;
    if (LAST) {
        double* o = out + p * 3u;
        o[0] = o0 * samples; o[1] = o1 * samples; o[2] = o2 * samples;
    } else {
        double2* o = reinterpret_cast<double2*>(out) + p * 2u;
        o[0] = make_double2(o0, o1); o[1] = make_double2(o2, 0.0);
    }
}

template <bool LAST, int STEP>
static int launch_filter_lds(const double2* ci, const double2* gd, double* out, uint32_t W, uint32_t H, double ic_i, double in, double ip, double samples, hipStream_t stream) {
    const uint32_t tiles_x = (W + DN_LDS_TILE - 1u) / DN_LDS_TILE, tiles_y = (H + DN_LDS_TILE - 1u) / DN_LDS_TILE;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((denoise_filter_lds_kernel<LAST, STEP>), dim3((uint32_t)blocks), dim3(256), 0, stream, ci, gd, out, W, H, tiles_x, ic_i, in, ip, samples);
    return (int)hipGetLastError();
}

int launch_denoise_pack(const double* d_rgb_sum, uint64_t samples, const double* d_hits, uint32_t flags, double* d_color, double* d_guide,
                        uint32_t n_px, void* stream) {
    const uint32_t threads = 256u, blocks = (n_px + threads - 1u) / threads;
    if (blocks == 0u) return (int)hipSuccess;
    hipLaunchKernelGGL(denoise_pack_kernel, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, d_rgb_sum, (double)samples,
                       reinterpret_cast<const double2*>(d_hits), flags, d_rgb_sum ? reinterpret_cast<double2*>(d_color) : nullptr,
                       d_hits ? reinterpret_cast<double2*>(d_guide) : nullptr, n_px);
    return (int)hipGetLastError();
}

int launch_denoise_filter(const double* d_color_in, const double* d_guide, double* d_color_out, double* d_rgb_sum_out, uint32_t W, uint32_t H,
                          uint32_t step, double ic_i, double in, double ip, uint64_t samples, void* stream) {
    const uint32_t tiles_x = (W + DN_BLOCK_X - 1u) / DN_BLOCK_X, tiles_y = (H + DN_BLOCK_Y - 1u) / DN_BLOCK_Y;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks == 0u) return (int)hipSuccess;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    const dim3 grid((uint32_t)blocks), block(DN_BLOCK_X, DN_BLOCK_Y);
    const double2* ci = reinterpret_cast<const double2*>(d_color_in); const double2* gd = reinterpret_cast<const double2*>(d_guide);
    // steps 1 and 2 from LDS tiles: *measured* 3.9x and 3.0x the direct form's rate at 3840 x 2160; RT_DENOISE_NO_LDS is the
    // A/B switch tools/denoise_probe.py measures that with
    if (step <= 2u && !std::getenv("RT_DENOISE_NO_LDS")) {
        double* o = d_rgb_sum_out ? d_rgb_sum_out : d_color_out;
        if (step == 1u) return d_rgb_sum_out ? launch_filter_lds<true, 1>(ci, gd, o, W, H, ic_i, in, ip, (double)samples, (hipStream_t)stream)
                                             : launch_filter_lds<false, 1>(ci, gd, o, W, H, ic_i, in, ip, (double)samples, (hipStream_t)stream);
        return d_rgb_sum_out ? launch_filter_lds<true, 2>(ci, gd, o, W, H, ic_i, in, ip, (double)samples, (hipStream_t)stream)
                             : launch_filter_lds<false, 2>(ci, gd, o, W, H, ic_i, in, ip, (double)samples, (hipStream_t)stream);
    }
    if (d_rgb_sum_out) hipLaunchKernelGGL(denoise_filter_kernel<true>, grid, block, 0, (hipStream_t)stream, ci, gd, d_rgb_sum_out, W, H, tiles_x, step, ic_i, in, ip, (double)samples);
    else hipLaunchKernelGGL(denoise_filter_kernel<false>, grid, block, 0, (hipStream_t)stream, ci, gd, d_color_out, W, H, tiles_x, step, ic_i, in, ip, (double)samples);
    return (int)hipGetLastError();
}

} // namespace rt

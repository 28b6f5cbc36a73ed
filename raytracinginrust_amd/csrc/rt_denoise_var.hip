// csrc/rt_denoise_var.hip — the variance-guided denoiser of rt_denoise_var.h on the device, and the variance frame of rt_moments.h (4) it
// takes as input, for rt_denoise_variance*, rt_moments_variance_device and rt_progressive_resolve_denoised_variance_rgb8
// (include/rt_amd.h).  A translation unit of its own: rt_denoise.hip's and rt_moments.hip's code objects — and every path-tracing, query and
// resolve object — do not change when this file does.
//
// Exactness: as in rt_denoise.hip.  The specification uses + - * / and comparisons only, the build's -ffp-contract=off -fno-fast-math keep
// every one of them a single IEEE f64 operation, in the order the host twin (rt_denoise_var_cpu.cpp) runs them; denoise_var_scalar,
// denoise_var_stop and moments_channel_variance are the host twin's own functions.
//
// Shape: rt_denoise.hip's.  The guide is packed by its launch_denoise_pack.  The pack kernel here writes {r, g, b, v} into the workspace's
// SECOND colour frame, the 3 x 3 prefilter of v reads that and writes the first, and the iterations alternate from there as they do in the
// plain filter: the same 128 bytes per pixel.  An iteration is one launch, one pixel per lane, the 25 taps unrolled; steps 1 and 2 stage a
// 16 x 16 tile and its halo in LDS — the tile holds the colour's fourth word already, so it is 38 400 B at step 1 and 55 296 B at step 2 as
// before — and larger steps read their taps from global memory.  Both forms share one tap function.  The last iteration writes 24-byte
// sums and, when asked, the 8-byte filtered variance.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "rt_denoise_var.h"
#include "rt_moments.h"

namespace rt {

typedef double d2 __attribute__((ext_vector_type(2)));

static const uint32_t DNV_BLOCK_X = 64u, DNV_BLOCK_Y = 4u;       // one wave per row segment, four rows per workgroup
static const uint32_t DNV_LDS_TILE = 16u;                       // the LDS form: 16 x 16 pixels per workgroup

__device__ __forceinline__ bool dnv_finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ double dnv_stop(double t) { return t > 0.0 ? t * t : 0.0; }

// ---- rt_moments.h (4): element-wise, 16 bytes per access when the three buffers are 16-byte aligned
__global__ __launch_bounds__(256) void moments_variance2_kernel(const d2* __restrict__ sum, const d2* __restrict__ sq, double Nd, double Bm1, d2* __restrict__ var, uint64_t n_pairs) {
    const uint64_t stride = (uint64_t)gridDim.x * DNV_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DNV_THREADS + threadIdx.x; i < n_pairs; i += stride) {
        const d2 s = sum[i], q = sq[i];
        d2 v;
        v.x = moments_channel_variance(s.x, q.x, Nd, Bm1);
        v.y = moments_channel_variance(s.y, q.y, Nd, Bm1);
        var[i] = v;
    }
}
__global__ __launch_bounds__(256) void moments_variance_kernel(const double* __restrict__ sum, const double* __restrict__ sq, double Nd, double Bm1, double* __restrict__ var, uint64_t first, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * DNV_THREADS;
    for (uint64_t i = first + (uint64_t)blockIdx.x * DNV_THREADS + threadIdx.x; i < n; i += stride) var[i] = moments_channel_variance(sum[i], sq[i], Nd, Bm1);
}

// ---- (B)
__global__ __launch_bounds__(256) void denoise_var_pack_kernel(const double* __restrict__ sum, double samples, const double* __restrict__ var, double2* __restrict__ color, uint32_t n_px) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_px) return;
    const double* s = sum + (size_t)p * 3u;
    const double* V = var + (size_t)p * 3u;
    const double r = s[0] / samples, g = s[1] / samples, b = s[2] / samples;
    const double v = denoise_var_scalar(V[0], V[1], V[2]);
    double2* c = color + (size_t)p * 2u;
    c[0] = make_double2(r, g); c[1] = make_double2(b, v);
}

// ---- (C): 9 taps of 16 bytes (the colour's {b, v} half) and 16 bytes (the guide's {x2, key} half)
__global__ __launch_bounds__(256) void denoise_var_prefilter_kernel(const double2* __restrict__ color_in, const double2* __restrict__ guide, double2* __restrict__ color_out,
                                                                    uint32_t W, uint32_t H, uint32_t tiles_x) {
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int64_t x = (int64_t)tile_x * DNV_BLOCK_X + threadIdx.x, y = (int64_t)tile_y * DNV_BLOCK_Y + threadIdx.y;
    if (x >= (int64_t)W || y >= (int64_t)H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const double key = guide[p * 4u + 3u].y;
    constexpr double b3[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};
    double acc = 0.0, wsum = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int64_t qy = y + dy;
        if (qy < 0 || qy >= (int64_t)H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int64_t qx = x + dx;
            if (qx < 0 || qx >= (int64_t)W) continue;
            const size_t q = (size_t)qy * W + (size_t)qx;
            if (guide[q * 4u + 3u].y != key) continue;
            const double k = b3[dy + 1] * b3[dx + 1];
            acc += k * color_in[q * 2u + 1u].y; wsum += k;
        }
    }
    const double2 c01 = color_in[p * 2u], c2v = color_in[p * 2u + 1u];
    color_out[p * 2u] = c01; color_out[p * 2u + 1u] = make_double2(c2v.x, acc / wsum);
}

// ---- (D)
struct DnvCentre {
    double c0, c1, c2, v, n0, n1, n2, inv_t, x0, x1, x2, key;
    bool c_finite, guided;
    __device__ __forceinline__ DnvCentre(double2 c01, double2 c2v, double2 g0, double2 g1, double2 g2, double2 g3)
        : c0(c01.x), c1(c01.y), c2(c2v.x), v(c2v.y), n0(g0.x), n1(g0.y), n2(g1.x), inv_t(g1.y), x0(g2.x), x1(g2.y), x2(g3.x), key(g3.y) {
        c_finite = dnv_finite(c0) && dnv_finite(c1) && dnv_finite(c2);
        guided = key != 0.0;
    }
};
struct DnvSums { double a0 = 0.0, a1 = 0.0, a2 = 0.0, va = 0.0, w = 0.0; };

// One tap whose key agrees: d01, d2v its colour, q2, q3 the guide's key half; normals(q0, q1) fetches the normal half, only for guided pixels.
template <class Normals>
__device__ __forceinline__ void dnv_tap(const DnvCentre& P, DnvSums& S, double k, double2 d01, double2 d2v, double2 q2, double2 q3, double kv, double in, double ip, Normals normals) {
    const double cq0 = d01.x, cq1 = d01.y, cq2 = d2v.x, vq = d2v.y;
    if (!(dnv_finite(cq0) && dnv_finite(cq1) && dnv_finite(cq2))) return;
    const double e0 = cq0 - P.c0, e1 = cq1 - P.c1, e2 = cq2 - P.c2;
    double d = (e0 * e0 + e1 * e1) + e2 * e2;
    double wc = denoise_var_stop(d, P.v, vq, kv);
    if (!P.c_finite) wc = 1.0;
    double wn = 1.0, wp = 1.0;
    if (P.guided) {
        double2 q0, q1;
        normals(q0, q1);
        const double m0 = q0.x - P.n0, m1 = q0.y - P.n1, m2 = q1.x - P.n2;
        d = (m0 * m0 + m1 * m1) + m2 * m2;
        wn = dnv_stop(1.0 - d * in);
        const double r0 = q2.x - P.x0, r1 = q2.y - P.x1, r2 = q3.x - P.x2;
        const double g = ((P.n0 * r0 + P.n1 * r1) + P.n2 * r2) * P.inv_t;
        wp = dnv_stop(1.0 - (g * g) * ip);
    }
    const double w = ((k * wc) * wn) * wp;
    S.a0 += w * cq0; S.a1 += w * cq1; S.a2 += w * cq2;
    S.va += (w * w) * vq;
    S.w += w;
}

// LAST: c * samples as 24-byte sums to `out` and, when given, v to var_out; else a packed colour {c, v} to `out`
template <bool LAST>
__device__ __forceinline__ void dnv_write(const DnvCentre& P, const DnvSums& S, size_t p, double* out, double* var_out, double samples) {
    const bool any = S.w > 0.0;
    const double o0 = any ? S.a0 / S.w : P.c0, o1 = any ? S.a1 / S.w : P.c1, o2 = any ? S.a2 / S.w : P.c2;
    const double ov = any ? S.va / (S.w * S.w) : P.v;
    if (LAST) {
        double* o = out + p * 3u;
        o[0] = o0 * samples; o[1] = o1 * samples; o[2] = o2 * samples;
        if (var_out) var_out[p] = ov;
    } else {
        double2* o = reinterpret_cast<double2*>(out) + p * 2u;
        o[0] = make_double2(o0, o1); o[1] = make_double2(o2, ov);
    }
}

template <bool LAST>
__global__ __launch_bounds__(256) void denoise_var_filter_kernel(const double2* __restrict__ color_in, const double2* __restrict__ guide, double* out, double* var_out,
                                                                 uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t step, double kv, double in, double ip, double samples) {
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int64_t x = (int64_t)tile_x * DNV_BLOCK_X + threadIdx.x, y = (int64_t)tile_y * DNV_BLOCK_Y + threadIdx.y;
    if (x >= (int64_t)W || y >= (int64_t)H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const DnvCentre P(color_in[p * 2u], color_in[p * 2u + 1u], guide[p * 4u], guide[p * 4u + 1u], guide[p * 4u + 2u], guide[p * 4u + 3u]);
    constexpr double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    DnvSums S;
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
            if (q3.y != P.key) continue;
            dnv_tap(P, S, h[dy + 2] * h[dx + 2], color_in[q * 2u], color_in[q * 2u + 1u], q2, q3, kv, in, ip,
                    [&](double2& q0, double2& q1) { q0 = guide[q * 4u]; q1 = guide[q * 4u + 1u]; });
        }
    }
    dnv_write<LAST>(P, S, p, out, var_out, samples);
}

// The same iteration for steps 1 and 2 with the taps' data staged in LDS, as denoise_filter_lds_kernel: the tile plus its halo of 2 * STEP
// pixels as six planes of 16-byte words.  (16 + 4 STEP)^2 x 96 bytes.  Entries outside the frame are never read.
template <bool LAST, int STEP>
__global__ __launch_bounds__(256) void denoise_var_filter_lds_kernel(const double2* __restrict__ color_in, const double2* __restrict__ guide, double* out, double* var_out,
                                                                     uint32_t W, uint32_t H, uint32_t tiles_x, double kv, double in, double ip, double samples) {
    constexpr int T = (int)DNV_LDS_TILE + 4 * STEP, N = T * T;
    __shared__ double2 tile[6 * N];                               // planes: c01, c2v, g0, g1, g2, g3
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int64_t x0 = (int64_t)tile_x * DNV_LDS_TILE - 2 * STEP, y0 = (int64_t)tile_y * DNV_LDS_TILE - 2 * STEP;
    for (int i = (int)threadIdx.x; i < N; i += 256) {
        const int64_t gy = y0 + i / T, gx = x0 + i % T;
        if (gy < 0 || gy >= (int64_t)H || gx < 0 || gx >= (int64_t)W) continue;
        const size_t q = (size_t)gy * W + (size_t)gx;
        tile[i] = color_in[q * 2u]; tile[N + i] = color_in[q * 2u + 1u];
        tile[2 * N + i] = guide[q * 4u]; tile[3 * N + i] = guide[q * 4u + 1u]; tile[4 * N + i] = guide[q * 4u + 2u]; tile[5 * N + i] = guide[q * 4u + 3u];
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x % DNV_LDS_TILE), ly = (int)(threadIdx.x / DNV_LDS_TILE);
    const int64_t x = (int64_t)tile_x * DNV_LDS_TILE + lx, y = (int64_t)tile_y * DNV_LDS_TILE + ly;
    if (x >= (int64_t)W || y >= (int64_t)H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const int c = (ly + 2 * STEP) * T + (lx + 2 * STEP);
    const DnvCentre P(tile[c], tile[N + c], tile[2 * N + c], tile[3 * N + c], tile[4 * N + c], tile[5 * N + c]);
    constexpr double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    DnvSums S;
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
            if (q3.y != P.key) continue;
            dnv_tap(P, S, h[dy + 2] * h[dx + 2], tile[q], tile[N + q], q2, q3, kv, in, ip,
                    [&](double2& q0, double2& q1) { q0 = tile[2 * N + q]; q1 = tile[3 * N + q]; });
        }
    }
    dnv_write<LAST>(P, S, p, out, var_out, samples);
}

template <bool LAST, int STEP>
static int launch_var_filter_lds(const double2* ci, const double2* gd, double* out, double* var_out, uint32_t W, uint32_t H, double kv, double in, double ip, double samples, hipStream_t stream) {
    const uint32_t tiles_x = (W + DNV_LDS_TILE - 1u) / DNV_LDS_TILE, tiles_y = (H + DNV_LDS_TILE - 1u) / DNV_LDS_TILE;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL((denoise_var_filter_lds_kernel<LAST, STEP>), dim3((uint32_t)blocks), dim3(256), 0, stream, ci, gd, out, var_out, W, H, tiles_x, kv, in, ip, samples);
    return (int)hipGetLastError();
}

static uint32_t variance_blocks_for(uint64_t n) {
    const uint64_t b = (n + DNV_THREADS - 1u) / DNV_THREADS;
    return (uint32_t)(b > DNV_MAX_BLOCKS ? DNV_MAX_BLOCKS : b);
}

int launch_moments_variance(const double* d_rgb_sum, const double* d_sq_sum, uint64_t samples, uint64_t passes, uint64_t n, double* d_var_out, void* stream) {
    if (n == 0u) return 0;
    const bool aligned16 = ((((uintptr_t)d_rgb_sum) | ((uintptr_t)d_sq_sum) | ((uintptr_t)d_var_out)) & 15u) == 0u;
    const uint64_t n_pairs = aligned16 ? n / 2u : 0u;
    const double Nd = (double)samples, Bm1 = (double)(passes - 1u);
    if (n_pairs) hipLaunchKernelGGL(moments_variance2_kernel, dim3(variance_blocks_for(n_pairs)), dim3(DNV_THREADS), 0, (hipStream_t)stream, (const d2*)d_rgb_sum, (const d2*)d_sq_sum, Nd, Bm1, (d2*)d_var_out, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(moments_variance_kernel, dim3(variance_blocks_for(n - 2u * n_pairs)), dim3(DNV_THREADS), 0, (hipStream_t)stream, d_rgb_sum, d_sq_sum, Nd, Bm1, d_var_out, 2u * n_pairs, n);
    return (int)hipGetLastError();
}

int launch_denoise_var_pack(const double* d_rgb_sum, uint64_t samples, const double* d_var, double* d_color, uint32_t n_px, void* stream) {
    const uint32_t blocks = (n_px + DNV_THREADS - 1u) / DNV_THREADS;
    if (blocks == 0u) return (int)hipSuccess;
    hipLaunchKernelGGL(denoise_var_pack_kernel, dim3(blocks), dim3(DNV_THREADS), 0, (hipStream_t)stream, d_rgb_sum, (double)samples, d_var, reinterpret_cast<double2*>(d_color), n_px);
    return (int)hipGetLastError();
}

int launch_denoise_var_prefilter(const double* d_color_in, const double* d_guide, double* d_color_out, uint32_t W, uint32_t H, void* stream) {
    const uint32_t tiles_x = (W + DNV_BLOCK_X - 1u) / DNV_BLOCK_X, tiles_y = (H + DNV_BLOCK_Y - 1u) / DNV_BLOCK_Y;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks == 0u) return (int)hipSuccess;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(denoise_var_prefilter_kernel, dim3((uint32_t)blocks), dim3(DNV_BLOCK_X, DNV_BLOCK_Y), 0, (hipStream_t)stream, reinterpret_cast<const double2*>(d_color_in),
                       reinterpret_cast<const double2*>(d_guide), reinterpret_cast<double2*>(d_color_out), W, H, tiles_x);
    return (int)hipGetLastError();
}

int launch_denoise_var_filter(const double* d_color_in, const double* d_guide, double* d_color_out, double* d_rgb_sum_out, double* d_var_out,
                              uint32_t W, uint32_t H, uint32_t step, double kv, double in, double ip, uint64_t samples, void* stream) {
    const uint32_t tiles_x = (W + DNV_BLOCK_X - 1u) / DNV_BLOCK_X, tiles_y = (H + DNV_BLOCK_Y - 1u) / DNV_BLOCK_Y;
    const uint64_t blocks = (uint64_t)tiles_x * tiles_y;
    if (blocks == 0u) return (int)hipSuccess;
    if (blocks > 0x7FFFFFFFull) return (int)hipErrorInvalidConfiguration;
    const dim3 grid((uint32_t)blocks), block(DNV_BLOCK_X, DNV_BLOCK_Y);
    const double2* ci = reinterpret_cast<const double2*>(d_color_in); const double2* gd = reinterpret_cast<const double2*>(d_guide);
    const hipStream_t s = (hipStream_t)stream;
    const double n = (double)samples;
    double* o = d_rgb_sum_out ? d_rgb_sum_out : d_color_out;
    // steps 1 and 2 from LDS tiles, as the plain filter's launch; RT_DENOISE_NO_LDS is the same A/B switch
    if (step <= 2u && !std::getenv("RT_DENOISE_NO_LDS")) {
        if (step == 1u) return d_rgb_sum_out ? launch_var_filter_lds<true, 1>(ci, gd, o, d_var_out, W, H, kv, in, ip, n, s) : launch_var_filter_lds<false, 1>(ci, gd, o, nullptr, W, H, kv, in, ip, n, s);
        return d_rgb_sum_out ? launch_var_filter_lds<true, 2>(ci, gd, o, d_var_out, W, H, kv, in, ip, n, s) : launch_var_filter_lds<false, 2>(ci, gd, o, nullptr, W, H, kv, in, ip, n, s);
    }
    if (d_rgb_sum_out) hipLaunchKernelGGL(denoise_var_filter_kernel<true>, grid, block, 0, s, ci, gd, o, d_var_out, W, H, tiles_x, step, kv, in, ip, n);
    else hipLaunchKernelGGL(denoise_var_filter_kernel<false>, grid, block, 0, s, ci, gd, o, (double*)nullptr, W, H, tiles_x, step, kv, in, ip, n);
    return (int)hipGetLastError();
}

} // namespace rt

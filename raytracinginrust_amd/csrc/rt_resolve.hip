// csrc/rt_resolve.hip — the other half of the reference's loop body on the device: Vec3::format_color (src/vec.rs:125-131) over a whole
// frame of per-pixel f64 sums, for progressive frames (rt_progressive_resolve_rgb8*, include/rt_amd.h).  A translation unit of its own:
// rt_kernel.hip and its code objects do not change when this file does.
//
// Exactness: the build's -ffp-contract=off -fno-fast-math make `/` and sqrt the IEEE-correct f64 operations (v_div_scale / v_div_fmas /
// v_div_fixup around the v_rcp_f64 refinement; v_sqrt_f64's estimate refined and fixed up) — no rcp / rsq shortcut — so every channel
// equals the host's rt_format_color (rt_host.cpp), which is the specification: NaN passes through the clamp (f64::clamp), `as u64`
// sends NaN and everything <= 0 (-0.0 and sqrt of a negative sum included) to 0, and the clamp keeps everything else <= 255.
//
// Shape: a pure stream, 24 B of sums + 3 B of the previous image in, 3 B out per pixel.  One lane takes FOUR consecutive pixels per
// step: 96 B of sums as six 16-byte loads (4 pixels x 24 B is the shortest run of pixels that is 16-byte periodic AND ends on a dword
// of RGB8), three dwords of the previous image, three dword stores.  Every cache line a wave touches is consumed whole by that wave's
// six loads.  The (< 4) pixels of a frame's tail are done byte-wise by one lane.  The changed-pixel count is summed per lane over the
// grid-stride loop, reduced across the wave with shuffles, and added with ONE atomic per wave.
#include <hip/hip_runtime.h>
#include "rt_resolve.h"

namespace rt {

__device__ __forceinline__ uint32_t format_channel(double sum, double samples) {
    double x = sqrt(sum / samples);
    if (x < 0.0) x = 0.0; else if (x > 0.999) x = 0.999;        // f64::clamp: NaN stays NaN
    const double y = 256.0 * x;
    return (y > 0.0) ? (uint32_t)y : 0u;                        // `as u64`: NaN -> 0, negative -> 0; y <= 255.744 here
}

__global__ __launch_bounds__(256) void resolve_rgb8_kernel(const double* __restrict__ sum, double samples, const uint8_t* rgb8_prev,
                                                           uint8_t* __restrict__ rgb8_out, unsigned long long* changed_px, uint32_t n_px) {
    const uint32_t n_groups = n_px / RT_RESOLVE_PX_PER_LANE;              // whole groups of four pixels
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t changed = 0u;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        const double2* in = reinterpret_cast<const double2*>(sum) + (size_t)g * 6u;       // 96 B per group: 16-byte aligned
        double2 v[6];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = in[k];
        uint32_t b[12];
#pragma unroll
        for (int k = 0; k < 6; k++) { b[2 * k] = format_channel(v[k].x, samples); b[2 * k + 1] = format_channel(v[k].y, samples); }
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        if (rgb8_prev) {
            const uint32_t* pv = reinterpret_cast<const uint32_t*>(rgb8_prev) + (size_t)g * 3u;
            const uint32_t x0 = pv[0] ^ w[0], x1 = pv[1] ^ w[1], x2 = pv[2] ^ w[2];
            // bytes 0..2 | 3..5 | 6..8 | 9..11 of the twelve are the four pixels
            changed += ((x0 & 0x00FFFFFFu) != 0u) + (((x0 >> 24) | (x1 & 0x0000FFFFu)) != 0u) + (((x1 >> 16) | (x2 & 0x000000FFu)) != 0u) + ((x2 >> 8) != 0u);
        } else changed += RT_RESOLVE_PX_PER_LANE;
        uint32_t* o = reinterpret_cast<uint32_t*>(rgb8_out) + (size_t)g * 3u;
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)                               // the frame's last n_px % 4 pixels
        for (uint32_t p = n_groups * RT_RESOLVE_PX_PER_LANE; p < n_px; p++) {
            bool differs = rgb8_prev == nullptr;
            for (uint32_t k = 0; k < 3u; k++) {
                const uint8_t c = (uint8_t)format_channel(sum[(size_t)p * 3u + k], samples);
                if (rgb8_prev && rgb8_prev[(size_t)p * 3u + k] != c) differs = true;
                rgb8_out[(size_t)p * 3u + k] = c;
            }
            changed += differs ? 1u : 0u;
        }
    for (int off = 32; off > 0; off >>= 1) changed += __shfl_xor(changed, off, 64);
    if ((threadIdx.x & 63u) == 0u && changed != 0u) atomicAdd(changed_px, (unsigned long long)changed);
}

hipError_t launch_resolve_rgb8(const double* sum, uint64_t samples, const uint8_t* rgb8_prev, uint8_t* rgb8_out,
                               unsigned long long* changed_px, uint32_t n_px, hipStream_t stream) {
    const uint32_t threads = RT_RESOLVE_THREADS;
    const uint64_t n_groups = n_px / RT_RESOLVE_PX_PER_LANE;
    uint64_t blocks = (n_groups + threads - 1u) / threads;
    if (blocks > RT_RESOLVE_MAX_BLOCKS) blocks = RT_RESOLVE_MAX_BLOCKS;      // grid-stride beyond that (rt_resolve.h)
    if (blocks == 0u) blocks = 1u;
    hipLaunchKernelGGL(resolve_rgb8_kernel, dim3((uint32_t)blocks), dim3(threads), 0, stream, sum, (double)samples, rgb8_prev, rgb8_out, changed_px, n_px);
    return hipGetLastError();
}

} // namespace rt

// csrc/rt_resolve.h — interface between the host library (rt_host.cpp, rt_frames.cpp) and the resolve kernel (rt_resolve.hip), the same kind of seam
// rt_launch.h is for the path-tracing kernels: plain C++ against the HIP headers, so that the sanitizer build compiles the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rt {
// Vec3::format_color (src/vec.rs:125-131) over a frame of per-pixel f64 sums, on the device: rgb8_out[3 p + k] =
// (256.0 * (sum[3 p + k] / samples).sqrt().clamp(0.0, 0.999)) as u64 — bit for bit what rt_format_color gives on the host — and
// *changed_px += the number of pixels whose triple differs from rgb8_prev's (rgb8_prev == nullptr: every pixel counts).  All pointers are
// DEVICE pointers; sum and the two rgb8 buffers are hipMalloc'ed (16-byte / 4-byte alignment is relied on); the caller zeroes
// *changed_px on the same stream first.  n_px <= 2^31 - 1.  Asynchronous on `stream`.
hipError_t launch_resolve_rgb8(const double* sum, uint64_t samples, const uint8_t* rgb8_prev, uint8_t* rgb8_out,
                               unsigned long long* changed_px, uint32_t n_px, hipStream_t stream);
// pixels one lane resolves per step of its grid-stride loop (tests choose frame sizes that are not multiples of it)
static const uint32_t RT_RESOLVE_PX_PER_LANE = 4u;
// the launch: workgroups of RT_RESOLVE_THREADS lanes, at most RT_RESOLVE_MAX_BLOCKS of them — 32 resident workgroups' worth per CU; a frame of
// more than MAX_BLOCKS x THREADS x PX_PER_LANE pixels goes through the kernel's grid-stride loop more than once (rt_debug_loop_limits)
static const uint32_t RT_RESOLVE_THREADS = 256u;
static const uint32_t RT_RESOLVE_MAX_BLOCKS = 8192u;
}

// csrc/rt_host_shared.h — where the host library's two units that see HIP meet: rt_host.cpp (scenes, uploads, launch planning, the
// path-tracing launches, the queries) and rt_frames.cpp (progressive frames and the image operations over them).  Everything else they
// share is the public C-ABI (include/rt_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/rt_amd.h"
#include "rt_scene.h"

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return rt::set_error(std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

#pragma GCC visibility push(hidden)     // (between the library's own units: none of this joins its exported symbols)
namespace rt {
// rt_host.cpp
int need_device_and_flat(Scene& s);                               // a HIP device and the flattened scene, or rt_last_error
int frame_prologue(rt_scene* sc, const rt_camera* cam, const double* bg, uint32_t W, uint32_t H, uint32_t spp);      // the frame's arguments, then the above
int query_aligned(const void* p, const char* what);               // 16-byte alignment of a device buffer of records
int render_any(rt_scene* sc, const rt_camera* cam, const double bg[3], uint32_t W, uint32_t H, uint32_t spp, uint32_t max_depth,
               uint64_t seed, uint32_t flags, uint32_t tile_px, uint32_t rank, uint32_t world, void* d_out, size_t d_out_bytes,
               void* d_samples, hipStream_t stream, bool may_calibrate, uint32_t first_sample = 0u, bool accumulate = false);
// the pixel-list kernel (rt_pixels.h) planned and launched on the current device for arguments rt_render_pixels_device has checked
int launch_pixel_list(Scene& s, const rt_camera* cam, const double bg[3], uint32_t W, uint32_t H, uint32_t n_samples, uint32_t max_depth,
                      uint64_t seed, uint32_t flags, const void* d_list, uint32_t n_list, const void* d_counts, void* d_out, hipStream_t stream);
// rt_frames.cpp
void frames_scene_gone(Scene& s);                                 // rt_scene_destroy: the scene's frames outlive it (they own their buffers)
} // namespace rt
#pragma GCC visibility pop

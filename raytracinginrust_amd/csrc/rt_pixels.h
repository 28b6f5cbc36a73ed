// csrc/rt_pixels.h — interface between the host library (rt_host.cpp) and the pixel-list path-tracing kernel (rt_adaptive.hip): the frames'
// bounce loop over a LIST of pixels of one view instead of the whole frame (rt_render_pixels_device, adaptive progressive frames).
#pragma once
#include <hip/hip_runtime.h>
#include "rt_ir.h"

namespace rt {
static const uint32_t PIXELS_THREADS = 256u;        // workgroup size of every pixel-list kernel
static const uint32_t PIXELS_CHUNK = 256u;          // consecutive paths a wave's cursor runs through before it takes its next chunk
// What a pixel-list launch needs beside KParams (the scene's tables, camera, W, H, background, max_depth, flags, seed, spp = the pass size
// n_b, out = the W*H*3 pass frame the sums are ADDED to).  Path p = k * n_b + s is sample counts[list[k]] + s (counts == nullptr: s) of
// output-order pixel list[k], drawn from rng_for_path(seed, pixel, sample).  Chunk c = paths [c * chunk, (c + 1) * chunk); wave w of W
// takes chunks w, w + W, ...  An entry that is not a pixel of the frame (>= n_px), or whose last sample would pass 2^32 - 1, is skipped:
// nothing is traced and nothing is written for it.  nonfinite: nullptr, or one u64 that the samples with a non-finite component are added to.
struct PixelsArgs { const uint32_t* list; const uint32_t* counts; unsigned long long* nonfinite; uint64_t n_paths, n_chunks; uint32_t chunk, n_px; };
// Resident workgroups per CU with `shmem` bytes of dynamic LDS (asks for more than the default 64 KB where needed); 0: the query failed
int pixels_blocks_per_cu(uint32_t scene_feats, size_t shmem);
hipError_t launch_pixels(const KParams<double>& P, const PixelsArgs& X, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream);
}

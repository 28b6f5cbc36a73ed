// csrc/rt_radiance.h — interface between the host library (rt_host.cpp) and the radiance-query kernels (rt_radiance.hip):
// ray_color(r, background, world, lights, depth) (main.rs:41-120) for rays the caller chooses.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_ir.h"

namespace rt {
static const uint32_t RADIANCE_THREADS = 256u;      // workgroup size of every radiance kernel
static const uint32_t RADIANCE_CHUNK = 256u;        // consecutive paths a wave's cursor runs through before it takes its next chunk
// What a radiance launch needs beside KParams (the scene's tables as for a ray query, plus background, max_depth, flags, spp, seed, out =
// the n x 3 sums, samples_out = nullptr or n x spp x 3).  Path p = k * spp + s is sample s of ray k (rays[7 k ..], 16-byte aligned base) and
// draws from rng_for_path(seed, k, s).  Chunk c = paths [c * chunk, (c + 1) * chunk); wave w of W takes chunks w, w + W, ...
// nonfinite: nullptr, or one u64 that the samples with a non-finite component are added to.
struct RadianceArgs { const double* rays; unsigned long long* nonfinite; uint64_t n_paths, n_chunks; uint32_t chunk; };
// Resident workgroups per CU with `shmem` bytes of dynamic LDS (asks for more than the default 64 KB where needed); 0: the query failed
int radiance_blocks_per_cu(uint32_t scene_feats, size_t shmem);
hipError_t launch_radiance(const KParams<double>& P, const RadianceArgs& R, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream);
}

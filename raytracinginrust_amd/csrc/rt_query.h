// csrc/rt_query.h — interface between the host library (rt_host.cpp) and the ray-query kernels (rt_query.hip): world.hit (main.rs:48)
// for rays the caller chooses, or for the camera rays of one sample of every pixel, with the hit record written out.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_ir.h"

namespace rt {
static const uint32_t QUERY_THREADS = 256u;         // workgroup size of every query kernel
static const uint32_t QUERY_RAY_DOUBLES = 7u;       // origin[3], direction[3], time
static const uint32_t QUERY_HIT_DOUBLES = 16u;      // the hit record of include/rt_amd.h (rt_query_hits)
// What a query launch needs beside the scene's tables (KParams: bind_tables, bvh_tame, n_cached; camera mode also cam, W, H).
// rays / rays_out / hits are 16-byte aligned device pointers.  Caller rays: ray k comes from rays[7 k ..] and draws from
// rng_for_stream(seed, k).  Camera mode (rays == nullptr): record p is output-order pixel p's camera ray of sample `sample`, generated as
// the frames generate it, its stream rng_for_path(seed, p, sample) continuing into the search; rays_out (may be nullptr) receives the ray.
struct QueryArgs { const double* rays; double* rays_out; double* hits; uint32_t n, sample; double t_min; uint64_t seed; };
// The FEATS template argument of the instantiation that serves a scene (pathtrace_kernel's rule without the scheduling variants)
uint32_t query_feats(uint32_t scene_feats);
// Resident workgroups per CU with `shmem` bytes of dynamic LDS (asks for more than the default 64 KB where needed); 0: the query failed
int query_blocks_per_cu(uint32_t scene_feats, bool camera, size_t shmem);
hipError_t launch_query(const KParams<double>& P, const QueryArgs& Q, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream);
}

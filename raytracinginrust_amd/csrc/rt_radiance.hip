// csrc/rt_radiance.hip — radiance queries: ray_color(r, background, world, lights, depth) (src/main.rs:41-120) for rays the caller chooses,
// samples_per_ray samples of each — what a host needs for another projection (panorama, orthographic, fisheye, a measured lens), a light or
// irradiance probe, a baked light map, "how bright is it along THIS ray" (include/rt_amd.h: rt_query_radiance).
//
// A translation unit of its own over rt_kernel.hip's device functions, as rt_query.hip is (RT_TU == 3 leaves that file's kernels and launch
// code out): the bounce loop is trace_lockstep's body — world_hit / world_hit_list, finalize_hit, shade_hit, add_radiance, flush_acc, the
// code the frames run — and nothing is added to the units the frames are built from (one more caller there changes other kernels' machine
// code, docs/history.md).  load_ray, the cursor's path_step, the staging loop and the scene-class dispatch are the query units' own:
// rt_query_dev.h.
//
// Work: path p = k * spp + s is sample s of ray k, one path per lane, ray-major: the lanes of a wave start on the same ray or on neighbouring
// ones.  A lane whose path has ended takes the wave's next path (__ballot + mbcnt prefix: the frames' regeneration without their LDS queue —
// a new path here is a 56-byte load and a key, no camera code worth batching).  The wave's cursor runs through chunks of R.chunk consecutive
// paths, dealt statically: wave w of W takes chunks w, w + W, ...  No global counter: nothing to zero, launches on different streams may
// overlap.  Every loop ends by max_depth or by the end of the wave's chunks; lanes past the last path never become alive and take part in
// every vote.  Sums: a lane keeps the partial sum of its current ray and hands it in (flush_acc: masked butterfly, one f64 atomic per
// channel) when it moves to another ray and at the end.
#define RT_TU 3
#include "rt_kernel.hip"
#include "rt_radiance.h"
#include "rt_query_dev.h"

namespace rt {

// Resident waves per SIMD the register allocation is held to, from -Rpass-analysis=kernel-resource-usage and the loop depth of every scratch
// access in the ISA (make asm, tools/scratch_map.py); the whole table is DESIGN §13's:
//   list scenes 5 (96 VGPRs, 2 registers spilled, read once per bounce outside the search); mesh scenes 4 (127 VGPRs, 2 spilled, the same);
//   everything but the principled material 3 (143 VGPRs, no scratch — held to 4 it spills 100 registers and reads scratch three loops deep);
//   everything 3 (168 VGPRs, 20 spilled, every access in the bounce loop's own body); with object leaves 1: held to 2 it spills 485
//   registers and reads scratch down to the innermost loops, with all 512 registers it spills 48 and the deepest accesses are in
//   shade_hit's loop over the lights.
template <uint32_t FEATS> struct RadianceWaves {
    static constexpr uint32_t v = FEATS == 0u ? 5u : ((FEATS & F_NESTED) ? 1u : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? 4u : 3u));
};

template <uint32_t FEATS>
__global__ void __launch_bounds__(RADIANCE_THREADS, RadianceWaves<FEATS>::v) radiance_kernel(const KParams<double> P, const RadianceArgs R) {
    typedef double T;
    if ((FEATS & F_BVH) && P.n_cached != 0u) stage_filter_tree<RADIANCE_THREADS>(P);      // once per workgroup
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_in_block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the wave's cursor (wave-uniform: scalar registers): next chunk, and paths [.., + left) of the current one starting at (cur_k, cur_s)
    const uint64_t n_waves = (uint64_t)gridDim.x * (RADIANCE_THREADS / 64u);
    uint64_t next_chunk = (uint64_t)blockIdx.x * (RADIANCE_THREADS / 64u) + wave_in_block;
    uint32_t left = 0u, cur_k = 0u, cur_s = 0u;
    // per-lane path state (trace_lockstep's)
    bool alive = false;
    RayT<T> ray; ray.o = mk<T>(T(0), T(0), T(0)); ray.d = ray.o; ray.tm = T(0);
    V3<T> beta = mk<T>(T(0), T(0), T(0));
    uint32_t depth_left = 0, path_s = 0;
    Rng rng; rng.s0 = rng.s1 = rng.s2 = rng.s3 = 0;
    uint32_t acc_k = NONE_PX;                                     // the ray the accumulator belongs to (n <= 2^31 - 1: never a ray's index)
    AccReg acc; acc.set(0, 0.0); acc.set(1, 0.0); acc.set(2, 0.0);
    uint32_t n_nonfinite = 0, n_flush = 0;

    for (;;) {
        // ---- lanes whose path has ended take the wave's next paths, in lane order
        bool got_new = false;
        uint32_t new_k = 0;
        for (;;) {
            const unsigned long long want = __ballot(!alive && !got_new);
            if (want == 0ull) break;
            if (left == 0u) {
                if (next_chunk >= R.n_chunks) break;              // the wave's chunks are used up
                const uint64_t p0 = next_chunk * R.chunk, rest = R.n_paths - p0;
                left = rest < (uint64_t)R.chunk ? (uint32_t)rest : R.chunk;
                const uint64_t k0 = p0 / P.spp;                   // (once per chunk, wave-uniform)
                cur_k = (uint32_t)k0; cur_s = (uint32_t)(p0 - k0 * P.spp);
                next_chunk += n_waves;
            }
            const uint32_t n_want = (uint32_t)__popcll(want);
            const uint32_t take = n_want < left ? n_want : left;
            const uint32_t rank = lane_rank(want);
            if (!alive && !got_new && rank < take) {
                got_new = true;
                path_step(cur_k, cur_s, rank, P.spp, new_k, path_s);
            }
            path_step(cur_k, cur_s, take, P.spp, cur_k, cur_s);
            left -= take;
        }
        if (__ballot(alive || got_new) == 0ull) break;            // no chunk left and every path finished

        // ---- lanes moving on to another ray hand in their partial sum
        flush_acc<T, AccReg, false>(P, got_new && acc_k != NONE_PX && acc_k != new_k, acc_k, acc, lane, n_flush);

        if (got_new) {
            if (acc_k != new_k) { acc_k = new_k; acc.set(0, 0.0); acc.set(1, 0.0); acc.set(2, 0.0); }
            load_ray(R.rays, new_k, ray);
            rng = rng_for_path(P.seed, new_k, path_s);            // the frames' keying with the ray's index in the pixel's place; no camera draws
            beta = mk<T>(T(1.0), T(1.0), T(1.0));
            depth_left = P.max_depth;
            alive = true;
        }

        // ---- one level of ray_color (main.rs:41-120) for every live lane
        if (alive) {
            bool done = false;
            V3<T> e = mk<T>(T(0), T(0), T(0));                    // terminal radiance of this path (times beta)
            if (depth_left == 0) {
                done = true;                                      // main.rs:42-45
            } else {
                T t_hit; HitId id; id.obj = 0; id.prim = 0;
                bool any_hit;                                                                            // main.rs:48
                if constexpr (FEATS == 0u) any_hit = world_hit_list<T>(P, ray, TMin<T>::v(), rng, t_hit, id);
                else any_hit = world_hit<T, FEATS>(P, ray, TMin<T>::v(), rng, t_hit, id, nullptr);
                if (!any_hit) {
                    e = ld3(P.background); done = true;                                                  // main.rs:118
                } else {
                    Rec<T> rec;
                    finalize_hit<T, FEATS>(P, ray, t_hit, id, true, rec);
                    shade_hit<T, FEATS>(P, rec, ray, beta, rng, depth_left, done, e);
                }
            }
            if (done) {
                add_radiance(P, beta * e, acc, n_nonfinite, acc_k, path_s);
                alive = false;
            }
        }
    }
    // ---- the wave's chunks are used up: hand in what is left
    flush_acc<T, AccReg, false>(P, acc_k != NONE_PX, acc_k, acc, lane, n_flush);
    if (R.nonfinite && n_nonfinite) atomicAdd(R.nonfinite, (unsigned long long)n_nonfinite);
}

// the instantiation: the five scene classes of the path-tracing forms — unlike the ray queries, with the principled material
template <typename G> static auto radiance_kernel_for(uint32_t scene_feats, G&& g) {
    return scene_class_dispatch_pbr(scene_feats, [&](auto feats) { return g(radiance_kernel<decltype(feats)::value>); });
}
int radiance_blocks_per_cu(uint32_t scene_feats, size_t shmem) {
    return radiance_kernel_for(scene_feats, [&](auto kernel) { return kernel_blocks_per_cu(kernel, RADIANCE_THREADS, shmem); });
}
hipError_t launch_radiance(const KParams<double>& P, const RadianceArgs& R, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return radiance_kernel_for(scene_feats, [&](auto kernel) { return kernel_launch(kernel, RADIANCE_THREADS, n_blocks, shmem, stream, P, R); });
}

} // namespace rt

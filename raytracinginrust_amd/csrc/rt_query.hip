// csrc/rt_query.hip — ray queries: world.hit(r, t_min, +inf) (src/main.rs:48, Hittable::hit) for rays the caller chooses, or for the
// camera ray of one sample of every pixel, and the hit record (hit.rs:9-24) written out — what a host needs for picking, auto-focus, depth /
// normal / material frames, visibility probes (include/rt_amd.h: rt_query_hits, rt_query_camera).
//
// A translation unit of its own over rt_kernel.hip's device functions (RT_TU == 3 leaves that file's kernels and launch code out): the
// search and the record are world_hit / world_hit_list / finalize_hit — the code the frames run, one ray per lane — and nothing is
// added to the two units the frames are built from (one more caller there changes other kernels' machine code, docs/history.md).
// What the six query units have in common — ray load and store, camera_ray, the dispatch by scene class, occupancy and launch — is in
// rt_query_dev.h, once.
//
// Shape: 256-thread workgroups, at most (CUs x resident workgroups) of them.  A workgroup stages the filter tree in LDS once when the
// WHOLE tree fits its share of the CU's LDS (pathtrace_kernel's staging loop with its links rewritten to LDS addresses; *measured*,
// profiles/ray_queries.log: random spheres +22 % with it, while the top levels of a tree that does not fit cost the final scene 18 % and
// the teapot room 7 % against no staging at all — so a tree that does not fit is walked from global memory), then takes batches of 256
// rays grid-stride: staging is paid per workgroup, not per ray.  The searches vote (__ballot), so a wave runs whole: lanes past n
// repeat the last ray and only their store is left out.  No atomics, no queue: the same call gives the same words.
#define RT_TU 3
#include "rt_kernel.hip"
#include "rt_query.h"
#include "rt_query_dev.h"

namespace rt {

// Resident waves per SIMD the register allocation is held to (workgroups of four waves, one per SIMD: this is also the resident
// workgroups per CU the registers allow).  From -Rpass-analysis=kernel-resource-usage and the loop depth of every scratch access in the
// ISA (make asm, tools/scratch_map.py) — f64, no shading code:
//   list scenes 5 (76 / 93 VGPRs caller rays / camera, no scratch); mesh scenes 5 (96 VGPRs, 4 / 14 registers spilled, every scratch access
//   outside the box-step and leaf-step loops); everything else without object leaves 3 (123 / 130 VGPRs, no scratch); with object leaves 1:
//   held to 2 that search spills 255 registers and reads scratch inside the box-step loops, with all 512 registers it does not.
template <uint32_t FEATS> struct QueryWaves {
    static constexpr uint32_t v = FEATS == 0u ? 5u : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? 5u : ((FEATS & F_NESTED) ? 1u : 3u));
};

template <uint32_t FEATS, bool CAMERA>
__global__ void __launch_bounds__(QUERY_THREADS, QueryWaves<FEATS>::v) query_kernel(const KParams<double> P, const QueryArgs Q) {
    if ((FEATS & F_BVH) && P.n_cached != 0u) {
        // the filter tree, once per workgroup: rt_query_dev.h's stage_filter_tree<QUERY_THREADS>(P), restated — with the call in its place a
        // kernel time of this family left the parent's spread in the A/B (docs/history.md), so the prologue stays the parent's to the line
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const uint32_t nodes_bytes = P.n_cached * (uint32_t)sizeof(DFNode);
        const u4* src = (const u4*)P.bvh_f; u4* dst = (u4*)lds_raw;
        const uint32_t base = lds_base();
        for (uint32_t i = threadIdx.x; i < nodes_bytes / 16u; i += QUERY_THREADS) {
            u4 w = src[i];
            if (i & 1u) {                                         // second half of a DFNode: max.z-side bounds, skip, info
                if (w.z != ST_DONE) w.z = base + w.z * (uint32_t)sizeof(DFNode);
                if (!(w.w & FNODE_LEAF)) w.w = base + w.w * (uint32_t)sizeof(DFNode);
            }
            dst[i] = w;
        }
        __syncthreads();                                          // the only barrier: the batches below need none
    }
    const uint32_t n = Q.n;
    for (uint64_t base = (uint64_t)blockIdx.x * QUERY_THREADS; base < n; base += (uint64_t)gridDim.x * QUERY_THREADS) {
        if (base + (threadIdx.x & ~63u) >= n) break;              // (wave-uniform: a wave with no ray at all, in the last batch only)
        const uint64_t i64 = base + threadIdx.x;
        const bool mine = i64 < n;
        const uint32_t k = mine ? (uint32_t)i64 : n - 1u;         // a partial last wave repeats the last ray: every lane takes part in the votes
        RayT<double> ray; Rng rng;
        if (CAMERA) camera_ray(P, Q.seed, k, Q.sample, ray, rng);
        else { load_ray(Q.rays, k, ray); rng = rng_for_stream(Q.seed, k); }
        double t_hit; HitId id; id.obj = 0u; id.prim = 0u;
        bool any;
        if constexpr (FEATS == 0u) any = world_hit_list<double>(P, ray, Q.t_min, rng, t_hit, id);
        else any = world_hit<double, FEATS>(P, ray, Q.t_min, rng, t_hit, id, nullptr);
        Rec<double> rec; rec.p = mk<double>(0.0, 0.0, 0.0); rec.n = rec.p; rec.t = 0.0; rec.u = rec.v = 0.0; rec.front = false; rec.mat = 0u;
        if (any) finalize_hit<double, FEATS>(P, ray, t_hit, id, true, rec);
        if (mine) {
            // (these sixteen words have twins in albedo_kernel and in chain_kernel's caller-ray form: as one function they move instructions
            // outside the staging prologue, docs/history.md)
            const bool medium = any && id.prim == PRIM_MEDIUM;    // (its Isotropic was appended by the flattener: no handle)
            const bool named = any && !medium;
            d2* o = (d2*)(Q.hits + 16ull * k);
            d2 w;
            w.x = any ? 1.0 : 0.0; w.y = any ? rec.t : 0.0; o[0] = w;
            w.x = rec.p.x; w.y = rec.p.y; o[1] = w;
            w.x = rec.p.z; w.y = rec.n.x; o[2] = w;
            w.x = rec.n.y; w.y = rec.n.z; o[3] = w;
            w.x = rec.front ? 1.0 : 0.0; w.y = rec.u; o[4] = w;
            w.x = rec.v; w.y = named ? (double)rec.mat : -1.0; o[5] = w;
            w.x = any ? (double)id.obj : -1.0; w.y = named ? (double)(id.prim >> 28) : -1.0; o[6] = w;
            w.x = named ? (double)(id.prim & 0x0FFFFFFFu) : -1.0; w.y = 0.0; o[7] = w;
            if (CAMERA && Q.rays_out) store_ray(Q.rays_out, k, ray);
        }
    }
}

// the instantiation: the four scene classes of the searches (the principled material changes no hit), caller rays or camera rays
template <typename G> static auto query_kernel_for(uint32_t scene_feats, bool camera, G&& g) {
    return scene_class_dispatch(scene_feats, [&](auto feats) {
        return flag_dispatch(camera, [&](auto cam) { return g(query_kernel<decltype(feats)::value, decltype(cam)::value>); });
    });
}
uint32_t query_feats(uint32_t scene_feats) {
    return scene_class_dispatch(scene_feats, [](auto feats) { return (uint32_t) decltype(feats)::value; });
}
int query_blocks_per_cu(uint32_t scene_feats, bool camera, size_t shmem) {
    return query_kernel_for(scene_feats, camera, [&](auto kernel) { return kernel_blocks_per_cu(kernel, QUERY_THREADS, shmem); });
}
hipError_t launch_query(const KParams<double>& P, const QueryArgs& Q, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return query_kernel_for(scene_feats, camera, [&](auto kernel) { return kernel_launch(kernel, QUERY_THREADS, n_blocks, shmem, stream, P, Q); });
}

} // namespace rt

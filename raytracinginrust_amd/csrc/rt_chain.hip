// csrc/rt_chain.hip — specular-chain guides (rt_query_chain*, rt_query_camera_chain_guide*): several closest-hit searches per ray, chained
// through mirrors and glass to the first non-specular surface; the specification and the link step are in rt_chain.h.
//
// A translation unit of its own over rt_kernel.hip's device functions (RT_TU == 3, as rt_query.hip, rt_albedo.hip and rt_guide.hip): the
// search and the record are world_hit / world_hit_list / finalize_hit — the code the frames run — and nothing is added to the units the
// frames and the filters are built from.  load_ray, camera_ray, albedo_of and the scene-class dispatch are the query units' own:
// rt_query_dev.h.
//
// Shape: guide_kernel's — 256-thread workgroups, at most (CUs x resident workgroups) of them, the filter tree staged in LDS when the WHOLE
// tree fits, batches of 256 lanes grid-stride, one ITEM per lane (a caller's ray, or a pixel that loops over its samples in ascending order),
// no atomics: the sum order is fixed and the same call gives the same words.
//
// The link loop is WAVE-UNIFORM.  The searches vote (__ballot in world_hit_list's clearance test and in every BVH walk), and the votes
// count on whole waves: lanes past n repeat the last item, as in every query kernel.  So the loop over the links runs while ANY lane of the
// wave is still chaining; a lane whose chain has ended searches its last ray again — a ray that has been searched before, so the search
// ends as it did — and the result is discarded: everything a lane carries out of the loop (accumulators, link count) and everything it
// stores is written under `live`, once, at the link where its chain ends, and `live` never turns true again within a chain.  A lane carries
// no finished record: it is written out (caller rays) or added to the guide's accumulators (camera) where the chain ends.
#define RT_TU 3
#include "rt_kernel.hip"
#define RT_CHAIN_QUERIES
#include "rt_chain.h"
#include "rt_query_dev.h"

namespace rt {

static_assert(CHAIN_KIND_METAL == (uint32_t)M_METAL && CHAIN_KIND_DIELECTRIC == (uint32_t)M_DIELECTRIC, "rt_chain.h restates rt_ir.h's material kinds");
static_assert(CHAIN_HIT_DOUBLES == QUERY_HIT_DOUBLES && CHAIN_RAY_DOUBLES == QUERY_RAY_DOUBLES, "rt_chain.h restates rt_query.h's record sizes");

// Resident waves per SIMD the register allocation is held to, from -Rpass-analysis=kernel-resource-usage (make asm) and the loop depth of
// every scratch access (tools/scratch_map.py); the table is in DESIGN §23.  GuideWaves' classes and values: across a search the lane carries
// guide_kernel's accumulators plus the weight, the path length, L_0, the current ray and the link count.
#ifndef RT_CHAIN_LIST_WAVES
#define RT_CHAIN_LIST_WAVES 4u
#endif
#ifndef RT_CHAIN_MESH_WAVES
#define RT_CHAIN_MESH_WAVES 4u
#endif
template <uint32_t FEATS> struct ChainWaves {
    static constexpr uint32_t v = FEATS == 0u ? RT_CHAIN_LIST_WAVES : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? RT_CHAIN_MESH_WAVES : ((FEATS & F_NESTED) ? 1u : 3u));
};

template <uint32_t FEATS, bool CAMERA, bool ALBEDO>
__global__ void __launch_bounds__(QUERY_THREADS, (ChainWaves<FEATS>::v)) chain_kernel(const KParams<double> P, const ChainArgs A) {
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
        __syncthreads();                                          // the only barrier
    }
    const uint32_t n = A.n;
    const uint32_t n_samples = CAMERA ? A.n_samples : 1u;         // uniform: every lane of a wave runs the same number of chains
    const uint32_t max_links = A.max_links;
    // the caller-ray form always finalizes with u, v (the record carries them); the camera form needs them for the albedo's texture only
    constexpr bool WANT_UV = !CAMERA || ALBEDO;
    for (uint64_t base = (uint64_t)blockIdx.x * QUERY_THREADS; base < n; base += (uint64_t)gridDim.x * QUERY_THREADS) {
        if (base + (threadIdx.x & ~63u) >= n) break;              // (wave-uniform: a wave with no lane at all, in the last batch only)
        const uint64_t i64 = base + threadIdx.x;
        const bool mine = i64 < n;
        const uint32_t k = mine ? (uint32_t)i64 : n - 1u;         // a partial last wave repeats the last item: every lane takes part in the votes
        // guide_kernel's accumulators (camera form).  (They and the eight stores below are rt_guide.hip's, written out in both files: as one
        // struct they move every instantiation's register allocation, docs/history.md)
        double st = 0.0, p0 = 0.0, p1 = 0.0, p2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        uint32_t h = 0u, hf = 0u, links_sum = 0u;
        int32_t m_first = -1, o_first = -1;
        bool m_same = true, o_same = true;
        for (uint32_t s = 0; s < n_samples; s++) {
            const uint32_t sample_index = CAMERA ? A.first_sample + s : 0u;
            RayT<double> ray; Rng rng;
            if (CAMERA) camera_ray(P, A.seed, k, sample_index, ray, rng);
            else { load_ray(A.rays, k, ray); rng = rng_for_stream(A.seed, k); }
            double wgt[3] = {1.0, 1.0, 1.0};
            double S = 0.0, L0 = 0.0;                             // (C6): the path length so far, and the first ray's length
            uint32_t links = 0u;
            bool live = true;
            for (uint32_t l = 0; ; l++) {
                double t_hit; HitId id; id.obj = 0u; id.prim = 0u;
                bool any;
                if constexpr (FEATS == 0u) any = world_hit_list<double>(P, ray, A.t_min, rng, t_hit, id);
                else any = world_hit<double, FEATS>(P, ray, A.t_min, rng, t_hit, id, nullptr);
                Rec<double> rec; rec.p = mk<double>(0.0, 0.0, 0.0); rec.n = rec.p; rec.t = 0.0; rec.u = rec.v = 0.0; rec.front = false; rec.mat = 0u;
                if (any) finalize_hit<double, FEATS>(P, ray, t_hit, id, WANT_UV, rec);
                if (live) {                                       // an ended lane's search above is discarded: nothing below runs for it
                    const double d[3] = {ray.d.x, ray.d.y, ray.d.z};
                    double new_d[3] = {0.0, 0.0, 0.0};
                    uint32_t status;
                    if (!any) status = CHAIN_END_MISS;
                    else if (l == max_links || id.prim == PRIM_MEDIUM) status = CHAIN_END_SURFACE;
                    else {
                        const DMaterial<double> mt = ld_mat(P.materials + rec.mat);
                        const double nn[3] = {rec.n.x, rec.n.y, rec.n.z};
                        status = chain_step(d, nn, rec.front, mt.kind, mt.param, mt.albedo, A.max_fuzz, new_d, wgt);
                    }
                    // (C6) word [1]: the record's own t with no link followed, else the path length over L_0
                    double t_word = any ? rec.t : 0.0;
                    if (l == 0u) {
                        if (status == CHAIN_CONTINUE) { L0 = chain_length(d); S = rec.t * L0; }
                    } else {
                        if (any) S = S + rec.t * chain_length(d);
                        t_word = S / L0;
                    }
                    if (status == CHAIN_CONTINUE) {
                        ray.o = rec.p; ray.d = mk<double>(new_d[0], new_d[1], new_d[2]);    // (C5); time unchanged
                        links++;
                    } else {
                        live = false;
                        V3<double> a = mk<double>(1.0, 1.0, 1.0);
                        if constexpr (ALBEDO) {
                            const V3<double> al = albedo_of<FEATS>(P, any, rec);
                            a = mk<double>(wgt[0] * al.x, wgt[1] * al.y, wgt[2] * al.z);
                        }
                        const bool medium = any && id.prim == PRIM_MEDIUM;    // (its Isotropic was appended by the flattener: no handle)
                        const bool named = any && !medium;
                        if constexpr (CAMERA) {
                            links_sum += links;
                            if constexpr (ALBEDO) { a0 += a.x; a1 += a.y; a2 += a.z; }
                            if (any) {                            // rt_guide.h's reduction of the chain record
                                const int32_t mw = medium ? -1 : (int32_t)rec.mat;
                                const int32_t ow = (int32_t)id.obj;
                                if (h == 0u) { m_first = mw; o_first = ow; }
                                else { m_same = m_same && mw == m_first; o_same = o_same && ow == o_first; }
                                h++;
                                hf += rec.front ? 1u : 0u;
                                st += t_word;
                                p0 += rec.p.x; p1 += rec.p.y; p2 += rec.p.z;
                                n0 += rec.n.x; n1 += rec.n.y; n2 += rec.n.z;
                            }
                        } else if (mine) {                        // the words query_kernel writes, but for [1] and [15] (a twin of its stores)
                            d2* o = (d2*)(A.hits + 16ull * k);
                            d2 w;
                            w.x = any ? 1.0 : 0.0; w.y = t_word; o[0] = w;
                            w.x = rec.p.x; w.y = rec.p.y; o[1] = w;
                            w.x = rec.p.z; w.y = rec.n.x; o[2] = w;
                            w.x = rec.n.y; w.y = rec.n.z; o[3] = w;
                            w.x = rec.front ? 1.0 : 0.0; w.y = rec.u; o[4] = w;
                            w.x = rec.v; w.y = named ? (double)rec.mat : -1.0; o[5] = w;
                            w.x = any ? (double)id.obj : -1.0; w.y = named ? (double)(id.prim >> 28) : -1.0; o[6] = w;
                            w.x = named ? (double)(id.prim & 0x0FFFFFFFu) : -1.0; w.y = (double)links; o[7] = w;
                            if constexpr (ALBEDO) { double* q = A.albedo + 3ull * k; q[0] = a.x; q[1] = a.y; q[2] = a.z; }
                        }
                    }
                }
                if (__ballot(live) == 0ull) break;                // wave-uniform: every lane of the wave leaves the loop at the same link
                rng = rng_for_stream(chain_link_seed(A.seed, sample_index, l + 1u), k);     // (C1); an ended lane's draws change nothing it keeps
            }
        }
        if (CAMERA && mine) {                                     // guide_kernel's stores
            const bool some = h != 0u;
            const double dh = (double)h;
            d2* o = (d2*)(A.hits + 16ull * k);
            d2 w;
            w.x = (some && 2ull * h >= n_samples) ? 1.0 : 0.0; w.y = some ? st / dh : 0.0; o[0] = w;
            w.x = some ? p0 / dh : 0.0; w.y = some ? p1 / dh : 0.0; o[1] = w;
            w.x = some ? p2 / dh : 0.0; w.y = some ? n0 / dh : 0.0; o[2] = w;
            w.x = some ? n1 / dh : 0.0; w.y = some ? n2 / dh : 0.0; o[3] = w;
            w.x = some ? (double)hf / dh : 0.0; w.y = 0.0; o[4] = w;
            w.x = 0.0; w.y = (some && m_same) ? (double)m_first : -1.0; o[5] = w;
            w.x = (some && o_same) ? (double)o_first : -1.0; w.y = -1.0; o[6] = w;
            w.x = -1.0; w.y = dh; o[7] = w;
            if constexpr (ALBEDO) { double* q = A.albedo + 3ull * k; q[0] = a0; q[1] = a1; q[2] = a2; }
            if (A.links) A.links[k] = links_sum;
        }
    }
}

// the instantiation: query_kernel's classes and forms, with the optional albedo output as a third argument
template <typename G> static auto chain_kernel_for(uint32_t scene_feats, bool camera, bool albedo, G&& g) {
    return scene_class_dispatch(scene_feats, [&](auto feats) {
        return flag_dispatch(camera, [&](auto cam) {
            return flag_dispatch(albedo, [&](auto alb) { return g(chain_kernel<decltype(feats)::value, decltype(cam)::value, decltype(alb)::value>); });
        });
    });
}
int chain_blocks_per_cu(uint32_t scene_feats, bool camera, bool albedo, size_t shmem) {
    return chain_kernel_for(scene_feats, camera, albedo, [&](auto kernel) { return kernel_blocks_per_cu(kernel, QUERY_THREADS, shmem); });
}
hipError_t launch_chain(const KParams<double>& P, const ChainArgs& A, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return chain_kernel_for(scene_feats, camera, A.albedo != nullptr, [&](auto kernel) { return kernel_launch(kernel, QUERY_THREADS, n_blocks, shmem, stream, P, A); });
}

} // namespace rt

// csrc/rt_guide.hip — the averaged denoising guide (rt_query_camera_guide*): the first-hit records of n_samples camera samples of every pixel
// reduced to one record in rt_query_camera's layout; the specification is in rt_guide.h.
//
// A translation unit of its own over rt_kernel.hip's device functions (RT_TU == 3, as rt_query.hip, rt_radiance.hip and rt_albedo.hip): the
// search and the record are world_hit / world_hit_list / finalize_hit — the code the frames run — and nothing is added to the units the
// frames and the filters are built from.  camera_ray, albedo_of and the scene-class dispatch are the query units' own: rt_query_dev.h.
//
// Shape: the camera form of albedo_kernel — 256-thread workgroups, at most (CUs x resident workgroups) of them, the filter tree staged in
// LDS when the WHOLE tree fits, batches of 256 lanes grid-stride, whole waves in every voting search (lanes past n repeat the last pixel
// and only skip their stores).  One PIXEL per lane, which loops over its samples in ascending order: n_samples is uniform, so the waves stay
// whole, and there are no atomics — the sum order is fixed and the same call gives the same words.  Per lane the loop carries seven f64
// accumulators (t, position, normal), two counters (hits, front faces), the material and object words of the first hitting sample and one
// "agree so far" bit each; with ALBEDO three more accumulators, the sums rt_query_camera_albedo writes, from the same search: a caller who
// wants both pays for one search per sample instead of two.  u, v are not part of the record: finalize_hit computes them only with ALBEDO.
#define RT_TU 3
#include "rt_kernel.hip"
#define RT_GUIDE_QUERIES
#include "rt_guide.h"
#include "rt_query_dev.h"

namespace rt {

// Resident waves per SIMD the register allocation is held to, from -Rpass-analysis=kernel-resource-usage (make asm), the loop depth of
// every scratch access (tools/scratch_map.py) and an A/B on the device; the table is in DESIGN §20.  AlbedoWaves' camera column for the two
// BVH classes with everything (3 and 1).  The list and mesh classes are held to 4 where the albedo kernels run 6 and 5: the seven (ten)
// accumulators live across the search, and at 5 waves (96 VGPRs) the list kernel spills 9 (19) registers and the mesh kernel 63 (89) —
// *measured* (profiles/denoise_guide.log): at 4 the mesh kernel is 26 % faster (no spill, 6 with ALBEDO), the list kernel 0–9 % (none).
// make KFLAGS="-DRT_GUIDE_LIST_WAVES=5u -DRT_GUIDE_MESH_WAVES=5u" builds the other side of that A/B.
#ifndef RT_GUIDE_LIST_WAVES
#define RT_GUIDE_LIST_WAVES 4u
#endif
#ifndef RT_GUIDE_MESH_WAVES
#define RT_GUIDE_MESH_WAVES 4u
#endif
template <uint32_t FEATS, bool ALBEDO> struct GuideWaves {
    static constexpr uint32_t v = FEATS == 0u ? RT_GUIDE_LIST_WAVES : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? RT_GUIDE_MESH_WAVES : ((FEATS & F_NESTED) ? 1u : 3u));
};

template <uint32_t FEATS, bool ALBEDO>
__global__ void __launch_bounds__(QUERY_THREADS, (GuideWaves<FEATS, ALBEDO>::v)) guide_kernel(const KParams<double> P, const GuideArgs A) {
    if ((FEATS & F_BVH) && P.n_cached != 0u) {
        // the filter tree, once per workgroup: rt_query_dev.h's stage_filter_tree<QUERY_THREADS>(P), restated — with the call in its place
        // this kernel's registers are numbered differently down to its stores, which the other five units' are not (docs/history.md)
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
    const uint32_t n_samples = A.n_samples;                       // uniform: every lane of a wave runs the same number of searches
    for (uint64_t base = (uint64_t)blockIdx.x * QUERY_THREADS; base < n; base += (uint64_t)gridDim.x * QUERY_THREADS) {
        if (base + (threadIdx.x & ~63u) >= n) break;              // (wave-uniform: a wave with no lane at all, in the last batch only)
        const uint64_t i64 = base + threadIdx.x;
        const bool mine = i64 < n;
        const uint32_t k = mine ? (uint32_t)i64 : n - 1u;         // a partial last wave repeats the last pixel: every lane takes part in the votes
        // (these accumulators and the eight stores below have a twin in rt_chain.hip's camera form, written out in both: as one struct they
        // move every instantiation's register allocation, docs/history.md)
        double st = 0.0, p0 = 0.0, p1 = 0.0, p2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        uint32_t h = 0u, hf = 0u;
        int32_t m_first = -1, o_first = -1;                       // words [11], [12] of the first hitting sample, as the integers they hold
        bool m_same = true, o_same = true;
        for (uint32_t s = 0; s < n_samples; s++) {
            RayT<double> ray; Rng rng;
            camera_ray(P, A.seed, k, A.first_sample + s, ray, rng);
            double t_hit; HitId id; id.obj = 0u; id.prim = 0u;
            bool any;
            if constexpr (FEATS == 0u) any = world_hit_list<double>(P, ray, A.t_min, rng, t_hit, id);
            else any = world_hit<double, FEATS>(P, ray, A.t_min, rng, t_hit, id, nullptr);
            Rec<double> rec; rec.p = mk<double>(0.0, 0.0, 0.0); rec.n = rec.p; rec.t = 0.0; rec.u = rec.v = 0.0; rec.front = false; rec.mat = 0u;
            if (any) finalize_hit<double, FEATS>(P, ray, t_hit, id, ALBEDO, rec);
            if constexpr (ALBEDO) {
                const V3<double> a = albedo_of<FEATS>(P, any, rec);
                a0 += a.x; a1 += a.y; a2 += a.z;
            }
            if (any) {
                const int32_t mw = id.prim == PRIM_MEDIUM ? -1 : (int32_t)rec.mat;    // (a medium's Isotropic was appended by the flattener: no handle)
                const int32_t ow = (int32_t)id.obj;
                if (h == 0u) { m_first = mw; o_first = ow; }
                else { m_same = m_same && mw == m_first; o_same = o_same && ow == o_first; }
                h++;
                hf += rec.front ? 1u : 0u;
                st += rec.t;
                p0 += rec.p.x; p1 += rec.p.y; p2 += rec.p.z;
                n0 += rec.n.x; n1 += rec.n.y; n2 += rec.n.z;
            }
        }
        if (mine) {
            const bool some = h != 0u;
            const double dh = (double)h;
            d2* o = (d2*)(A.guide + 16ull * k);
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
        }
    }
}

// the instantiation: query_kernel's classes, with the optional output in the camera flag's place
template <typename G> static auto guide_kernel_for(uint32_t scene_feats, bool albedo, G&& g) {
    return scene_class_dispatch(scene_feats, [&](auto feats) {
        return flag_dispatch(albedo, [&](auto alb) { return g(guide_kernel<decltype(feats)::value, decltype(alb)::value>); });
    });
}
int guide_blocks_per_cu(uint32_t scene_feats, bool albedo, size_t shmem) {
    return guide_kernel_for(scene_feats, albedo, [&](auto kernel) { return kernel_blocks_per_cu(kernel, QUERY_THREADS, shmem); });
}
hipError_t launch_guide(const KParams<double>& P, const GuideArgs& A, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return guide_kernel_for(scene_feats, A.albedo != nullptr, [&](auto kernel) { return kernel_launch(kernel, QUERY_THREADS, n_blocks, shmem, stream, P, A); });
}

} // namespace rt

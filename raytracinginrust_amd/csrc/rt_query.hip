// csrc/rt_query.hip — ray queries: world.hit(r, t_min, +inf) (src/main.rs:48, Hittable::hit) for rays the caller chooses, or for the
// camera ray of one sample of every pixel, and the hit record (hit.rs:9-24) written out — what a host needs for picking, auto-focus, depth /
// normal / material frames, visibility probes (include/rt_amd.h: rt_query_hits, rt_query_camera).
//
// A translation unit of its own over rt_kernel.hip's device functions (RT_TU == 3 leaves that file's kernels and launch code out): the
// search and the record are world_hit / world_hit_list / finalize_hit — the code the frames run, one ray per lane — and nothing is
// added to the two units the frames are built from (one more caller there changes other kernels' machine code, docs/history.md).
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

namespace rt {

typedef double d2 __attribute__((ext_vector_type(2)));

// Resident waves per SIMD the register allocation is held to (workgroups of four waves, one per SIMD: this is also the resident
// workgroups per CU the registers allow).  From -Rpass-analysis=kernel-resource-usage and the loop depth of every scratch access in the
// ISA (make asm, tools/scratch_map.py) — f64, no shading code:
//   list scenes 5 (76 / 93 VGPRs caller rays / camera, no scratch); mesh scenes 5 (96 VGPRs, 4 / 14 registers spilled, every scratch access
//   outside the box-step and leaf-step loops); everything else without object leaves 3 (123 / 130 VGPRs, no scratch); with object leaves 1:
//   held to 2 that search spills 255 registers and reads scratch inside the box-step loops, with all 512 registers it does not.
template <uint32_t FEATS> struct QueryWaves {
    static constexpr uint32_t v = FEATS == 0u ? 5u : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? 5u : ((FEATS & F_NESTED) ? 1u : 3u));
};

// seven doubles at a 16-byte aligned base + 56 k bytes: 16-byte aligned for even k, 8 bytes past that for odd k — three 16-byte accesses
// and one of 8 bytes either way
DEV void load_ray(const double* rays, uint32_t k, RayT<double>& ray) {
    const double* p = rays + 7ull * k;
    const uint32_t odd = k & 1u;
    const d2* q = (const d2*)(p + odd);
    const d2 a = q[0], b = q[1], c = q[2];
    const double s = odd ? p[0] : p[6];
    ray.o = odd ? mk<double>(s, a.x, a.y) : mk<double>(a.x, a.y, b.x);
    ray.d = odd ? mk<double>(b.x, b.y, c.x) : mk<double>(b.y, c.x, c.y);
    ray.tm = odd ? c.y : s;
}
DEV void store_ray(double* rays, uint32_t k, const RayT<double>& ray) {
    double* p = rays + 7ull * k;
    const uint32_t odd = k & 1u;
    d2* q = (d2*)(p + odd);
    d2 a, b, c;
    if (odd) { a.x = ray.o.y; a.y = ray.o.z; b.x = ray.d.x; b.y = ray.d.y; c.x = ray.d.z; c.y = ray.tm; p[0] = ray.o.x; }
    else { a.x = ray.o.x; a.y = ray.o.y; b.x = ray.o.z; b.y = ray.d.x; c.x = ray.d.y; c.y = ray.d.z; p[6] = ray.tm; }
    q[0] = a; q[1] = b; q[2] = c;
}

// Camera::get_ray for sample `sample` of output-order pixel gp: refill_queue's arithmetic (main.rs:813-820, camera.rs:51-59), expression
// for expression, the draws in its order — u, v, the lens disk's rejection loop, time.  `g` is left where the path's stream stands then.
DEV void camera_ray(const KParams<double>& P, uint64_t seed, uint32_t gp, uint32_t sample, RayT<double>& ray, Rng& g) {
    typedef double T;
    const uint32_t row = gp / P.W;
    const uint32_t g_i = gp - row * P.W, g_j = P.H - 1u - row;      // row 0 is j = H-1, main.rs:772
    g = rng_for_path(seed, gp, sample);
    T random_u = rng_u01(g, T(0));
    T random_v = rng_u01(g, T(0));
    T u = (T(g_i) + random_u) / T(P.W - 1u);
    T v = (T(g_j) + random_v) / T(P.H - 1u);
    T da, db;
    for (;;) {
        da = rng_range(g, T(-1.0), T(1.0));
        db = rng_range(g, T(-1.0), T(1.0));
        V3<T> pd = mk<T>(da, db, T(0));
        if (dot(pd, pd) < T(1.0)) break;
    }
    V3<T> rd = P.cam.lens_radius * mk<T>(da, db, T(0));
    V3<T> offset = ld3(P.cam.cu) * rd.x + ld3(P.cam.cv) * rd.y;
    T time = P.cam.time0 + rng_u01(g, T(0)) * (P.cam.time1 - P.cam.time0);
    ray.o = ld3(P.cam.origin) + offset;
    ray.d = ld3(P.cam.lower_left_corner) + u * ld3(P.cam.horizontal) + v * ld3(P.cam.vertical) - (ld3(P.cam.origin) + offset);
    ray.tm = time;
}

template <uint32_t FEATS, bool CAMERA>
__global__ void __launch_bounds__(QUERY_THREADS, QueryWaves<FEATS>::v) query_kernel(const KParams<double> P, const QueryArgs Q) {
    if ((FEATS & F_BVH) && P.n_cached != 0u) {
        // the filter tree, once per workgroup (pathtrace_kernel's staging of a tree that fits: the host stages the whole tree or nothing):
        // 16-byte pieces, consecutive threads consecutive pieces; links become LDS addresses (a node state IS where its record lies:
        // bvh_hit_filt), a leaf's info stays its id
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

// the instantiation by scene class: pathtrace_kernel's rule (rt_kernel.hip dispatch) without its scheduling variants — reference order,
// no persistent loop, no walk-ahead — and without the principled material, which changes no hit
static const uint32_t QF_MESH = F_BVH | F_TRIS, QF_NO_PBR = F_ALL & ~F_PBR, QF_NESTED = F_ALL | F_NESTED;
template <typename F> static auto query_dispatch(uint32_t scene_feats, bool camera, F&& f) {
    auto by_mode = [&](auto feats) { return camera ? f(feats, std::true_type()) : f(feats, std::false_type()); };
    if (scene_feats == 0u) return by_mode(std::integral_constant<uint32_t, 0u>());
    if (scene_feats & F_NESTED) return by_mode(std::integral_constant<uint32_t, QF_NESTED>());
    if ((scene_feats & ~QF_MESH) == 0u) return by_mode(std::integral_constant<uint32_t, QF_MESH>());
    return by_mode(std::integral_constant<uint32_t, QF_NO_PBR>());
}
uint32_t query_feats(uint32_t scene_feats) {
    return query_dispatch(scene_feats, false, [](auto feats, auto) { return (uint32_t) decltype(feats)::value; });
}
template <uint32_t FEATS, bool CAMERA> static hipError_t query_allow_lds(size_t shmem) {     // more than the default 64 KB of dynamic LDS needs to be asked for
    if (shmem <= 65536u) return hipSuccess;
    return hipFuncSetAttribute((const void*)query_kernel<FEATS, CAMERA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
}
int query_blocks_per_cu(uint32_t scene_feats, bool camera, size_t shmem) {
    return query_dispatch(scene_feats, camera, [&](auto feats, auto cam) {
        constexpr uint32_t FEATS = decltype(feats)::value; constexpr bool CAMERA = decltype(cam)::value;
        int nb = 0;
        if (query_allow_lds<FEATS, CAMERA>(shmem) != hipSuccess) return 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, query_kernel<FEATS, CAMERA>, (int)QUERY_THREADS, shmem) != hipSuccess) return 0;
        return nb;
    });
}
hipError_t launch_query(const KParams<double>& P, const QueryArgs& Q, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return query_dispatch(scene_feats, camera, [&](auto feats, auto cam) {
        constexpr uint32_t FEATS = decltype(feats)::value; constexpr bool CAMERA = decltype(cam)::value;
        const hipError_t e = query_allow_lds<FEATS, CAMERA>(shmem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((query_kernel<FEATS, CAMERA>), dim3(n_blocks), dim3(QUERY_THREADS), shmem, stream, P, Q);
        return hipGetLastError();
    });
}

} // namespace rt

// csrc/rt_albedo.hip — the first-hit albedo query (rt_query_albedo*, rt_query_camera_albedo*) and the two element-wise kernels of
// albedo-demodulated denoising (rt_denoise_albedo*); the specifications are in rt_albedo.h.
//
// A translation unit of its own over rt_kernel.hip's device functions (RT_TU == 3, as rt_query.hip and rt_radiance.hip): the search, the
// record and the texture walk are world_hit / world_hit_list / finalize_hit / tex_eval — the code the frames run — and nothing is added to
// the units the frames and the filter are built from.  load_ray, camera_ray, albedo_of and the scene-class dispatch are the query units' own:
// rt_query_dev.h.
//
// Shape: query_kernel's — 256-thread workgroups, at most (CUs x resident workgroups) of them, the filter tree staged in LDS when the WHOLE
// tree fits, batches of 256 lanes grid-stride, whole waves in every voting search (lanes past n repeat the last lane's work and only skip
// their stores).  Caller rays: one ray per lane.  Camera form: one PIXEL per lane, which loops over its samples in ascending order and adds
// into three f64 registers that start at +0.0 — n_samples is uniform, so the waves stay whole, and there are no atomics: the sum order is
// fixed and the same call gives the same words.
#define RT_TU 3
#include "rt_kernel.hip"
#define RT_ALBEDO_QUERIES
#include "rt_albedo.h"
#include "rt_query_dev.h"

namespace rt {

// Resident waves per SIMD the register allocation is held to, from -Rpass-analysis=kernel-resource-usage (make asm) and the loop depth of
// every scratch access (tools/scratch_map.py); the table is in DESIGN §15.  QueryWaves' classes: tex_eval (Perlin turbulence, the image
// fetch) lives after the search and adds no register pressure inside the box-step and leaf-step loops.
template <uint32_t FEATS> struct AlbedoWaves {
    static constexpr uint32_t v = FEATS == 0u ? 5u : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? 5u : ((FEATS & F_NESTED) ? 1u : 3u));
};

template <uint32_t FEATS, bool CAMERA>
__global__ void __launch_bounds__(QUERY_THREADS, AlbedoWaves<FEATS>::v) albedo_kernel(const KParams<double> P, const AlbedoArgs A) {
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
    const uint32_t n_samples = CAMERA ? A.n_samples : 1u;         // uniform: every lane of a wave runs the same number of searches
    for (uint64_t base = (uint64_t)blockIdx.x * QUERY_THREADS; base < n; base += (uint64_t)gridDim.x * QUERY_THREADS) {
        if (base + (threadIdx.x & ~63u) >= n) break;              // (wave-uniform: a wave with no lane at all, in the last batch only)
        const uint64_t i64 = base + threadIdx.x;
        const bool mine = i64 < n;
        const uint32_t k = mine ? (uint32_t)i64 : n - 1u;         // a partial last wave repeats the last ray / pixel: every lane takes part in the votes
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (uint32_t s = 0; s < n_samples; s++) {
            RayT<double> ray; Rng rng;
            if (CAMERA) camera_ray(P, A.seed, k, A.first_sample + s, ray, rng);
            else { load_ray(A.rays, k, ray); rng = rng_for_stream(A.seed, k); }
            double t_hit; HitId id; id.obj = 0u; id.prim = 0u;
            bool any;
            if constexpr (FEATS == 0u) any = world_hit_list<double>(P, ray, A.t_min, rng, t_hit, id);
            else any = world_hit<double, FEATS>(P, ray, A.t_min, rng, t_hit, id, nullptr);
            Rec<double> rec; rec.p = mk<double>(0.0, 0.0, 0.0); rec.n = rec.p; rec.t = 0.0; rec.u = rec.v = 0.0; rec.front = false; rec.mat = 0u;
            if (any) finalize_hit<double, FEATS>(P, ray, t_hit, id, true, rec);
            const V3<double> a = albedo_of<FEATS>(P, any, rec);
            if (CAMERA) { s0 += a.x; s1 += a.y; s2 += a.z; }
            else {
                s0 = a.x; s1 = a.y; s2 = a.z;
                if (mine && A.hits) {                             // the words query_kernel writes (a twin of its stores, as chain_kernel's are)
                    const bool medium = any && id.prim == PRIM_MEDIUM;
                    const bool named = any && !medium;
                    d2* o = (d2*)(A.hits + 16ull * k);
                    d2 w;
                    w.x = any ? 1.0 : 0.0; w.y = any ? rec.t : 0.0; o[0] = w;
                    w.x = rec.p.x; w.y = rec.p.y; o[1] = w;
                    w.x = rec.p.z; w.y = rec.n.x; o[2] = w;
                    w.x = rec.n.y; w.y = rec.n.z; o[3] = w;
                    w.x = rec.front ? 1.0 : 0.0; w.y = rec.u; o[4] = w;
                    w.x = rec.v; w.y = named ? (double)rec.mat : -1.0; o[5] = w;
                    w.x = any ? (double)id.obj : -1.0; w.y = named ? (double)(id.prim >> 28) : -1.0; o[6] = w;
                    w.x = named ? (double)(id.prim & 0x0FFFFFFFu) : -1.0; w.y = 0.0; o[7] = w;
                }
            }
        }
        if (mine) { double* o = A.albedo + 3ull * k; o[0] = s0; o[1] = s1; o[2] = s2; }
    }
}

// the instantiation: query_kernel's classes and forms
template <typename G> static auto albedo_kernel_for(uint32_t scene_feats, bool camera, G&& g) {
    return scene_class_dispatch(scene_feats, [&](auto feats) {
        return flag_dispatch(camera, [&](auto cam) { return g(albedo_kernel<decltype(feats)::value, decltype(cam)::value>); });
    });
}
int albedo_blocks_per_cu(uint32_t scene_feats, bool camera, size_t shmem) {
    return albedo_kernel_for(scene_feats, camera, [&](auto kernel) { return kernel_blocks_per_cu(kernel, QUERY_THREADS, shmem); });
}
hipError_t launch_albedo(const KParams<double>& P, const AlbedoArgs& A, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return albedo_kernel_for(scene_feats, camera, [&](auto kernel) { return kernel_launch(kernel, QUERY_THREADS, n_blocks, shmem, stream, P, A); });
}

// ------------------------------------------------------------------ demodulate / remodulate (rt_albedo.h (2)): element-wise over the 3 n_px
// doubles of a frame; the PAIR forms move 16 bytes per access and serve buffers that are all 16-byte aligned, the tail (an odd count) and
// any other buffer go through the scalar forms
__global__ __launch_bounds__(256) void albedo_demodulate2_kernel(const d2* __restrict__ sum, const d2* __restrict__ alb, double albedo_samples, d2* __restrict__ x, uint64_t n_pairs) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pairs) return;
    const d2 s = sum[i], a = alb[i];
    d2 r;
    r.x = albedo_demodulate(s.x, albedo_modulation(a.x, albedo_samples));
    r.y = albedo_demodulate(s.y, albedo_modulation(a.y, albedo_samples));
    x[i] = r;
}
__global__ __launch_bounds__(256) void albedo_demodulate1_kernel(const double* __restrict__ sum, const double* __restrict__ alb, double albedo_samples, double* __restrict__ x, uint64_t first, uint64_t n) {
    const uint64_t i = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    x[i] = albedo_demodulate(sum[i], albedo_modulation(alb[i], albedo_samples));
}
__global__ __launch_bounds__(256) void albedo_remodulate2_kernel(d2* __restrict__ io, const d2* __restrict__ alb, double albedo_samples, uint64_t n_pairs) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pairs) return;
    const d2 y = io[i], a = alb[i];
    d2 r;
    r.x = albedo_remodulate(y.x, albedo_modulation(a.x, albedo_samples));
    r.y = albedo_remodulate(y.y, albedo_modulation(a.y, albedo_samples));
    io[i] = r;
}
__global__ __launch_bounds__(256) void albedo_remodulate1_kernel(double* __restrict__ io, const double* __restrict__ alb, double albedo_samples, uint64_t first, uint64_t n) {
    const uint64_t i = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    io[i] = albedo_remodulate(io[i], albedo_modulation(alb[i], albedo_samples));
}

static bool aligned16(const void* a, const void* b, const void* c) { return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15u) == 0u; }
static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }     // n <= 3 * (2^31 - 1): fits

int launch_albedo_demodulate(const double* d_rgb_sum, const double* d_albedo_sum, uint64_t albedo_samples, double* d_x, uint64_t n, void* stream) {
    const uint64_t n_pairs = aligned16(d_rgb_sum, d_albedo_sum, d_x) ? n / 2u : 0u;
    if (n_pairs) hipLaunchKernelGGL(albedo_demodulate2_kernel, dim3(blocks_for(n_pairs)), dim3(256), 0, (hipStream_t)stream, (const d2*)d_rgb_sum, (const d2*)d_albedo_sum, (double)albedo_samples, (d2*)d_x, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(albedo_demodulate1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(256), 0, (hipStream_t)stream, d_rgb_sum, d_albedo_sum, (double)albedo_samples, d_x, 2u * n_pairs, n);
    return (int)hipGetLastError();
}
int launch_albedo_remodulate(double* d_io, const double* d_albedo_sum, uint64_t albedo_samples, uint64_t n, void* stream) {
    const uint64_t n_pairs = aligned16(d_io, d_albedo_sum, nullptr) ? n / 2u : 0u;
    if (n_pairs) hipLaunchKernelGGL(albedo_remodulate2_kernel, dim3(blocks_for(n_pairs)), dim3(256), 0, (hipStream_t)stream, (d2*)d_io, (const d2*)d_albedo_sum, (double)albedo_samples, n_pairs);
    if (2u * n_pairs < n) hipLaunchKernelGGL(albedo_remodulate1_kernel, dim3(blocks_for(n - 2u * n_pairs)), dim3(256), 0, (hipStream_t)stream, d_io, d_albedo_sum, (double)albedo_samples, 2u * n_pairs, n);
    return (int)hipGetLastError();
}

} // namespace rt

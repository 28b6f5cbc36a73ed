// csrc/rt_query_dev.h — what the query units share: rt_query.hip, rt_radiance.hip, rt_albedo.hip, rt_adaptive.hip, rt_guide.hip and
// rt_chain.hip, the translation units over rt_kernel.hip's device functions (RT_TU == 3).  Each of them includes this file after
// rt_kernel.hip.  Device side: a caller's ray in and out of memory, the camera ray of a sample, the step of a wave's path cursor, the
// albedo at a hit, and the staging of the filter tree in LDS (called by the two path-tracing forms; the four search kernels restate it,
// each with the reason beside it).  Host side: the instantiation by scene class, the occupancy query and the launch.  Every device function is force-inlined (DEV): a kernel's machine code is what it was with the function's text written out in it,
// but for the register numbering of the staging prologue (docs/history.md has the comparison, and why the sixteen words of a hit record
// are not here).
#pragma once
#include <type_traits>

#if !defined(RT_TU) || RT_TU != 3
#error "rt_query_dev.h belongs behind rt_kernel.hip in a query unit (RT_TU == 3)"
#endif

namespace rt {

typedef double d2 __attribute__((ext_vector_type(2)));

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

// the cursor of the path-tracing forms (radiance_kernel, pixels_kernel): (k, s) + add paths, add <= 64, s < spp — no 64-bit division;
// with spp >= 64 the sample index wraps at most once
DEV void path_step(uint32_t k, uint32_t s, uint32_t add, uint32_t spp, uint32_t& k_out, uint32_t& s_out) {
    const uint64_t t = (uint64_t)s + add;
    if (spp >= 64u) {
        const bool wrap = t >= spp;
        k_out = k + (wrap ? 1u : 0u); s_out = (uint32_t)(wrap ? t - spp : t);
    } else {
        const uint32_t q = (uint32_t)t / spp;
        k_out = k + q; s_out = (uint32_t)t - q * spp;
    }
}

// the table of rt_albedo.h (1) on a finalized record.  List scenes (FEATS == 0: constant textures only) take the colour from the material
// record, as the frames' const_or_tex does; the others walk the texture graph.
template <uint32_t FEATS> DEV V3<double> albedo_of(const KParams<double>& P, bool any, const Rec<double>& rec) {
    const V3<double> one = mk<double>(1.0, 1.0, 1.0);
    if (!any) return one;
    const DMaterial<double> mt = ld_mat(P.materials + rec.mat);
    if (mt.kind == M_METAL) return ld3(mt.albedo);
    if (mt.kind == M_LAMBERTIAN || mt.kind == M_PBR || mt.kind == M_ISOTROPIC) {
        if constexpr (FEATS == 0u) return ld3(mt.albedo);
        else return tex_eval<double, FEATS>(P, mt.tex, rec.u, rec.v, rec.p);
    }
    return one;                                                     // Dielectric, DiffuseLight
}

// The filter tree into LDS, once per workgroup of THREADS threads (pathtrace_kernel's staging of a tree that fits: the host stages the whole
// tree or nothing): 16-byte pieces, consecutive threads consecutive pieces; links become LDS addresses (a node state IS where its record
// lies: bvh_hit_filt), a leaf's info stays its id.  Ends with the kernel's only barrier: the caller asks (FEATS & F_BVH) && P.n_cached != 0u
// first, which is uniform over the workgroup.
template <uint32_t THREADS> DEV void stage_filter_tree(const KParams<double>& P) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const uint32_t nodes_bytes = P.n_cached * (uint32_t)sizeof(DFNode);
    const u4* src = (const u4*)P.bvh_f; u4* dst = (u4*)lds_raw;
    const uint32_t base = lds_base();
    for (uint32_t i = threadIdx.x; i < nodes_bytes / 16u; i += THREADS) {
        u4 w = src[i];
        if (i & 1u) {                                         // second half of a DFNode: max.z-side bounds, skip, info
            if (w.z != ST_DONE) w.z = base + w.z * (uint32_t)sizeof(DFNode);
            if (!(w.w & FNODE_LEAF)) w.w = base + w.w * (uint32_t)sizeof(DFNode);
        }
        dst[i] = w;
    }
    __syncthreads();
}

// ------------------------------------------------------------------ host side
// The instantiation by scene class: pathtrace_kernel's rule (rt_kernel.hip dispatch) without its scheduling variants — reference order, no
// persistent loop, no walk-ahead, so no BVH stack.  f(std::integral_constant<uint32_t, FEATS>) for the class that serves `scene_feats`:
// list scenes, object leaves, meshes, everything else.  PBR_CLASS: the principled material has a class of its own (the path-tracing
// forms, which shade); without it that material rides in the "everything else" class (the searches: it changes no hit).
static const uint32_t SC_MESH = F_BVH | F_TRIS, SC_NO_PBR = F_ALL & ~F_PBR, SC_NESTED = F_ALL | F_NESTED;
template <bool PBR_CLASS, typename F> static auto scene_class_dispatch_as(uint32_t scene_feats, F&& f) {
    if (scene_feats == 0u) return f(std::integral_constant<uint32_t, 0u>());
    if (scene_feats & F_NESTED) return f(std::integral_constant<uint32_t, SC_NESTED>());
    if ((scene_feats & ~SC_MESH) == 0u) return f(std::integral_constant<uint32_t, SC_MESH>());
    // (the classes stand in the order the kernels have always been instantiated in: that is their order in the code object)
    if constexpr (!PBR_CLASS) return f(std::integral_constant<uint32_t, SC_NO_PBR>());
    else return (scene_feats & ~SC_NO_PBR) == 0u ? f(std::integral_constant<uint32_t, SC_NO_PBR>()) : f(std::integral_constant<uint32_t, (uint32_t)F_ALL>());
}
template <typename F> static auto scene_class_dispatch(uint32_t scene_feats, F&& f) { return scene_class_dispatch_as<false>(scene_feats, f); }
template <typename F> static auto scene_class_dispatch_pbr(uint32_t scene_feats, F&& f) { return scene_class_dispatch_as<true>(scene_feats, f); }
// ... and a run-time flag of a kernel (camera form, albedo output) as std::true_type / std::false_type
template <typename F> static auto flag_dispatch(bool flag, F&& f) { return flag ? f(std::true_type()) : f(std::false_type()); }

// more than the default 64 KB of dynamic LDS needs to be asked for
template <typename K> static hipError_t kernel_allow_lds(K kernel, size_t shmem) {
    if (shmem <= 65536u) return hipSuccess;
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
}
// Resident workgroups per CU of `kernel` with `shmem` bytes of dynamic LDS; 0: the query failed
template <typename K> static int kernel_blocks_per_cu(K kernel, uint32_t threads, size_t shmem) {
    int nb = 0;
    if (kernel_allow_lds(kernel, shmem) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, (int)threads, shmem) != hipSuccess) return 0;
    return nb;
}
template <typename A> static hipError_t kernel_launch(void (*kernel)(KParams<double>, A), uint32_t threads, uint32_t n_blocks, size_t shmem, hipStream_t stream,
                                                      const KParams<double>& P, const A& args) {
    const hipError_t e = kernel_allow_lds(kernel, shmem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(threads), shmem, stream, P, args);
    return hipGetLastError();
}

} // namespace rt

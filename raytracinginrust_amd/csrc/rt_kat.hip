// csrc/rt_kat.hip — known-answer access to the SHADING side of rt_kernel.hip: the hand-written sincos_0_2pi, the device libm as the
// kernels call it (m_sin ... m_pow), the Vec3 / f64 division in both of its forms, onb_from_w, the principled material's helpers,
// pbr_brdf / brdf_pdf_value, and one call of shade_hit — each run on caller operands, one record per lane (include/rt_amd.h: rt_debug_math,
// rt_debug_brdf, rt_debug_shade).
//
// A translation unit of its own over rt_kernel.hip's device functions (RT_TU == 4 leaves that file's kernels and launch code out, as
// RT_TU == 3 does for the query units), so nothing is added to the units the frames are built from.  It is compiled TWICE (csrc/Makefile),
// once per code shape of those units: -DRT_SHAPE=1 with the lean unit's flags (MERGE_ARMS, SHORT_*, no pre-RA scheduler), -DRT_SHAPE=2
// with the other unit's (SHARED_DIV3).  The kernels are templates over the shape, so the two objects' symbols differ.
//
// Shape: 256-thread workgroups, one record per lane.  Lanes past n repeat the last record and only their store is left out (some of the
// functions vote per wave: a wave runs whole).  No bounds are computed from operands: every index is the lane's record number below n.
#define RT_TU 4
#ifndef RT_SHAPE
#error "rt_kat.hip is compiled with -DRT_SHAPE=1 (the lean unit's code shape) or -DRT_SHAPE=2 (the other unit's)"
#endif
#include "rt_kernel.hip"
#include "rt_kat.h"

namespace rt {

template <int SHAPE>
__global__ void __launch_bounds__(KAT_THREADS) math_kat_kernel(uint32_t op, uint32_t w, uint32_t n, const double* a, const double* b, double* out) {
    const uint64_t i64 = (uint64_t)blockIdx.x * KAT_THREADS + threadIdx.x;
    const bool mine = i64 < n;
    const uint64_t k = mine ? i64 : (uint64_t)n - 1u;
    double o[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    switch (op) {                                                  // (wave-uniform)
    case KAT_SINCOS_0_2PI: sincos_0_2pi(a[k], o[0], o[1]); break;
    case KAT_SIN: o[0] = m_sin(a[k]); break;
    case KAT_COS: o[0] = m_cos(a[k]); break;
    case KAT_TAN: o[0] = m_tan(a[k]); break;
    case KAT_ATAN: o[0] = m_atan(a[k]); break;
    case KAT_ATAN2: o[0] = m_atan2(a[k], b[k]); break;
    case KAT_ACOS: o[0] = m_acos(a[k]); break;
    case KAT_LOG: o[0] = m_log(a[k]); break;
    case KAT_LOG2: o[0] = m_log2(a[k]); break;
    case KAT_POW: o[0] = m_pow(a[k], b[k]); break;
    case KAT_DIV3: {
        // the quotient through the operator the kernels' expressions use; the form from div3 itself, on the same operands
        const V3<double> v = mk<double>(a[3u * k], a[3u * k + 1u], a[3u * k + 2u]);
        const V3<double> q = v / b[k];
        bool shared; (void)div3(v, b[k], shared);
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = shared ? 1.0 : 0.0;
    } break;
    case KAT_ONB: {
        const Onb<double> u = onb_from_w(mk<double>(a[3u * k], a[3u * k + 1u], a[3u * k + 2u]));
        o[0] = u.u.x; o[1] = u.u.y; o[2] = u.u.z; o[3] = u.v.x; o[4] = u.v.y; o[5] = u.v.z; o[6] = u.w.x; o[7] = u.w.y; o[8] = u.w.z;
    } break;
    case KAT_GTR_1: o[0] = GTR_1(a[k], b[k]); break;
    case KAT_GTR_2_ANISO: o[0] = GTR_2_aniso(a[3u * k], a[3u * k + 1u], a[3u * k + 2u], b[2u * k], b[2u * k + 1u]); break;
    case KAT_SMITHG_GGX: o[0] = smithG_GGX(a[k], b[k]); break;
    case KAT_SMITHG_GGX_ANISO: o[0] = smithG_GGX_aniso(a[3u * k], a[3u * k + 1u], a[3u * k + 2u], b[2u * k], b[2u * k + 1u]); break;
    case KAT_SCHLICK: o[0] = schlick_fresnel(a[k]); break;
    default: break;
    }
    if (mine) {                                                    // w: the op's doubles per record of out (rt_kat.h KAT_RECORDS), <= 9
        for (uint32_t j = 0; j < w; j++) out[(uint64_t)w * k + j] = o[j];
    }
}

// Material::brdf (pbr_brdf) and PDF::BRDF value (brdf_pdf_value, on the basis shade_hit gives it: onb_from_w(normal)) of entry `pbr`
template <int SHAPE>
__global__ void __launch_bounds__(KAT_THREADS) brdf_kat_kernel(const KParams<double> P, uint32_t n, uint32_t pbr, const double* in, double* out) {
    const uint64_t i64 = (uint64_t)blockIdx.x * KAT_THREADS + threadIdx.x;
    const bool mine = i64 < n;
    const uint64_t k = mine ? i64 : (uint64_t)n - 1u;
    const double* p = in + KAT_BRDF_IN * k;
    const V3<double> r_in = mk<double>(p[0], p[1], p[2]), r_out = mk<double>(p[3], p[4], p[5]), normal = mk<double>(p[6], p[7], p[8]), base = mk<double>(p[9], p[10], p[11]);
    const DPbr<double> pm = ld_pbr(P.pbr + pbr);
    const V3<double> f = pbr_brdf(pm, base, r_in, r_out, normal);
    const Onb<double> uvw = onb_from_w(normal);
    const double pv = brdf_pdf_value(pm, uvw, r_in, r_out);
    if (mine) { double* o = out + KAT_BRDF_OUT * k; o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = pv; }
}

// ONE call of shade_hit per lane (rt_debug_shade): the hit record, the incoming ray and the path state are the caller's, the stream is
// rng_for_path(seed, lane's record number, 0) — the frames' keying with the record in the pixel's place.  in: KAT_SHADE_IN doubles per record
// (the host builds and checks it: material and rect indices lie inside the scene's tables), out: KAT_SHADE_OUT.
template <int SHAPE, uint32_t FEATS>
__global__ void __launch_bounds__(KAT_THREADS) shade_kat_kernel(const KParams<double> P, const ShadeKatArgs A) {
    typedef double T;
    const uint64_t i64 = (uint64_t)blockIdx.x * KAT_THREADS + threadIdx.x;
    const bool mine = i64 < A.n;
    const uint32_t k = mine ? (uint32_t)i64 : A.n - 1u;           // a partial last wave repeats the last record: every lane takes part in the votes
    const double* p = A.in + (uint64_t)KAT_SHADE_IN * k;
    Rec<T> rec;
    rec.p = mk<T>(p[0], p[1], p[2]); rec.n = mk<T>(p[3], p[4], p[5]); rec.t = p[6]; rec.u = p[7]; rec.v = p[8]; rec.front = p[9] != 0.0;
    rec.mat = (uint32_t)p[10];
    const uint32_t rect = (uint32_t)p[11];
    RayT<T> ray; ray.o = mk<T>(p[12], p[13], p[14]); ray.d = mk<T>(p[15], p[16], p[17]); ray.tm = p[18];
    V3<T> beta = mk<T>(A.beta[0], A.beta[1], A.beta[2]);
    Rng rng = rng_for_path(A.seed, k, 0u);
    uint32_t depth_left = A.depth_left;
    bool done = false;
    V3<T> e = mk<T>(T(0), T(0), T(0));
    if constexpr (FEATS == 0u) shade_hit<T, FEATS>(P, rec, ray, beta, rng, depth_left, done, e, rect);
    else shade_hit<T, FEATS>(P, rec, ray, beta, rng, depth_left, done, e);
    if (mine) {
        double* o = A.out + (uint64_t)KAT_SHADE_OUT * k;
        o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z; o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z; o[6] = ray.tm;
        o[7] = beta.x; o[8] = beta.y; o[9] = beta.z; o[10] = e.x; o[11] = e.y; o[12] = e.z;
        o[13] = done ? 1.0 : 0.0; o[14] = (double)depth_left;
        o[15] = (double)rng.s0; o[16] = (double)rng.s1; o[17] = (double)rng.s2; o[18] = (double)rng.s3;
    }
}

#if RT_SHAPE == 1
// The same call as the COMPACT lean f64 kernel makes it (RT_KAT_TABLE_W; the lean shape only, so the other shape's object is not touched):
// the top of trace_shade_fill<double, 0u, true>'s material section — the rect word with `front` and the normal's three sign bits, the
// normal rebuilt from the ONB table, shade_hit<double, 0u, true> on that word (merged_arms_table_w: w, v, u from the table).  Records,
// stream, columns and the partial last wave are shade_kat_kernel's.  The host has checked that P.onb holds a valid entry for every rect
// and that each record's normal has its rect's magnitudes (Lemma N's premise) and a Lambertian or Metal material (the loop ends every
// other path before this call).
// The columns mean what they mean under the other forms: "the ray afterwards" is the incoming ray where nothing scatters.  The compact arm
// forms Metal's scattered ray in place before it knows whether the lane is absorbed (the loop does not read a finished lane's ray again),
// so a record that ends without a scatter — `done` with depth_left untouched — reports the ray it came with.
__global__ void __launch_bounds__(KAT_THREADS) shade_kat_table_w_kernel(const KParams<double> P, const ShadeKatArgs A) {
    typedef double T;
    const uint64_t i64 = (uint64_t)blockIdx.x * KAT_THREADS + threadIdx.x;
    const bool mine = i64 < A.n;
    const uint32_t k = mine ? (uint32_t)i64 : A.n - 1u;
    const double* p = A.in + (uint64_t)KAT_SHADE_IN * k;
    Rec<T> rec;
    rec.p = mk<T>(p[0], p[1], p[2]); rec.t = p[6]; rec.u = p[7]; rec.v = p[8]; rec.front = p[9] != 0.0;
    rec.mat = (uint32_t)p[10];
    const uint32_t word = ring_pack_signs((uint32_t)p[11] | (rec.front ? 0x80000000u : 0u), mk<T>(p[3], p[4], p[5]));
    rec.n = ring_normal(P.onb, word);
    RayT<T> ray; ray.o = mk<T>(p[12], p[13], p[14]); ray.d = mk<T>(p[15], p[16], p[17]); ray.tm = p[18];
    const RayT<T> came = ray;
    V3<T> beta = mk<T>(A.beta[0], A.beta[1], A.beta[2]);
    Rng rng = rng_for_path(A.seed, k, 0u);
    uint32_t depth_left = A.depth_left;
    bool done = false;
    V3<T> e = mk<T>(T(0), T(0), T(0));
    shade_hit<T, 0u, true>(P, rec, ray, beta, rng, depth_left, done, e, word);
    if (done && depth_left == A.depth_left) ray = came;
    if (mine) {
        double* o = A.out + (uint64_t)KAT_SHADE_OUT * k;
        o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z; o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z; o[6] = ray.tm;
        o[7] = beta.x; o[8] = beta.y; o[9] = beta.z; o[10] = e.x; o[11] = e.y; o[12] = e.z;
        o[13] = done ? 1.0 : 0.0; o[14] = (double)depth_left;
        o[15] = (double)rng.s0; o[16] = (double)rng.s1; o[17] = (double)rng.s2; o[18] = (double)rng.s3;
    }
}
#define KAT_NAME(f) f##_lean
#else
#define KAT_NAME(f) f##_rest
#endif
hipError_t KAT_NAME(launch_math_kat)(uint32_t op, uint32_t n, const double* d_a, const double* d_b, double* d_out, hipStream_t stream) {
    if (op >= KAT_N_OPS) return hipErrorInvalidValue;
    hipLaunchKernelGGL((math_kat_kernel<RT_SHAPE>), dim3((n + KAT_THREADS - 1u) / KAT_THREADS), dim3(KAT_THREADS), 0, stream, op, KAT_RECORDS[op][2], n, d_a, d_b, d_out);
    return hipGetLastError();
}
hipError_t KAT_NAME(launch_brdf_kat)(const KParams<double>& P, uint32_t n, uint32_t pbr, const double* d_in, double* d_out, hipStream_t stream) {
    hipLaunchKernelGGL((brdf_kat_kernel<RT_SHAPE>), dim3((n + KAT_THREADS - 1u) / KAT_THREADS), dim3(KAT_THREADS), 0, stream, P, n, pbr, d_in, d_out);
    return hipGetLastError();
}
// the lean unit's shape serves its own instantiation (FEATS == 0: list scenes); the other unit's the all-features ones, with object leaves
// and nested light lists where the scene has them
#if RT_SHAPE == 1
hipError_t launch_shade_kat_lean(const KParams<double>& P, const ShadeKatArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL((shade_kat_kernel<RT_SHAPE, 0u>), dim3((A.n + KAT_THREADS - 1u) / KAT_THREADS), dim3(KAT_THREADS), 0, stream, P, A);
    return hipGetLastError();
}
// ... and the compact kernel's (shade_hit<double, 0u, true>): P.onb is not null and every record's entry is valid (rt_host.cpp rt_debug_shade)
hipError_t launch_shade_kat_table_w(const KParams<double>& P, const ShadeKatArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(shade_kat_table_w_kernel, dim3((A.n + KAT_THREADS - 1u) / KAT_THREADS), dim3(KAT_THREADS), 0, stream, P, A);
    return hipGetLastError();
}
#else
hipError_t launch_shade_kat_rest(const KParams<double>& P, const ShadeKatArgs& A, bool nested, hipStream_t stream) {
    const dim3 grid((A.n + KAT_THREADS - 1u) / KAT_THREADS);
    if (nested) hipLaunchKernelGGL((shade_kat_kernel<RT_SHAPE, (uint32_t)(F_ALL | F_NESTED)>), grid, dim3(KAT_THREADS), 0, stream, P, A);
    else hipLaunchKernelGGL((shade_kat_kernel<RT_SHAPE, (uint32_t)F_ALL>), grid, dim3(KAT_THREADS), 0, stream, P, A);
    return hipGetLastError();
}
#endif

} // namespace rt

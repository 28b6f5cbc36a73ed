// csrc/rt_kat.h — interface between the host library (rt_host.cpp) and the known-answer kernels over rt_kernel.hip's shading-side device
// functions (csrc/rt_kat.hip).  That source is compiled twice, once per code shape of the frames' two units (rt_kernel.hip RT_SHAPE):
// `lean` = the list-scene unit's choices and flags (MERGE_ARMS, SHORT_*, LEANFLAGS), `rest` = the other unit's (SHARED_DIV3, NOLICM).
#pragma once
#include <hip/hip_runtime.h>
#include "rt_ir.h"

namespace rt {
// rt_debug_math's ops (include/rt_amd.h says what each computes) and their records: doubles per lane of a, of b, of out
enum KatOp : uint32_t {
    KAT_SINCOS_0_2PI = 0, KAT_SIN, KAT_COS, KAT_TAN, KAT_ATAN, KAT_ATAN2, KAT_ACOS, KAT_LOG, KAT_LOG2, KAT_POW, KAT_DIV3, KAT_ONB,
    KAT_GTR_1, KAT_GTR_2_ANISO, KAT_SMITHG_GGX, KAT_SMITHG_GGX_ANISO, KAT_SCHLICK, KAT_N_OPS
};
static const uint32_t KAT_RECORDS[KAT_N_OPS][3] = {
    {1u, 0u, 2u}, {1u, 0u, 1u}, {1u, 0u, 1u}, {1u, 0u, 1u}, {1u, 0u, 1u}, {1u, 1u, 1u}, {1u, 0u, 1u}, {1u, 0u, 1u}, {1u, 0u, 1u}, {1u, 1u, 1u},
    {3u, 1u, 4u}, {3u, 0u, 9u}, {1u, 1u, 1u}, {3u, 2u, 1u}, {1u, 1u, 1u}, {3u, 2u, 1u}, {1u, 0u, 1u}};
static const uint32_t KAT_THREADS = 256u;
static const uint32_t KAT_BRDF_IN = 12u, KAT_BRDF_OUT = 4u;      // r_in[3], r_out[3], normal[3], base[3] -> brdf[3], pdf value

// rt_debug_shade: per record in = position[3], normal[3], t, u, v, front_face, material, rect (the ONB memo's entry; lean only), ray origin[3],
// direction[3], time, 0; out = the ray afterwards (7), beta[3], e[3], done, depth_left, the stream's four state words
static const uint32_t KAT_SHADE_IN = 20u, KAT_SHADE_OUT = 19u;
struct ShadeKatArgs { uint32_t n; const double* in; double* out; double beta[3]; uint64_t seed; uint32_t depth_left; };

hipError_t launch_math_kat_lean(uint32_t op, uint32_t n, const double* d_a, const double* d_b, double* d_out, hipStream_t stream);
hipError_t launch_math_kat_rest(uint32_t op, uint32_t n, const double* d_a, const double* d_b, double* d_out, hipStream_t stream);
// pbr: the material's entry of KParams::pbr
hipError_t launch_brdf_kat_lean(const KParams<double>& P, uint32_t n, uint32_t pbr, const double* d_in, double* d_out, hipStream_t stream);
hipError_t launch_brdf_kat_rest(const KParams<double>& P, uint32_t n, uint32_t pbr, const double* d_in, double* d_out, hipStream_t stream);
// one call of shade_hit per record: shade_hit<double, 0> under the lean shape, <double, F_ALL> or (nested) <double, F_ALL | F_NESTED> under the other
hipError_t launch_shade_kat_lean(const KParams<double>& P, const ShadeKatArgs& A, hipStream_t stream);
hipError_t launch_shade_kat_rest(const KParams<double>& P, const ShadeKatArgs& A, bool nested, hipStream_t stream);
// the call as the compact lean f64 kernel's material section makes it (lean shape): the rect word packed with the normal's sign bits, the normal
// rebuilt from the ONB table, shade_hit<double, 0, true>.  For scenes with the compact ring and records that satisfy Lemma N's premise only.
hipError_t launch_shade_kat_table_w(const KParams<double>& P, const ShadeKatArgs& A, hipStream_t stream);
}

// csrc/rt_guide.h — the averaged denoising guide: first-hit records of N camera samples of a pixel reduced to ONE record in the 16-double
// layout of rt_query_camera (include/rt_amd.h HIT_FIELDS), so that every `hits` parameter of the denoise family takes it unchanged.  The
// specification, the host twin's seam (rt_guide_cpu.cpp, plain C++) and the launch of the HIP kernel (rt_guide.hip) as the host library
// sees it.  No HIP include unless RT_GUIDE_QUERIES asks for the kernel's interface at the end, as in rt_albedo.h.
//
// THE GUIDE of one pixel.  Only +, /, comparisons and integer counts, every operation rounded once (-ffp-contract=off), in this order.
// r_s, s = first_sample .. first_sample + n_samples - 1 ascending, are the very 16 doubles rt_query_camera(sample = s) writes.
//     h   = the number of records with hit != 0;  hf = the number of those with front_face != 0
//     St (1), Sp (3), Sn (3) = the sums of t, position, normal over the hitting records only, added in ascending sample order into
//          accumulators that start at +0.0
//     M   = the common value of word [11] (material; a medium's -1 is a value like any other) over the hitting records when they all
//          compare equal to the first of them, else -1
//     O   = the same for word [12] (object)
// The record:
//     [0]      hit         1.0 if h >= 1 && 2 h >= n_samples, else 0.0: the majority, a tie counting as hit
//     [1]      t           h ? St / h : 0.0
//     [2..4]   position    h ? Sp / h : 0
//     [5..7]   normal      h ? Sn / h : 0 — NOT renormalised: no square root in the specification, and an edge pixel's short normal is
//                          information
//     [8]      front_face  h ? hf / h : 0.0, a fraction
//     [9] [10] u, v        0.0
//     [11]     material    h ? M : -1
//     [12]     object      h ? O : -1
//     [13] [14] prim_kind, prim_index   -1
//     [15]     hits        (double) h, the coverage count (rt_query_camera writes 0.0 in this word and no reader uses it)
// What follows from it:
//   * n_samples = 1: words [0]-[8], [11], [12] equal rt_query_camera's AS VALUES.  A -0.0 component of a hitting record becomes +0.0:
//     +0.0 + -0.0 = +0.0 in the accumulator and +0.0 / 1 = +0.0.  (A miss's record is all +0.0 there already.)
//   * a pixel whose samples mix materials has material -1: key 1 under RT_DENOISE_SAME_MATERIAL, the key a medium has — never a miss's 0.
//   * a pixel whose samples mostly miss is a miss to the filter; words [1]-[8] and [15] still carry what the hitting samples saw.
//   * a NaN t of a hitting record (a NaN closest hit) makes St and word [1] NaN; NaN payloads are not specified.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rt {

static const uint32_t GUIDE_DOUBLES = 16u;                       // = QUERY_HIT_DOUBLES = DENOISE_HIT_DOUBLES

// The specification as code (arguments already checked): hits is [n_samples][n_px][16], guide_out [n_px][16]; they may not overlap.
void guide_from_hits_host(const double* hits, uint32_t n_samples, uint64_t n_px, double* guide_out);

} // namespace rt

// ---- the kernel (rt_guide.hip), for the translation units that see HIP (rt_guide.hip, rt_host.cpp)
#ifdef RT_GUIDE_QUERIES
#include "rt_query.h"
namespace rt {
// What a guide launch needs beside the scene's tables: guide[16 p ..] = the record above of output-order pixel p over samples first_sample ..
// first_sample + n_samples - 1, each sample's ray and stream those of rt_query_camera; albedo != nullptr: albedo[3 p ..] = the words
// rt_query_camera_albedo writes for the same samples (rt_albedo.h (1)), from the same searches.  guide 16-byte aligned, albedo 8-byte.
struct GuideArgs { double* guide; double* albedo; uint32_t n, first_sample, n_samples; double t_min; uint64_t seed; };
int guide_blocks_per_cu(uint32_t scene_feats, bool albedo, size_t shmem);
hipError_t launch_guide(const KParams<double>& P, const GuideArgs& A, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream);
}
#endif

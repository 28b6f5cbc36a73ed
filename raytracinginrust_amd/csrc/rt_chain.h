// csrc/rt_chain.h — specular-chain guides: the hit record and the albedo at the first NON-specular surface along the deterministic specular
// path of a ray (mirrors reflect about the centre of their lobe, glass takes the likelier Fresnel branch), the albedo multiplied by the
// mirrors' tints on the way.  The specification, the link step (one __host__ __device__ function: the HIP kernel of rt_chain.hip and the host
// twin rt_chain_cpu.cpp both call it, as reproject_pixel of rt_reproject.h is called), the host twin's seams, and the launch of the kernel as the
// host library sees it.  No HIP include unless RT_CHAIN_QUERIES asks for the kernel's interface at the end, as in rt_guide.h.
//
// Only + - * /, sqrt, fmin (f64::min: of a number and a NaN the number), fabs, comparisons and integer counts; every operation is rounded once
// (-ffp-contract=off), in the order written.  "finite" is v - v == 0; every comparison with a NaN is false; dot(a, b) = (a0*b0 + a1*b1) + a2*b2;
// a scalar times a vector multiplies each component by the scalar.  The HIP kernel, chain_step_host and the NumPy restatement of
// tests/chain_cases.py give the same 64-bit words.
//
// A chain starts from a ray r_0 and has up to max_links links (0 <= max_links <= 64); max_fuzz >= 0, finite or +inf.
//
// (C1) SEARCH.  Link l searches world.hit(r_l, t_min, +inf) with the frames' own search and record, exactly as rt_query_hits does.  The stream
//      of link 0: caller-ray form rng_for_stream(seed, k) (rt_query_hits'); camera form the sample's own stream continued after the camera's
//      draws (rt_query_camera's).  The stream of link l >= 1 of item k (the ray's index, or the output-order pixel):
//          rng_for_stream(seed_link, k),   seed_link = seed + ((sample_index << 8) | l) * 0x9E3779B97F4A7C15   (mod 2^64; sample_index as 64 bits)
//      with sample_index = 0 in the caller-ray form: link l of ALL items is one call rt_query_hits(rays_l, t_min, seed_link).  The step draws
//      no random number.
// (C2) END.  The chain ends with the current record when, in this order: the search misses (status 2); l == max_links (status 1, the step is
//      not evaluated); the hit is a medium hit or its material is neither Metal nor Dielectric (1); the material is Metal with !(fuzz <=
//      max_fuzz) — a NaN fuzz counts (5); the step's new direction is not finite in all three components (4); Metal only: !(dot(new_d, n) > 0)
//      — the frames would absorb the path, main.rs:108-110 (3).  Otherwise the link is FOLLOWED (status 0).
// (C3) METAL, fuzz <= max_fuzz (mat.rs:280-293 with the fuzz term left out: the centre of the lobe), d the ray's direction, n the record's normal:
//          dn = d + (((-dot(d, n)) * 2) * n);   new_d = dn / sqrt(dot(dn, dn));   weight <- weight * albedo, per channel
// (C4) DIELECTRIC (mat.rs:343-374, expression for expression; ir the index, front the record's front_face):
//          refraction_ratio = front ? 1 / ir : ir;   unit_direction = d / sqrt(dot(d, d))
//          cos_theta = fmin(dot(-1 * unit_direction, n), 1);   sin_theta = sqrt(1 - cos_theta * cos_theta)
//          cannot_refract = refraction_ratio * sin_theta > 1
//          q = (1 - refraction_ratio) / (1 + refraction_ratio);  r0 = q * q;  m1 = 1 - cos_theta;  m2 = m1 * m1;  refl = r0 + (1 - r0) * (m1 * (m2 * m2))
//          will_reflect = refl > 0.5                          (in the place of the random draw)
//          cannot_refract || will_reflect:  new_d = unit_direction + (((-dot(unit_direction, n)) * 2) * n)
//          else:  perp = refraction_ratio * (unit_direction + cos_theta * n);  len = sqrt(dot(perp, perp))
//                 new_d = perp + ((-1 * sqrt(fabs(1 - len * len))) * n)
//      The weight is unchanged.
// (C5) NEW RAY.  origin = the record's position, direction = new_d, time unchanged.
// (C6) RESULT RECORD: 16 doubles in rt_query_hits' layout, the LAST link's record, but for
//          [1]  0 links followed: that record's own t, bit for bit.  Otherwise S / L_0 with L_l = sqrt(dot(d_l, d_l)), S = t_0 * L_0 and then
//               S = S + t_l * L_l for l = 1, 2, ... ascending over the links whose search hit (a final miss adds no term): the path length
//               in the units of the first ray's parameter, which rt_denoise.h divides by
//          [15] the number of links followed, as a double (rt_query_hits writes 0.0 there and no reader uses it)
//      A chain that ends in a miss has hit = 0 and a miss's words elsewhere.
// (C7) CHAIN ALBEDO.  weight * a per channel, a from the table of rt_albedo.h (1) on the last record ((1, 1, 1) for a miss: a mirrored sky
//      keeps the mirror's tint); the weight starts at (1, 1, 1).
// (C8) CAMERA FORM.  For samples first_sample .. first_sample + n_samples - 1 ascending the chain record of each sample's camera ray
//      (sample_index = the sample's number, t_min = 0.00001), reduced by rt_guide.h's rule unchanged — word [15] of the guide is the hit count,
//      as there; the albedo sums are the per-sample chain albedos added in ascending order into +0.0; `links` (optional) is the per-pixel sum
//      of the links followed over all samples, uint32.
// With max_links = 0, (C6) and (C7) give the very words of rt_query_hits, rt_query_albedo, rt_query_camera_guide and rt_query_camera_albedo.
//
// Not done: chain records in reprojection (a mirror image moves as a virtual image, not as the surface), the Fresnel split as two weighted
// branches, refilling ended lanes with new items, f32, rt_render_multi, adaptive frames beyond what rt_denoise_frame already takes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define RT_CHAIN_FN __host__ __device__ inline
#else
#define RT_CHAIN_FN inline
#endif

namespace rt {

static const uint32_t CHAIN_MAX_LINKS = 64u;
static const uint32_t CHAIN_HIT_DOUBLES = 16u;                  // = QUERY_HIT_DOUBLES
static const uint32_t CHAIN_RAY_DOUBLES = 7u;                   // = QUERY_RAY_DOUBLES
static const uint32_t CHAIN_KIND_METAL = 1u, CHAIN_KIND_DIELECTRIC = 2u;    // = M_METAL, M_DIELECTRIC (rt_ir.h; rt_chain.hip asserts it)
enum ChainStatus : uint32_t { CHAIN_CONTINUE = 0, CHAIN_END_SURFACE = 1, CHAIN_END_MISS = 2, CHAIN_END_ABSORBED = 3, CHAIN_END_NONFINITE = 4, CHAIN_END_FUZZ = 5 };

RT_CHAIN_FN double chain_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RT_CHAIN_FN bool chain_finite(double v) { return v - v == 0.0; }
RT_CHAIN_FN double chain_length(const double* d) { return __builtin_sqrt(chain_dot(d, d)); }
// (C1): the seed of link l >= 1 of sample sample_index
RT_CHAIN_FN uint64_t chain_link_seed(uint64_t seed, uint32_t sample_index, uint32_t l) {
    return seed + (((uint64_t)sample_index << 8) | (uint64_t)l) * 0x9E3779B97F4A7C15ull;
}

// (C2)-(C4), the material's part: a record that hit a surface of material (kind, param = fuzz or index, albedo) with normal n and front face
// `front`, reached along direction d.  CHAIN_CONTINUE: new_d is the next ray's direction and weight has been multiplied (Metal).  Any other
// status: new_d and weight are untouched.
RT_CHAIN_FN uint32_t chain_step(const double* d, const double* n, bool front, uint32_t kind, double param, const double* albedo, double max_fuzz,
                                double* new_d, double* weight) {
    if (kind == CHAIN_KIND_METAL) {
        if (!(param <= max_fuzz)) return CHAIN_END_FUZZ;
        const double s = (-chain_dot(d, n)) * 2.0;
        const double dn[3] = {d[0] + s * n[0], d[1] + s * n[1], d[2] + s * n[2]};
        const double len = __builtin_sqrt(chain_dot(dn, dn));
        const double r[3] = {dn[0] / len, dn[1] / len, dn[2] / len};
        if (!(chain_finite(r[0]) && chain_finite(r[1]) && chain_finite(r[2]))) return CHAIN_END_NONFINITE;
        if (!(chain_dot(r, n) > 0.0)) return CHAIN_END_ABSORBED;
        new_d[0] = r[0]; new_d[1] = r[1]; new_d[2] = r[2];
        weight[0] = weight[0] * albedo[0]; weight[1] = weight[1] * albedo[1]; weight[2] = weight[2] * albedo[2];
        return CHAIN_CONTINUE;
    }
    if (kind == CHAIN_KIND_DIELECTRIC) {
        const double refraction_ratio = front ? 1.0 / param : param;
        const double dl = __builtin_sqrt(chain_dot(d, d));
        const double u[3] = {d[0] / dl, d[1] / dl, d[2] / dl};
        const double mu[3] = {-1.0 * u[0], -1.0 * u[1], -1.0 * u[2]};
        const double cos_theta = __builtin_fmin(chain_dot(mu, n), 1.0);
        const double sin_theta = __builtin_sqrt(1.0 - cos_theta * cos_theta);
        const bool cannot_refract = refraction_ratio * sin_theta > 1.0;
        const double q = (1.0 - refraction_ratio) / (1.0 + refraction_ratio);
        const double r0 = q * q;
        const double m1 = 1.0 - cos_theta, m2 = m1 * m1;
        const double refl = r0 + (1.0 - r0) * (m1 * (m2 * m2));
        const bool will_reflect = refl > 0.5;
        double r[3];
        if (cannot_refract || will_reflect) {
            const double s = (-chain_dot(u, n)) * 2.0;
            r[0] = u[0] + s * n[0]; r[1] = u[1] + s * n[1]; r[2] = u[2] + s * n[2];
        } else {
            const double perp[3] = {refraction_ratio * (u[0] + cos_theta * n[0]), refraction_ratio * (u[1] + cos_theta * n[1]), refraction_ratio * (u[2] + cos_theta * n[2])};
            const double len = __builtin_sqrt(chain_dot(perp, perp));
            const double p = -1.0 * __builtin_sqrt(__builtin_fabs(1.0 - len * len));
            r[0] = perp[0] + p * n[0]; r[1] = perp[1] + p * n[1]; r[2] = perp[2] + p * n[2];
        }
        if (!(chain_finite(r[0]) && chain_finite(r[1]) && chain_finite(r[2]))) return CHAIN_END_NONFINITE;
        new_d[0] = r[0]; new_d[1] = r[1]; new_d[2] = r[2];
        return CHAIN_CONTINUE;
    }
    return CHAIN_END_SURFACE;
}

// What the step reads of a material: the host library fills the table from the scene's own (kind without its flag bits)
struct ChainMaterial { uint32_t kind; double param; double albedo[3]; };

// What the entry points check before they touch an item: "" or the message.
std::string chain_check(uint32_t max_links, double max_fuzz, uint32_t flags);
// The link step on n (ray, record) pairs, rt_chain_step_host's body (arguments already checked but for the records' material words): rays
// [n][7], hits [n][16]; next_rays [n][7] — the ray of (C5) where status is 0, else the input ray unchanged; weight [n][3] — the factor this
// link multiplies the weight by: the Metal's albedo where status is 0 and the material is Metal, else (1, 1, 1); status [n].  "" or the message
// (a word [11] that names no material and is not a medium's -1); nothing is written then.
std::string chain_step_host(const ChainMaterial* materials, size_t n_materials, uint32_t n, const double* rays, const double* hits, double max_fuzz,
                            double* next_rays_out, double* weight_out, uint32_t* status_out);

} // namespace rt

// ---- the kernel (rt_chain.hip), for the translation units that see HIP (rt_chain.hip, rt_host.cpp)
#ifdef RT_CHAIN_QUERIES
#include "rt_query.h"
namespace rt {
// What a chain launch needs beside the scene's tables.  Caller-ray form (rays != nullptr): item k is ray k of rays[7 k ..]; hits[16 k ..] takes
// its chain record, albedo[3 k ..] (may be nullptr) its chain albedo; first_sample, n_samples and links are not read.  Camera form: item p is
// output-order pixel p; hits[16 p ..] takes the guide of (C8), albedo[3 p ..] (may be nullptr) the albedo sums, links[p] (may be nullptr) the sum
// of links followed.  rays and hits 16-byte aligned, albedo 8-byte, links 4-byte.
struct ChainArgs {
    const double* rays; double* hits; double* albedo; uint32_t* links;
    uint32_t n, first_sample, n_samples, max_links; double t_min, max_fuzz; uint64_t seed;
};
int chain_blocks_per_cu(uint32_t scene_feats, bool camera, bool albedo, size_t shmem);
hipError_t launch_chain(const KParams<double>& P, const ChainArgs& A, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream);
}
#endif

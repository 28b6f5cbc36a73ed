// csrc/rt_albedo.h — the first-hit albedo query and albedo-demodulated denoising: the two specifications, the host twin's seams
// (rt_albedo_cpu.cpp, plain C++) and the launches of the HIP kernels (rt_albedo.hip) as the host library (rt_host.cpp, rt_frames.cpp) sees them.  No HIP
// include unless RT_ALBEDO_QUERIES asks for the query kernels' interface at the end: for the element-wise kernels a stream travels as a
// void* and a HIP status as an int (0 = hipSuccess), as in rt_denoise.h, so that the host twin and its stand-alone sanitizer program
// compile with any C++ compiler.
//
// (1) ALBEDO of a ray: the closest hit is found exactly as rt_query_hits / rt_query_camera find it (the same search, the same stream, the
//     same finalized record).  Three doubles:
//         Lambertian                                  texture.mapping(u, v, p) of its texture (the frames' const_or_tex / tex_eval on the record)
//         PBR                                         mapping(u, v, p) of its base-colour texture
//         Isotropic (a ConstantMedium hit, handle -1) mapping(u, v, p) of the medium's texture
//         Metal                                       its albedo
//         Dielectric, DiffuseLight, miss              (1, 1, 1): radiance of emitters and of the background is not reflectance and stays
//                                                     un-demodulated
//     u, v are the record's — computed only where the material reads them, as in the frames.
//     Out of scope: following a specular chain (Metal, Dielectric) to the first diffuse surface behind it; the albedo is the first hit's.
//     The camera form sums the albedo of samples first_sample .. first_sample + n_samples - 1 of a pixel in ascending order into three f64
//     accumulators that start at +0.0: one pixel per lane, no atomics, so the same call gives the same words and a host can restate it.
//
// (2) DEMODULATED DENOISING.  Only + - * / and comparisons, every operation rounded once (-ffp-contract=off), in this order.  Per pixel and
//     channel, eps = 2^-8:
//         a = albedo_sum / albedo_samples
//         m = (a - a == 0) ? a : 1                  a non-finite albedo demodulates nothing
//         d = (m >= eps) ? m : eps
//         x = rgb_sum / d
//         y = rt_denoise(x, samples, hits, iterations, sigma, flags)      the filter of rt_denoise.h on the demodulated frame, unchanged
//         out = y * m
//     eps is one output code value of format_color per unit of irradiance.  A channel darker than that is divided by eps and multiplied
//     back by its true m: a black channel stays black and cannot be lit by its neighbours.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include "rt_denoise.h"

#if defined(__HIPCC__)
#define RT_ALBEDO_FN __host__ __device__ inline
#else
#define RT_ALBEDO_FN inline
#endif

namespace rt {

static const double ALBEDO_EPS = 0.00390625;                     // 2^-8
// the extra frame of a demodulated run: x, 3 doubles per pixel, behind the filter's own workspace
static const size_t DENOISE_ALBEDO_WORKSPACE_BYTES_PER_PX = DENOISE_WORKSPACE_BYTES_PER_PX + 3u * sizeof(double);

// steps 1-2 and 3-4 and 6 of (2), one channel: the arithmetic the kernels and the host twin share word for word
RT_ALBEDO_FN double albedo_modulation(double albedo_sum, double albedo_samples) {
    const double a = albedo_sum / albedo_samples;
    return (a - a == 0.0) ? a : 1.0;
}
RT_ALBEDO_FN double albedo_demodulate(double rgb_sum, double m) {
    const double d = (m >= ALBEDO_EPS) ? m : ALBEDO_EPS;
    return rgb_sum / d;
}
RT_ALBEDO_FN double albedo_remodulate(double y, double m) { return y * m; }

// What every demodulated entry point checks beside denoise_check: "" or the message
std::string denoise_albedo_check(uint64_t samples, uint64_t albedo_samples, uint32_t W, uint32_t H, uint32_t iterations, const double* sigma, uint32_t flags);
// The specification as code (arguments already checked).  rgb_sum_out may alias rgb_sum.
void denoise_albedo_host(const double* rgb_sum, uint64_t samples, const double* albedo_sum, uint64_t albedo_samples, const double* hits,
                         uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out);

// ---- the element-wise kernels (rt_albedo.hip).  DEVICE pointers, 8-byte aligned (16-byte accesses are used when all three are 16-byte
// aligned); n = the number of doubles (3 per pixel); asynchronous on `stream`; the return value is the hipError_t of the launch.
// x[i] = rgb_sum[i] / d(albedo_sum[i])
int launch_albedo_demodulate(const double* d_rgb_sum, const double* d_albedo_sum, uint64_t albedo_samples, double* d_x, uint64_t n, void* stream);
// io[i] = io[i] * m(albedo_sum[i])
int launch_albedo_remodulate(double* d_io, const double* d_albedo_sum, uint64_t albedo_samples, uint64_t n, void* stream);

} // namespace rt

// ---- the query kernels (rt_albedo.hip), for the translation units that ask for them (rt_albedo.hip, rt_host.cpp: they see HIP; the host
// twin and its sanitizer program do not)
#ifdef RT_ALBEDO_QUERIES
#include "rt_query.h"
namespace rt {
// What an albedo launch needs beside the scene's tables (as QueryArgs).  Caller rays (rays != nullptr): ray k comes from rays[7 k ..], draws
// from rng_for_stream(seed, k), its albedo goes to albedo[3 k ..] and — hits != nullptr — its record to hits[16 k ..], the words rt_query_hits
// writes.  Camera mode (rays == nullptr): albedo[3 p ..] = the ascending sum over samples first_sample .. first_sample + n_samples - 1 of
// output-order pixel p, each sample's ray and stream those of rt_query_camera.  rays and hits 16-byte aligned, albedo 8-byte.
struct AlbedoArgs { const double* rays; double* albedo; double* hits; uint32_t n, first_sample, n_samples; double t_min; uint64_t seed; };
int albedo_blocks_per_cu(uint32_t scene_feats, bool camera, size_t shmem);
hipError_t launch_albedo(const KParams<double>& P, const AlbedoArgs& A, uint32_t scene_feats, bool camera, uint32_t n_blocks, size_t shmem, hipStream_t stream);
}
#endif

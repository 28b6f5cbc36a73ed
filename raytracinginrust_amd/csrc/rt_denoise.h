// csrc/rt_denoise.h — the denoiser's seams: the host twin (rt_denoise_cpu.cpp, plain C++) and the launches of the HIP kernels
// (rt_denoise.hip) as the host library (rt_frames.cpp) sees them.  No HIP include: a stream travels as a void* and a HIP status as an int
// (0 = hipSuccess), so that the host twin and its stand-alone sanitizer program compile with any C++ compiler.
//
// The filter is the edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) over the f64 sum frame, guided by the hit
// records of rt_query_camera.  It is DEFINED by the arithmetic below — only + - * / and comparisons, every operation rounded once, in
// this order — and the HIP kernels, denoise_host and the NumPy restatement of tests/test_denoise_host.py give the same 64-bit words.
//
// Per pixel, once:  c = rgb_sum / samples (per channel);  n, x = the record's normal and position;  inv_t = 1.0 / t;
//                   key = hit ? (flags & RT_DENOISE_SAME_MATERIAL ? material + 2 : 1) : 0.
// On the host, once: ic = 1 / (sigma_c * sigma_c), in = 1 / (sigma_n * sigma_n), ip = 1 / (sigma_p * sigma_p).
// Iteration i = 0 .. K-1, step s = 2^i, ic_i = ic * 4^i, reads the previous iteration's c and writes a new frame:
//     acc = 0,0,0; wsum = 0;  c_p_finite = all three channels of c_p finite
//     for dy = -2..2, for dx = -2..2 (this order): q = (y + dy*s, x + dx*s); outside the frame: skip
//       key_q != key_p: skip;   c_q not finite in all three channels: skip
//       k  = h[dy+2]*h[dx+2],  h = (1/16, 1/4, 3/8, 1/4, 1/16)
//       e  = c_q - c_p;  d = (e0*e0 + e1*e1) + e2*e2;  t = 1 - d*ic_i;  wc = t > 0 ? t*t : 0;  if !c_p_finite: wc = 1
//       if key_p != 0:  m = n_q - n_p;  d = (m0*m0 + m1*m1) + m2*m2;  t = 1 - d*in;  wn = t > 0 ? t*t : 0
//                       r = x_q - x_p;  g = ((n_p0*r0 + n_p1*r1) + n_p2*r2) * inv_t_p;  t = 1 - (g*g)*ip;  wp = t > 0 ? t*t : 0
//       else wn = wp = 1
//       w = ((k*wc)*wn)*wp;   acc += w*c_q (per channel);   wsum += w
//     out = wsum > 0 ? acc / wsum : c_p
// The result is c_K * samples: sum units again, so rt_write_ppm, rt_format_color and the resolve kernel apply to it unchanged.
// Every comparison with a NaN is false: non-finite taps are left out, a non-finite centre takes its neighbours' values, 0 * inf ends as
// weight 0.  ("finite" is v - v == 0.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace rt {

static const uint32_t DENOISE_MAX_ITERATIONS = 8u;
static const uint32_t DENOISE_KNOWN_FLAGS = 1u;                  // RT_DENOISE_SAME_MATERIAL
static const uint32_t DENOISE_COLOR_DOUBLES = 4u;                // a packed mean: {r, g, b, 0}                 (32 bytes)
static const uint32_t DENOISE_GUIDE_DOUBLES = 8u;                // a packed guide: {n0, n1, n2, inv_t | x0, x1, x2, key}   (64 bytes)
static const uint32_t DENOISE_HIT_DOUBLES = 16u;                 // a record of rt_query_camera
// the workspace of one run: two packed colour frames (the iterations alternate between them) and the packed guide
static const size_t DENOISE_WORKSPACE_BYTES_PER_PX = (2u * DENOISE_COLOR_DOUBLES + DENOISE_GUIDE_DOUBLES) * sizeof(double);

// What every entry point checks before it touches a pixel: "" if the arguments are a filter, else the message.
std::string denoise_check(uint64_t samples, uint32_t W, uint32_t H, uint32_t iterations, const double* sigma, uint32_t flags);
// The three inverse squares the iterations use, from sigma (+inf gives 0: that stop is off)
void denoise_inverse_squares(const double sigma[3], double inv3[3]);
// The specification as code (arguments already checked).  rgb_sum_out may alias rgb_sum.
void denoise_host(const double* rgb_sum, uint64_t samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations,
                  const double sigma[3], uint32_t flags, double* rgb_sum_out);

// ---- the kernels (rt_denoise.hip).  DEVICE pointers; d_hits, d_color and d_guide 16-byte aligned; asynchronous on `stream`
// (a hipStream_t); the return value is the hipError_t of the launch.
// Pack: d_rgb_sum (24 B / pixel) -> d_color, when both are given; d_hits (128 B / pixel) -> d_guide, when both are given.
int launch_denoise_pack(const double* d_rgb_sum, uint64_t samples, const double* d_hits, uint32_t flags, double* d_color, double* d_guide,
                        uint32_t n_px, void* stream);
// One iteration with step `step` and colour stop ic_i, from d_color_in to d_color_out (packed, 32 B / pixel) — or, the last one, to
// d_rgb_sum_out (24 B / pixel, multiplied by samples) when that is given instead.
int launch_denoise_filter(const double* d_color_in, const double* d_guide, double* d_color_out, double* d_rgb_sum_out, uint32_t W, uint32_t H,
                          uint32_t step, double ic_i, double in, double ip, uint64_t samples, void* stream);

} // namespace rt

// csrc/rt_reproject.h — temporal accumulation: the history of a frame reprojected into a new view of the same scene, and the blend of a
// frame with such a history.  The specification, the host twin's seams (rt_reproject_cpu.cpp, plain C++) and the launches of the HIP kernels
// (rt_reproject.hip) as the host library (rt_frames.cpp) sees them.  No HIP include: a stream travels as a void* and a HIP status as an int
// (0 = hipSuccess), as in rt_denoise_frame.h.
//
// Only + - * /, floor, comparisons and integer conversion, every operation rounded once (-ffp-contract=off), in the order written.
// "finite" is v - v == 0; every comparison with a NaN is false; dot(a, b) = (a0*b0 + a1*b1) + a2*b2.  The HIP kernel, reproject_host and the
// NumPy restatement of tests/reproject_cases.py give the same 64-bit words.
//
// Inputs: prev_sum (W*H*3 doubles, output order) and prev_counts (W*H uint32, or null: prev_samples holds for every pixel) — the previous
// view's frame; prev_hits, cur_hits (W*H records of 16 doubles, rt_query_camera or rt_query_camera_guide) — the first-hit records of the
// previous and of the new view; prev_cam; max_history 0 .. 2^31 - 1; sigma = {normal_min in [0, 1], sigma_p > 0 (+inf: that stop is off)}.
//
// (R0) ONCE, on the host, from rt_camera_fields(prev_cam)'s o (origin), llc (lower left corner), h (horizontal), v (vertical):
//         F  = ((o - h/2) - v/2) - llc            focus_dist * w: from the focus plane's centre back to the lens centre
//         FF = dot(F, F);  hh = dot(h, h);  vv = dot(v, v);  Wm = (double)(W - 1);  Hm = (double)(H - 1)
// (R1) THE CENTRE, pixel p of the new view:  c = cur_hits[p].  No history if c[0] == 0 or !(c[12] >= 0) (the second: a pixel of an averaged
//      guide whose samples saw different objects).  P = c[2..4], n = c[5..7], key = c[12].
// (R2) PROJECTION through the previous camera's lens centre:
//         d = P - o;  den = 0.0 - dot(d, F);  no history if !(den > 0)               (the point lies in or behind the lens plane)
//         tau = FF / den;  q = d * tau                                                q ends on the focus plane
//         s = dot(q, h) / hh + 0.5;  t = dot(q, v) / vv + 0.5
//         x = s * Wm - 0.5;  y = t * Hm - 0.5                                         pixel centres sit at integers; y counts from the BOTTOM row
//         no history if !(x > -1 && x < W && y > -1 && y < H)                         (src/main.rs:817-818: u = (i + r) / (W - 1), j from the bottom)
// (R3) TAP SET-UP:
//         xf = floor(x);  yf = floor(y);  fx = x - xf;  fy = y - yf
//         dd = dot(d, d);  nn = dot(n, n);  lim = ((sigma_p * sigma_p) * dd) * nn;  nm = (normal_min * normal_min) * nn
// (R4) FOUR TAPS in the order (b, a) = (0,0), (0,1), (1,0), (1,1): column xf + a, OUTPUT row H - 1 - (yf + b), weight w = wx * wy with
//      wx = a ? fx : 1 - fx and wy = b ? fy : 1 - fy.  A tap is skipped when it lies outside the frame; when !(w > 0); when the previous
//      record g has g[0] == 0 or g[12] != key; when its count Nq (prev_counts[q], or prev_samples) is 0; when a channel of prev_sum[q] is not
//      finite; when, with m = g[5..7] and dn = dot(n, m), !(dn > 0 && dn*dn >= nm * dot(m, m)) (averaged guides carry short normals, so the
//      test has no square root); when, with e = P - g[2..4] and pe = dot(e, n), !(pe*pe <= lim) (the plane distance relative to the distance
//      from the previous camera: no scene scale).  A tap that passes adds, per channel,
//         acc += w * (prev_sum[q] / (double)Nq);      and once      wsum += w;  nacc += w * (double)Nq
//      into accumulators that start at +0.0.
// (R5) THE RESULT: no history if !(wsum > 0).  mean = acc / wsum;  N_h = (uint32) floor(min(nacc, (double)max_history));  no history if
//      N_h == 0;  hist_sum[p] = mean * (double)N_h,  hist_counts[p] = N_h.  "No history" writes +0.0 to the three sums and 0 to the count.
//      nacc is not divided by wsum: a footprint that is only partly valid carries less weight.
//
// (B) THE BLEND, element-wise:  sum_out = rgb_sum + hist_sum;  counts_out = min((uint64)N + hist_counts, 2^32 - 1) with N = counts ?
//     counts[p] : samples.  The result is a (sum, counts) frame in the adaptive frames' layout (rt_adaptive.h): rt_adaptive_resolve_rgb8_*
//     and rt_denoise_frame*(counts = ...) take it unchanged.
//
// Not done: adaptive frames inside rt_progressive_set_view, history for pixels that miss, a wider search when all four taps fail, moving
// objects, specular chains, f32.  (A variance frame travels through rt_reproject_var.h, which restates reproject_pixel's tap loop.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define RT_REPROJECT_FN __host__ __device__ inline
#else
#define RT_REPROJECT_FN inline
#endif

namespace rt {

static const uint32_t REPROJECT_HIT_DOUBLES = 16u;              // = QUERY_HIT_DOUBLES
static const uint32_t REPROJECT_MAX_HISTORY = 0x7FFFFFFFu;
static const uint32_t REPROJECT_THREADS = 256u;                  // one pixel (reproject) or one pair of doubles (blend) per lane, no loop

// (R0) and what else is the same for every pixel; passed to the kernel by value
struct ReprojectConsts {
    double o[3], F[3], h[3], v[3];
    double FF, hh, vv, Wm, Hm, Wd, Hd;
    double sp2, nm2, cap;                                         // sigma_p * sigma_p, normal_min * normal_min, (double)max_history
    double Ns;                                                    // (double)prev_samples, used where prev_counts is null
    uint32_t W, H;
};

RT_REPROJECT_FN double reproject_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RT_REPROJECT_FN bool reproject_finite(double v) { return v - v == 0.0; }

// fields: rt_camera_fields(prev_cam)'s 21 doubles
inline ReprojectConsts reproject_consts(const double* fields, uint64_t prev_samples, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2]) {
    ReprojectConsts K;
    const double* o = fields; const double* llc = fields + 3; const double* h = fields + 6; const double* v = fields + 9;
    for (int k = 0; k < 3; k++) {
        K.o[k] = o[k]; K.h[k] = h[k]; K.v[k] = v[k];
        K.F[k] = ((o[k] - h[k] / 2.0) - v[k] / 2.0) - llc[k];
    }
    K.FF = reproject_dot(K.F, K.F); K.hh = reproject_dot(K.h, K.h); K.vv = reproject_dot(K.v, K.v);
    K.Wm = (double)(W - 1u); K.Hm = (double)(H - 1u); K.Wd = (double)W; K.Hd = (double)H;
    K.sp2 = sigma[1] * sigma[1]; K.nm2 = sigma[0] * sigma[0]; K.cap = (double)max_history;
    K.Ns = (double)prev_samples;
    K.W = W; K.H = H;
    return K;
}

// (R1)-(R5) of output-order pixel p: the three sums into out3, the count returned.  The reads: the pixel's own record, and of each of up to
// four previous records words [0], [2..7] and [12], three sums and a count.  (Its twin: reproject_variance_pixel, rt_reproject_var.h.)
RT_REPROJECT_FN uint32_t reproject_pixel(const ReprojectConsts& K, const double* prev_sum, const uint32_t* prev_counts, const double* prev_hits,
                                         const double* cur_hits, uint64_t p, double* out3) {
    out3[0] = 0.0; out3[1] = 0.0; out3[2] = 0.0;
    const double* c = cur_hits + p * REPROJECT_HIT_DOUBLES;
    const double key = c[12];
    if (c[0] == 0.0 || !(key >= 0.0)) return 0u;
    const double P[3] = {c[2], c[3], c[4]}, n[3] = {c[5], c[6], c[7]};
    const double d[3] = {P[0] - K.o[0], P[1] - K.o[1], P[2] - K.o[2]};
    const double den = 0.0 - reproject_dot(d, K.F);
    if (!(den > 0.0)) return 0u;
    const double tau = K.FF / den;
    const double q[3] = {d[0] * tau, d[1] * tau, d[2] * tau};
    const double s = reproject_dot(q, K.h) / K.hh + 0.5, t = reproject_dot(q, K.v) / K.vv + 0.5;
    const double x = s * K.Wm - 0.5, y = t * K.Hm - 0.5;
    if (!(x > -1.0 && x < K.Wd && y > -1.0 && y < K.Hd)) return 0u;
    const double xf = __builtin_floor(x), yf = __builtin_floor(y);
    const double fx = x - xf, fy = y - yf;
    const double dd = reproject_dot(d, d), nn = reproject_dot(n, n);
    const double lim = ((K.sp2) * dd) * nn, nm = K.nm2 * nn;
    const int64_t xi = (int64_t)xf, yi = (int64_t)yf;             // -1 .. W - 1, -1 .. H - 1
    double acc[3] = {0.0, 0.0, 0.0}, wsum = 0.0, nacc = 0.0;
    for (int b = 0; b < 2; b++) for (int a = 0; a < 2; a++) {
        const int64_t col = xi + a, up = yi + b;
        if (col < 0 || col >= (int64_t)K.W || up < 0 || up >= (int64_t)K.H) continue;
        const double wx = a ? fx : 1.0 - fx, wy = b ? fy : 1.0 - fy;
        const double w = wx * wy;
        if (!(w > 0.0)) continue;
        const uint64_t qi = (uint64_t)((int64_t)K.H - 1 - up) * K.W + (uint64_t)col;
        const double* g = prev_hits + qi * REPROJECT_HIT_DOUBLES;
        if (g[0] == 0.0 || g[12] != key) continue;
        const double Nq = prev_counts ? (double)prev_counts[qi] : K.Ns;
        if (Nq == 0.0) continue;
        const double* S = prev_sum + qi * 3u;
        const double S0 = S[0], S1 = S[1], S2 = S[2];
        if (!(reproject_finite(S0) && reproject_finite(S1) && reproject_finite(S2))) continue;
        const double m[3] = {g[5], g[6], g[7]};
        const double dn = reproject_dot(n, m);
        if (!(dn > 0.0 && dn * dn >= nm * reproject_dot(m, m))) continue;
        const double e[3] = {P[0] - g[2], P[1] - g[3], P[2] - g[4]};
        const double pe = reproject_dot(e, n);
        if (!(pe * pe <= lim)) continue;
        acc[0] += w * (S0 / Nq); acc[1] += w * (S1 / Nq); acc[2] += w * (S2 / Nq);
        wsum += w;
        nacc += w * Nq;
    }
    if (!(wsum > 0.0)) return 0u;
    const uint32_t Nh = (uint32_t)__builtin_floor(nacc < K.cap ? nacc : K.cap);
    if (Nh == 0u) return 0u;
    const double Nd = (double)Nh;
    out3[0] = (acc[0] / wsum) * Nd; out3[1] = (acc[1] / wsum) * Nd; out3[2] = (acc[2] / wsum) * Nd;
    return Nh;
}

// (B), one count
RT_REPROJECT_FN uint32_t blend_count(uint64_t N, uint32_t hist) {
    const uint64_t t = (N > 0xFFFFFFFFull ? 0xFFFFFFFFull : N) + (uint64_t)hist;
    return (uint32_t)(t > 0xFFFFFFFFull ? 0xFFFFFFFFull : t);
}

// What the entry points check before they touch a pixel: "" or the message.
std::string reproject_frame_check(uint32_t W, uint32_t H);
std::string reproject_check(bool has_counts, uint64_t prev_samples, uint32_t W, uint32_t H, uint32_t max_history, const double* sigma, uint32_t flags);
// The specifications as code (arguments already checked).  The outputs may overlap no input of reproject_host; sum_out may be rgb_sum and
// counts_out may be counts in temporal_blend_host.
void reproject_host(const ReprojectConsts& K, const double* prev_sum, const uint32_t* prev_counts, const double* prev_hits, const double* cur_hits,
                    double* hist_sum_out, uint32_t* hist_counts_out);
void temporal_blend_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* hist_sum, const uint32_t* hist_counts, uint64_t n_px,
                         double* sum_out, uint32_t* counts_out);

// ---- the kernels (rt_reproject.hip).  DEVICE pointers: records 16-byte aligned, sums 8-byte, counts 4-byte; asynchronous on `stream`; the
// return value is the hipError_t of the launch.
int launch_reproject(const ReprojectConsts& K, const double* d_prev_sum, const uint32_t* d_prev_counts, const double* d_prev_hits, const double* d_cur_hits,
                     double* d_hist_sum_out, uint32_t* d_hist_counts_out, void* stream);
int launch_temporal_blend(const double* d_rgb_sum, const uint32_t* d_counts, uint64_t samples, const double* d_hist_sum, const uint32_t* d_hist_counts,
                          uint32_t n_px, double* d_sum_out, uint32_t* d_counts_out, void* stream);

} // namespace rt

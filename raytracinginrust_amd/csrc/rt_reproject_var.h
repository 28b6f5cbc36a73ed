// csrc/rt_reproject_var.h — temporal variance: the variance of a frame's per-pixel mean carried through a camera move beside the frame's
// history (rt_reproject.h), and the blend of a frame's variance with such a history's.  The specification, the host twin's seams
// (rt_reproject_var_cpu.cpp, plain C++) and the launches of the HIP kernels (rt_reproject_var.hip) as the host library (rt_frames.cpp) sees
// them.  No HIP include, as in rt_reproject.h, whose constants, dot and finite this header uses; nothing of rt_reproject.h changes.
//
// Only + - * /, floor, comparisons and integer conversion, every operation rounded once (-ffp-contract=off), in the order written.  The HIP
// kernels, the host twin and the NumPy restatement of tests/reproject_var_cases.py give the same 64-bit words.
//
// A variance v is KNOWN when v - v == 0 && v >= 0 (-0.0 is known).  Everything else — NaN, +-inf, negative — is UNKNOWN and is written as
// +inf: what rt_denoise_frame.h (E) writes for a pixel with fewer than two passes and what rt_denoise_var.h (B) reads as "no information".
// Every word (V) and (BV) write is known or +inf, never NaN: a product or sum of known terms that overflows gives +inf, and no quotient
// below has a zero or infinite divisor.
//
// (V) REPROJECTION WITH VARIANCE.  The inputs are rt_reproject's and prev_var: W*H*3 doubles, the variance of the previous frame's per-pixel
//     mean (rt_moments.h (4), rt_denoise_frame.h (E), or a previous (BV)).  (R1)-(R5) of rt_reproject.h run unchanged — the same taps in the
//     same order — and hist_sum and hist_counts are rt_reproject's word for word.  In addition a tap that passes (R4) is VAR-KNOWN when all
//     three channels of prev_var[q] are known; such a tap adds, per channel,
//         vacc += w * (prev_var[q] * Nq);      and once      wv += w
//     into accumulators that start at +0.0.  prev_var[q] * Nq is the PER-SAMPLE variance at the tap: a property of the surface point, so the
//     quantity that may be interpolated (the variance of a mean is not: it depends on how long the tap was looked at).
//     THE RESULT, per channel: a pixel with history (N_h > 0) and wv > 0 gets  hist_var = (vacc / wv) / (double)N_h;  a pixel with history
//     but !(wv > 0) gets +inf;  "no history" writes +0.0, as it does to the sums.
//     In words: the history is N_h samples whose per-sample variance is the var-known taps' weighted mean.  max_history caps what the past
//     is worth, so a capped history claims a larger variance.  The averaging over the bilinear footprint is deliberately NOT credited (no sum
//     of w^2): neighbouring output pixels share taps, so their histories are correlated, and the filter's stop (rt_denoise_var.h) assumes
//     independent pixels — a variance reduced by the footprint would make it stop at differences that are noise.
//
// (BV) THE BLEND OF VARIANCES, per pixel p and channel k.  N = counts ? counts[p] : samples;  h = hist_counts[p];  Nd, hd: N and h converted
//     to double once;  T = Nd + hd (not saturated);  V = var ? var[p][k] : +inf;  Vh = hist_var[p][k].
//         h == 0                 (N > 0 && known(V)) ? V : +inf              (V's own bits)
//         N == 0                 known(Vh) ? Vh : +inf                       (Vh's own bits)
//         V and Vh known         ((Nd*Nd)*V + (hd*hd)*Vh) / (T*T)            the variance of the count-weighted mean of two independent means
//         only Vh known          (Vh*hd) / T                                 the new samples borrow the history's per-sample variance Vh*h:
//                                                                            the resolve one pass after a move
//         only V known           (V*Nd) / T                                  the history borrows the frame's
//         neither                +inf
//     var_out may be var.  The result is what rt_denoise_frame*(counts = rt_reproject.h (B)'s counts, var = ...) takes unchanged.
//
// Not done: adaptive frames inside rt_progressive_set_view, history for pixels that miss, a wider search when all four taps fail, moving
// objects, specular chains, f32, history in checkpoints.
#pragma once
#include "rt_reproject.h"

namespace rt {

RT_REPROJECT_FN bool variance_known(double v) { return v - v == 0.0 && v >= 0.0; }
RT_REPROJECT_FN double variance_unknown() { return __builtin_huge_val(); }

// (V) of output-order pixel p: the three sums into out3, the three variances into var3, the count returned.
// THE TAP LOOP IS reproject_pixel's (rt_reproject.h), restated so that rt_reproject.o stays what it is: a change to (R1)-(R5) is made in both.
RT_REPROJECT_FN uint32_t reproject_variance_pixel(const ReprojectConsts& K, const double* prev_sum, const uint32_t* prev_counts, const double* prev_var,
                                                  const double* prev_hits, const double* cur_hits, uint64_t p, double* out3, double* var3) {
    out3[0] = 0.0; out3[1] = 0.0; out3[2] = 0.0;
    var3[0] = 0.0; var3[1] = 0.0; var3[2] = 0.0;
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
    double vacc[3] = {0.0, 0.0, 0.0}, wv = 0.0;
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
        const double* V = prev_var + qi * 3u;
        const double V0 = V[0], V1 = V[1], V2 = V[2];
        if (!(variance_known(V0) && variance_known(V1) && variance_known(V2))) continue;
        vacc[0] += w * (V0 * Nq); vacc[1] += w * (V1 * Nq); vacc[2] += w * (V2 * Nq);
        wv += w;
    }
    if (!(wsum > 0.0)) return 0u;
    const uint32_t Nh = (uint32_t)__builtin_floor(nacc < K.cap ? nacc : K.cap);
    if (Nh == 0u) return 0u;
    const double Nd = (double)Nh;
    out3[0] = (acc[0] / wsum) * Nd; out3[1] = (acc[1] / wsum) * Nd; out3[2] = (acc[2] / wsum) * Nd;
    if (wv > 0.0) { var3[0] = (vacc[0] / wv) / Nd; var3[1] = (vacc[1] / wv) / Nd; var3[2] = (vacc[2] / wv) / Nd; }
    else { var3[0] = variance_unknown(); var3[1] = variance_unknown(); var3[2] = variance_unknown(); }
    return Nh;
}

// (BV), one channel of one pixel; V is +inf where there is no variance frame
RT_REPROJECT_FN double blend_variance(uint64_t N, uint32_t h, double V, double Vh) {
    if (h == 0u) return (N > 0u && variance_known(V)) ? V : variance_unknown();
    if (N == 0u) return variance_known(Vh) ? Vh : variance_unknown();
    const double Nd = (double)N, hd = (double)h;
    const double T = Nd + hd;
    const bool kv = variance_known(V), kh = variance_known(Vh);
    if (kv && kh) return ((Nd * Nd) * V + (hd * hd) * Vh) / (T * T);
    if (kh) return (Vh * hd) / T;
    if (kv) return (V * Nd) / T;
    return variance_unknown();
}

// What rt_temporal_blend_variance_* check before they touch a pixel: "" or the message.
std::string blend_variance_check(uint64_t n_px);
// The specifications as code (arguments already checked).  The outputs may overlap no input of reproject_variance_host; var_out may be var in
// temporal_blend_variance_host.
void reproject_variance_host(const ReprojectConsts& K, const double* prev_sum, const uint32_t* prev_counts, const double* prev_var, const double* prev_hits,
                             const double* cur_hits, double* hist_sum_out, uint32_t* hist_counts_out, double* hist_var_out);
void temporal_blend_variance_host(const double* var, const uint32_t* counts, uint64_t samples, const double* hist_var, const uint32_t* hist_counts, uint64_t n_px,
                                  double* var_out);

// ---- the kernels (rt_reproject_var.hip).  DEVICE pointers: records 16-byte aligned, sums and variances 8-byte, counts 4-byte; asynchronous on
// `stream`; the return value is the hipError_t of the launch.
int launch_reproject_variance(const ReprojectConsts& K, const double* d_prev_sum, const uint32_t* d_prev_counts, const double* d_prev_var, const double* d_prev_hits,
                              const double* d_cur_hits, double* d_hist_sum_out, uint32_t* d_hist_counts_out, double* d_hist_var_out, void* stream);
int launch_temporal_blend_variance(const double* d_var, const uint32_t* d_counts, uint64_t samples, const double* d_hist_var, const uint32_t* d_hist_counts,
                                   uint32_t n_px, double* d_var_out, void* stream);

} // namespace rt

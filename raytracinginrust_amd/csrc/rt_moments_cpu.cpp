// csrc/rt_moments_cpu.cpp — the host twin of the moments of a progressive frame: the specification of rt_moments.h as plain C++ (no HIP, no
// device), the argument checks every entry point shares, and rt_moments_merge_host / rt_moments_error_host / rt_moments_variance_host / rt_moments_stats_host of
// include/rt_amd.h.  Built with -ffp-contract=off like the rest of the library: every operation rounds once, which is what makes its words
// the ones the HIP kernels (rt_moments.hip) produce.
#include <cstring>
#include "../../include/rt_amd.h"
#include "rt_moments.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string moments_merge_check(uint64_t n_samples) {
    if (n_samples == 0u) return "moments: n_samples must be >= 1 (a pass's square is divided by its sample count)";
    return "";
}
std::string moments_error_check(uint64_t samples, uint64_t passes, uint32_t W, uint32_t H) {
    if (passes < 2u) return "moments: passes must be >= 2 (the error is estimated from the spread between passes)";
    if (samples == 0u) return "moments: samples must be >= 1";
    if (W == 0u || H == 0u) return "moments: W and H must be >= 1";
    if ((uint64_t)W * H > 0x7FFFFFFFull) return "moments: frame too large: W*H must be <= 2^31 - 1";
    return "";
}
std::string moments_tau_check(double tau) {
    if (!(tau >= 0.0)) return "moments: tau must be >= 0 (a standard error in display units; 1/256 is one code value)";
    return "";
}

void moments_merge_host(const double* pass_sum, uint64_t n_samples, double* rgb_sum, double* sq_sum, uint64_t n_doubles) {
    const double nb = (double)n_samples;
    for (uint64_t i = 0; i < n_doubles; i++) moments_merge(pass_sum[i], nb, rgb_sum[i], sq_sum[i]);
}
void moments_error_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint64_t n_px, double* e2_out) {
    const double Nd = (double)samples, Bm1 = (double)(passes - 1u);
    for (uint64_t p = 0; p < n_px; p++) e2_out[p] = moments_pixel_e2(rgb_sum + 3u * p, sq_sum + 3u * p, Nd, Bm1);
}
void moments_variance_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint64_t n_doubles, double* var_out) {
    const double Nd = (double)samples, Bm1 = (double)(passes - 1u);
    for (uint64_t i = 0; i < n_doubles; i++) var_out[i] = moments_channel_variance(rgb_sum[i], sq_sum[i], Nd, Bm1);
}
void moments_stats_host(const double* e2, uint64_t n_px, double tau, uint64_t stats_out[4]) {
    const double tau2 = tau * tau;
    uint64_t conv = 0, unconv = 0, nonfinite = 0;
    double mx = 0.0;
    for (uint64_t p = 0; p < n_px; p++) {
        const double e = e2[p];
        if (!moments_finite(e)) { nonfinite++; continue; }
        if (e <= tau2) conv++; else unconv++;
        if (e > mx) mx = e;
    }
    stats_out[MOMENTS_CONVERGED] = conv; stats_out[MOMENTS_UNCONVERGED] = unconv; stats_out[MOMENTS_NONFINITE] = nonfinite;
    std::memcpy(&stats_out[MOMENTS_MAX_E2], &mx, sizeof(mx));
}

} // namespace rt

extern "C" {

int rt_moments_merge_host(const double* pass_sum, uint64_t n_samples, double* rgb_sum, double* sq_sum, uint64_t n_doubles) {
    if (!pass_sum || !rgb_sum || !sq_sum) return rt::set_error("null argument");
    const std::string problem = rt::moments_merge_check(n_samples);
    if (!problem.empty()) return rt::set_error(problem);
    rt::moments_merge_host(pass_sum, n_samples, rgb_sum, sq_sum, n_doubles);
    return 0;
}
int rt_moments_error_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H, double* e2_out) {
    if (!rgb_sum || !sq_sum || !e2_out) return rt::set_error("null argument");
    const std::string problem = rt::moments_error_check(samples, passes, W, H);
    if (!problem.empty()) return rt::set_error(problem);
    rt::moments_error_host(rgb_sum, sq_sum, samples, passes, (uint64_t)W * H, e2_out);
    return 0;
}
int rt_moments_variance_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H, double* var_out) {
    if (!rgb_sum || !sq_sum || !var_out) return rt::set_error("null argument");
    const std::string problem = rt::moments_error_check(samples, passes, W, H);
    if (!problem.empty()) return rt::set_error(problem);
    rt::moments_variance_host(rgb_sum, sq_sum, samples, passes, (uint64_t)W * H * 3u, var_out);
    return 0;
}
int rt_moments_stats_host(const double* e2, uint64_t n_px, double tau, uint64_t stats_out[4]) {
    if (!e2 || !stats_out) return rt::set_error("null argument");
    const std::string problem = rt::moments_tau_check(tau);
    if (!problem.empty()) return rt::set_error(problem);
    rt::moments_stats_host(e2, n_px, tau, stats_out);
    return 0;
}

} // extern "C"

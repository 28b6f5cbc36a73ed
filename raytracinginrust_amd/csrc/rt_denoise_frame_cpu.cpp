// csrc/rt_denoise_frame_cpu.cpp — the host twin of rt_denoise_frame.h: the two specifications as plain C++ (no HIP, no device) around
// denoise_host (rt_denoise_cpu.cpp) and denoise_variance_host (rt_denoise_var_cpu.cpp), the argument check every entry point shares, and
// rt_adaptive_variance_host / rt_denoise_frame_host of include/rt_amd.h.  Built with -ffp-contract=off like the rest of the library: every
// operation rounds once, which is what makes its words the ones the HIP kernels (rt_denoise_frame.hip around the filters' own) produce.
#include <vector>
#include "../../include/rt_amd.h"
#include "rt_denoise_frame.h"
#include "rt_adaptive.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string denoise_frame_check(bool has_counts, uint64_t samples, bool has_var, bool has_albedo, uint64_t albedo_samples, uint32_t W, uint32_t H,
                                uint32_t iterations, const double* sigma, uint32_t flags, bool wants_var_out) {
    const uint64_t n = has_counts ? 1u : samples;                 // counts given: samples is ignored
    const std::string problem = has_var ? denoise_variance_check(n, W, H, iterations, sigma, flags) : denoise_check(n, W, H, iterations, sigma, flags);
    if (!problem.empty()) return problem;
    if (has_albedo && albedo_samples == 0u) return "denoise: albedo_samples must be >= 1 (the frame is demodulated by albedo_sum / albedo_samples)";
    if (wants_var_out && !has_var) return "denoise: var_out needs var (the filtered variance exists only under the variance stop)";
    return "";
}

void adaptive_variance_host(const double* S, const double* Q, const uint32_t* n, const uint32_t* b, uint64_t n_px, double* var_out) {
    for (uint64_t p = 0; p < n_px; p++)
        for (uint32_t k = 0; k < 3u; k++) var_out[3u * p + k] = frame_channel_variance(S[3u * p + k], Q[3u * p + k], n[p], b[p]);
}

void denoise_frame_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* var, const double* albedo_sum, uint64_t albedo_samples,
                        const double* hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out,
                        double* var_out) {
    const size_t n_px = (size_t)W * H, n = n_px * 3u;
    const double Ns = (double)samples, na = (double)albedo_samples;
    std::vector<double> m(n), c(n), vd;
    for (size_t i = 0; i < n; i++) {
        const double N = counts ? (double)counts[i / 3u] : Ns;
        m[i] = frame_modulation(albedo_sum != nullptr, albedo_sum ? albedo_sum[i] : 0.0, na);
        c[i] = frame_mean(rgb_sum[i], m[i], N);
    }
    if (var && albedo_sum) {
        vd.resize(n);
        for (size_t i = 0; i < n; i++) vd[i] = frame_variance(var[i], m[i]);
    }
    if (var) denoise_variance_host(c.data(), 1u, vd.empty() ? var : vd.data(), hits, W, H, iterations, sigma, flags, c.data(), var_out);
    else denoise_host(c.data(), 1u, hits, W, H, iterations, sigma, flags, c.data());
    for (size_t i = 0; i < n; i++) {
        const double N = counts ? (double)counts[i / 3u] : Ns;
        rgb_sum_out[i] = frame_sum(c[i], m[i], N);
    }
}

} // namespace rt

extern "C" {

int rt_adaptive_variance_host(const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes, uint32_t W, uint32_t H, double* var_out) {
    if (!rgb_sum || !sq_sum || !counts || !passes || !var_out) return rt::set_error("null argument");
    const std::string problem = rt::adaptive_frame_check(W, H);
    if (!problem.empty()) return rt::set_error(problem);
    rt::adaptive_variance_host(rgb_sum, sq_sum, counts, passes, (uint64_t)W * H, var_out);
    return 0;
}

int rt_denoise_frame_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* var, const double* albedo_sum, uint64_t albedo_samples,
                          const double* hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out,
                          double* var_out) {
    if (!rgb_sum || !hits || !sigma || !rgb_sum_out) return rt::set_error("null argument");
    const std::string problem = rt::denoise_frame_check(counts != nullptr, samples, var != nullptr, albedo_sum != nullptr, albedo_samples, W, H, iterations, sigma,
                                                        flags, var_out != nullptr);
    if (!problem.empty()) return rt::set_error(problem);
    rt::denoise_frame_host(rgb_sum, counts, samples, var, albedo_sum, albedo_samples, hits, W, H, iterations, sigma, flags, rgb_sum_out, var_out);
    return 0;
}

} // extern "C"

// csrc/rt_albedo_cpu.cpp — albedo-demodulated denoising's host twin: specification (2) of rt_albedo.h as plain C++ (no HIP, no device)
// around denoise_host (rt_denoise_cpu.cpp), the extra argument checks every demodulated entry point shares, and rt_denoise_albedo_host of
// include/rt_amd.h.  Built with -ffp-contract=off like the rest of the library: every / and * below rounds once, which is what makes its
// words the ones the HIP kernels (rt_albedo.hip around rt_denoise.hip) produce.
#include <vector>
#include "../../include/rt_amd.h"
#include "rt_albedo.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string denoise_albedo_check(uint64_t samples, uint64_t albedo_samples, uint32_t W, uint32_t H, uint32_t iterations, const double* sigma, uint32_t flags) {
    const std::string problem = denoise_check(samples, W, H, iterations, sigma, flags);
    if (!problem.empty()) return problem;
    if (albedo_samples == 0u) return "denoise: albedo_samples must be >= 1 (the frame is demodulated by albedo_sum / albedo_samples)";
    return "";
}

void denoise_albedo_host(const double* rgb_sum, uint64_t samples, const double* albedo_sum, uint64_t albedo_samples, const double* hits,
                         uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out) {
    const size_t n = (size_t)W * H * 3u;
    const double n_albedo = (double)albedo_samples;
    std::vector<double> m(n), x(n);
    for (size_t i = 0; i < n; i++) {
        m[i] = albedo_modulation(albedo_sum[i], n_albedo);
        x[i] = albedo_demodulate(rgb_sum[i], m[i]);
    }
    denoise_host(x.data(), samples, hits, W, H, iterations, sigma, flags, x.data());
    for (size_t i = 0; i < n; i++) rgb_sum_out[i] = albedo_remodulate(x[i], m[i]);
}

} // namespace rt

extern "C" int rt_denoise_albedo_host(const double* rgb_sum, uint64_t samples, const double* albedo_sum, uint64_t albedo_samples, const double* hits,
                                      uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out) {
    if (!rgb_sum || !albedo_sum || !hits || !sigma || !rgb_sum_out) return rt::set_error("null argument");
    const std::string problem = rt::denoise_albedo_check(samples, albedo_samples, W, H, iterations, sigma, flags);
    if (!problem.empty()) return rt::set_error(problem);
    rt::denoise_albedo_host(rgb_sum, samples, albedo_sum, albedo_samples, hits, W, H, iterations, sigma, flags, rgb_sum_out);
    return 0;
}

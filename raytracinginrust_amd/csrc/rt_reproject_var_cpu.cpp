// csrc/rt_reproject_var_cpu.cpp — temporal variance on the host: rt_reproject_var.h's specification as code, plain C++ (no HIP include; it is
// also compiled stand-alone under sanitizers by tests/test_reproject_var_host.py, together with rt_reproject_cpu.cpp whose argument checks
// it uses), and rt_reproject_variance_host / rt_temporal_blend_variance_host of include/rt_amd.h.  Built with -ffp-contract=off like the
// rest of the library: every operation rounds once, which is what makes its words the ones the HIP kernels (rt_reproject_var.hip) produce.
#include <string>
#include "../../include/rt_amd.h"
#include "rt_reproject_var.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string blend_variance_check(uint64_t n_px) {
    if (n_px > 0x7FFFFFFFull) return "reproject: frame too large: n_px must be <= 2^31 - 1";
    return "";
}

void reproject_variance_host(const ReprojectConsts& K, const double* prev_sum, const uint32_t* prev_counts, const double* prev_var, const double* prev_hits,
                             const double* cur_hits, double* hist_sum_out, uint32_t* hist_counts_out, double* hist_var_out) {
    const uint64_t n_px = (uint64_t)K.W * K.H;
    for (uint64_t p = 0; p < n_px; p++)
        hist_counts_out[p] = reproject_variance_pixel(K, prev_sum, prev_counts, prev_var, prev_hits, cur_hits, p, hist_sum_out + 3u * p, hist_var_out + 3u * p);
}

void temporal_blend_variance_host(const double* var, const uint32_t* counts, uint64_t samples, const double* hist_var, const uint32_t* hist_counts, uint64_t n_px,
                                  double* var_out) {
    for (uint64_t p = 0; p < n_px; p++) {
        const uint64_t N = counts ? (uint64_t)counts[p] : samples;
        for (uint64_t k = 0; k < 3u; k++) {
            const uint64_t i = 3u * p + k;
            var_out[i] = blend_variance(N, hist_counts[p], var ? var[i] : variance_unknown(), hist_var[i]);
        }
    }
}

} // namespace rt

extern "C" int rt_reproject_variance_host(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_var, const double* prev_hits,
                                          const rt_camera* prev_cam, const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2],
                                          uint32_t flags, double* hist_sum_out, uint32_t* hist_counts_out, double* hist_var_out) {
    if (!prev_sum || !prev_var || !prev_hits || !prev_cam || !cur_hits || !sigma || !hist_sum_out || !hist_counts_out || !hist_var_out) return rt::set_error("null argument");
    const std::string problem = rt::reproject_check(prev_counts != nullptr, prev_samples, W, H, max_history, sigma, flags);
    if (!problem.empty()) return rt::set_error(problem);
    double fields[21];
    rt_camera_fields(prev_cam, fields);
    rt::reproject_variance_host(rt::reproject_consts(fields, prev_samples, W, H, max_history, sigma), prev_sum, prev_counts, prev_var, prev_hits, cur_hits, hist_sum_out,
                                hist_counts_out, hist_var_out);
    return 0;
}

extern "C" int rt_temporal_blend_variance_host(const double* var, const uint32_t* counts, uint64_t samples, const double* hist_var, const uint32_t* hist_counts,
                                               uint64_t n_px, double* var_out) {
    if (!hist_var || !hist_counts || !var_out) return rt::set_error("null argument");
    const std::string problem = rt::blend_variance_check(n_px);
    if (!problem.empty()) return rt::set_error(problem);
    rt::temporal_blend_variance_host(var, counts, samples, hist_var, hist_counts, n_px, var_out);
    return 0;
}

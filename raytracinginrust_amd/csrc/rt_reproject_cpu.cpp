// csrc/rt_reproject_cpu.cpp — temporal accumulation on the host: rt_reproject.h's specification as code, plain C++ (no HIP include; it is
// also compiled stand-alone under sanitizers by tests/test_reproject_host.py), the argument checks every entry point shares, and
// rt_reproject_host / rt_temporal_blend_host of include/rt_amd.h.  Built with -ffp-contract=off like the rest of the library: every operation
// rounds once, which is what makes its words the ones the HIP kernels (rt_reproject.hip) produce.
#include <string>
#include "../../include/rt_amd.h"
#include "rt_reproject.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string reproject_frame_check(uint32_t W, uint32_t H) {
    if (W < 2u || H < 2u) return "reproject: W and H must be >= 2 (a pixel's place in the view is i / (W - 1), j / (H - 1))";
    if ((uint64_t)W * H > 0x7FFFFFFFull) return "reproject: frame too large: W*H must be <= 2^31 - 1";
    return "";
}
std::string reproject_check(bool has_counts, uint64_t prev_samples, uint32_t W, uint32_t H, uint32_t max_history, const double* sigma, uint32_t flags) {
    const std::string frame = reproject_frame_check(W, H);
    if (!frame.empty()) return frame;
    if (max_history > REPROJECT_MAX_HISTORY) return "reproject: max_history must be <= 2^31 - 1";
    if (!(sigma[0] >= 0.0 && sigma[0] <= 1.0)) return "reproject: normal_min (sigma[0]) must be in [0, 1]";
    if (!(sigma[1] > 0.0)) return "reproject: sigma_p (sigma[1]) must be > 0 (+inf switches the plane stop off)";
    if (flags != 0u) return "reproject: flags must be 0";
    if (!has_counts && prev_samples == 0u) return "reproject: prev_samples must be >= 1 when prev_counts is NULL (a mean divides by the count)";
    return "";
}

void reproject_host(const ReprojectConsts& K, const double* prev_sum, const uint32_t* prev_counts, const double* prev_hits, const double* cur_hits,
                    double* hist_sum_out, uint32_t* hist_counts_out) {
    const uint64_t n_px = (uint64_t)K.W * K.H;
    for (uint64_t p = 0; p < n_px; p++) hist_counts_out[p] = reproject_pixel(K, prev_sum, prev_counts, prev_hits, cur_hits, p, hist_sum_out + 3u * p);
}

void temporal_blend_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* hist_sum, const uint32_t* hist_counts, uint64_t n_px,
                         double* sum_out, uint32_t* counts_out) {
    for (uint64_t i = 0; i < 3u * n_px; i++) sum_out[i] = rgb_sum[i] + hist_sum[i];
    for (uint64_t p = 0; p < n_px; p++) counts_out[p] = blend_count(counts ? (uint64_t)counts[p] : samples, hist_counts[p]);
}

} // namespace rt

extern "C" int rt_reproject_host(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_hits, const rt_camera* prev_cam,
                                 const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2], uint32_t flags,
                                 double* hist_sum_out, uint32_t* hist_counts_out) {
    if (!prev_sum || !prev_hits || !prev_cam || !cur_hits || !sigma || !hist_sum_out || !hist_counts_out) return rt::set_error("null argument");
    const std::string problem = rt::reproject_check(prev_counts != nullptr, prev_samples, W, H, max_history, sigma, flags);
    if (!problem.empty()) return rt::set_error(problem);
    double fields[21];
    rt_camera_fields(prev_cam, fields);
    rt::reproject_host(rt::reproject_consts(fields, prev_samples, W, H, max_history, sigma), prev_sum, prev_counts, prev_hits, cur_hits, hist_sum_out, hist_counts_out);
    return 0;
}

extern "C" int rt_temporal_blend_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* hist_sum, const uint32_t* hist_counts,
                                      uint32_t W, uint32_t H, double* sum_out, uint32_t* counts_out) {
    if (!rgb_sum || !hist_sum || !hist_counts || !sum_out || !counts_out) return rt::set_error("null argument");
    const std::string problem = rt::reproject_frame_check(W, H);
    if (!problem.empty()) return rt::set_error(problem);
    rt::temporal_blend_host(rgb_sum, counts, samples, hist_sum, hist_counts, (uint64_t)W * H, sum_out, counts_out);
    return 0;
}

// csrc/rt_adaptive_cpu.cpp — the host twin of adaptive progressive frames: the specification of rt_adaptive.h as plain C++ (no HIP, no
// device), the argument checks every entry point shares, and rt_adaptive_*_host of include/rt_amd.h.  Built with -ffp-contract=off like
// the rest of the library: every operation rounds once, which is what makes its words the ones the HIP kernels (rt_adaptive.hip) produce.
#include <cstring>
#include <vector>
#include "../../include/rt_amd.h"
#include "rt_adaptive.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string adaptive_frame_check(uint32_t W, uint32_t H) {
    if (W == 0u || H == 0u) return "adaptive: W and H must be >= 1";
    if ((uint64_t)W * H > 0x7FFFFFFFull) return "adaptive: frame too large: W*H must be <= 2^31 - 1";
    return "";
}
std::string adaptive_select_check(uint32_t W, uint32_t H, uint32_t n_b, double tau, uint64_t max_samples, uint32_t spread) {
    const std::string frame = adaptive_frame_check(W, H);
    if (!frame.empty()) return frame;
    if (n_b == 0u) return "adaptive: n_samples must be >= 1";
    if (!(tau >= 0.0)) return "adaptive: tau must be >= 0 (a standard error in display units; 1/256 is one code value)";
    if (max_samples > ADAPTIVE_MAX_SAMPLES) return "adaptive: max_samples must be <= 2^32 - 1 (the sample field of a path's RNG key is 32 bits, csrc/rt_rng.h)";
    if (spread > 1u) return "adaptive: spread must be 0 or 1";
    return "";
}

void adaptive_error_host(const double* S, const double* Q, const uint32_t* n, const uint32_t* b, uint64_t n_px, double* e2_out) {
    for (uint64_t p = 0; p < n_px; p++) e2_out[p] = adaptive_pixel_e2(S + 3u * p, Q + 3u * p, n[p], b[p]);
}
uint32_t adaptive_select_host(const double* S, const double* Q, const uint32_t* n, const uint32_t* b, uint32_t W, uint32_t H, uint32_t n_b, double tau,
                              uint64_t max_samples, uint32_t spread, uint32_t* list_out) {
    const double tau2 = tau * tau;
    const uint64_t n_px = (uint64_t)W * H;
    std::vector<uint8_t> need(n_px);
    for (uint64_t p = 0; p < n_px; p++) need[p] = adaptive_need(adaptive_pixel_e2(S + 3u * p, Q + 3u * p, n[p], b[p]), b[p], tau2) ? 1u : 0u;
    uint32_t count = 0;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const uint64_t p = (uint64_t)y * W + x;
            bool needed = need[p] != 0u;
            if (!needed && spread) {
                const uint32_t y0 = y ? y - 1u : 0u, y1 = y + 1u < H ? y + 1u : y, x0 = x ? x - 1u : 0u, x1 = x + 1u < W ? x + 1u : x;
                for (uint32_t yy = y0; yy <= y1; yy++)
                    for (uint32_t xx = x0; xx <= x1; xx++) needed = needed || need[(uint64_t)yy * W + xx] != 0u;
            }
            if (needed && adaptive_room(n[p], n_b, max_samples)) list_out[count++] = (uint32_t)p;
        }
    return count;
}
void adaptive_merge_host(double* pass, uint32_t n_b, double* S, double* Q, uint32_t* n, uint32_t* b, const uint32_t* list, uint32_t n_list) {
    const double nb = (double)n_b;
    for (uint32_t k = 0; k < n_list; k++) {
        const uint64_t p = list[k];
        for (uint32_t c = 0; c < 3u; c++) { moments_merge(pass[3u * p + c], nb, S[3u * p + c], Q[3u * p + c]); pass[3u * p + c] = 0.0; }
        n[p] += n_b; b[p] += 1u;
    }
}
uint64_t adaptive_resolve_host(const double* S, const uint32_t* n, const uint8_t* rgb8_prev, uint8_t* rgb8_out, uint64_t n_px) {
    uint64_t changed = 0;
    for (uint64_t p = 0; p < n_px; p++) {
        bool differs = rgb8_prev == nullptr;
        for (uint32_t c = 0; c < 3u; c++) {
            const uint8_t v = (uint8_t)adaptive_format_channel(S[3u * p + c], n[p]);
            if (rgb8_prev && rgb8_prev[3u * p + c] != v) differs = true;
            rgb8_out[3u * p + c] = v;
        }
        changed += differs ? 1u : 0u;
    }
    return changed;
}

} // namespace rt

extern "C" {

int rt_adaptive_error_host(const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes, uint32_t W, uint32_t H,
                           double* e2_out, double tau, uint64_t stats_out[4]) {
    if (!rgb_sum || !sq_sum || !counts || !passes) return rt::set_error("null argument");
    std::string problem = rt::adaptive_frame_check(W, H);
    if (problem.empty() && stats_out) problem = rt::moments_tau_check(tau);
    if (!problem.empty()) return rt::set_error(problem);
    if (!e2_out && !stats_out) return 0;
    const uint64_t n_px = (uint64_t)W * H;
    std::vector<double> own;
    double* e2 = e2_out;
    if (!e2) { own.resize(n_px); e2 = own.data(); }
    rt::adaptive_error_host(rgb_sum, sq_sum, counts, passes, n_px, e2);
    if (stats_out) rt::moments_stats_host(e2, n_px, tau, stats_out);
    return 0;
}
int rt_adaptive_select_host(const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes, uint32_t W, uint32_t H,
                            uint32_t n_samples, double tau, uint64_t max_samples, uint32_t spread, uint32_t* list_out, uint32_t* n_list_out) {
    if (!rgb_sum || !sq_sum || !counts || !passes || !list_out || !n_list_out) return rt::set_error("null argument");
    const std::string problem = rt::adaptive_select_check(W, H, n_samples, tau, max_samples, spread);
    if (!problem.empty()) return rt::set_error(problem);
    *n_list_out = rt::adaptive_select_host(rgb_sum, sq_sum, counts, passes, W, H, n_samples, tau, max_samples, spread, list_out);
    return 0;
}
int rt_adaptive_merge_host(double* pass_sum, uint32_t n_samples, double* rgb_sum, double* sq_sum, uint32_t* counts, uint32_t* passes,
                           const uint32_t* list, uint32_t n_list, uint32_t W, uint32_t H) {
    if (!pass_sum || !rgb_sum || !sq_sum || !counts || !passes || (!list && n_list)) return rt::set_error("null argument");
    const std::string problem = rt::adaptive_frame_check(W, H);
    if (!problem.empty()) return rt::set_error(problem);
    if (n_samples == 0u) return rt::set_error("adaptive: n_samples must be >= 1 (a pass's square is divided by its sample count)");
    const uint64_t n_px = (uint64_t)W * H;
    for (uint32_t k = 0; k < n_list; k++) {
        if (list[k] >= n_px) return rt::set_error("adaptive: a listed pixel lies outside the W x H frame");
        if (k && list[k] <= list[k - 1u]) return rt::set_error("adaptive: the list must be ascending (each pixel once)");
        if (!rt::adaptive_room(counts[list[k]], n_samples, rt::ADAPTIVE_MAX_SAMPLES)) return rt::set_error("adaptive: samples done + n_samples must be <= 2^32 - 1 for every listed pixel");
    }
    rt::adaptive_merge_host(pass_sum, n_samples, rgb_sum, sq_sum, counts, passes, list, n_list);
    return 0;
}
int rt_adaptive_resolve_rgb8_host(const double* rgb_sum, const uint32_t* counts, uint32_t W, uint32_t H, const uint8_t* rgb8_prev, uint8_t* rgb8_out,
                                  uint64_t* changed_px_out) {
    if (!rgb_sum || !counts || !rgb8_out) return rt::set_error("null argument");
    const std::string problem = rt::adaptive_frame_check(W, H);
    if (!problem.empty()) return rt::set_error(problem);
    const uint64_t changed = rt::adaptive_resolve_host(rgb_sum, counts, rgb8_prev, rgb8_out, (uint64_t)W * H);
    if (changed_px_out) *changed_px_out = changed;
    return 0;
}

} // extern "C"

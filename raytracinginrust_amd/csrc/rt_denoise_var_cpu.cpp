// csrc/rt_denoise_var_cpu.cpp — the variance-guided denoiser's host twin: the specification of rt_denoise_var.h as plain C++ (no HIP, no
// device), the argument check its entry points share, and rt_denoise_variance_host of include/rt_amd.h.  Built with -ffp-contract=off like
// the rest of the library: every + - * / below rounds once, which is what makes its words the ones the HIP kernels (rt_denoise_var.hip)
// produce.
#include <vector>
#include "../../include/rt_amd.h"
#include "rt_denoise_var.h"

namespace rt {

int set_error(const std::string& m);          // rt_host.cpp: rt_last_error()'s message; returns -1

std::string denoise_variance_check(uint64_t samples, uint32_t W, uint32_t H, uint32_t iterations, const double* sigma, uint32_t flags) {
    if (!sigma) return "null argument";
    for (int k = 0; k < 3; k++)
        if (!(sigma[k] > 0.0)) return "denoise: sigma_v, sigma_n and sigma_p must be > 0 (+inf switches a stop off; 0, negative and NaN are refused)";
    return denoise_check(samples, W, H, iterations, sigma, flags);
}

namespace {
struct Pixel { double c[3], v; };
struct Guide { double n[3], inv_t, x[3], key; };
inline bool finite3(const double c[3]) { return c[0] - c[0] == 0.0 && c[1] - c[1] == 0.0 && c[2] - c[2] == 0.0; }
inline double stop(double t) { return t > 0.0 ? t * t : 0.0; }
}

void denoise_variance_host(const double* rgb_sum, uint64_t samples, const double* var, const double* hits, uint32_t W, uint32_t H,
                           uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out, double* var_out) {
    const size_t n_px = (size_t)W * H;
    const double n_samples = (double)samples;
    std::vector<Pixel> a(n_px), b(n_px);
    std::vector<Guide> guide(n_px);
    // (B)
    for (size_t p = 0; p < n_px; p++) {
        const double* r = hits + p * DENOISE_HIT_DOUBLES;
        for (int k = 0; k < 3; k++) { b[p].c[k] = rgb_sum[p * 3 + k] / n_samples; guide[p].n[k] = r[5 + k]; guide[p].x[k] = r[2 + k]; }
        b[p].v = denoise_var_scalar(var[p * 3], var[p * 3 + 1], var[p * 3 + 2]);
        guide[p].inv_t = 1.0 / r[1];
        guide[p].key = r[0] != 0.0 ? ((flags & 1u) ? r[11] + 2.0 : 1.0) : 0.0;
    }
    // (C)
    static const double b3[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};
    for (int64_t y = 0; y < (int64_t)H; y++) for (int64_t x = 0; x < (int64_t)W; x++) {
        const size_t p = (size_t)y * W + (size_t)x;
        double acc = 0.0, wsum = 0.0;
        for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
            const int64_t qy = y + dy, qx = x + dx;
            if (qy < 0 || qy >= (int64_t)H || qx < 0 || qx >= (int64_t)W) continue;
            const size_t q = (size_t)qy * W + (size_t)qx;
            if (guide[q].key != guide[p].key) continue;
            const double k = b3[dy + 1] * b3[dx + 1];
            acc += k * b[q].v; wsum += k;
        }
        a[p] = b[p];
        a[p].v = acc / wsum;
    }
    // (D)
    const double kv = sigma[0] * sigma[0];
    double inv[3];
    denoise_inverse_squares(sigma, inv);
    const double in = inv[1], ip = inv[2];
    static const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    const Pixel* src = a.data(); Pixel* dst = b.data();
    for (uint32_t i = 0; i < iterations; i++) {
        const int64_t s = (int64_t)1 << i;
        for (int64_t y = 0; y < (int64_t)H; y++) for (int64_t x = 0; x < (int64_t)W; x++) {
            const size_t p = (size_t)y * W + (size_t)x;
            const Pixel& cp = src[p]; const Guide& gp = guide[p];
            const bool cp_finite = finite3(cp.c);
            double acc[3] = {0.0, 0.0, 0.0}, vacc = 0.0, wsum = 0.0;
            for (int dy = -2; dy <= 2; dy++) for (int dx = -2; dx <= 2; dx++) {
                const int64_t qy = y + dy * s, qx = x + dx * s;
                if (qy < 0 || qy >= (int64_t)H || qx < 0 || qx >= (int64_t)W) continue;
                const size_t q = (size_t)qy * W + (size_t)qx;
                const Pixel& cq = src[q]; const Guide& gq = guide[q];
                if (gq.key != gp.key) continue;
                if (!finite3(cq.c)) continue;
                const double k = h[dy + 2] * h[dx + 2];
                const double e0 = cq.c[0] - cp.c[0], e1 = cq.c[1] - cp.c[1], e2 = cq.c[2] - cp.c[2];
                double d = (e0 * e0 + e1 * e1) + e2 * e2;
                double wc = denoise_var_stop(d, cp.v, cq.v, kv);
                if (!cp_finite) wc = 1.0;
                double wn = 1.0, wp = 1.0;
                if (gp.key != 0.0) {
                    const double m0 = gq.n[0] - gp.n[0], m1 = gq.n[1] - gp.n[1], m2 = gq.n[2] - gp.n[2];
                    d = (m0 * m0 + m1 * m1) + m2 * m2;
                    wn = stop(1.0 - d * in);
                    const double r0 = gq.x[0] - gp.x[0], r1 = gq.x[1] - gp.x[1], r2 = gq.x[2] - gp.x[2];
                    const double g = ((gp.n[0] * r0 + gp.n[1] * r1) + gp.n[2] * r2) * gp.inv_t;
                    wp = stop(1.0 - (g * g) * ip);
                }
                const double w = ((k * wc) * wn) * wp;
                acc[0] += w * cq.c[0]; acc[1] += w * cq.c[1]; acc[2] += w * cq.c[2];
                vacc += (w * w) * cq.v;
                wsum += w;
            }
            for (int k = 0; k < 3; k++) dst[p].c[k] = wsum > 0.0 ? acc[k] / wsum : cp.c[k];
            dst[p].v = wsum > 0.0 ? vacc / (wsum * wsum) : cp.v;
        }
        const Pixel* done = dst; dst = const_cast<Pixel*>(src); src = done;
    }
    for (size_t p = 0; p < n_px; p++) {
        for (int k = 0; k < 3; k++) rgb_sum_out[p * 3 + k] = src[p].c[k] * n_samples;
        if (var_out) var_out[p] = src[p].v;
    }
}

} // namespace rt

extern "C" int rt_denoise_variance_host(const double* rgb_sum, uint64_t samples, const double* var, const double* hits, uint32_t W, uint32_t H,
                                        uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out, double* var_out) {
    if (!rgb_sum || !var || !hits || !sigma || !rgb_sum_out) return rt::set_error("null argument");
    const std::string problem = rt::denoise_variance_check(samples, W, H, iterations, sigma, flags);
    if (!problem.empty()) return rt::set_error(problem);
    rt::denoise_variance_host(rgb_sum, samples, var, hits, W, H, iterations, sigma, flags, rgb_sum_out, var_out);
    return 0;
}

// tests/denoise_variance_san_main.cpp — a stand-alone program around the host twins of the variance-guided denoiser
// (csrc/rt_denoise_var_cpu.cpp, over csrc/rt_denoise_cpu.cpp's checks) and of the variance frame (csrc/rt_moments_cpu.cpp) for a sanitizer
// build: tests/test_denoise_variance_host.py compiles the four files with g++ -fsanitize=address,undefined and runs the result.  It drives
// rt_moments_variance_host and rt_denoise_variance_host over the frame shapes of the tests with every iteration count, finite and infinite
// sigmas, both flag values, non-finite colours and variances, with and without var_out, in place and into buffers of exactly the size the
// header states, and through the arguments they have to refuse.  Exit status 0 and "ok" on stdout: every run returned what it should.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "../include/rt_amd.h"

static std::string g_message;
namespace rt { int set_error(const std::string& m) { g_message = m; return -1; } }      // (rt_host.cpp's, in the library)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                                   // xorshift64*: any deterministic stream will do
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t shapes[5][2] = {{1, 1}, {3, 5}, {1, 40}, {23, 37}, {67, 130}};          // H, W
    const double sigmas[3][3] = {{1.5, 1.2, 1.0}, {inf, inf, inf}, {inf, 1.2, inf}};
    int runs = 0;
    for (const auto& shape : shapes) {
        const uint32_t H = shape[0], W = shape[1];
        const size_t n = (size_t)W * H;
        std::vector<double> sum(n * 3), sq(n * 3), var(n * 3, -1.0), hits(n * 16, 0.0);
        for (size_t p = 0; p < n; p++) {
            for (int k = 0; k < 3; k++) { sum[p * 3 + k] = 5.0 * uniform(); sq[p * 3 + k] = sum[p * 3 + k] * sum[p * 3 + k] / 5.0 + 0.5 * uniform(); }
            double* r = &hits[p * 16];
            if (uniform() > 0.3) {
                r[0] = 1.0; r[1] = 0.5 + 2.5 * uniform();
                double len = 0.0;
                for (int k = 0; k < 3; k++) { r[2 + k] = 2.0 * uniform() - 1.0; r[5 + k] = 2.0 * uniform() - 1.0; len += r[5 + k] * r[5 + k]; }
                for (int k = 0; k < 3; k++) r[5 + k] /= std::sqrt(len);
                r[11] = uniform() < 0.1 ? -1.0 : std::floor(3.0 * uniform());
            } else for (int k = 11; k < 15; k++) r[k] = -1.0;
        }
        if (n > 1) { sum[0] = nan; sum[n * 3 - 1] = inf; sum[(n * 3) / 2] = -inf; sq[4] = inf; sq[5] = nan; }
        if (rt_moments_variance_host(sum.data(), sq.data(), 5, 3, W, H, var.data()) != 0) { std::printf("variance failed: %s\n", g_message.c_str()); return 1; }
        for (size_t i = 0; i < n * 3; i++) if (!(var[i] >= 0.0)) { std::printf("variance: entry %zu is not >= 0\n", i); return 1; }
        if (n > 1) { var[3] = nan; var[n * 3 - 2] = -2.0; }
        runs++;
        for (uint32_t K = 1; K <= 8; K++) {
            if (K > 5 && !(H == 3 && W == 5)) continue;
            for (const auto& sg : sigmas) for (uint32_t flags = 0; flags < 2; flags++) {
                std::vector<double> out(n * 3, -1.0), out2(n * 3, -1.0), v_out(n, -1.0), in_place(sum);
                if (rt_denoise_variance_host(sum.data(), 5, var.data(), hits.data(), W, H, K, sg, flags, out.data(), v_out.data()) != 0) { std::printf("failed: %s\n", g_message.c_str()); return 1; }
                if (rt_denoise_variance_host(sum.data(), 5, var.data(), hits.data(), W, H, K, sg, flags, out2.data(), nullptr) != 0) { std::printf("failed without var_out: %s\n", g_message.c_str()); return 1; }
                if (rt_denoise_variance_host(in_place.data(), 5, var.data(), hits.data(), W, H, K, sg, flags, in_place.data(), nullptr) != 0) { std::printf("failed in place: %s\n", g_message.c_str()); return 1; }
                if (std::memcmp(out.data(), in_place.data(), n * 3 * sizeof(double)) != 0 || std::memcmp(out.data(), out2.data(), n * 3 * sizeof(double)) != 0) { std::printf("forms differ: %u x %u, K = %u\n", W, H, K); return 1; }
                for (size_t p = 0; p < n; p++) if (!(v_out[p] >= 0.0)) { std::printf("var_out: pixel %zu is not >= 0\n", p); return 1; }
                runs += 3;
            }
        }
    }
    // what has to be refused, with a message and without a write
    double px[3] = {1.0, 2.0, 3.0}, vr[3] = {0.1, 0.1, 0.1}, rec[16] = {0.0}, out[3] = {7.0, 7.0, 7.0};
    const double good[3] = {1.0, 1.0, 1.0}, zero[3] = {1.0, 0.0, 1.0}, neg[3] = {-1.0, 1.0, 1.0}, bad[3] = {1.0, 1.0, nan};
    int refused = 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 0, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 9, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 1, zero, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 1, neg, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 1, bad, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 0, vr, rec, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 0, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 0, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 1, good, 2, out, nullptr) != 0;
    refused += rt_denoise_variance_host(nullptr, 1, vr, rec, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, nullptr, rec, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, nullptr, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 1, nullptr, 0, out, nullptr) != 0;
    refused += rt_denoise_variance_host(px, 1, vr, rec, 1, 1, 1, good, 0, nullptr, nullptr) != 0;
    refused += rt_moments_variance_host(px, vr, 4, 1, 1, 1, out) != 0;
    refused += rt_moments_variance_host(px, vr, 0, 2, 1, 1, out) != 0;
    refused += rt_moments_variance_host(px, vr, 4, 2, 0, 1, out) != 0;
    refused += rt_moments_variance_host(nullptr, vr, 4, 2, 1, 1, out) != 0;
    refused += rt_moments_variance_host(px, vr, 4, 2, 1, 1, nullptr) != 0;
    if (refused != 19 || g_message.empty() || out[0] != 7.0 || out[1] != 7.0 || out[2] != 7.0) { std::printf("arguments: %d of 19 refused\n", refused); return 1; }
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

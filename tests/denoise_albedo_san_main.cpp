// tests/denoise_albedo_san_main.cpp — a stand-alone program around albedo-demodulated denoising's host twin (csrc/rt_albedo_cpu.cpp over
// csrc/rt_denoise_cpu.cpp) for a sanitizer build: tests/test_denoise_albedo_host.py compiles the three files with g++
// -fsanitize=address,undefined and runs the result.  It drives rt_denoise_albedo_host on a 23 x 37 frame (no multiple of any tile) with
// every iteration count, finite and infinite sigmas, both flag values, non-finite colours, albedo channels that are zero, below eps, above
// one, NaN and infinite, albedo_samples 1 and 5, in place and into a buffer of exactly W*H*3 doubles, checks that a black channel stays
// black, and goes through the arguments it has to refuse.  Exit status 0 and "ok" on stdout: every run returned what it should.
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
    const uint32_t H = 23, W = 37;
    const size_t n = (size_t)W * H;
    const double sigmas[3][3] = {{0.7, 1.2, 1.0}, {inf, inf, inf}, {inf, 1.2, inf}};
    int runs = 0;
    for (uint64_t n_alb = 1; n_alb <= 5; n_alb += 4) {
        std::vector<double> sum(n * 3), alb(n * 3), hits(n * 16, 0.0);
        for (size_t p = 0; p < n; p++) {
            for (int k = 0; k < 3; k++) { sum[p * 3 + k] = 5.0 * uniform(); alb[p * 3 + k] = 1.25 * uniform() * (double)n_alb; }
            double* r = &hits[p * 16];
            if (uniform() > 0.3) {
                r[0] = 1.0; r[1] = 0.5 + 2.5 * uniform();
                double len = 0.0;
                for (int k = 0; k < 3; k++) { r[2 + k] = 2.0 * uniform() - 1.0; r[5 + k] = 2.0 * uniform() - 1.0; len += r[5 + k] * r[5 + k]; }
                for (int k = 0; k < 3; k++) r[5 + k] /= std::sqrt(len);
                r[11] = uniform() < 0.1 ? -1.0 : std::floor(3.0 * uniform());
            } else for (int k = 11; k < 15; k++) r[k] = -1.0;
        }
        sum[0] = nan; sum[n * 3 - 1] = inf; sum[(n * 3) / 2] = -inf;
        const size_t black = 3 * (10 * W + 7) + 1;
        alb[black] = 0.0; alb[5] = 0.001 * (double)n_alb; alb[8] = nan; alb[11] = inf; alb[14] = -inf; alb[17] = 3.0 * (double)n_alb;
        for (uint32_t K = 1; K <= 5; K++) for (const auto& sg : sigmas) for (uint32_t flags = 0; flags < 2; flags++) {
            std::vector<double> out(n * 3, -1.0), in_place(sum);
            if (rt_denoise_albedo_host(sum.data(), 5, alb.data(), n_alb, hits.data(), W, H, K, sg, flags, out.data()) != 0) { std::printf("failed: %s\n", g_message.c_str()); return 1; }
            if (rt_denoise_albedo_host(in_place.data(), 5, alb.data(), n_alb, hits.data(), W, H, K, sg, flags, in_place.data()) != 0) { std::printf("failed in place: %s\n", g_message.c_str()); return 1; }
            if (std::memcmp(out.data(), in_place.data(), n * 3 * sizeof(double)) != 0) { std::printf("in place differs: K = %u\n", K); return 1; }
            if (out[black] != 0.0) { std::printf("a black channel came back as %g: K = %u\n", out[black], K); return 1; }
            runs += 2;
        }
    }
    // what has to be refused, with a message and without a write
    double px[3] = {1.0, 2.0, 3.0}, al[3] = {1.0, 1.0, 1.0}, rec[16] = {0.0}, out[3] = {7.0, 7.0, 7.0};
    const double good[3] = {1.0, 1.0, 1.0}, zero[3] = {1.0, 0.0, 1.0};
    int refused = 0;
    refused += rt_denoise_albedo_host(px, 1, al, 0, rec, 1, 1, 1, good, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, nullptr, 1, rec, 1, 1, 1, good, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, al, 1, rec, 1, 1, 1, good, 2, out) != 0;
    refused += rt_denoise_albedo_host(px, 0, al, 1, rec, 1, 1, 1, good, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, al, 1, rec, 1, 1, 0, good, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, al, 1, rec, 1, 1, 1, zero, 0, out) != 0;
    refused += rt_denoise_albedo_host(nullptr, 1, al, 1, rec, 1, 1, 1, good, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, al, 1, nullptr, 1, 1, 1, good, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, al, 1, rec, 1, 1, 1, nullptr, 0, out) != 0;
    refused += rt_denoise_albedo_host(px, 1, al, 1, rec, 1, 1, 1, good, 0, nullptr) != 0;
    if (refused != 10 || g_message.empty() || out[0] != 7.0 || out[1] != 7.0 || out[2] != 7.0) { std::printf("arguments: %d of 10 refused\n", refused); return 1; }
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

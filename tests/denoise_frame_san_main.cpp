// tests/denoise_frame_san_main.cpp — a stand-alone program around the host twins of csrc/rt_denoise_frame.h (csrc/rt_denoise_frame_cpu.cpp,
// over the filters' own twins in csrc/rt_denoise_cpu.cpp and csrc/rt_denoise_var_cpu.cpp) for a sanitizer build:
// tests/test_denoise_frame_host.py compiles the files with g++ -fsanitize=address,undefined and runs the result.  It drives
// rt_adaptive_variance_host and rt_denoise_frame_host over the frame shapes of the tests in all eight combinations of {counts, variance,
// albedo}, with counts of 0 and 1, non-finite colours, variances and albedos, with and without var_out, in place and into buffers of exactly
// the size the header states, and through the arguments they have to refuse.  Exit status 0 and "ok" on stdout: every run returned what it
// should.
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
    const double sigmas[2][3] = {{1.5, 1.2, 1.0}, {inf, 1.2, inf}};
    int runs = 0;
    for (const auto& shape : shapes) {
        const uint32_t H = shape[0], W = shape[1];
        const size_t n = (size_t)W * H;
        std::vector<double> sum(n * 3), sq(n * 3), var(n * 3, -1.0), alb(n * 3), hits(n * 16, 0.0);
        std::vector<uint32_t> cnt(n), pas(n);
        for (size_t p = 0; p < n; p++) {
            cnt[p] = 2u + (uint32_t)(8.0 * uniform()); pas[p] = 2u + (uint32_t)(uniform() * (double)(cnt[p] - 1u));
            for (int k = 0; k < 3; k++) { sum[p * 3 + k] = 5.0 * uniform(); sq[p * 3 + k] = sum[p * 3 + k] * sum[p * 3 + k] / 5.0 + 0.5 * uniform(); alb[p * 3 + k] = 4.0 * uniform(); }
            double* r = &hits[p * 16];
            if (uniform() > 0.3) {
                r[0] = 1.0; r[1] = 0.5 + 2.5 * uniform();
                double len = 0.0;
                for (int k = 0; k < 3; k++) { r[2 + k] = 2.0 * uniform() - 1.0; r[5 + k] = 2.0 * uniform() - 1.0; len += r[5 + k] * r[5 + k]; }
                for (int k = 0; k < 3; k++) r[5 + k] /= std::sqrt(len);
                r[11] = uniform() < 0.1 ? -1.0 : std::floor(3.0 * uniform());
            } else for (int k = 11; k < 15; k++) r[k] = -1.0;
        }
        if (n > 1) {
            sum[0] = nan; sum[n * 3 - 1] = inf; sum[(n * 3) / 2] = -inf; sq[4] = inf; sq[5] = nan;
            alb[1] = 0.0; alb[2] = nan; alb[n * 3 - 2] = inf; alb[n * 3 - 3] = 0.001;
            cnt[n - 1] = 0u; pas[n - 1] = 0u; cnt[n / 2] = 1u; pas[n / 2] = 1u; pas[n / 3] = 0u;
        }
        if (rt_adaptive_variance_host(sum.data(), sq.data(), cnt.data(), pas.data(), W, H, var.data()) != 0) { std::printf("variance failed: %s\n", g_message.c_str()); return 1; }
        for (size_t i = 0; i < n * 3; i++) if (!(var[i] >= 0.0) && !(cnt[i / 3] == 0u)) { std::printf("variance: entry %zu is not >= 0\n", i); return 1; }
        if (n > 1 && (var[(n - 1) * 3] != inf || var[(n / 2) * 3 + 1] != inf)) { std::printf("variance: a pixel with fewer than two passes is not +inf\n"); return 1; }
        if (n > 1) { var[3] = nan; var[n * 3 - 5] = -2.0; }
        runs++;
        for (uint32_t K = 1; K <= 8; K += (K < 3 ? 1 : (K == 3 ? 2 : 3))) {                 // 1, 2, 3, 5, 8
            if (K > 5 && !(H == 3 && W == 5)) continue;
            for (const auto& sg : sigmas) for (uint32_t combo = 0; combo < 8; combo++) {
                const uint32_t* c = (combo & 1u) ? cnt.data() : nullptr;
                const double* v = (combo & 2u) ? var.data() : nullptr;
                const double* a = (combo & 4u) ? alb.data() : nullptr;
                const uint32_t flags = (combo ^ K) & 1u;
                std::vector<double> out(n * 3, -1.0), out2(n * 3, -1.0), v_out(n, -1.0), in_place(sum);
                if (rt_denoise_frame_host(sum.data(), c, 5, v, a, 3, hits.data(), W, H, K, sg, flags, out.data(), v ? v_out.data() : nullptr) != 0) { std::printf("failed: %s\n", g_message.c_str()); return 1; }
                if (rt_denoise_frame_host(sum.data(), c, 5, v, a, 3, hits.data(), W, H, K, sg, flags, out2.data(), nullptr) != 0) { std::printf("failed without var_out: %s\n", g_message.c_str()); return 1; }
                if (rt_denoise_frame_host(in_place.data(), c, 5, v, a, 3, hits.data(), W, H, K, sg, flags, in_place.data(), nullptr) != 0) { std::printf("failed in place: %s\n", g_message.c_str()); return 1; }
                if (std::memcmp(out.data(), in_place.data(), n * 3 * sizeof(double)) != 0 || std::memcmp(out.data(), out2.data(), n * 3 * sizeof(double)) != 0) { std::printf("forms differ: %u x %u, K = %u, combination %u\n", W, H, K, combo); return 1; }
                if (v) for (size_t p = 0; p < n; p++) if (!(v_out[p] >= 0.0)) { std::printf("var_out: pixel %zu is not >= 0\n", p); return 1; }
                if (c && n > 1 && !a) for (int k = 0; k < 3; k++) if (out[(n - 1) * 3 + k] != 0.0 || std::signbit(out[(n - 1) * 3 + k])) { std::printf("a pixel without samples is not +0.0\n"); return 1; }
                runs += 3;
            }
        }
    }
    // what has to be refused, with a message and without a write
    double px[3] = {1.0, 2.0, 3.0}, vr[3] = {0.1, 0.1, 0.1}, al[3] = {1.0, 1.0, 1.0}, rec[16] = {0.0}, out[3] = {7.0, 7.0, 7.0}, vo[1] = {7.0};
    uint32_t one[1] = {1u};
    const double good[3] = {1.0, 1.0, 1.0}, zero[3] = {1.0, 0.0, 1.0}, bad[3] = {1.0, 1.0, nan};
    int refused = 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 1, 0, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 1, 9, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 1, 1, zero, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, nullptr, al, 1, rec, 1, 1, 1, bad, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, nullptr, 0, vr, al, 1, rec, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 0, rec, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, nullptr, al, 1, rec, 1, 1, 1, good, 0, out, vo) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 0, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 0, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 1, 1, good, 2, out, nullptr) != 0;
    refused += rt_denoise_frame_host(nullptr, one, 1, vr, al, 1, rec, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, nullptr, 1, 1, 1, good, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 1, 1, nullptr, 0, out, nullptr) != 0;
    refused += rt_denoise_frame_host(px, one, 1, vr, al, 1, rec, 1, 1, 1, good, 0, nullptr, nullptr) != 0;
    refused += rt_adaptive_variance_host(px, vr, one, one, 0, 1, out) != 0;
    refused += rt_adaptive_variance_host(nullptr, vr, one, one, 1, 1, out) != 0;
    refused += rt_adaptive_variance_host(px, vr, nullptr, one, 1, 1, out) != 0;
    refused += rt_adaptive_variance_host(px, vr, one, one, 1, 1, nullptr) != 0;
    if (refused != 18 || g_message.empty() || out[0] != 7.0 || out[1] != 7.0 || out[2] != 7.0 || vo[0] != 7.0) { std::printf("arguments: %d of 18 refused\n", refused); return 1; }
    // ... and the smallest call that is not
    if (rt_denoise_frame_host(px, one, 0, vr, al, 1, rec, 1, 1, 1, good, 0, out, vo) != 0 || out[0] != 1.0 || out[1] != 2.0 || out[2] != 3.0) { std::printf("1 x 1: %s\n", g_message.c_str()); return 1; }
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

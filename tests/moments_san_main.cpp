// tests/moments_san_main.cpp — a stand-alone program around the moments' host twin (csrc/rt_moments_cpu.cpp) for a sanitizer build:
// tests/test_moments_host.py compiles the two files with g++ -fsanitize=address,undefined and runs the result.  It merges passes of unequal
// size into frames of exactly W*H*3 doubles (1 x 1, 15 x 11, 64 x 3), with NaN, infinite, tiny and overflowing pass values and an infinite
// second moment, takes the error map into a buffer of exactly W*H doubles and its statistics, checks the invariants that need no second implementation (the counts add up
// to W*H, a constant pixel has e2 = 0, the maximum is the largest finite value) and goes through the arguments that have to be refused.
// Exit status 0 and "ok" on stdout: every run returned what it should.
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
    const uint32_t shapes[3][2] = {{1, 1}, {15, 11}, {64, 3}};
    const uint64_t sizes[4] = {3, 5, 8, 16};
    int runs = 0;
    for (const auto& wh : shapes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        std::vector<double> S(n * 3, 0.0), Q(n * 3, 0.0);
        uint64_t N = 0;
        for (int b = 0; b < 4; b++) {
            std::vector<double> p(n * 3);
            for (double& v : p) v = uniform() * (double)sizes[b];
            if (n > 40) {
                if (b == 1) { p[3] = nan; p[13] = inf; p[23] = -inf; p[52] = 1e160; }      // (1e160: p * p and S * S both overflow)
                p[60] = 1e-4 * (double)sizes[b];
                for (int k = 0; k < 3; k++) p[90 + k] = 0.3 * (double)sizes[b];          // pixel 30: constant
            }
            const std::vector<double> before(p);
            if (rt_moments_merge_host(p.data(), sizes[b], S.data(), Q.data(), n * 3) != 0) { std::printf("merge failed: %s\n", g_message.c_str()); return 1; }
            if (std::memcmp(before.data(), p.data(), n * 3 * sizeof(double)) != 0) { std::printf("the host merge wrote to the pass frame\n"); return 1; }
            N += sizes[b];
            if (b == 0) continue;
            if (n > 40 && b == 3) Q[57] = inf;                 // an infinite second moment beside a finite sum, as a loaded checkpoint may hold: e2 = +inf
            std::vector<double> e2(n, -1.0);
            if (rt_moments_error_host(S.data(), Q.data(), N, (uint64_t)b + 1u, W, H, e2.data()) != 0) { std::printf("error map failed: %s\n", g_message.c_str()); return 1; }
            uint64_t st[4] = {9, 9, 9, 9};
            if (rt_moments_stats_host(e2.data(), n, 1.0 / 16.0, st) != 0) { std::printf("stats failed: %s\n", g_message.c_str()); return 1; }
            if (st[0] + st[1] + st[2] != n) { std::printf("the counts do not add up: %llu + %llu + %llu != %zu\n", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], n); return 1; }
            double mx = 0.0;
            for (double v : e2) if (v - v == 0.0 && v > mx) mx = v;
            double got; std::memcpy(&got, &st[3], sizeof(got));
            if (got != mx) { std::printf("max_e2 %g, want %g\n", got, mx); return 1; }
            if (n > 40 && b == 3 && !(e2[30] >= 0.0 && e2[30] < 1e-25)) { std::printf("a constant pixel has e2 = %g\n", e2[30]); return 1; }
            if (n > 40 && b == 3 && st[2] != 1) { std::printf("an infinite second moment beside a finite sum: nonfinite = %llu, want 1\n", (unsigned long long)st[2]); return 1; }
            runs++;
        }
    }
    // what has to be refused, with a message and without a write
    double s[3] = {1.0, 2.0, 3.0}, q[3] = {1.0, 2.0, 3.0}, p[3] = {1.0, 1.0, 1.0}, e = 7.0;
    uint64_t st[4] = {7, 7, 7, 7};
    int refused = 0;
    refused += rt_moments_merge_host(p, 0, s, q, 3) != 0;
    refused += rt_moments_merge_host(nullptr, 1, s, q, 3) != 0;
    refused += rt_moments_merge_host(p, 1, nullptr, q, 3) != 0;
    refused += rt_moments_merge_host(p, 1, s, nullptr, 3) != 0;
    refused += rt_moments_error_host(s, q, 4, 1, 1, 1, &e) != 0;
    refused += rt_moments_error_host(s, q, 0, 2, 1, 1, &e) != 0;
    refused += rt_moments_error_host(s, q, 4, 2, 0, 1, &e) != 0;
    refused += rt_moments_error_host(nullptr, q, 4, 2, 1, 1, &e) != 0;
    refused += rt_moments_error_host(s, nullptr, 4, 2, 1, 1, &e) != 0;
    refused += rt_moments_error_host(s, q, 4, 2, 1, 1, nullptr) != 0;
    refused += rt_moments_stats_host(&e, 1, -1.0, st) != 0;
    refused += rt_moments_stats_host(&e, 1, nan, st) != 0;
    refused += rt_moments_stats_host(nullptr, 1, 1.0, st) != 0;
    refused += rt_moments_stats_host(&e, 1, 1.0, nullptr) != 0;
    if (refused != 14 || g_message.empty() || e != 7.0 || st[0] != 7 || st[3] != 7 || s[0] != 1.0 || q[2] != 3.0) { std::printf("arguments: %d of 14 refused\n", refused); return 1; }
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

// tests/adaptive_san_main.cpp — a stand-alone program around the adaptive frames' host twin (csrc/rt_adaptive_cpu.cpp, with csrc/rt_moments_cpu.cpp
// for the statistics) for a sanitizer build: tests/test_adaptive_host.py compiles the three files with g++ -fsanitize=address,undefined and runs
// the result.  It drives a frame through adaptive passes entirely on the host — select, a synthetic pass frame for the listed pixels, list
// merge, error, resolve — in buffers of exactly W*H (x 3) elements (1 x 1, 15 x 11, 64 x 3), with spread 0 and 1, a sample cap, NaN and
// infinite pass values, checks the invariants that need no second implementation (the list is ascending and inside the frame, counts
// advance for exactly the listed pixels, unlisted pixels keep every word, the statistics add up to W*H, a pixel with no samples resolves to
// 0) and goes through the arguments that have to be refused.  Exit status 0 and "ok" on stdout: every run returned what it should.
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
#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t shapes[3][2] = {{1, 1}, {15, 11}, {64, 3}};
    int runs = 0;
    for (const auto& wh : shapes)
        for (uint32_t spread = 0; spread < 2; spread++) {
            const uint32_t W = wh[0], H = wh[1], n_b = 4;
            const size_t n = (size_t)W * H;
            const uint64_t cap = 24;
            std::vector<double> S(n * 3, 0.0), Q(n * 3, 0.0), P(n * 3, 0.0), noise(n);
            std::vector<uint32_t> cnt(n, 0u), pas(n, 0u), list(n, 0xFFFFFFFFu);
            for (double& v : noise) v = uniform() < 0.3 ? 0.0 : uniform();              // some pixels are constant: they finish after two passes
            uint64_t total = 0;
            for (int pass = 0; pass < 10; pass++) {
                uint32_t n_list = 0xFFFFFFFFu;
                if (rt_adaptive_select_host(S.data(), Q.data(), cnt.data(), pas.data(), W, H, n_b, 1.0 / 64.0, cap, spread, list.data(), &n_list) != 0) FAIL("select failed: %s", g_message.c_str());
                if (n_list > n) FAIL("a list of %u pixels for a frame of %zu", n_list, n);
                if (pass < 2 && n_list != n) FAIL("pass %d lists %u of %zu pixels: every pixel needs two passes", pass, n_list, n);
                for (uint32_t k = 0; k < n_list; k++) {
                    if (list[k] >= n || (k && list[k] <= list[k - 1])) FAIL("the list is not ascending inside the frame at %u", k);
                    if ((uint64_t)cnt[list[k]] + n_b > cap) FAIL("pixel %u is listed past the cap", list[k]);
                }
                if (n_list == 0) break;
                for (uint32_t k = 0; k < n_list; k++)
                    for (int c = 0; c < 3; c++) P[3 * (size_t)list[k] + c] = n_b * (0.4 + noise[list[k]] * (uniform() - 0.5));
                if (n > 40 && pass == 2 && n_list > 2) { P[3 * (size_t)list[0]] = nan; P[3 * (size_t)list[1] + 1] = inf; }
                const std::vector<double> S0(S), Q0(Q); const std::vector<uint32_t> c0(cnt), p0(pas);
                if (rt_adaptive_merge_host(P.data(), n_b, S.data(), Q.data(), cnt.data(), pas.data(), list.data(), n_list, W, H) != 0) FAIL("merge failed: %s", g_message.c_str());
                std::vector<uint8_t> listed(n, 0);
                for (uint32_t k = 0; k < n_list; k++) listed[list[k]] = 1;
                for (size_t p = 0; p < n; p++) {
                    if (cnt[p] != c0[p] + (listed[p] ? n_b : 0u) || pas[p] != p0[p] + (listed[p] ? 1u : 0u)) FAIL("the counts of pixel %zu moved wrongly", p);
                    if (!listed[p] && (std::memcmp(&S[3 * p], &S0[3 * p], 24) != 0 || std::memcmp(&Q[3 * p], &Q0[3 * p], 24) != 0)) FAIL("an unlisted pixel changed");
                    for (int c = 0; c < 3; c++) { uint64_t w; std::memcpy(&w, &P[3 * p + c], 8); if (w != 0) FAIL("the pass frame is not +0.0 after the merge"); }
                }
                total += (uint64_t)n_list * n_b;
                std::vector<double> e2(n, -1.0);
                uint64_t st[4] = {9, 9, 9, 9};
                if (rt_adaptive_error_host(S.data(), Q.data(), cnt.data(), pas.data(), W, H, e2.data(), 1.0 / 64.0, st) != 0) FAIL("error map failed: %s", g_message.c_str());
                if (st[0] + st[1] + st[2] != n) FAIL("the statistics do not add up");
                if (pass == 0 && st[2] != n) FAIL("after one pass every pixel's error is +inf");
                std::vector<uint8_t> img(n * 3, 7), img2(n * 3, 7);
                uint64_t changed = 99;
                if (rt_adaptive_resolve_rgb8_host(S.data(), cnt.data(), W, H, nullptr, img.data(), &changed) != 0 || changed != n) FAIL("resolve failed: %s", g_message.c_str());
                if (rt_adaptive_resolve_rgb8_host(S.data(), cnt.data(), W, H, img.data(), img2.data(), &changed) != 0 || changed != 0 || img != img2) FAIL("a second resolve differs");
                runs++;
            }
            uint64_t sum = 0;
            for (uint32_t c : cnt) { sum += c; if (c > cap) FAIL("a pixel holds %u samples, past the cap", c); }
            if (sum != total) FAIL("the counts sum to %llu, the passes rendered %llu", (unsigned long long)sum, (unsigned long long)total);
        }
    {   // a pixel that holds nothing resolves to 0
        double s[3] = {5.0, nan, inf}; uint32_t c = 0; uint8_t px[3] = {9, 9, 9};
        if (rt_adaptive_resolve_rgb8_host(s, &c, 1, 1, nullptr, px, nullptr) != 0 || px[0] || px[1] || px[2]) FAIL("n = 0 does not resolve to 0");
    }
    // what has to be refused, with a message and without a write
    double s[6] = {1, 2, 3, 4, 5, 6}, q[6] = {1, 2, 3, 4, 5, 6}, p[6] = {1, 1, 1, 1, 1, 1}, e[2] = {7.0, 7.0};
    uint32_t c[2] = {4, 4}, b[2] = {2, 2}, lst[2] = {9, 9}, n_list = 7, bad_order[2] = {1, 0}, outside[2] = {0, 2}, ok_list[2] = {0, 1};
    uint8_t img[6] = {9, 9, 9, 9, 9, 9};
    uint64_t st[4] = {7, 7, 7, 7}, changed = 7;
    int refused = 0;
    refused += rt_adaptive_error_host(nullptr, q, c, b, 2, 1, e, 0.1, st) != 0;
    refused += rt_adaptive_error_host(s, q, nullptr, b, 2, 1, e, 0.1, st) != 0;
    refused += rt_adaptive_error_host(s, q, c, b, 0, 1, e, 0.1, st) != 0;
    refused += rt_adaptive_error_host(s, q, c, b, 2, 1, e, -1.0, st) != 0;
    refused += rt_adaptive_error_host(s, q, c, b, 2, 1, e, nan, st) != 0;
    refused += rt_adaptive_select_host(s, q, c, b, 2, 1, 0, 0.1, 100, 1, lst, &n_list) != 0;
    refused += rt_adaptive_select_host(s, q, c, b, 2, 1, 4, -0.1, 100, 1, lst, &n_list) != 0;
    refused += rt_adaptive_select_host(s, q, c, b, 2, 1, 4, 0.1, 1ull << 32, 1, lst, &n_list) != 0;
    refused += rt_adaptive_select_host(s, q, c, b, 2, 1, 4, 0.1, 100, 2, lst, &n_list) != 0;
    refused += rt_adaptive_select_host(s, q, c, b, 2, 1, 4, 0.1, 100, 1, nullptr, &n_list) != 0;
    refused += rt_adaptive_select_host(s, q, c, b, 2, 1, 4, 0.1, 100, 1, lst, nullptr) != 0;
    refused += rt_adaptive_merge_host(p, 0, s, q, c, b, ok_list, 2, 2, 1) != 0;
    refused += rt_adaptive_merge_host(p, 4, s, q, c, b, bad_order, 2, 2, 1) != 0;
    refused += rt_adaptive_merge_host(p, 4, s, q, c, b, outside, 2, 2, 1) != 0;
    refused += rt_adaptive_merge_host(p, 4, s, q, c, b, nullptr, 2, 2, 1) != 0;
    refused += rt_adaptive_merge_host(nullptr, 4, s, q, c, b, ok_list, 2, 2, 1) != 0;
    c[1] = 0xFFFFFFFFu - 3u;
    refused += rt_adaptive_merge_host(p, 4, s, q, c, b, ok_list, 2, 2, 1) != 0;
    c[1] = 4;
    refused += rt_adaptive_resolve_rgb8_host(nullptr, c, 2, 1, nullptr, img, &changed) != 0;
    refused += rt_adaptive_resolve_rgb8_host(s, c, 2, 1, nullptr, nullptr, &changed) != 0;
    refused += rt_adaptive_resolve_rgb8_host(s, c, 2, 0, nullptr, img, &changed) != 0;
    if (refused != 20 || g_message.empty() || e[0] != 7.0 || st[0] != 7 || st[3] != 7 || s[0] != 1.0 || q[5] != 6.0 || p[0] != 1.0 || c[0] != 4 || b[1] != 2 || lst[0] != 9 || n_list != 7 ||
        img[0] != 9 || changed != 7) FAIL("arguments: %d of 20 refused, or a refused call wrote", refused);
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

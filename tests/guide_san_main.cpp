// tests/guide_san_main.cpp — a stand-alone program around the averaged guide's host twin (csrc/rt_guide_cpu.cpp) for a sanitizer build:
// tests/test_guide_host.py compiles the two files with g++ -fsanitize=address,undefined and runs the result.  It drives
// rt_guide_from_hits_host on stacks of 1, 2, 3, 5 and 8 samples of 253 pixels (buffers of exactly the sizes the call names) holding hits,
// misses, media, mixed materials, -0.0, NaN and infinite words, checks the counts, the majority rule and the agreement words against a
// plain recount, and goes through the arguments it has to refuse.  Exit status 0 and "ok" on stdout: every run returned what it should.
#include <cmath>
#include <cstdint>
#include <cstdio>
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
    const uint64_t n_px = 253;
    const uint32_t counts[5] = {1, 2, 3, 5, 8};
    int runs = 0;
    for (uint32_t n_samples : counts) {
        std::vector<double> hits((size_t)n_samples * n_px * 16, 0.0), guide(n_px * 16, -7.0);
        for (uint32_t s = 0; s < n_samples; s++) for (uint64_t p = 0; p < n_px; p++) {
            double* r = &hits[((size_t)s * n_px + p) * 16];
            const double chance = (double)(p % 5) / 4.0;    // pixels that always miss, mostly miss, ..., always hit
            if (uniform() < chance || chance == 1.0) {
                r[0] = 1.0; r[1] = 0.5 + 20.0 * uniform();
                for (int k = 0; k < 3; k++) { r[2 + k] = 40.0 * uniform() - 20.0; r[5 + k] = 2.0 * uniform() - 1.0; }
                r[8] = uniform() < 0.5 ? 1.0 : 0.0; r[9] = uniform(); r[10] = uniform();
                r[11] = p % 7 == 0 ? -1.0 : (p % 3 == 0 ? std::floor(3.0 * uniform()) : 2.0);
                r[12] = p % 4 == 0 ? std::floor(5.0 * uniform()) : 9.0;
                r[13] = 1.0; r[14] = (double)p;
                if (p % 11 == 0) r[5] = -0.0;
                if (p % 13 == 0) r[1] = nan;
                if (p % 17 == 0) r[2] = s % 2 ? inf : -inf;
            } else for (int k = 11; k < 15; k++) r[k] = -1.0;
        }
        if (rt_guide_from_hits_host(hits.data(), n_samples, n_px, guide.data()) != 0) { std::printf("failed: %s\n", g_message.c_str()); return 1; }
        for (uint64_t p = 0; p < n_px; p++) {
            uint32_t h = 0, hf = 0; bool m_same = true, o_same = true; double m = -1.0, o = -1.0;
            for (uint32_t s = 0; s < n_samples; s++) {
                const double* r = &hits[((size_t)s * n_px + p) * 16];
                if (r[0] == 0.0) continue;
                if (h == 0) { m = r[11]; o = r[12]; } else { m_same = m_same && r[11] == m; o_same = o_same && r[12] == o; }
                h++; hf += r[8] != 0.0;
            }
            const double* g = &guide[p * 16];
            const bool ok = g[15] == (double)h && g[0] == ((h >= 1 && 2 * h >= n_samples) ? 1.0 : 0.0) && g[8] == (h ? (double)hf / (double)h : 0.0) &&
                            g[11] == ((h && m_same) ? m : -1.0) && g[12] == ((h && o_same) ? o : -1.0) && g[9] == 0.0 && g[10] == 0.0 && g[13] == -1.0 && g[14] == -1.0 &&
                            (h != 0 || (g[1] == 0.0 && g[2] == 0.0 && g[7] == 0.0));
            if (!ok) { std::printf("pixel %llu of %u samples: a word is not what a recount gives\n", (unsigned long long)p, n_samples); return 1; }
        }
        runs++;
    }
    // what has to be refused, with a message and without a write
    double rec[32] = {0.0}, out[16];
    for (double& x : out) x = 7.0;
    int refused = 0;
    refused += rt_guide_from_hits_host(nullptr, 2, 1, out) != 0;
    refused += rt_guide_from_hits_host(rec, 2, 1, nullptr) != 0;
    refused += rt_guide_from_hits_host(rec, 0, 1, out) != 0;
    bool untouched = true;
    for (double x : out) untouched = untouched && x == 7.0;
    if (refused != 3 || g_message.empty() || !untouched) { std::printf("arguments: %d of 3 refused\n", refused); return 1; }
    if (rt_guide_from_hits_host(rec, 2, 1, out) != 0 || out[0] != 0.0 || out[11] != -1.0 || out[15] != 0.0) { std::printf("two all-zero records are not a miss\n"); return 1; }
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

// tests/reproject_var_san_main.cpp — a stand-alone program around the host twin of temporal variance (csrc/rt_reproject_var_cpu.cpp, with
// csrc/rt_reproject_cpu.cpp for the argument checks) for a sanitizer build: tests/test_reproject_var_host.py compiles the three files with
// g++ -fsanitize=address,undefined and runs the result.  It drives rt_reproject_variance_host and rt_temporal_blend_variance_host on frames
// of 23 x 11 and 2 x 2 pixels (buffers of exactly the sizes the calls name) with the records, sums and counts of tests/reproject_san_main.cpp
// and hostile variances (NaN, +-inf, negative, -0.0, denormal, huge), checks what must hold of any result — the sums and counts are
// rt_reproject_host's, every variance is known or +inf, +0.0 exactly where there is no history — and goes through the arguments it has to
// refuse.  Exit status 0 and "ok" on stdout: every run returned what it should.
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

// (rt_host.cpp's, in the library: the construction of tests/reproject_san_main.cpp — this program needs a camera's fields, not their last bit)
extern "C" void rt_camera_fields(const rt_camera* c, double out21[21]) {
    double a[15];
    std::memcpy(a, c, sizeof(a));
    const double* from = a; const double* at = a + 3; const double* vup = a + 6;
    const double vfov = a[9], aspect = a[10], aperture = a[11], focus = a[12];
    const double hh = std::tan(vfov * 3.14159265358979323846 / 180.0 / 2.0), vh = 2.0 * hh, vw = aspect * vh;
    double w[3] = {from[0] - at[0], from[1] - at[1], from[2] - at[2]};
    const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (double& x : w) x /= wl;
    double u[3] = {vup[1] * w[2] - vup[2] * w[1], vup[2] * w[0] - vup[0] * w[2], vup[0] * w[1] - vup[1] * w[0]};
    const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (double& x : u) x /= ul;
    const double v[3] = {w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]};
    for (int k = 0; k < 3; k++) {
        out21[k] = from[k];
        out21[6 + k] = focus * vw * u[k];
        out21[9 + k] = focus * vh * v[k];
        out21[3 + k] = from[k] - out21[6 + k] / 2.0 - out21[9 + k] / 2.0 - focus * w[k];
        out21[12 + k] = u[k]; out21[15 + k] = v[k];
    }
    out21[18] = aperture / 2.0; out21[19] = a[13]; out21[20] = a[14];
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                                   // xorshift64*: any deterministic stream will do
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
static bool known(double v) { return v - v == 0.0 && v >= 0.0; }
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    rt_camera cam;
    {
        const double a[15] = {0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 60.0, 23.0 / 11.0, 0.0, 10.0, 0.0, 1.0};
        static_assert(sizeof(rt_camera) == sizeof(a), "rt_camera is fifteen doubles");
        std::memcpy(&cam, a, sizeof(a));
    }
    const uint32_t sizes[2][2] = {{23, 11}, {2, 2}};
    const uint32_t caps[3] = {0u, 5u, 0x7FFFFFFFu};
    int runs = 0;
    for (const auto& wh : sizes) for (int with_counts = 0; with_counts < 2; with_counts++) for (uint32_t cap : caps) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        std::vector<double> sum(n * 3), var(n * 3), prev(n * 16, 0.0), cur(n * 16, 0.0), hsum(n * 3, -7.0), hvar(n * 3, -7.0), psum(n * 3, -7.0);
        std::vector<uint32_t> cnt(n), hcnt(n, 7u), pcnt(n, 7u);
        for (size_t p = 0; p < n; p++) {
            cnt[p] = p % 13 == 0 ? 0u : (p % 17 == 0 ? 0xFFFFFFFFu : (p % 5 == 0 ? 1u : 1u + (uint32_t)(40.0 * uniform())));
            for (int k = 0; k < 3; k++) { sum[3 * p + k] = 4.0 * uniform() * (double)cnt[p]; var[3 * p + k] = 2.0 * uniform() / (double)(cnt[p] ? cnt[p] : 1u); }
            if (p % 19 == 0) sum[3 * p] = nan;
            if (p % 23 == 0) sum[3 * p + 1] = p % 2 ? inf : -inf;
            if (p % 29 == 0) sum[3 * p + 2] = -0.0;
            if (p % 7 == 0) var[3 * p] = nan;
            if (p % 11 == 1) var[3 * p + 1] = p % 2 ? inf : -inf;
            if (p % 13 == 2) var[3 * p + 2] = -0.5;
            if (p % 17 == 3) { var[3 * p] = -0.0; var[3 * p + 1] = 5e-324; var[3 * p + 2] = 1e300; }
            for (std::vector<double>* recs : {&prev, &cur}) {
                double* r = recs->data() + p * 16;
                if (uniform() < 0.1) { for (int k = 11; k < 15; k++) r[k] = -1.0; continue; }           // a miss
                // a point on a wall z = -5 in front of the camera, spread so that it projects inside, on the edge of and outside the frame
                r[0] = 1.0; r[1] = 5.0;
                r[2] = 16.0 * uniform() - 8.0; r[3] = 8.0 * uniform() - 4.0; r[4] = -5.0;
                r[5] = 0.0; r[6] = 0.0; r[7] = 1.0; r[8] = 1.0;
                r[11] = 2.0; r[12] = uniform() < 0.9 ? 3.0 : 4.0; r[13] = 0.0; r[14] = 3.0;
                const double h = uniform();
                if (h < 0.03) r[12] = -1.0;
                else if (h < 0.06) { r[5] = 0.0; r[6] = 0.0; r[7] = 0.0; }
                else if (h < 0.09) r[2] = nan;
                else if (h < 0.12) r[3] = p % 2 ? inf : -inf;
                else if (h < 0.15) r[4] = 5.0;                                                        // behind the camera
                else if (h < 0.18) { r[2] = 1e300; r[3] = -1e300; }
                else if (h < 0.21) r[7] = 0.5;
            }
        }
        const double sigma[2] = {0.9, with_counts ? 0.01 : inf};
        const uint32_t* counts = with_counts ? cnt.data() : nullptr;
        if (rt_reproject_variance_host(sum.data(), counts, 9, var.data(), prev.data(), &cam, cur.data(), W, H, cap, sigma, 0, hsum.data(), hcnt.data(), hvar.data()) != 0 ||
            rt_reproject_host(sum.data(), counts, 9, prev.data(), &cam, cur.data(), W, H, cap, sigma, 0, psum.data(), pcnt.data()) != 0) {
            std::printf("failed: %s\n", g_message.c_str()); return 1;
        }
        size_t with_history = 0, with_known = 0, with_unknown = 0;
        for (size_t p = 0; p < n; p++) {
            bool ok = hcnt[p] == pcnt[p] && hcnt[p] <= cap;
            for (int k = 0; k < 3; k++) {
                const double v = hvar[3 * p + k];
                ok = ok && same_bits(hsum[3 * p + k], psum[3 * p + k]) && (known(v) || v == inf) && (hcnt[p] != 0u || same_bits(v, 0.0));
                ok = ok && (v == inf) == (hvar[3 * p] == inf);                                      // a pixel's variance is known in all channels or in none
            }
            if (!ok) { std::printf("pixel %zu of %u x %u, cap %u: not what any history can be\n", p, W, H, cap); return 1; }
            with_history += hcnt[p] != 0u; with_known += hcnt[p] != 0u && hvar[3 * p] != inf; with_unknown += hcnt[p] != 0u && hvar[3 * p] == inf;
        }
        if (cap == 0u && with_history) { std::printf("max_history 0 gave history\n"); return 1; }
        if (cap != 0u && W > 2u && (with_known < n / 16 || with_unknown < 2)) {
            std::printf("%u x %u, cap %u: %zu pixels with known and %zu with unknown history variance\n", W, H, cap, with_known, with_unknown); return 1;
        }
        // the blend, out of place and in place, with and without a variance frame
        std::vector<double> out(n * 3, -7.0), none(n * 3, -7.0), frame(var);
        std::vector<uint32_t> frame_n(n);
        for (size_t p = 0; p < n; p++) frame_n[p] = p % 6 == 0 ? 0u : (p % 31 == 0 ? 0xFFFFFFFFu : 4u);
        if (rt_temporal_blend_variance_host(frame.data(), with_counts ? frame_n.data() : nullptr, 4, hvar.data(), hcnt.data(), n, out.data()) != 0 ||
            rt_temporal_blend_variance_host(nullptr, with_counts ? frame_n.data() : nullptr, 4, hvar.data(), hcnt.data(), n, none.data()) != 0 ||
            rt_temporal_blend_variance_host(frame.data(), with_counts ? frame_n.data() : nullptr, 4, hvar.data(), hcnt.data(), n, frame.data()) != 0) {
            std::printf("blend failed: %s\n", g_message.c_str()); return 1;
        }
        for (size_t i = 0; i < 3 * n; i++) {
            const size_t p = i / 3;
            const uint64_t N = with_counts ? frame_n[p] : 4u;
            bool ok = (known(out[i]) || out[i] == inf) && (known(none[i]) || none[i] == inf) && same_bits(out[i], frame[i]);
            if (hcnt[p] == 0u) ok = ok && none[i] == inf && (N > 0u && known(var[i]) ? same_bits(out[i], var[i]) : out[i] == inf);
            else if (N == 0u) ok = ok && same_bits(out[i], hvar[i]) && same_bits(none[i], hvar[i]);
            else ok = ok && (none[i] == inf) == (hvar[i] == inf) && (out[i] == inf) == (hvar[i] == inf && !known(var[i]));
            if (!ok) { std::printf("double %zu: not what the blend of variances can be\n", i); return 1; }
        }
        runs++;
    }
    // what has to be refused, with a message and without a write
    double s[12] = {0.0}, g[64] = {0.0}, hs[12], hv[12];
    uint32_t c4[4] = {1, 1, 1, 1}, hc[4] = {7, 7, 7, 7};
    for (double& x : hs) x = 7.0;
    for (double& x : hv) x = 7.0;
    const double good[2] = {0.9, 0.01}, bad_n[2] = {1.5, 0.01}, bad_p[2] = {0.9, 0.0}, nan_n[2] = {nan, 0.01}, nan_p[2] = {0.9, nan};
    int refused = 0;
    refused += rt_reproject_variance_host(nullptr, c4, 0, s, g, &cam, g, 2, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, nullptr, g, &cam, g, 2, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, nullptr, &cam, g, 2, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, nullptr, g, 2, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, nullptr, 2, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, nullptr, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, good, 0, nullptr, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, good, 0, hs, nullptr, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, good, 0, hs, hc, nullptr) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 1, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 1, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 65536, 32768, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 0x80000000u, good, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, bad_n, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, nan_n, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, bad_p, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, nan_p, 0, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, good, 1, hs, hc, hv) != 0;
    refused += rt_reproject_variance_host(s, nullptr, 0, s, g, &cam, g, 2, 2, 8, good, 0, hs, hc, hv) != 0;
    refused += rt_temporal_blend_variance_host(s, c4, 0, nullptr, c4, 4, hv) != 0;
    refused += rt_temporal_blend_variance_host(s, c4, 0, s, nullptr, 4, hv) != 0;
    refused += rt_temporal_blend_variance_host(s, c4, 0, s, c4, 4, nullptr) != 0;
    refused += rt_temporal_blend_variance_host(s, c4, 0, s, c4, 0x80000000ull, hv) != 0;
    bool untouched = true;
    for (double x : hs) untouched = untouched && x == 7.0;
    for (double x : hv) untouched = untouched && x == 7.0;
    for (uint32_t x : hc) untouched = untouched && x == 7u;
    if (refused != 23 || g_message.empty() || !untouched) { std::printf("arguments: %d of 23 refused\n", refused); return 1; }
    if (rt_reproject_variance_host(s, c4, 0, s, g, &cam, g, 2, 2, 8, good, 0, hs, hc, hv) != 0 || hs[0] != 0.0 || hc[3] != 0u || hv[11] != 0.0) {
        std::printf("all-zero records are not misses\n"); return 1;
    }
    std::printf("ok %d runs, %d refusals\n", runs, refused);
    return 0;
}

// tests/reproject_var_mirror_main.cpp — the C++ mirror of temporal variance (include/raytracinginrust.hpp: rtr::reproject_variance,
// rtr::temporal_blend_variance, rtr::Progressive::history_variance / rgb8_temporal_variance), compiled against librt_amd.so by
// tests/test_reproject_var_mirrors.py.
//   reproject_var_mirror host   no device: rtr::temporal_blend_variance on known numbers, one per row of (BV)'s table; rtr::reproject_variance(host =
//                               true) on records that all miss, and on a wall seen twice by the same camera with prev_var = 2 / 4 in every pixel
//                               (the per-sample variance 2 comes back over the history's count), and with one channel of every pixel unknown; what both refuse
//   reproject_var_mirror gpu    a checker ground and two spheres, 23 x 11, two views: rtr::reproject_variance word for word its host form; a
//                               progressive frame with moments through set_view: history_variance() is the host form on (BV) of variance(), and
//                               rgb8_temporal_variance() is the counts-aware resolve of denoise_frame over the two blends
// Exit status 0 and "ok" on stdout: everything was what it should be.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "../include/raytracinginrust.hpp"

using namespace rtr;

static int fail(const char* what) { std::printf("failed: %s\n", what); return 1; }
static bool same_words(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}
static bool same(const HistoryVariance& a, const HistoryVariance& b) {
    return same_words(a.history.sum, b.history.sum) && a.history.counts == b.history.counts && same_words(a.var, b.var);
}

static int host() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // (BV): pixel by pixel one row of the table; N = 4 unless counts say otherwise
    {
        const std::vector<uint32_t> counts = {4, 0, 4, 4, 4, 4}, hist_counts = {0, 12, 12, 12, 12, 12};
        std::vector<double> var(18, 0.5), hist_var(18, 0.25);
        for (int k = 0; k < 3; k++) { var[9 + k] = nan; hist_var[12 + k] = inf; var[15 + k] = -1.0; hist_var[15 + k] = nan; }
        const std::vector<double> out = temporal_blend_variance(&var, &counts, 0, hist_var, hist_counts);
        const double want[6] = {0.5, 0.25, (16.0 * 0.5 + 144.0 * 0.25) / 256.0, (0.25 * 12.0) / 16.0, (0.5 * 4.0) / 16.0, inf};
        for (int p = 0; p < 6; p++) for (int k = 0; k < 3; k++) if (out[3 * p + k] != want[p]) return fail("temporal_blend_variance: known numbers");
        const std::vector<double> none = temporal_blend_variance(nullptr, nullptr, 4, hist_var, hist_counts);
        if (none[0] != inf || none[3] != 0.25 * 12.0 / 16.0 || none[12] != inf) return fail("temporal_blend_variance without a variance frame");
        try { std::vector<double> bad(17, 0.0); temporal_blend_variance(&bad, nullptr, 4, hist_var, hist_counts); return fail("a variance of another size accepted"); } catch (const Error&) {}
    }
    const uint32_t W = 4, H = 3; const size_t n = (size_t)W * H;
    std::vector<double> frame(n * 3, 1.25), var(n * 3, 0.5);
    const Camera cam = Camera::new_(Point3(0.0, 0.0, 0.0), Point3(0.0, 0.0, -1.0), Vec3(0.0, 1.0, 0.0), 60.0, (double)W / H, 0.0, 10.0, 0.0, 1.0);
    std::vector<double> miss(n * 16, 0.0);
    HistoryVariance e = reproject_variance(frame, nullptr, 4, var, miss, cam, miss, W, H, ReprojectSettings(), true);
    for (size_t p = 0; p < n; p++) if (e.history.counts[p] != 0u || e.history.sum[p * 3] != 0.0 || e.var[p * 3 + 2] != 0.0) return fail("records that miss gave history");
    // the wall of tests/reproject_mirror_main.cpp: every pixel's place in the previous view is its own centre up to rounding
    double f[21]; rt_camera_fields(&cam.c, f);
    std::vector<double> wall(n * 16, 0.0);
    for (uint32_t r = 0; r < H; r++) for (uint32_t i = 0; i < W; i++) {
        double* g = &wall[((size_t)r * W + i) * 16];
        const double s = ((double)i + 0.5) / (W - 1), t = ((double)(H - 1 - r) + 0.5) / (H - 1);
        double dir[3];
        for (int k = 0; k < 3; k++) dir[k] = f[3 + k] + s * f[6 + k] + t * f[9 + k] - f[k];
        const double tt = -5.0 / dir[2];
        g[0] = 1.0; g[1] = tt; g[2] = dir[0] * tt; g[3] = dir[1] * tt; g[4] = -5.0; g[7] = 1.0; g[8] = 1.0; g[11] = 0.0; g[12] = 0.0;
    }
    ReprojectSettings r8; r8.max_history = 8;
    e = reproject_variance(frame, nullptr, 4, var, wall, cam, wall, W, H, r8, true);
    const History plain = reproject(frame, nullptr, 4, wall, cam, wall, W, H, r8, true);
    if (!same_words(e.history.sum, plain.sum) || e.history.counts != plain.counts) return fail("reproject_variance's sums and counts are not reproject's");
    size_t kept = 0;
    for (size_t p = 0; p < n; p++) {
        if (e.history.counts[p] != 3u && e.history.counts[p] != 4u) return fail("a wall seen twice by one camera: the count");
        for (int k = 0; k < 3; k++) {
            const double v = e.var[p * 3 + k];
            // per-sample variance 0.5 * 4 = 2 over 3 or 4 samples; a neighbour's share of about 1e-16 changes nothing that 1e-9 sees
            const double want = 2.0 / (double)e.history.counts[p];
            if (!(v > want - 1e-9 && v < want + 1e-9)) return fail("a wall seen twice by one camera: the variance");
        }
        kept++;
    }
    // one unknown channel makes a tap var-unknown: with one in every pixel no pixel's history knows its variance
    for (size_t p = 0; p < n; p++) var[p * 3 + p % 3] = p % 2 ? -1.0 : nan;
    e = reproject_variance(frame, nullptr, 4, var, wall, cam, wall, W, H, r8, true);
    for (size_t i = 0; i < n * 3; i++) if (e.var[i] != inf) return fail("an unknown variance came back known");
    if (!same_words(e.history.sum, plain.sum)) return fail("the variances changed the sums");
    for (size_t p = 0; p < n; p++) var[p * 3 + p % 3] = 0.5;
    try { std::vector<double> bad(n * 3 - 1, 0.0); reproject_variance(frame, nullptr, 4, bad, wall, cam, wall, W, H, r8, true); return fail("a variance of another size accepted"); } catch (const Error&) {}
    try { reproject_variance(frame, nullptr, 0, var, wall, cam, wall, W, H, r8, true); return fail("prev_samples = 0 without counts accepted"); } catch (const Error&) {}
    std::printf("ok host, %zu pixels kept\n", kept);
    return 0;
}

static int gpu() {
    const uint32_t W = 23, H = 11; const uint64_t seed = 0x5EED + 31;
    const size_t n = (size_t)W * H;
    Scene s;
    HittableList world(s);
    Material ground = Lambertian::new_(s, CheckTexture::new_(s, ConstantTexture::new_(s, Color(0.2, 0.3, 0.1)), ConstantTexture::new_(s, Color(0.9, 0.9, 0.9))));
    world.push(Sphere::new_(s, Point3(0.0, -1000.0, 0.0), 1000.0, ground));
    world.push(Sphere::new_(s, Point3(0.0, 1.0, 0.0), 1.0, Lambertian::new_(s, ConstantTexture::new_(s, Color(0.7, 0.2, 0.2)))));
    world.push(Sphere::new_(s, Point3(2.0, 0.8, -1.8), 0.8, Metal::new_(s, Color(0.8, 0.8, 0.8), 0.1)));
    s.set(world, {});
    const Camera cam = Camera::new_(Point3(7.0, 2.5, 5.0), Point3(0.0, 0.8, 0.0), Vec3(0.0, 1.0, 0.0), 30.0, (double)W / H, 0.0, 8.9, 0.0, 1.0);
    const Camera cam2 = Camera::new_(Point3(6.7, 2.5, 5.4), Point3(0.0, 0.8, 0.0), Vec3(0.0, 1.0, 0.0), 30.0, (double)W / H, 0.0, 8.9, 0.0, 1.0);
    const Color bg(0.7, 0.8, 1.0);
    const std::vector<double> g0 = query_camera_records(s, cam, W, H, 0, seed), g1 = query_camera_records(s, cam2, W, H, 0, seed + 1);
    ReprojectSettings r; r.max_history = 24;
    Progressive frame(s, cam, bg, W, H, 8, seed);
    frame.enable_moments();
    frame.add(2); frame.add(2);
    const std::vector<double> sums = frame.sum(), var = frame.variance();
    const HistoryVariance want = reproject_variance(sums, nullptr, 4, var, g0, cam, g1, W, H, r, true);
    if (!same(reproject_variance(sums, nullptr, 4, var, g0, cam, g1, W, H, r), want)) return fail("rtr::reproject_variance on the device is not the host twin's");
    size_t held = 0;
    for (size_t p = 0; p < n; p++) held += want.history.counts[p] != 0u && want.var[3 * p] != std::numeric_limits<double>::infinity();
    if (held < n / 10) return fail("the two views test nothing");
    // the progressive frame through the move: (BV) with a history that is not there hands the frame's variance on
    frame.set_view(cam2, seed + 1, r);
    const std::vector<double> zeros(n * 3, 0.0); const std::vector<uint32_t> zeros_n(n, 0u);
    const HistoryVariance h = reproject_variance(sums, nullptr, 4, temporal_blend_variance(&var, nullptr, 4, zeros, zeros_n), g0, cam, g1, W, H, r, true);
    if (!same_words(frame.history_variance(), h.var) || !same_words(frame.history().sum, h.history.sum)) return fail("history_variance() is not rtr::reproject_variance of the frame");
    frame.add(2);                                                   // one pass: the frame has no variance of its own
    const History b = temporal_blend(frame.sum(), nullptr, 2, h.history, W, H);
    const std::vector<double> bv = temporal_blend_variance(nullptr, nullptr, 2, h.var, h.history.counts);
    DenoiseVarianceSettings dv;
    std::vector<double> den(n * 3);
    if (rt_denoise_frame_host(b.sum.data(), b.counts.data(), 0, bv.data(), nullptr, 1, g1.data(), W, H, dv.iterations, dv.sigma, dv.flags, den.data(), nullptr) != 0)
        throw Error(rt_last_error());
    std::vector<uint8_t> image(n * 3);
    if (rt_adaptive_resolve_rgb8_host(den.data(), b.counts.data(), W, H, nullptr, image.data(), nullptr) != 0) throw Error(rt_last_error());
    if (frame.rgb8_temporal_variance(dv) != image) return fail("rgb8_temporal_variance() after one pass");
    frame.reset();
    for (double v : frame.history_variance()) if (v != 0.0) return fail("reset kept the history variance");
    Progressive plain(s, cam, bg, W, H, 8, seed);
    plain.add(2);
    try { plain.rgb8_temporal_variance(dv); return fail("a frame without moments resolved through the variance stop"); } catch (const Error&) {}
    try { plain.history_variance(); return fail("a frame without moments has a history variance"); } catch (const Error&) {}
    std::printf("ok gpu, %zu pixels with a known history variance\n", held);
    return 0;
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "host";
        return mode == "gpu" ? gpu() : host();
    } catch (const Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}

// tests/reproject_mirror_main.cpp — the C++ mirror of temporal accumulation (include/raytracinginrust.hpp: rtr::reproject,
// rtr::temporal_blend, rtr::Progressive::set_view / history / rgb8_temporal), compiled against librt_amd.so by tests/test_reproject_mirrors.py.
//   reproject_mirror host   no device: rtr::temporal_blend on known numbers; rtr::reproject(host = true) on records that all miss, and on a
//                           wall seen twice by the same camera (every pixel's point is the pixel centre's: the history is the frame), and
//                           what both refuse
//   reproject_mirror gpu    a checker ground and two spheres, 23 x 11, two views: rtr::reproject word for word rtr::reproject(host = true);
//                           a progressive frame through set_view: history() is rtr::reproject(host) of sum(), and rgb8_temporal() is the
//                           counts-aware resolve of rtr::temporal_blend — with 0 new samples and with 4
// Exit status 0 and "ok" on stdout: everything was what it should be.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/raytracinginrust.hpp"

using namespace rtr;

static int fail(const char* what) { std::printf("failed: %s\n", what); return 1; }
static bool same(const History& a, const History& b) {
    return a.sum.size() == b.sum.size() && a.counts == b.counts && std::memcmp(a.sum.data(), b.sum.data(), a.sum.size() * sizeof(double)) == 0;
}

static int host() {
    const uint32_t W = 4, H = 3; const size_t n = (size_t)W * H;
    History h; h.sum.assign(n * 3, 0.5); h.counts.assign(n, 2u); h.counts[5] = 0xFFFFFFFFu;
    std::vector<double> frame(n * 3, 1.25);
    const History b = temporal_blend(frame, nullptr, 4, h, W, H);
    for (size_t p = 0; p < n; p++) if (b.sum[p * 3 + 1] != 1.75 || b.counts[p] != (p == 5 ? 0xFFFFFFFFu : 6u)) return fail("temporal_blend: known numbers");
    std::vector<uint32_t> counts(n, 1u);
    if (temporal_blend(frame, &counts, 0, h, W, H).counts[0] != 3u) return fail("temporal_blend with counts");
    try { temporal_blend(frame, nullptr, 4, h, W, H + 1); return fail("a frame of another size accepted"); } catch (const Error&) {}
    // all misses: an empty history
    const Camera cam = Camera::new_(Point3(0.0, 0.0, 0.0), Point3(0.0, 0.0, -1.0), Vec3(0.0, 1.0, 0.0), 60.0, (double)W / H, 0.0, 10.0, 0.0, 1.0);
    std::vector<double> miss(n * 16, 0.0);
    History e = reproject(frame, nullptr, 4, miss, cam, miss, W, H, ReprojectSettings(), true);
    for (size_t p = 0; p < n; p++) if (e.counts[p] != 0u || e.sum[p * 3] != 0.0) return fail("records that miss gave history");
    // a wall at z = -5 whose records sit on the rays of the pixels' centres (the jitter's mean): s = (i + 0.5) / (W - 1), t = (j + 0.5) / (H - 1), j from the bottom row
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
    for (size_t p = 0; p < n; p++) for (int k = 0; k < 3; k++) frame[p * 3 + k] = 4.0 * (double)(p + 1);
    ReprojectSettings r8; r8.max_history = 8;
    e = reproject(frame, nullptr, 4, wall, cam, wall, W, H, r8, true);
    size_t kept = 0;
    for (size_t p = 0; p < n; p++) {
        // the place is the pixel's own centre up to rounding, so the footprint's weight is 1 up to rounding: 3 or 4 samples' worth of the pixel's own
        // mean (p + 1), or a neighbour's share of about 1e-16 beside it
        if (e.counts[p] != 3u && e.counts[p] != 4u) return fail("a wall seen twice by one camera: the count");
        const double mean = e.sum[p * 3] / (double)e.counts[p];
        if (!(mean > (double)(p + 1) - 1e-9 && mean < (double)(p + 1) + 1e-9)) return fail("a wall seen twice by one camera: the mean");
        kept++;
    }
    try { ReprojectSettings bad; bad.sigma[0] = 1.5; reproject(frame, nullptr, 4, wall, cam, wall, W, H, bad, true); return fail("normal_min = 1.5 accepted"); } catch (const Error&) {}
    try { reproject(frame, nullptr, 0, wall, cam, wall, W, H, r8, true); return fail("prev_samples = 0 without counts accepted"); } catch (const Error&) {}
    std::printf("ok host, %zu pixels kept\n", kept);
    return 0;
}

static int gpu() {
    const uint32_t W = 23, H = 11; const uint64_t seed = 0x5EED + 31;
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
    const std::vector<double> sums = render(s, cam, bg, W, H, 4, 8, seed);
    ReprojectSettings r; r.max_history = 24;
    const History want = reproject(sums, nullptr, 4, g0, cam, g1, W, H, r, true);
    if (!same(reproject(sums, nullptr, 4, g0, cam, g1, W, H, r), want)) return fail("rtr::reproject on the device is not the host twin's");
    size_t held = 0;
    for (uint32_t c : want.counts) held += c != 0u;
    if (held < 50 || held == (size_t)W * H) return fail("the two views test nothing");
    // a progressive frame
    Progressive frame(s, cam, bg, W, H, 8, seed);
    frame.add(4);
    const std::vector<double> before = frame.sum();
    frame.set_view(cam2, seed + 1, r);
    const History h = frame.history();
    if (!same(h, reproject(before, nullptr, 4, g0, cam, g1, W, H, r, true))) return fail("history() is not rtr::reproject of sum()");
    if (frame.samples() != 0) return fail("the moved frame holds samples");
    auto resolved = [&](const History& b) {
        std::vector<uint8_t> out((size_t)W * H * 3);
        if (rt_adaptive_resolve_rgb8_host(b.sum.data(), b.counts.data(), W, H, nullptr, out.data(), nullptr) != 0) throw Error(rt_last_error());
        return out;
    };
    const std::vector<double> zeros((size_t)W * H * 3, 0.0);
    if (frame.rgb8_temporal() != resolved(temporal_blend(zeros, nullptr, 0, h, W, H))) return fail("rgb8_temporal() with 0 samples");
    frame.add(4);
    if (frame.rgb8_temporal() != resolved(temporal_blend(frame.sum(), nullptr, 4, h, W, H))) return fail("rgb8_temporal() with 4 samples");
    frame.reset();
    for (uint32_t c : frame.history().counts) if (c != 0u) return fail("reset kept the history");
    try { frame.rgb8_temporal(); return fail("a frame with neither samples nor history resolved"); } catch (const Error&) {}
    std::printf("ok gpu, %zu pixels with history\n", held);
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

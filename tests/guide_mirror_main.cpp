// tests/guide_mirror_main.cpp — the C++ mirror of the averaged guide (include/raytracinginrust.hpp: rtr::guide_from_hits,
// rtr::query_camera_guide, rtr::Progressive::set_guide_samples / guide_info), compiled against librt_amd.so by tests/test_guide_cpp_gpu.py.
//   guide_mirror host   no device: rtr::guide_from_hits on three stacked records of two pixels, the known answers of the specification
//   guide_mirror gpu    a checker ground and two spheres behind a thin lens, 23 x 11: rtr::query_camera_guide (with its albedo output) word
//                       for word rtr::guide_from_hits of the stacked rtr::query_camera_records and rtr::query_camera_albedo; a progressive
//                       frame with set_guide_samples(3) resolves to format_color of rtr::denoise_host on that guide, builds it once, and
//                       refuses 0
// Exit status 0 and "ok" on stdout: everything was what it should be.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/raytracinginrust.hpp"

using namespace rtr;

static int fail(const char* what) { std::printf("failed: %s\n", what); return 1; }
static bool same_words(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static int host() {
    // pixel 0: samples 0 and 2 hit (materials 3 and 4), sample 1 misses; pixel 1: only sample 1 hits, a medium
    std::vector<double> st(3 * 2 * 16, 0.0);
    auto rec = [&](int s, int p) { return &st[((size_t)s * 2 + p) * 16]; };
    for (int s = 0; s < 3; s++) for (int p = 0; p < 2; p++) for (int k = 11; k < 15; k++) rec(s, p)[k] = -1.0;
    double* r = rec(0, 0); r[0] = 1.0; r[1] = 2.0; r[2] = 1.0; r[5] = 1.0; r[8] = 1.0; r[11] = 3.0; r[12] = 6.0;
    r = rec(2, 0); r[0] = 1.0; r[1] = 4.0; r[2] = 3.0; r[6] = 1.0; r[11] = 4.0; r[12] = 6.0;
    r = rec(1, 1); r[0] = 1.0; r[1] = 8.0; r[4] = -0.0; r[5] = 1.0; r[12] = 2.0;
    const std::vector<double> g = guide_from_hits(st, 3, 2);
    const double want0[16] = {1.0, 3.0, 2.0, 0.0, 0.0, 0.5, 0.5, 0.0, 0.5, 0.0, 0.0, -1.0, 6.0, -1.0, -1.0, 2.0};
    const double want1[16] = {0.0, 8.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 2.0, -1.0, -1.0, 1.0};
    if (g.size() != 32 || std::memcmp(&g[0], want0, sizeof(want0)) != 0 || std::memcmp(&g[16], want1, sizeof(want1)) != 0) return fail("guide_from_hits: known answers");
    try { guide_from_hits(st, 0, 2); return fail("n_samples = 0 accepted"); } catch (const Error&) {}
    try { guide_from_hits(st, 2, 2); return fail("a stack of another size accepted"); } catch (const Error&) {}
    std::printf("ok host\n");
    return 0;
}

static int gpu() {
    const uint32_t W = 23, H = 11; const uint64_t seed = 0x5EED + 5;
    Scene s;
    HittableList world(s);
    Material ground = Lambertian::new_(s, CheckTexture::new_(s, ConstantTexture::new_(s, Color(0.2, 0.3, 0.1)), ConstantTexture::new_(s, Color(0.9, 0.9, 0.9))));
    world.push(Sphere::new_(s, Point3(0.0, -1000.0, 0.0), 1000.0, ground));
    world.push(Sphere::new_(s, Point3(0.0, 1.0, 0.0), 1.0, Lambertian::new_(s, ConstantTexture::new_(s, Color(0.7, 0.2, 0.2)))));
    world.push(Sphere::new_(s, Point3(2.0, 0.8, -1.8), 0.8, Metal::new_(s, Color(0.8, 0.8, 0.8), 0.1)));
    s.set(world, {});
    const Camera cam = Camera::new_(Point3(7.0, 2.5, 5.0), Point3(0.0, 0.8, 0.0), Vec3(0.0, 1.0, 0.0), 30.0, (double)W / H, 0.6, 8.9, 0.0, 1.0);
    std::vector<double> stack;
    for (uint32_t k = 1; k <= 3; k++) { const std::vector<double> one = query_camera_records(s, cam, W, H, k, seed); stack.insert(stack.end(), one.begin(), one.end()); }
    const std::vector<double> want = guide_from_hits(stack, 3, (uint64_t)W * H);
    std::vector<double> alb;
    const std::vector<double> fused = query_camera_guide(s, cam, W, H, 1, 3, seed, &alb);
    if (!same_words(query_camera_guide(s, cam, W, H, 1, 3, seed), want) || !same_words(fused, want)) return fail("query_camera_guide is not guide_from_hits of the stacked records");
    if (!same_words(alb, query_camera_albedo(s, cam, W, H, 1, 3, seed))) return fail("the fused albedo sums are not query_camera_albedo's");
    size_t partial = 0;
    for (size_t p = 0; p < (size_t)W * H; p++) partial += want[p * 16 + 15] > 0.0 && want[p * 16 + 15] < 3.0;
    if (partial == 0) return fail("no partly covered pixel: the view tests nothing");
    // a progressive frame
    const Color bg(0.7, 0.8, 1.0);
    Progressive frame(s, cam, bg, W, H, 8, seed);
    if (frame.guide_info().guide_samples != 1u || frame.guide_info().builds != 0u) return fail("a new frame's guide_info");
    frame.set_guide_samples(3);
    try { frame.set_guide_samples(0); return fail("guide_samples = 0 accepted"); } catch (const Error&) {}
    frame.add(4);
    const std::vector<uint8_t> img = frame.rgb8_denoised();
    if (frame.guide_info().guide_samples != 3u || frame.guide_info().builds != 1u) return fail("guide_info after the first denoised resolve");
    std::vector<double> stack0;
    for (uint32_t k = 0; k < 3; k++) { const std::vector<double> one = query_camera_records(s, cam, W, H, k, seed); stack0.insert(stack0.end(), one.begin(), one.end()); }
    const std::vector<double> filtered = denoise_host(frame.sum(), frame.samples(), guide_from_hits(stack0, 3, (uint64_t)W * H), W, H);
    for (size_t p = 0; p < (size_t)W * H; p++) {
        uint64_t c[3]; rt_format_color(&filtered[p * 3], frame.samples(), c);
        for (int k = 0; k < 3; k++) if (img[p * 3 + k] != (uint8_t)c[k]) return fail("the progressive resolve is not format_color of denoise_host on the averaged guide");
    }
    frame.rgb8_denoised();
    if (frame.guide_info().builds != 1u) return fail("the guide was built twice");
    std::printf("ok gpu, %zu partly covered pixels\n", partial);
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

// tests/chain_mirror_main.cpp — the C++ mirror of the specular-chain guides (include/raytracinginrust.hpp: rtr::query_chain,
// rtr::query_camera_chain_guide, rtr::Progressive::set_guide_chain), compiled against librt_amd.so by tests/test_chain_mirrors.py.
//   chain_mirror host   no device: rt_chain_step_host on a mirror, a known answer
//   chain_mirror gpu    a checker ground, a mirror ball, a glass ball and a diffuse ball, 23 x 11: rtr::query_chain word for word the chain
//                       composed here link by link from rt_query_albedo (records and albedo of link l, seed_link) and rt_chain_step_host —
//                       entry points that tests/test_albedo_query_gpu.py and tests/test_chain_host.py pin; max_links = 0 is
//                       rtr::query_camera_records; rtr::query_camera_chain_guide of one sample carries the same links; a progressive frame
//                       with set_guide_chain(4) resolves to format_color of rtr::denoise_host on that guide
// Exit status 0 and "ok" on stdout: everything was what it should be.
#include <cmath>
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
    Scene s;
    HittableList world(s);
    world.push(Sphere::new_(s, Point3(0.0, 0.0, 0.0), 1.0, Metal::new_(s, Color(0.9, 0.8, 0.7), 0.0)));      // material 0
    s.set(world, {});
    const double ray[7] = {0.0, 0.0, -5.0, 0.0, 0.0, 2.0, 0.25};
    double rec[16] = {1.0, 2.0, 0.0, 0.0, -1.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
    double next[7], w[3]; uint32_t status = 9;
    if (rt_chain_step_host(s.raw(), 1, ray, rec, 0.0, next, w, &status) != 0) return fail(rt_last_error());
    const double want[7] = {0.0, 0.0, -1.0, 0.0, 0.0, -1.0, 0.25};
    if (status != 0u || std::memcmp(next, want, sizeof(want)) != 0 || w[0] != 0.9 || w[1] != 0.8 || w[2] != 0.7) return fail("the mirror's known answer");
    rec[0] = 0.0;
    if (rt_chain_step_host(s.raw(), 1, ray, rec, 0.0, next, w, &status) != 0 || status != 2u || std::memcmp(next, ray, sizeof(ray)) != 0 || w[0] != 1.0) return fail("a miss");
    if (rt_chain_step_host(s.raw(), 1, ray, rec, -1.0, next, w, &status) == 0) return fail("max_fuzz = -1 accepted");
    std::printf("ok host\n");
    return 0;
}

static int gpu() {
    const uint32_t W = 23, H = 11, n = W * H, L = 4; const uint64_t seed = 0x5EED + 7; const double t_min = 1e-5;
    Scene s;
    HittableList world(s);
    Material ground = Lambertian::new_(s, CheckTexture::new_(s, ConstantTexture::new_(s, Color(0.2, 0.3, 0.1)), ConstantTexture::new_(s, Color(0.9, 0.9, 0.9))));
    world.push(Sphere::new_(s, Point3(0.0, -1000.0, 0.0), 1000.0, ground));
    world.push(Sphere::new_(s, Point3(0.0, 1.0, 0.0), 1.0, Metal::new_(s, Color(0.9, 0.8, 0.7), 0.0)));
    world.push(Sphere::new_(s, Point3(-2.2, 1.0, 1.5), 1.0, Dielectric::new_(s, 1.5)));
    world.push(Sphere::new_(s, Point3(2.0, 0.8, -1.8), 0.8, Lambertian::new_(s, ConstantTexture::new_(s, Color(0.7, 0.2, 0.2)))));
    s.set(world, {});
    const Camera cam = Camera::new_(Point3(7.0, 2.5, 5.0), Point3(0.0, 0.8, 0.0), Vec3(0.0, 1.0, 0.0), 30.0, (double)W / H, 0.0, 8.9, 0.0, 1.0);
    std::vector<double> rays((size_t)n * 7), first((size_t)n * 16);
    if (rt_query_camera(s.raw(), &cam.c, W, H, 0, seed, 0, rays.data(), first.data()) != 0) return fail(rt_last_error());
    // the chain, link by link (csrc/rt_chain.h (C1)-(C7)), from entry points that are not under test here
    std::vector<double> cur = rays, want((size_t)n * 16), want_alb((size_t)n * 3), weight((size_t)n * 3, 1.0), S(n, 0.0), L0(n, 1.0);
    std::vector<uint32_t> links(n, 0u); std::vector<char> live(n, 1);
    for (uint32_t l = 0; l <= L; l++) {
        const uint64_t seed_l = l ? seed + (uint64_t)l * 0x9E3779B97F4A7C15ull : seed;
        std::vector<double> hits((size_t)n * 16), alb((size_t)n * 3), next((size_t)n * 7), factor((size_t)n * 3);
        std::vector<uint32_t> status(n);
        if (rt_query_albedo(s.raw(), n, cur.data(), t_min, seed_l, 0, alb.data(), hits.data()) != 0) return fail(rt_last_error());
        if (rt_chain_step_host(s.raw(), n, cur.data(), hits.data(), 0.0, next.data(), factor.data(), status.data()) != 0) return fail(rt_last_error());
        for (uint32_t k = 0; k < n; k++) {
            if (!live[k]) continue;
            const double* d = &cur[(size_t)k * 7 + 3]; const double* r = &hits[(size_t)k * 16];
            const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            double t_word = r[1];
            if (l == 0) { S[k] = r[1] * len; L0[k] = len; }
            else { if (r[0] != 0.0) S[k] = S[k] + r[1] * len; t_word = S[k] / L0[k]; }
            if (status[k] == 0u && l < L) {
                for (int j = 0; j < 3; j++) weight[(size_t)k * 3 + j] = weight[(size_t)k * 3 + j] * factor[(size_t)k * 3 + j];
                std::memcpy(&cur[(size_t)k * 7], &next[(size_t)k * 7], 7 * sizeof(double));
                links[k]++;
            } else {
                live[k] = 0;
                std::memcpy(&want[(size_t)k * 16], r, 16 * sizeof(double));
                want[(size_t)k * 16 + 1] = t_word; want[(size_t)k * 16 + 15] = (double)links[k];
                for (int j = 0; j < 3; j++) want_alb[(size_t)k * 3 + j] = weight[(size_t)k * 3 + j] * alb[(size_t)k * 3 + j];
            }
        }
    }
    ChainSettings c; c.max_links = L; c.max_fuzz = 0.0;
    std::vector<double> alb;
    const std::vector<double> got = query_chain(s, rays, c, t_min, seed, &alb);
    if (!same_words(got, want)) return fail("query_chain is not the chain composed link by link");
    if (!same_words(alb, want_alb)) return fail("query_chain's albedo is not the weight times the last record's albedo");
    if (!same_words(query_chain(s, rays, c, t_min, seed), want)) return fail("query_chain without the albedo");
    size_t followed = 0, deep = 0;
    for (uint32_t k = 0; k < n; k++) { followed += links[k] >= 1u; deep += links[k] >= 2u; }
    if (followed == 0 || deep == 0) return fail("no chain follows a link: the view tests nothing");
    ChainSettings none; none.max_links = 0;
    if (!same_words(query_chain(s, rays, none, t_min, seed), first)) return fail("max_links = 0 is not rt_query_camera's records of these rays");
    // the camera form of one sample: the same links (the guide's reduction turns -0.0 into +0.0 and keeps other words: rt_guide.h)
    std::vector<uint32_t> cam_links; std::vector<double> cam_alb;
    const std::vector<double> guide = query_camera_chain_guide(s, cam, W, H, c, 0, 1, seed, &cam_alb, &cam_links);
    for (uint32_t k = 0; k < n; k++) if (cam_links[k] != links[k] || guide[(size_t)k * 16] != want[(size_t)k * 16]) return fail("query_camera_chain_guide of one sample: links or hit");
    if (!same_words(query_camera_chain_guide(s, cam, W, H, c, 0, 1, seed), guide)) return fail("query_camera_chain_guide without its optional outputs");
    try { ChainSettings bad; bad.max_links = 65; query_chain(s, rays, bad); return fail("max_links = 65 accepted"); } catch (const Error&) {}
    // a progressive frame
    const Color bg(0.7, 0.8, 1.0);
    Progressive frame(s, cam, bg, W, H, 8, seed);
    if (frame.guide_chain().max_links != 0u) return fail("a new frame's guide_chain");
    frame.set_guide_chain(L, 0.0);
    try { frame.set_guide_chain(65, 0.0); return fail("set_guide_chain(65) accepted"); } catch (const Error&) {}
    if (frame.guide_chain().max_links != L || frame.guide_chain().max_fuzz != 0.0) return fail("guide_chain after set_guide_chain");
    frame.add(4);
    const std::vector<uint8_t> img = frame.rgb8_denoised();
    if (frame.guide_info().builds != 1u) return fail("guide_info after the first denoised resolve");
    const std::vector<double> filtered = denoise_host(frame.sum(), frame.samples(), guide, W, H);
    for (size_t p = 0; p < (size_t)n; p++) {
        uint64_t col[3]; rt_format_color(&filtered[p * 3], frame.samples(), col);
        for (int k = 0; k < 3; k++) if (img[p * 3 + k] != (uint8_t)col[k]) return fail("the progressive resolve is not format_color of denoise_host on the chain guide");
    }
    std::printf("ok gpu, %zu chains follow a link, %zu two or more\n", followed, deep);
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

// host/main.cpp — the reference's `main` (src/main.rs:577-836) with its render loop replaced by ONE call into
// librt_amd.so.  Scene functions, cameras, the `Scene` enum and the PPM-on-stdout contract follow main.rs; the
// reference is Rust, this environment has no Rust toolchain, so the host is C++ over include/raytracinginrust.hpp
// (same constructor names and argument order).  Usage mirrors `cargo run --release > image.ppm` (README.md:4):
//
//     rtrender [--scene cornell|random|final|teapot|two_sphere|two_perlin|earth|light_room|smoke|progress] [--width W] [--height H] [--spp N] [--depth D]
//              [--seed S] [--obj teapot.obj] [--earth earth.ppm] [--f32] [--fast-bvh] [--gpus N] [--progressive N] [--aov normal|depth|material|albedo FILE] [--panorama FILE]
//              [--denoise K[,SIGMA_C,SIGMA_N,SIGMA_P]] [--denoise-albedo N] [--denoise-variance SIGMA_V] [--until-error TAU] [--max-samples M] [--aov error FILE]
//              [--adaptive] [--aov samples FILE] [--denoise-guide N] [--aov coverage FILE] [--denoise-chain LINKS[,FUZZ]] [--aov links FILE]
//              [--orbit FRAMES,DEGREES [--history CAP] [--out FILE]] > image.ppm
//
// --denoise K[,c,n,p] (opt-in): the frame through the edge-avoiding a-trous filter before it is written (rt_denoise: K iterations, guided by
// sample 0's camera hits of this --seed, or --denoise-guide's record); with --progressive the frame resolves itself denoised on the device (rt_progressive_resolve_denoised_rgb8).
// --denoise-albedo N (with --denoise): the filter runs on the frame divided by its first-hit albedo — the mean over samples [0, N) of this --seed,
// rt_query_camera_albedo — and the result is multiplied back (rt_denoise_albedo*): what a textured scene needs.
// --denoise-guide N (with --denoise): the filter is guided by the averaged first-hit record of samples [0, N) of this --seed
// (rt_query_camera_guide: what the lens, the shutter and the pixel's area see) instead of sample 0's; with --progressive the frame builds it
// (rt_progressive_set_guide_samples).  --aov coverage FILE: that record's hit count / N as a grey image.
// --denoise-chain LINKS[,FUZZ] (with --denoise): the guide — and with --denoise-albedo the albedo, then over --denoise-guide N's samples — is taken at
// the first non-specular surface behind up to LINKS (1 .. 64) mirrors (fuzz <= FUZZ, default 0) and glass surfaces (rt_query_camera_chain_guide);
// with --progressive the frame builds it (rt_progressive_set_guide_chain).  --aov links FILE: the links followed per pixel over those samples,
// grey, 255 at LINKS per sample.
// --denoise-variance SIGMA_V (with --progressive N and --denoise K): the colour stop is SIGMA_V standard deviations of the frame's own
// per-pixel variance instead of SIGMA_C (rt_progressive_resolve_denoised_variance_rgb8); the frame keeps moments and needs at least two passes.
// With --denoise-albedo as well, and on an --adaptive frame with any of the three, the frame is denoised as it is — per-pixel counts, its
// variance divided by the albedo squared — by rt_progressive_resolve_denoised_frame_rgb8; every other combination takes the call named above.
//
// --progressive N (opt-in, one GPU): the frame in passes of N samples per pixel (rt_progressive_*), the reference's style of progress on
// stderr (main.rs:772-775), and the same PPM bytes at the end, built from the image the device resolved.
//
// --until-error TAU [--max-samples M] (with --progressive N): the frame keeps moments (rt_progressive_enable_moments) and stops at the first
// pass — the second at the earliest — after which no pixel's estimated standard error exceeds TAU display units (1/256 = 0.00390625 is one code
// value), at the latest after M samples per pixel (default: --spp); the progress line carries the three pixel counts.
// --adaptive (with --progressive N and --until-error TAU): an adaptive frame (rt_progressive_enable_adaptive) — every pass samples only the pixels
// whose estimated standard error still exceeds TAU, and their neighbours, no pixel beyond --max-samples (default: --spp); the frame ends with the
// pass that lists no pixel.  --aov samples FILE (with --adaptive, beside the frame): the per-pixel sample counts when it ends.
// --orbit FRAMES,DEGREES [--history CAP] [--out FILE] (with --progressive N; --denoise K[,c,n,p] allowed): FRAMES views on a circle around lookat about
// vup, DEGREES apart, each with a new seed (--seed + view) and N samples; from the second view on the frame carries its history along
// (rt_progressive_set_view, at most CAP samples' worth per pixel, default 64; 0: none) and FILE_000.ppm, FILE_001.ppm ... (default orbit) are the
// temporal resolves (rt_progressive_resolve_temporal_rgb8), through K iterations of the frame filter with --denoise.  Nothing goes to stdout.
// With --denoise K --denoise-variance SIGMA_V [--denoise-albedo N] the frame keeps moments, its history carries its variance from view to view
// and every view resolves through the variance stop (rt_progressive_resolve_temporal_variance_rgb8); a view's N samples are then two passes,
// (N + 1) / 2 and the rest, so that the frame has a variance to hand on.
// --aov error FILE (with --progressive N, beside the frame): the frame's error map when it ends (rt_progressive_error_map).
//
// --aov KIND FILE (opt-in, one GPU, instead of the frame): a feature frame for a denoiser or a compositor — the closest hit of sample 0's
// camera ray of every pixel (rt_query_camera: the ray the frame traces for that sample) as a P3 PPM in FILE ("-": stdout); AOV_HELP has the mappings.
//
// --panorama FILE (opt-in, one GPU, instead of the frame): the 2:1 equirectangular image of everything around the scene's lookfrom —
// image_width x image_width/2 rays through rt_query_radiance (ray_color for caller rays), the scene's spp, depth and background — as the
// frame's kind of PPM in FILE ("-": stdout).
//
// The reference hard-codes its settings as consts (main.rs:579-583, :623); they are flags here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include "../../include/raytracinginrust.hpp"

using namespace rtr;

static const uint32_t STREAM_RANDOM_SCENE = 0, STREAM_FINAL_SCENE = 1, STREAM_TWO_PERLIN = 2;

// src/main.rs:212-227
static void two_spehre(Scene& s) {
    HittableList world(s);
    Material top_mat = Lambertian::new_(s, CheckTexture::new_(s, ConstantTexture::new_(s, Color(1.0, 1.0, 1.0)), ConstantTexture::new_(s, Color(0.3, 0.3, 1.0))));
    Material bottom_mat = Lambertian::new_(s, CheckTexture::new_(s, ConstantTexture::new_(s, Color(1.0, 1.0, 1.0)), ConstantTexture::new_(s, Color(0.3, 0.3, 1.0))));
    world.push(Sphere::new_(s, Point3(0.0, 10.0, 0.0), 10.0, top_mat));
    world.push(Sphere::new_(s, Point3(0.0, -10.0, 0.0), 10.0, bottom_mat));
    s.set(world, {});
}
// src/main.rs:229-245
static void two_perlin_sphere(Scene& s, uint64_t seed) {
    Rng rng(seed, STREAM_TWO_PERLIN);
    HittableList world(s);
    Material top_mat = Lambertian::new_(s, NoiseTexture::new_(s, 2.0, rng));
    Material bottom_mat = Lambertian::new_(s, NoiseTexture::new_(s, 2.0, rng));
    world.push(Sphere::new_(s, Point3(1000.0, 2.0, 1000.0), 2.0, top_mat));
    world.push(Sphere::new_(s, Point3(1000.0, -1000.0, 1000.0), 1000.0, bottom_mat));
    s.set(world, {});
}
// src/main.rs:247-255
static void earth(Scene& s, const std::vector<uint8_t>& data, uint32_t w, uint32_t h) {
    s.set(Sphere::new_(s, Vec3(0.0, 0.0, 0.0), 2.0, Lambertian::new_(s, ImageTexture::new_(s, data, w, h))), {});
}
// src/main.rs:257-276
static void light_room(Scene& s) {
    HittableList world(s);
    Material bottom_mat = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.7, 0.7, 0.7)));
    Material top_mat = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.0, 0.1843, 0.6549)));
    Material emitted = DiffuseLight::new_(s, ConstantTexture::new_(s, Color(4.0, 4.0, 4.0)));
    world.push(Sphere::new_(s, Point3(0.0, -1000.0, 0.0), 1000.0, bottom_mat));
    world.push(Sphere::new_(s, Point3(0.0, 2.0, 0.0), 2.0, top_mat));
    Hittable plane = AARect::new_(s, Plane::XY, 3.0, 5.0, 1.0, 3.0, -2.0, emitted);
    world.push(plane);
    s.set(world, {plane});
}
// src/main.rs:313-346
static void cornell_box_with_smoke(Scene& s) {
    Material red = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.65, 0.05, 0.05)));
    Material white = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.73, 0.73, 0.73)));
    Material green = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.12, 0.45, 0.15)));
    Material light = DiffuseLight::new_(s, ConstantTexture::new_(s, Color(15.0, 15.0, 15.0)));
    Hittable rect_light = FlipNormal::new_(s, AARect::new_(s, Plane::XZ, 213.0, 343.0, 227.0, 332.0, 554.0, light));
    HittableList world(s);
    world.push(AARect::new_(s, Plane::YZ, 0.0, 555.0, 0.0, 555.0, 555.0, green));
    world.push(AARect::new_(s, Plane::YZ, 0.0, 555.0, 0.0, 555.0, 0.0, red));
    world.push(rect_light);
    world.push(AARect::new_(s, Plane::XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white));
    world.push(AARect::new_(s, Plane::XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white));
    world.push(AARect::new_(s, Plane::XY, 0.0, 555.0, 0.0, 555.0, 555.0, white));
    Hittable box1 = Translate::new_(s, Rotate::new_(s, Axis::Y, Cube::new_(s, Point3(0.0, 0.0, 0.0), Point3(165.0, 165.0, 165.0), white), -18.0), Vec3(130.0, 0.0, 65.0));
    Hittable box2 = Translate::new_(s, Rotate::new_(s, Axis::Y, Cube::new_(s, Point3(0.0, 0.0, 0.0), Point3(165.0, 330.0, 165.0), white), 15.0), Vec3(265.0, 0.0, 295.0));
    world.push(ConstantMedium::new_(s, box1, 0.01, ConstantTexture::new_(s, Color(1.0, 1.0, 1.0))));
    world.push(ConstantMedium::new_(s, box2, 0.01, ConstantTexture::new_(s, Color(0.0, 0.0, 0.0))));
    s.set(world, {rect_light});
}
// src/main.rs:515-562: the body is entirely commented out
static void progress_showcase(Scene& s) { HittableList world(s); s.set(world, {}); }

// src/main.rs:153-210
static void random_scene(Scene& s, uint64_t seed) {
    Rng rng(seed, STREAM_RANDOM_SCENE);
    std::vector<Hittable> world;
    Material ground_mat = Lambertian::new_(s, CheckTexture::new_(s, ConstantTexture::new_(s, Color(1.0, 1.0, 1.0)), ConstantTexture::new_(s, Color(0.3, 0.3, 1.0))));
    world.push_back(Sphere::new_(s, Point3(0.0, -1000.0, 0.0), 1000.0, ground_mat));
    for (int a = -11; a <= 11; a++) for (int b = -11; b <= 11; b++) {
        double choose_mat = rng.gen_f64();
        double cx = (double)a + rng.gen_range(0.0, 0.9);
        double cz = (double)b + rng.gen_range(0.0, 0.9);
        Point3 center(cx, 0.2, cz);
        if (choose_mat < 0.8) {
            Color c1 = rng.color_random(0.0, 1.0); Color c2 = rng.color_random(0.0, 1.0);
            Material m = Lambertian::new_(s, ConstantTexture::new_(s, c1 * c2));
            Point3 center1 = center + Vec3(0.0, rng.gen_range(0.0, 0.01), 0.0);
            world.push_back(MovingSphere::new_(s, center, center1, 0.0, 1.0, 0.2, m));
        } else if (choose_mat < 0.95) {
            Color albedo = rng.color_random(0.4, 1.0);
            double fuzz = rng.gen_range(0.0, 0.5);
            world.push_back(Sphere::new_(s, center, 0.2, Metal::new_(s, albedo, fuzz)));
        } else {
            world.push_back(Sphere::new_(s, center, 0.2, Dielectric::new_(s, 1.5)));
        }
    }
    world.push_back(Sphere::new_(s, Point3(0.0, 1.0, 0.0), 1.0, Dielectric::new_(s, 1.5)));
    world.push_back(Sphere::new_(s, Point3(-4.0, 1.0, 0.0), 1.0, Lambertian::new_(s, ConstantTexture::new_(s, Color(0.4, 0.2, 0.1)))));
    world.push_back(Sphere::new_(s, Point3(4.0, 1.0, 0.0), 1.0, Metal::new_(s, Color(0.7, 0.6, 0.5), 0.0)));
    s.set(BVH::new_(s, world, 0.0, 1.0), {});      // `lights` is empty in the reference (main.rs:207): cosine-only fallback, DESIGN.md D2
}

// src/main.rs:278-311
static void cornell_box(Scene& s) {
    Material red = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.65, 0.05, 0.05)));
    Material white = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.73, 0.73, 0.73)));
    Material green = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.12, 0.45, 0.15)));
    Material metal = Metal::new_(s, Color(0.8, 0.85, 0.88), 0.0);
    Material light = DiffuseLight::new_(s, ConstantTexture::new_(s, Color(15.0, 15.0, 15.0)));
    Hittable rect_light = FlipNormal::new_(s, AARect::new_(s, Plane::XZ, 213.0, 343.0, 227.0, 332.0, 554.0, light));
    HittableList world(s);
    world.push(AARect::new_(s, Plane::YZ, 0.0, 555.0, 0.0, 555.0, 555.0, green));
    world.push(AARect::new_(s, Plane::YZ, 0.0, 555.0, 0.0, 555.0, 0.0, red));
    world.push(rect_light);
    world.push(AARect::new_(s, Plane::XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white));
    world.push(AARect::new_(s, Plane::XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white));
    world.push(AARect::new_(s, Plane::XY, 0.0, 555.0, 0.0, 555.0, 555.0, white));
    world.push(Translate::new_(s, Rotate::new_(s, Axis::Y, Cube::new_(s, Point3(0.0, 0.0, 0.0), Point3(165.0, 165.0, 165.0), white), -18.0), Vec3(130.0, 0.0, 65.0)));
    world.push(Translate::new_(s, Rotate::new_(s, Axis::Y, Cube::new_(s, Point3(0.0, 0.0, 0.0), Point3(165.0, 330.0, 165.0), metal), 15.0), Vec3(265.0, 0.0, 295.0)));
    s.set(world, {rect_light});
}

// src/main.rs:348-451 as committed, with teapot.obj standing in for the absent Venus.obj (placement: DESIGN.md)
static void cornell_test(Scene& s, const std::string& obj_path) {
    Material white = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.73, 0.73, 0.73)));
    Material desire = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.922, 0.238, 0.331)));
    Material safety_orange = Lambertian::new_(s, ConstantTexture::new_(s, Color(1.000, 0.471, 0.0)));
    Material color_80cf00 = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.502, 0.812, 0.002)));
    Material light0 = DiffuseLight::new_(s, ConstantTexture::new_(s, Color(1.0, 1.0, 0.88) * 2.2));
    HittableList world(s);
    world.push(AARect::new_(s, Plane::YZ, 0.0, 555.0, 0.0, 555.0, 555.0, desire));
    world.push(AARect::new_(s, Plane::YZ, 0.0, 555.0, 0.0, 555.0, 0.0, safety_orange));
    world.push(AARect::new_(s, Plane::XZ, 0.0, 555.0, 0.0, 555.0, 0.0, white));
    world.push(AARect::new_(s, Plane::XZ, 0.0, 555.0, 0.0, 555.0, 555.0, white));
    world.push(AARect::new_(s, Plane::XY, 0.0, 555.0, 0.0, 555.0, 555.0, white));
    Hittable rect_light0 = FlipNormal::new_(s, AARect::new_(s, Plane::XZ, 128.0, 428.0, 115.0, 270.0, 554.0, light0));
    Mesh obj = Mesh::load_obj(s, obj_path, Vec3(268.0, 340.0, 258.0), 1.5, color_80cf00);
    world.push(rect_light0);
    world.push(BVH::of_list(s, obj.tris, 0.0, 1.0));
    s.set(world, {rect_light0});
}

// src/main.rs:453-513
static void final_scene(Scene& s, uint64_t seed, const std::vector<uint8_t>& earth, uint32_t ew, uint32_t eh) {
    Rng rng(seed, STREAM_FINAL_SCENE);
    HittableList world(s);
    Material ground = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.48, 0.83, 0.53)));
    std::vector<Hittable> box_list1;
    const int boxes_per_side = 20;
    for (int i = 0; i < boxes_per_side; i++) for (int j = 0; j < boxes_per_side; j++) {
        double w = 100.0;
        double x0 = -1000.0 + (double)i * w, z0 = -1000.0 + (double)j * w, y0 = 0.0;
        double x1 = x0 + w, y1 = 100.0 * (rng.gen_f64() + 0.01), z1 = z0 + w;
        box_list1.push_back(Cube::new_(s, Point3(x0, y0, z0), Point3(x1, y1, z1), ground));
    }
    world.push(BVH::new_(s, box_list1, 0.0, 1.0));
    Material light = DiffuseLight::new_(s, ConstantTexture::new_(s, Color(7.0, 7.0, 7.0)));
    Hittable rect_light = FlipNormal::new_(s, AARect::new_(s, Plane::XZ, 147.0, 412.0, 123.0, 423.0, 554.0, light));
    world.push(rect_light);
    Point3 center(400.0, 400.0, 200.0);
    world.push(MovingSphere::new_(s, center, center + Point3(30.0, 0.0, 0.0), 0.0, 1.0, 50.0, Lambertian::new_(s, ConstantTexture::new_(s, Color(0.7, 0.3, 0.1)))));
    world.push(Sphere::new_(s, Point3(260.0, 150.0, 45.0), 50.0, Dielectric::new_(s, 1.5)));
    world.push(Sphere::new_(s, Point3(0.0, 150.0, 145.0), 50.0, Metal::new_(s, Color(0.8, 0.8, 0.9), 1.0)));
    Hittable boundary = Sphere::new_(s, Point3(360.0, 150.0, 145.0), 70.0, Dielectric::new_(s, 1.5));
    world.push(boundary);
    world.push(ConstantMedium::new_(s, boundary, 0.2, ConstantTexture::new_(s, Color(0.2, 0.4, 0.9))));
    boundary = Sphere::new_(s, Point3(0.0, 0.0, 0.0), 5000.0, Dielectric::new_(s, 1.5));
    world.push(ConstantMedium::new_(s, boundary, 0.0001, ConstantTexture::new_(s, Color(1.0, 1.0, 1.0))));
    world.push(Sphere::new_(s, Point3(400.0, 200.0, 400.0), 100.0, Lambertian::new_(s, ImageTexture::new_(s, earth, ew, eh))));
    world.push(Sphere::new_(s, Point3(220.0, 280.0, 300.0), 80.0, Lambertian::new_(s, NoiseTexture::new_(s, 0.1, rng))));
    Material white = Lambertian::new_(s, ConstantTexture::new_(s, Color(0.73, 0.73, 0.73)));
    std::vector<Hittable> box_list2;
    for (int k = 0; k < 1000; k++) {
        double x = 165.0 * rng.gen_f64(), y = 165.0 * rng.gen_f64(), z = 165.0 * rng.gen_f64();
        box_list2.push_back(Sphere::new_(s, Point3(x, y, z), 10.0, white));
    }
    world.push(Translate::new_(s, Rotate::new_(s, Axis::Y, BVH::new_(s, box_list2, 0.0, 0.1), 15.0), Point3(-100.0, 270.0, 395.0)));
    s.set(world, {rect_light});
}

// binary PPM (P6) reader for the decoded earthmap texels (image::open(..).to_rgb8() in the reference, main.rs:491)
static bool read_p6(const std::string& path, std::vector<uint8_t>& data, uint32_t& w, uint32_t& h) {
    std::ifstream f(path, std::ios::binary);
    std::string magic; int maxv = 0;
    if (!(f >> magic >> w >> h >> maxv) || magic != "P6" || maxv != 255) return false;
    f.get();
    data.resize((size_t)w * h * 3);
    f.read((char*)data.data(), (std::streamsize)data.size());
    return (bool)f;
}

// image::open(path).to_rgb8() (main.rs:248,491): a baseline JPEG goes through the library's decoder, a P6 file is read directly
static bool read_image(const std::string& path, std::vector<uint8_t>& data, uint32_t& w, uint32_t& h) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.size() > 2 && bytes[0] == 0xFF && bytes[1] == 0xD8) {
        uint8_t* rgb = rt_decode_jpeg_rgb8(bytes.data(), bytes.size(), &w, &h);
        if (!rgb) { std::fprintf(stderr, "%s\n", rt_last_error()); return false; }
        data.assign(rgb, rgb + (size_t)w * h * 3);
        rt_free(rgb);
        return true;
    }
    return read_p6(path, data, w, h);
}

static const char* AOV_HELP =
    "  --aov normal|depth|material|albedo FILE   write a feature frame instead of the image: the closest hit of the camera ray of sample 0 of\n"
    "                                     every pixel (the ray the frame with this --seed traces), as a P3 PPM in FILE (- = stdout):\n"
    "      normal    r g b = 0.5 * (n + 1) * 255.999 truncated, per component of the hit's normal (a miss has the zero normal: 127 127 127)\n"
    "      depth     grey, linear in the hit's t between the frame's smallest finite t (255) and its largest (0): (max - t) / (max - min) *\n"
    "                255.999 truncated; a miss is 0\n"
    "      material  grey, the hit's material handle mod 256 (a miss or a ConstantMedium hit, handle -1: 255)\n"
    "      albedo    r g b = the first hit's albedo held to [0, 1], times 255.999, truncated (no gamma); the mean over the samples [0, N) of\n"
    "                --denoise-albedo N when that is given, else sample 0's (a miss, glass and emitters: 255 255 255)\n"
    "      coverage  grey, the fraction of the samples [0, N) of --denoise-guide N (default 1) whose camera ray hits anything: hits / N * 255.999\n"
    "                truncated (rt_query_camera_guide's word 15)\n"
    "      links     (with --denoise-chain LINKS[,FUZZ]) grey, the links followed through mirrors and glass over the samples [0, N) of\n"
    "                --denoise-guide N (default 1): links / (N * LINKS) * 255.999 truncated (rt_query_camera_chain_guide's links_out)\n"
    "      error     (with --progressive N, written BESIDE the image when the frame ends) grey, the estimated standard error of the pixel in\n"
    "                display units: sqrt(e2) * 256 * 8 truncated, held to 255 — one code value of standard error is grey 8; not finite: 255\n"
    "      samples   (with --adaptive, written BESIDE the image when the frame ends) grey, the samples the pixel holds: 255 * n / the largest n, truncated\n";

// One channel value of the mappings above (a NaN gives 0)
static unsigned aov_level(double x) { return x >= 0.0 ? (x > 255.0 ? 255u : (unsigned)x) : 0u; }
static void write_albedo_aov(const std::string& path, const std::vector<double>& albedo_sum, uint32_t n_samples, uint32_t W, uint32_t H) {
    std::vector<uint8_t> img(albedo_sum.size());
    for (size_t i = 0; i < albedo_sum.size(); i++) {
        const double a = albedo_sum[i] / (double)n_samples;
        img[i] = (uint8_t)aov_level((a >= 0.0 ? (a > 1.0 ? 1.0 : a) : 0.0) * 255.999);
    }
    write_ppm_rgb8(path.c_str(), img, W, H);
}
static void write_coverage_aov(const std::string& path, const std::vector<double>& guide, uint32_t n_samples, uint32_t W, uint32_t H) {
    std::vector<uint8_t> img(guide.size() / 16u * 3u);
    for (size_t p = 0; p < guide.size() / 16u; p++) img[p * 3] = img[p * 3 + 1] = img[p * 3 + 2] = (uint8_t)aov_level(guide[p * 16 + 15] / (double)n_samples * 255.999);
    write_ppm_rgb8(path.c_str(), img, W, H);
}
static void write_links_aov(const std::string& path, const std::vector<uint32_t>& links, uint32_t n_samples, uint32_t max_links, uint32_t W, uint32_t H) {
    std::vector<uint8_t> img(links.size() * 3u);
    for (size_t p = 0; p < links.size(); p++) img[p * 3] = img[p * 3 + 1] = img[p * 3 + 2] = (uint8_t)aov_level((double)links[p] / ((double)n_samples * (double)max_links) * 255.999);
    write_ppm_rgb8(path.c_str(), img, W, H);
}
static void write_error_aov(const std::string& path, const std::vector<double>& e2, uint32_t W, uint32_t H) {
    std::vector<uint8_t> img(e2.size() * 3);
    for (size_t p = 0; p < e2.size(); p++) {
        const uint8_t g = (uint8_t)(e2[p] - e2[p] == 0.0 ? aov_level(std::sqrt(e2[p]) * 256.0 * 8.0) : 255u);
        img[p * 3] = img[p * 3 + 1] = img[p * 3 + 2] = g;
    }
    write_ppm_rgb8(path.c_str(), img, W, H);
}
static void write_samples_aov(const std::string& path, const std::vector<uint32_t>& counts, uint32_t W, uint32_t H) {
    uint32_t most = 1u;
    for (uint32_t n : counts) most = std::max(most, n);
    std::vector<uint8_t> img(counts.size() * 3);
    for (size_t p = 0; p < counts.size(); p++) img[p * 3] = img[p * 3 + 1] = img[p * 3 + 2] = (uint8_t)((uint64_t)counts[p] * 255u / most);
    write_ppm_rgb8(path.c_str(), img, W, H);
}
static void write_aov(const std::string& kind, const std::string& path, const std::vector<Hit>& hits, uint32_t W, uint32_t H) {
    double lo = 0.0, hi = 0.0; bool have = false;
    for (const Hit& h : hits) if (h.hit && h.t - h.t == 0.0) { lo = have ? std::min(lo, h.t) : h.t; hi = have ? std::max(hi, h.t) : h.t; have = true; }
    std::vector<uint8_t> img(hits.size() * 3);
    for (size_t p = 0; p < hits.size(); p++) {
        const Hit& h = hits[p];
        unsigned c[3];
        if (kind == "normal") for (int k = 0; k < 3; k++) c[k] = aov_level(0.5 * (h.normal.e[k] + 1.0) * 255.999);
        else if (kind == "depth") {
            unsigned g = 0u;
            if (h.hit && h.t - h.t == 0.0) g = hi > lo ? aov_level((hi - h.t) / (hi - lo) * 255.999) : 255u;
            c[0] = c[1] = c[2] = g;
        } else c[0] = c[1] = c[2] = (unsigned)((long long)h.material & 255);
        for (int k = 0; k < 3; k++) img[p * 3 + k] = (uint8_t)c[k];
    }
    write_ppm_rgb8(path.c_str(), img, W, H);
}

enum class SceneKind { Random, TwoSphere, TwoPerlinSphere, Earth, LightRoom, CornellBox, CornellSmoke, CornellTest, FinalScene, Progress };   // src/main.rs:564-575

int main(int argc, char** argv) {
    SceneKind scene = SceneKind::CornellBox;
    uint32_t image_width = 500, image_height = 500, samples_per_pixel = 800, max_depth = 100;    // main.rs:579-583
    uint64_t seed = 0x5EED; uint32_t flags = RT_F64; bool fast_bvh = false;
    std::string aov_kind, aov_path;                                         // --aov KIND FILE: a feature frame instead of the image
    std::string panorama_path;                                              // --panorama FILE: the equirectangular image around lookfrom instead
    bool want_denoise = false; DenoiseSettings dn;                          // --denoise K[,sigma_c,sigma_n,sigma_p]: filter the frame before it is written
    uint32_t guide_samples = 0;                                             // --denoise-guide N: guide the filter by the averaged record of samples [0, N) (0: sample 0's)
    uint32_t albedo_samples = 0;                                            // --denoise-albedo N: demodulate by the albedo of samples [0, N) (0: the plain filter)
    ChainSettings chain; chain.max_links = 0u;                              // --denoise-chain LINKS[,FUZZ]: guide and albedo behind mirrors and glass (0: first hits)
    double sigma_v = 0.0;                                                   // --denoise-variance SIGMA_V: the variance-guided colour stop (0: the plain filter)
    uint32_t progressive = 0;                                               // --progressive N: passes of N samples per pixel (0: one call)
    bool adaptive = false;                                                  // --adaptive: sample only the pixels whose estimated error still exceeds --until-error
    double until_error = -1.0; uint32_t max_samples = 0;                    // --until-error TAU [--max-samples M]: stop when no pixel's standard error exceeds TAU
    uint32_t orbit_frames = 0; double orbit_degrees = 0.0;                  // --orbit FRAMES,DEGREES: views on a circle around lookat, with temporal accumulation
    ReprojectSettings history; std::string orbit_out = "orbit";             // --history CAP, --out FILE
    int gpus = 1;                                                           // --gpus N: the first N devices (0 = all) through rt_render_multi
    std::string obj_path = "teapot.obj", earth_path = "earthmap.jpg";       // the reference's asset names (main.rs:248,491)
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--scene") {
            std::string v = next();
            scene = v == "random" ? SceneKind::Random : v == "final" ? SceneKind::FinalScene : v == "teapot" ? SceneKind::CornellTest
                  : v == "two_sphere" ? SceneKind::TwoSphere : v == "two_perlin" ? SceneKind::TwoPerlinSphere : v == "earth" ? SceneKind::Earth
                  : v == "light_room" ? SceneKind::LightRoom : v == "smoke" ? SceneKind::CornellSmoke : v == "progress" ? SceneKind::Progress
                  : SceneKind::CornellBox;
        }
        else if (a == "--isotropic-scatter") flags |= RT_ISOTROPIC_SCATTER;
        else if (a == "--width") image_width = (uint32_t)std::atoi(next());
        else if (a == "--height") image_height = (uint32_t)std::atoi(next());
        else if (a == "--spp") samples_per_pixel = (uint32_t)std::atoi(next());
        else if (a == "--depth") max_depth = (uint32_t)std::atoi(next());
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 0);
        else if (a == "--obj") obj_path = next();
        else if (a == "--earth") earth_path = next();
        else if (a == "--f32") flags |= RT_F32;
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--progressive") { const int n = std::atoi(next()); if (n < 1) { std::fprintf(stderr, "--progressive needs a pass size >= 1\n"); return 2; } progressive = (uint32_t)n; }
        else if (a == "--aov") {
            aov_kind = next(); aov_path = next();
            if (aov_kind != "normal" && aov_kind != "depth" && aov_kind != "material" && aov_kind != "albedo" && aov_kind != "error" && aov_kind != "samples" && aov_kind != "coverage" && aov_kind != "links") { std::fprintf(stderr, "--aov needs normal, depth, material, albedo, coverage, links, error or samples\n%s", AOV_HELP); return 2; }
        }
        else if (a == "--panorama") panorama_path = next();
        else if (a == "--until-error") { until_error = std::atof(next()); if (!(until_error >= 0.0)) { std::fprintf(stderr, "--until-error needs a standard error >= 0 in display units (0.00390625 is one code value)\n"); return 2; } }
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--max-samples") { const int n = std::atoi(next()); if (n < 1) { std::fprintf(stderr, "--max-samples needs a sample count >= 1\n"); return 2; } max_samples = (uint32_t)n; }
        else if (a == "--denoise") {
            const std::string v = next();
            unsigned k = 0; double c = dn.sigma[0], n = dn.sigma[1], p = dn.sigma[2];
            const int got = std::sscanf(v.c_str(), "%u,%lf,%lf,%lf", &k, &c, &n, &p);
            if (got != 1 && got != 4) { std::fprintf(stderr, "--denoise needs K or K,SIGMA_C,SIGMA_N,SIGMA_P\n"); return 2; }
            want_denoise = true; dn.iterations = k; dn.sigma[0] = c; dn.sigma[1] = n; dn.sigma[2] = p;
        }
        else if (a == "--denoise-albedo") { const int n = std::atoi(next()); if (n < 1) { std::fprintf(stderr, "--denoise-albedo needs a sample count >= 1\n"); return 2; } albedo_samples = (uint32_t)n; }
        else if (a == "--denoise-guide") { const int n = std::atoi(next()); if (n < 1) { std::fprintf(stderr, "--denoise-guide needs a sample count >= 1\n"); return 2; } guide_samples = (uint32_t)n; }
        else if (a == "--denoise-chain") {
            unsigned links = 0; double fuzz = 0.0;
            const int got = std::sscanf(next(), "%u,%lf", &links, &fuzz);
            if ((got != 1 && got != 2) || links < 1u || links > 64u || !(fuzz >= 0.0)) { std::fprintf(stderr, "--denoise-chain needs LINKS (1 .. 64) or LINKS,FUZZ (FUZZ >= 0)\n"); return 2; }
            chain.max_links = links; chain.max_fuzz = fuzz;
        }
        else if (a == "--denoise-variance") { sigma_v = std::atof(next()); if (!(sigma_v > 0.0)) { std::fprintf(stderr, "--denoise-variance needs a colour stop > 0 in standard deviations (inf switches it off)\n"); return 2; } }
        else if (a == "--orbit") {
            unsigned n = 0;
            if (std::sscanf(next(), "%u,%lf", &n, &orbit_degrees) != 2 || n < 1u) { std::fprintf(stderr, "--orbit needs FRAMES,DEGREES with FRAMES >= 1\n"); return 2; }
            orbit_frames = n;
        }
        else if (a == "--history") { const long long n = std::atoll(next()); if (n < 0 || n > 0x7FFFFFFFll) { std::fprintf(stderr, "--history needs a cap of 0 .. 2^31 - 1 samples\n"); return 2; } history.max_history = (uint32_t)n; }
        else if (a == "--out") orbit_out = next();
        else if (a == "--help" || a == "-h") {
            std::printf("rtrender [--scene cornell|random|final|teapot|two_sphere|two_perlin|earth|light_room|smoke|progress] [--width W] [--height H] [--spp N]\n"
                        "         [--depth D] [--seed S] [--obj teapot.obj] [--earth earth.ppm] [--f32] [--fast-bvh] [--gpus N] [--progressive N] > image.ppm\n%s"
                        "  --denoise K[,SIGMA_C,SIGMA_N,SIGMA_P]  write the frame through K (1 .. 8) iterations of the edge-avoiding a-trous filter, guided by\n"
                        "                                     the camera hits of sample 0 or of --denoise-guide N (default sigmas 4, 0.5, 0.02; inf switches a stop off); also with --progressive\n"
                        "  --denoise-albedo N                 with --denoise: filter the frame divided by its first-hit albedo (the mean over samples 0 .. N-1)\n"
                        "                                     and multiply back: textures are kept (textured scenes need it); also with --progressive\n"
                        "  --denoise-guide N                  with --denoise: guide the filter by the averaged first-hit record of samples 0 .. N-1 (lens, shutter and\n"
                        "                                     pixel area) instead of sample 0's; also with --progressive\n"
                        "  --denoise-chain LINKS[,FUZZ]       with --denoise: guide (and albedo) at the first non-specular surface behind up to LINKS mirrors\n"
                        "                                     (fuzz <= FUZZ, default 0) and glass surfaces; --aov links FILE: the links followed per pixel\n"
                        "  --denoise-variance SIGMA_V         with --progressive N and --denoise K: the colour stop in standard deviations of the frame's own\n"
                        "                                     per-pixel variance instead of SIGMA_C; needs at least two passes (--spp more than N);\n"
                        "                                     also with --denoise-albedo, and all three also with --adaptive\n"
                        "  --until-error TAU [--max-samples M]  with --progressive N: stop at the first pass after which no pixel's estimated standard error\n"
                        "                                     exceeds TAU display units (0.00390625 = one code value), at the latest after M samples (default --spp)\n"
                        "  --adaptive                         with --progressive N and --until-error TAU: every pass samples only the pixels whose estimated standard\n"
                        "                                     error still exceeds TAU (and their neighbours), none beyond M samples; ends when no pixel is left\n"
                        "  --orbit FRAMES,DEGREES             with --progressive N: FRAMES views on a circle around lookat, DEGREES apart, N samples and a new seed each;\n"
                        "    [--history CAP] [--out FILE]     the frame carries its history from view to view (at most CAP samples' worth, default 64, 0: none) and\n"
                        "                                     FILE_000.ppm ... (default orbit) are the temporal resolves; with --denoise K through the frame filter,\n"
                        "                                     with --denoise-variance SIGMA_V [--denoise-albedo N] as well through its variance stop (the history carries the variance)\n"
                        "  --panorama FILE                    write the 2:1 equirectangular image (width x width/2) of everything around the scene's\n"
                        "                                     lookfrom instead of the image: --spp samples per ray, --depth, the scene's background\n", AOV_HELP);
            return 0;
        }
        else if (a == "--collective") flags |= RT_MULTI_COLLECTIVE;         // with --gpus 1: run the RCCL gather anyway
        else if (a == "--fast-bvh") { fast_bvh = true; flags |= RT_NEAR_FIRST_BVH; }      // opt-in, not the reference's tree / visiting order
        else { std::fprintf(stderr, "unknown flag %s\n", a.c_str()); return 2; }
    }
    if ((until_error >= 0.0 || max_samples != 0u || aov_kind == "error") && progressive == 0u) { std::fprintf(stderr, "--until-error, --max-samples and --aov error go with --progressive N\n"); return 2; }
    if (adaptive && (progressive == 0u || until_error < 0.0)) { std::fprintf(stderr, "--adaptive goes with --progressive N and --until-error TAU\n"); return 2; }
    if (aov_kind == "samples" && !adaptive) { std::fprintf(stderr, "--aov samples goes with --adaptive\n"); return 2; }
    if (max_samples != 0u && until_error < 0.0) { std::fprintf(stderr, "--max-samples goes with --until-error TAU\n"); return 2; }
    if (albedo_samples != 0u && !want_denoise && aov_kind != "albedo") { std::fprintf(stderr, "--denoise-albedo goes with --denoise K (or --aov albedo)\n"); return 2; }
    if (guide_samples != 0u && !want_denoise && aov_kind != "coverage" && aov_kind != "links") { std::fprintf(stderr, "--denoise-guide goes with --denoise K (or --aov coverage)\n"); return 2; }
    if (chain.max_links != 0u && !want_denoise && aov_kind != "links") { std::fprintf(stderr, "--denoise-chain goes with --denoise K (or --aov links)\n"); return 2; }
    if (aov_kind == "links" && chain.max_links == 0u) { std::fprintf(stderr, "--aov links goes with --denoise-chain LINKS\n"); return 2; }
    if (sigma_v != 0.0 && (!want_denoise || progressive == 0u)) { std::fprintf(stderr, "--denoise-variance goes with --progressive N and --denoise K\n"); return 2; }
    if (orbit_frames != 0u && (progressive == 0u || adaptive || until_error >= 0.0 || !aov_kind.empty() || (albedo_samples != 0u && sigma_v == 0.0))) {
        std::fprintf(stderr, "--orbit goes with --progressive N, and of the other options only with --denoise K, --denoise-guide N and --denoise-variance SIGMA_V [--denoise-albedo N]\n"); return 2;
    }
    const double aspect_ratio = (double)image_width / (double)image_height;
    try {
        Scene s;
        if (fast_bvh) s.set_bvh_builder(RT_BVH_SAH);
        Color background; Camera camera;
        Vec3 vup(0.0, 1.0, 0.0);
        switch (scene) {                                                    // main.rs:624-765
        case SceneKind::Random:
            random_scene(s, seed);
            background = Color(0.7, 0.8, 1.0);
            camera = Camera::new_(Point3(13.0, 2.0, 3.0), Point3(0.0, 0.0, 0.0), vup, 20.0, aspect_ratio, 0.1, 10.0, 0.0, 1.0);
            break;
        case SceneKind::TwoSphere:
            two_spehre(s);
            background = Color(0.7, 0.8, 1.0);
            camera = Camera::new_(Point3(13.0, 2.0, 3.0), Point3(0.0, 0.0, 0.0), vup, 20.0, aspect_ratio, 0.0, 10.0, 0.0, 1.0);
            break;
        case SceneKind::TwoPerlinSphere:
            two_perlin_sphere(s, seed);
            background = Color(0.7, 0.8, 1.0);
            camera = Camera::new_(Point3(1013.0, 2.0, 1003.0), Point3(1000.0, 0.0, 1000.0), vup, 20.0, aspect_ratio, 0.0, 10.0, 0.0, 1.0);
            break;
        case SceneKind::Earth: {
            std::vector<uint8_t> tex; uint32_t ew = 0, eh = 0;
            if (!read_image(earth_path, tex, ew, eh)) throw Error("image not found: " + earth_path);      // main.rs:248
            earth(s, tex, ew, eh);
            background = Color(0.7, 0.8, 1.0);
            camera = Camera::new_(Point3(13.0, 2.0, 3.0), Point3(0.0, 0.0, 0.0), vup, 20.0, aspect_ratio, 0.1, 10.0, 0.0, 1.0);
            break;
        }
        case SceneKind::LightRoom:
            light_room(s);
            background = Color(0.0, 0.0, 0.0);
            camera = Camera::new_(Point3(26.0, 3.0, 6.0), Point3(0.0, 2.0, 0.0), vup, 20.0, aspect_ratio, 0.0, 10.0, 0.0, 1.0);
            break;
        case SceneKind::CornellSmoke:
            cornell_box_with_smoke(s);
            background = Color(0.0, 0.0, 0.0);
            camera = Camera::new_(Point3(278.0, 278.0, -800.0), Point3(278.0, 278.0, 0.0), vup, 40.0, aspect_ratio, 0.05, 10.0, 0.0, 1.0);
            break;
        case SceneKind::Progress:
            progress_showcase(s);
            background = Color(0.0, 0.0, 0.0);
            camera = Camera::new_(Point3(-3.3, 6.8, -9.8), Point3(0.0, 1.0, 0.0), vup, 40.0, aspect_ratio, 0.2, 12.0, 0.0, 1.0);
            break;
        case SceneKind::CornellBox:
            cornell_box(s);
            background = Color(0.0, 0.0, 0.0);
            camera = Camera::new_(Point3(278.0, 278.0, -800.0), Point3(278.0, 278.0, 0.0), vup, 40.0, aspect_ratio, 0.05, 10.0, 0.0, 1.0);
            break;
        case SceneKind::CornellTest:
            cornell_test(s, obj_path);
            background = Color(0.0, 0.0, 0.0);
            camera = Camera::new_(Point3(199.0, 439.0, -200.0), Point3(278.0, 375.0, 258.0), vup, 30.0, aspect_ratio, 0.01, 10.0, 0.0, 1.0);
            break;
        case SceneKind::FinalScene: {
            std::vector<uint8_t> earth; uint32_t ew = 0, eh = 0;
            if (!read_image(earth_path, earth, ew, eh)) throw Error("image not found: " + earth_path);    // main.rs:491 .expect("image not found")
            final_scene(s, seed, earth, ew, eh);
            background = Color(0.0, 0.0, 0.0);
            camera = Camera::new_(Point3(478.0, 278.0, -600.0), Point3(278.0, 278.0, 0.0), vup, 40.0, aspect_ratio, 0.01, 10.0, 0.0, 1.0);
            break;
        }
        }
        if (!aov_kind.empty() && aov_kind != "error" && aov_kind != "samples") {
            if (flags & RT_F32) throw Error("--aov runs in f64");
            if (aov_kind == "albedo") {
                const uint32_t n = albedo_samples ? albedo_samples : 1u;
                write_albedo_aov(aov_path, query_camera_albedo(s, camera, image_width, image_height, 0u, n, seed), n, image_width, image_height);
            } else if (aov_kind == "coverage") {
                const uint32_t n = guide_samples ? guide_samples : 1u;
                write_coverage_aov(aov_path, query_camera_guide(s, camera, image_width, image_height, 0u, n, seed), n, image_width, image_height);
            } else if (aov_kind == "links") {
                const uint32_t n = guide_samples ? guide_samples : 1u;
                std::vector<uint32_t> links;
                query_camera_chain_guide(s, camera, image_width, image_height, chain, 0u, n, seed, nullptr, &links);
                write_links_aov(aov_path, links, n, chain.max_links, image_width, image_height);
            } else
            write_aov(aov_kind, aov_path, query_camera(s, camera, image_width, image_height, 0u, seed), image_width, image_height);
            std::fprintf(stderr, "Done.\n");
            return 0;
        }
        if (!panorama_path.empty()) {
            if (flags & RT_F32) throw Error("--panorama runs in f64");
            const uint32_t pw = image_width, ph = image_width / 2u;
            if (ph == 0u) throw Error("--panorama needs --width >= 2");
            const Point3 from(camera.c.lookfrom[0], camera.c.lookfrom[1], camera.c.lookfrom[2]);
            write_ppm(panorama_path.c_str(), query_radiance(s, equirect_rays(from, pw, ph), samples_per_pixel, max_depth, background, seed,
                                                            flags & (uint32_t)RT_ISOTROPIC_SCATTER), pw, ph, samples_per_pixel);
            std::fprintf(stderr, "Done.\n");
            return 0;
        }
        // main.rs:772-833: the whole loop nest is this one call
        if (progressive) {
            if (gpus != 1 || (flags & RT_MULTI_COLLECTIVE)) throw Error("--progressive renders on one GPU");
            Progressive frame(s, camera, background, image_width, image_height, max_depth, seed, flags);
            const bool want_moments = until_error >= 0.0 || aov_kind == "error" || sigma_v != 0.0;
            if (want_moments) frame.enable_moments();
            if (guide_samples) frame.set_guide_samples(guide_samples);
            if (chain.max_links) frame.set_guide_chain(chain.max_links, chain.max_fuzz);
            if (orbit_frames) {
                // the views: lookfrom turned about the axis vup through lookat (Rodrigues' rotation), everything else the scene's camera
                const rt_camera& c0 = camera.c;
                const double al = std::sqrt(c0.vup[0] * c0.vup[0] + c0.vup[1] * c0.vup[1] + c0.vup[2] * c0.vup[2]);
                const double k[3] = {c0.vup[0] / al, c0.vup[1] / al, c0.vup[2] / al};
                const double r[3] = {c0.lookfrom[0] - c0.lookat[0], c0.lookfrom[1] - c0.lookat[1], c0.lookfrom[2] - c0.lookat[2]};
                for (uint32_t f = 0; f < orbit_frames; f++) {
                    if (f) {
                        const double a = orbit_degrees * (double)f * 3.141592653589793 / 180.0, ca = std::cos(a), sa = std::sin(a);
                        const double kr = k[0] * r[0] + k[1] * r[1] + k[2] * r[2];
                        const double x[3] = {k[1] * r[2] - k[2] * r[1], k[2] * r[0] - k[0] * r[2], k[0] * r[1] - k[1] * r[0]};
                        Camera view = camera;
                        for (int e = 0; e < 3; e++) view.c.lookfrom[e] = c0.lookat[e] + r[e] * ca + x[e] * sa + k[e] * kr * (1.0 - ca);
                        frame.set_view(view, seed + f, history);
                    }
                    // with the variance stop a view's N samples come as two passes (N + 1) / 2 and the rest: a frame's own variance needs two, and a
                    // history knows a variance only if some view before it had one
                    if (sigma_v != 0.0 && progressive >= 2u) { frame.add((progressive + 1u) / 2u); frame.add(progressive / 2u); }
                    else frame.add(progressive);
                    char name[32]; std::snprintf(name, sizeof(name), "_%03u.ppm", f);
                    const uint64_t held = [&]() { uint64_t w[2] = {0, 0}; rt_progressive_history_info(frame.raw(), w); return w[1]; }();
                    if (sigma_v != 0.0) {               // the variance stop on the blend's own variance (the frame has moments: want_moments above)
                        DenoiseVarianceSettings dv;
                        dv.iterations = dn.iterations; dv.sigma[0] = sigma_v; dv.sigma[1] = dn.sigma[1]; dv.sigma[2] = dn.sigma[2];
                        write_ppm_rgb8((orbit_out + name).c_str(), frame.rgb8_temporal_variance(dv, albedo_samples), image_width, image_height);
                    } else {
                        write_ppm_rgb8((orbit_out + name).c_str(), frame.rgb8_temporal(want_denoise ? dn.iterations : 0u, dn), image_width, image_height);
                    }
                    std::fprintf(stderr, "\rView %u / %u: %u samples, history in %llu pixels", f + 1u, orbit_frames, progressive, (unsigned long long)held);
                }
                std::fprintf(stderr, "\nDone.\n");
                return 0;
            }
            const uint32_t limit = until_error >= 0.0 && max_samples ? max_samples : samples_per_pixel;
            if (adaptive) {
                frame.enable_adaptive();
                for (;;) {
                    const Progressive::AdaptiveInfo info = frame.add_adaptive(progressive, until_error, limit);
                    if (info.listed == 0) break;
                    std::fprintf(stderr, "\rSamples: up to %llu / %u  pixels sampled %llu  mean samples %.1f", (unsigned long long)frame.samples(), limit,
                                 (unsigned long long)info.listed, (double)info.total / ((double)image_width * image_height));
                }
                if (aov_kind == "samples") write_samples_aov(aov_path, frame.counts(), image_width, image_height);
            }
            while (!adaptive && frame.samples() < limit) {
                frame.add((uint32_t)std::min<uint64_t>(progressive, limit - frame.samples()));
                std::fprintf(stderr, "\rSamples: %llu / %u", (unsigned long long)frame.samples(), limit);    // main.rs:772-775
                if (until_error >= 0.0 && frame.passes() >= 2) {
                    const ErrorStats st = frame.error_stats(until_error);
                    std::fprintf(stderr, "  converged %llu  unconverged %llu  nonfinite %llu", (unsigned long long)st.converged, (unsigned long long)st.unconverged, (unsigned long long)st.nonfinite);
                    if (st.unconverged == 0) break;
                }
            }
            std::fprintf(stderr, "\n");
            if (aov_kind == "error") {
                if (frame.passes() < 2) throw Error("--aov error needs at least two passes: --spp must be more than the pass size of --progressive");
                write_error_aov(aov_path, frame.error_map(), image_width, image_height);
            }
            if (want_denoise && (adaptive || (sigma_v != 0.0 && albedo_samples != 0u))) {
                // the frame as it is: per-pixel counts, and the variance stop together with demodulation (rt_progressive_resolve_denoised_frame_rgb8)
                if (sigma_v != 0.0 && !adaptive && frame.passes() < 2) throw Error("--denoise-variance needs at least two passes: --spp must be more than the pass size of --progressive");
                DenoiseFrameSettings df;
                df.variance = sigma_v != 0.0; df.albedo_samples = albedo_samples;
                df.iterations = dn.iterations; df.sigma[0] = df.variance ? sigma_v : dn.sigma[0]; df.sigma[1] = dn.sigma[1]; df.sigma[2] = dn.sigma[2];
                write_ppm_rgb8("-", frame.rgb8_denoised_frame(df), image_width, image_height);
                std::fprintf(stderr, "Done.\n");
                return 0;
            }
            if (sigma_v != 0.0) {
                if (frame.passes() < 2) throw Error("--denoise-variance needs at least two passes: --spp must be more than the pass size of --progressive");
                DenoiseVarianceSettings dv;
                dv.iterations = dn.iterations; dv.sigma[0] = sigma_v; dv.sigma[1] = dn.sigma[1]; dv.sigma[2] = dn.sigma[2];
                write_ppm_rgb8("-", frame.rgb8_denoised_variance(dv), image_width, image_height);
                std::fprintf(stderr, "Done.\n");
                return 0;
            }
            write_ppm_rgb8("-", want_denoise ? (albedo_samples ? frame.rgb8_denoised_albedo(albedo_samples, dn) : frame.rgb8_denoised(dn)) : frame.rgb8(), image_width, image_height);     // main.rs:767-769,832
            std::fprintf(stderr, "Done.\n");                                                    // main.rs:835
            return 0;
        }
        std::vector<double> pixel_sums;
        if (gpus == 1 && !(flags & RT_MULTI_COLLECTIVE)) {
            pixel_sums = render(s, camera, background, image_width, image_height, samples_per_pixel, max_depth, seed, flags);
        } else {                                                            // every GPU of the node from this one process
            if (gpus < 0 || gpus > 32) throw Error("--gpus must be 0 (all) .. 32");
            const uint32_t mask = gpus == 0 ? 0u : (gpus == 32 ? 0xFFFFFFFFu : ((1u << gpus) - 1u));
            pixel_sums = render_multi(s, camera, background, image_width, image_height, samples_per_pixel, max_depth, mask, seed, flags);
            double ms[4]; rt_last_multi_ms(s.raw(), ms);
            std::fprintf(stderr, "rt_render_multi: slowest kernel %.2f ms, gather %.3f ms, un-permute %.3f ms, call %.2f ms\n", ms[0], ms[1], ms[2], ms[3]);
        }
        // the guide: sample 0's records, or the averaged records of samples [0, --denoise-guide N)
        if (want_denoise && chain.max_links) {                              // guide and albedo from one chain query over the guide's samples
            const uint32_t n = guide_samples ? guide_samples : 1u;
            std::vector<double> albedo_sum;
            const std::vector<double> guide = query_camera_chain_guide(s, camera, image_width, image_height, chain, 0u, n, seed, albedo_samples ? &albedo_sum : nullptr);
            pixel_sums = albedo_samples ? denoise_albedo(pixel_sums, samples_per_pixel, albedo_sum, n, guide, image_width, image_height, dn)
                                        : denoise(pixel_sums, samples_per_pixel, guide, image_width, image_height, dn);
            want_denoise = false;
        }
        auto guide_records = [&]() { return guide_samples > 1u ? query_camera_guide(s, camera, image_width, image_height, 0u, guide_samples, seed)
                                                               : query_camera_records(s, camera, image_width, image_height, 0u, seed); };
        if (want_denoise && albedo_samples)
            pixel_sums = denoise_albedo(pixel_sums, samples_per_pixel, query_camera_albedo(s, camera, image_width, image_height, 0u, albedo_samples, seed), albedo_samples,
                                        guide_records(), image_width, image_height, dn);
        else if (want_denoise) pixel_sums = denoise(pixel_sums, samples_per_pixel, guide_records(), image_width, image_height, dn);
        write_ppm("-", pixel_sums, image_width, image_height, samples_per_pixel);              // main.rs:767-769,832
        std::fprintf(stderr, "Done.\n");                                                      // main.rs:835
    } catch (const Error& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

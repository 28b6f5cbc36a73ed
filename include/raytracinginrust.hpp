// include/raytracinginrust.hpp — C++ host API mirroring the reference's Rust scene-builder surface
// (4meame/RayTracingInRust) over the C-ABI of include/rt_amd.h.
//
// The reference is one Rust binary whose `main` builds `(world, lights)` with constructors such as
// `Sphere::new`, `AARect::new(Plane::XZ, ..)`, `Translate::new(Rotate::new(Axis::Y, Cube::new(..), -18.0), ..)`
// (src/main.rs:278-311) and then runs the per-pixel sample loop (src/main.rs:772-833).  No Rust toolchain exists in
// this environment, so the host side is C++ with the same names and argument order; every `T::new_(..)` below
// forwards to the C-ABI entry point a Rust `extern "C"` block would bind.  Failures the
// reference reports by panic (src/bvh.rs:55, src/main.rs:431) surface as rtr::Error.
#pragma once
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "rt_amd.h"

namespace rtr {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

struct Vec3 {                                    // src/vec.rs:10-22
    double e[3];
    Vec3() : e{0, 0, 0} {}
    Vec3(double a, double b, double c) : e{a, b, c} {}
    static Vec3 new_(double a, double b, double c) { return Vec3(a, b, c); }
    double x() const { return e[0]; } double y() const { return e[1]; } double z() const { return e[2]; }
    Vec3 operator+(const Vec3& o) const { return Vec3(e[0] + o.e[0], e[1] + o.e[1], e[2] + o.e[2]); }
    Vec3 operator*(const Vec3& o) const { return Vec3(e[0] * o.e[0], e[1] * o.e[1], e[2] * o.e[2]); }
    Vec3 operator*(double s) const { return Vec3(e[0] * s, e[1] * s, e[2] * s); }
};
using Point3 = Vec3;
using Color = Vec3;

enum class Plane { XY = RT_PLANE_XY, XZ = RT_PLANE_XZ, YZ = RT_PLANE_YZ };   // src/rect.rs:9-13
enum class Axis { X = RT_AXIS_X, Y = RT_AXIS_Y, Z = RT_AXIS_Z };             // src/rotate.rs:8-12

// rand::thread_rng() stand-in for scene construction (seeded; csrc/rt_rng.h)
class Rng {
public:
    Rng(uint64_t seed, uint32_t stream) : r_(rt_rng_create(seed, stream)) {}
    ~Rng() { rt_rng_destroy(r_); }
    Rng(const Rng&) = delete; Rng& operator=(const Rng&) = delete;
    double gen_f64() { return rt_rng_f64(r_); }                                  // rng.gen::<f64>()
    double gen_range(double a, double b) { return rt_rng_range(r_, a, b); }      // rng.gen_range(a..b)
    Color color_random(double a, double b) { double x = gen_range(a, b), y = gen_range(a, b), z = gen_range(a, b); return Color(x, y, z); }   // Color::random, vec.rs:70-76
    rt_rng* raw() { return r_; }
private:
    rt_rng* r_;
};

// One scene: owns the C handle.  Texture / Material / Hittable are typed ids into it.
class Scene;
struct Texture { int id; };
struct Material { int id; };
struct Hittable { int id; };

class Scene {
public:
    Scene() : s_(rt_scene_create()) { if (!s_) throw Error("rt_scene_create failed"); }
    ~Scene() { rt_scene_destroy(s_); }
    Scene(const Scene&) = delete; Scene& operator=(const Scene&) = delete;
    rt_scene* raw() const { return s_; }
    int chk(int rc) const { if (rc < 0) throw Error(rt_scene_error(s_)); return rc; }
    void set(Hittable world, const std::vector<Hittable>& lights) {              // the (world, lights) pair, main.rs:153
        chk(rt_scene_set_world(s_, world.id));
        for (auto l : lights) chk(rt_lights_push(s_, l.id));
    }
    // not in the reference: opt-in SAH tree for `BVH::new_` (default: the reference's widest-axis object-median split, bvh.rs:18-73)
    void set_bvh_builder(rt_bvh_builder mode) { if (rt_scene_set_bvh_builder(s_, (int)mode) != 0) throw Error(rt_last_error()); }
private:
    rt_scene* s_;
};

// ---- textures (src/texture.rs)
struct ConstantTexture { static Texture new_(Scene& s, Color c) { return {s.chk(rt_texture_constant(s.raw(), c.e))}; } };
struct CheckTexture { static Texture new_(Scene& s, Texture odd, Texture even) { return {s.chk(rt_texture_check(s.raw(), odd.id, even.id))}; } };
struct NoiseTexture { static Texture new_(Scene& s, double scale, Rng& rng) { return {s.chk(rt_texture_noise(s.raw(), scale, rng.raw()))}; } };
struct ImageTexture { static Texture new_(Scene& s, const std::vector<uint8_t>& data, uint32_t w, uint32_t h) { return {s.chk(rt_texture_image(s.raw(), data.data(), w, h))}; } };

// ---- materials (src/mat.rs)
struct Lambertian { static Material new_(Scene& s, Texture albedo) { return {s.chk(rt_material_lambertian(s.raw(), albedo.id))}; } };
struct Metal { static Material new_(Scene& s, Color albedo, double fuzz) { return {s.chk(rt_material_metal(s.raw(), albedo.e, fuzz))}; } };
struct Dielectric { static Material new_(Scene& s, double ir) { return {s.chk(rt_material_dielectric(s.raw(), ir))}; } };
struct DiffuseLight { static Material new_(Scene& s, Texture emit) { return {s.chk(rt_material_diffuse_light(s.raw(), emit.id))}; } };
struct Isotropic { static Material new_(Scene& s, Texture albedo) { return {s.chk(rt_material_isotropic(s.raw(), albedo.id))}; } };
struct PBR {                                            // src/mat.rs:101
    static Material new_(Scene& s, Texture base_color, double metallic, double subsurface, double specular, double roughness, double specular_tint,
                         double anisotropic, double sheen, double sheen_tint, double clearcoat, double clearcoat_gloss) {
        const double p[10] = {metallic, subsurface, specular, roughness, specular_tint, anisotropic, sheen, sheen_tint, clearcoat, clearcoat_gloss};
        return {s.chk(rt_material_pbr(s.raw(), base_color.id, p))};
    }
};

// ---- hittables
struct Sphere { static Hittable new_(Scene& s, Point3 c, double r, Material m) { return {s.chk(rt_sphere(s.raw(), c.e, r, m.id))}; } };
struct MovingSphere { static Hittable new_(Scene& s, Point3 c0, Point3 c1, double t0, double t1, double r, Material m) { return {s.chk(rt_moving_sphere(s.raw(), c0.e, c1.e, t0, t1, r, m.id))}; } };
struct AARect { static Hittable new_(Scene& s, Plane p, double a0, double a1, double b0, double b1, double k, Material m) { return {s.chk(rt_aarect(s.raw(), (int)p, a0, a1, b0, b1, k, m.id))}; } };
struct Cube { static Hittable new_(Scene& s, Point3 mn, Point3 mx, Material m) { return {s.chk(rt_cube(s.raw(), mn.e, mx.e, m.id))}; } };
struct Triangle { static Hittable new_(Scene& s, const std::array<Point3, 3>& v, Material m) { double f[9]; for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) f[i * 3 + k] = v[i].e[k]; return {s.chk(rt_triangle(s.raw(), f, m.id))}; } };
struct FlipNormal { static Hittable new_(Scene& s, Hittable h) { return {s.chk(rt_flip_normal(s.raw(), h.id))}; } };
struct Translate { static Hittable new_(Scene& s, Hittable h, Vec3 off) { return {s.chk(rt_translate(s.raw(), h.id, off.e))}; } };
struct Rotate { static Hittable new_(Scene& s, Axis a, Hittable h, double angle) { return {s.chk(rt_rotate(s.raw(), (int)a, h.id, angle))}; } };
struct ConstantMedium { static Hittable new_(Scene& s, Hittable boundary, double density, Texture t) { return {s.chk(rt_constant_medium(s.raw(), boundary.id, density, t.id))}; } };

class HittableList {                                    // src/hit.rs:46-56
public:
    explicit HittableList(Scene& s) : s_(s), h_{s.chk(rt_list_create(s.raw()))} {}
    void push(Hittable h) { s_.chk(rt_list_push(s_.raw(), h_.id, h.id)); }
    operator Hittable() const { return h_; }
    Hittable handle() const { return h_; }
private:
    Scene& s_; Hittable h_;
};

struct BVH {                                            // src/bvh.rs:18
    static Hittable new_(Scene& s, const std::vector<Hittable>& hit, double t0, double t1) {
        std::vector<int> ids; for (auto h : hit) ids.push_back(h.id);
        return {s.chk(rt_bvh(s.raw(), ids.data(), (uint32_t)ids.size(), t0, t1))};
    }
    static Hittable of_list(Scene& s, Hittable list, double t0, double t1) { return {s.chk(rt_bvh_of_list(s.raw(), list.id, t0, t1))}; }   // BVH::new(obj.tris.list, ..), main.rs:442
};

struct Mesh {                                           // src/mesh.rs
    Hittable tris;                                      // the `tris` HittableList
    static Mesh new_(Scene& s, const std::vector<Vec3>& positions, const std::vector<uint32_t>& indices, Material m) {
        std::vector<double> p; for (auto& v : positions) { p.push_back(v.e[0]); p.push_back(v.e[1]); p.push_back(v.e[2]); }
        return Mesh{{s.chk(rt_mesh(s.raw(), p.data(), (uint32_t)positions.size(), indices.data(), (uint32_t)indices.size(), m.id))}};
    }
    // Mesh::load_obj(path, offset, scale, material) -> Result<Mesh, String>, src/mesh.rs:33-61 (throws on failure)
    static Mesh load_obj(Scene& s, const std::string& path, Vec3 offset, double scale, Material m) {
        return Mesh{{s.chk(rt_mesh_load_obj(s.raw(), path.c_str(), offset.e, scale, m.id))}};
    }
};

struct Camera {                                         // src/camera.rs:19
    rt_camera c;
    static Camera new_(Point3 lookfrom, Point3 lookat, Vec3 vup, double vfov, double aspect_ratio, double aperture,
                       double focus_dist, double time0, double time1) {
        Camera k;
        for (int i = 0; i < 3; i++) { k.c.lookfrom[i] = lookfrom.e[i]; k.c.lookat[i] = lookat.e[i]; k.c.vup[i] = vup.e[i]; }
        k.c.vfov = vfov; k.c.aspect = aspect_ratio; k.c.aperture = aperture; k.c.focus_dist = focus_dist; k.c.time0 = time0; k.c.time1 = time1;
        return k;
    }
};

// The render loop of src/main.rs:772-833 as one call: per-pixel sums of ray_color in output order.
inline std::vector<double> render(Scene& s, const Camera& cam, Color background, uint32_t W, uint32_t H, uint32_t samples_per_pixel,
                                  uint32_t max_depth, uint64_t seed = 0x5EED, uint32_t flags = RT_F64) {
    std::vector<double> out((size_t)W * H * 3);
    if (rt_render(s.raw(), &cam.c, background.e, W, H, samples_per_pixel, max_depth, seed, flags, out.data()) != 0) throw Error(rt_last_error());
    return out;
}
// The same loop on several GPUs of this node (device_mask: bit d = HIP device d, 0 = all visible): tiles dealt round-robin, one RCCL
// gather to the first device, un-permuted there (rt_render_multi).
inline std::vector<double> render_multi(Scene& s, const Camera& cam, Color background, uint32_t W, uint32_t H, uint32_t samples_per_pixel,
                                        uint32_t max_depth, uint32_t device_mask, uint64_t seed = 0x5EED, uint32_t flags = RT_F64, uint32_t tile_px = 0) {
    std::vector<double> out((size_t)W * H * 3);
    if (rt_render_multi(s.raw(), &cam.c, background.e, W, H, samples_per_pixel, max_depth, seed, flags, device_mask, tile_px, out.data()) != 0) throw Error(rt_last_error());
    return out;
}
// main.rs:767-769,832
inline void write_ppm(const char* path, const std::vector<double>& rgb_sum, uint32_t W, uint32_t H, uint64_t spp) {
    if (rt_write_ppm(path, rgb_sum.data(), W, H, spp) != 0) throw Error(rt_last_error());
}

// Ray queries (rt_query_*): `world.hit(&r, 0.00001, f64::INFINITY)` (src/main.rs:48) as a call — the closest hit of rays of the caller's, or
// of the camera rays of one sample of every pixel (picking, auto-focus, depth / normal / material-id frames).  Hit is HitRecord
// (src/hit.rs:9-24) plus what identifies the thing that was hit; `material` is the id of the Material the builder returned (-1: a
// ConstantMedium's, or a miss), `object` the index in the flattened object table, prim_kind 0 rect, 1 sphere, 2 moving sphere, 3 triangle
// (-1: a medium, or a miss).
struct Hit {
    bool hit = false; double t = 0.0; Point3 position; Vec3 normal; bool front_face = false; double u = 0.0, v = 0.0;
    int material = -1, object = -1, prim_kind = -1, prim_index = -1;
    static Hit from_record(const double* r) {
        Hit h; h.hit = r[0] != 0.0; h.t = r[1]; h.position = Point3(r[2], r[3], r[4]); h.normal = Vec3(r[5], r[6], r[7]); h.front_face = r[8] != 0.0;
        h.u = r[9]; h.v = r[10]; h.material = (int)r[11]; h.object = (int)r[12]; h.prim_kind = (int)r[13]; h.prim_index = (int)r[14];
        return h;
    }
};
struct Ray { Point3 origin; Vec3 direction; double time = 0.0; };        // src/ray.rs:6-10
// world.hit(ray, t_min, +inf) for every ray; ray k draws from the stream Rng(seed, k) where a ConstantMedium needs a random number
inline std::vector<Hit> query_hits(Scene& s, const std::vector<Ray>& rays, double t_min = 0.00001, uint64_t seed = 0) {
    std::vector<double> in(rays.size() * 7), rec(rays.size() * 16);
    for (size_t k = 0; k < rays.size(); k++) {
        for (int a = 0; a < 3; a++) { in[k * 7 + a] = rays[k].origin.e[a]; in[k * 7 + 3 + a] = rays[k].direction.e[a]; }
        in[k * 7 + 6] = rays[k].time;
    }
    if (rt_query_hits(s.raw(), (uint32_t)rays.size(), in.data(), t_min, seed, 0, rec.data()) != 0) throw Error(rt_last_error());
    std::vector<Hit> out(rays.size());
    for (size_t k = 0; k < rays.size(); k++) out[k] = Hit::from_record(&rec[k * 16]);
    return out;
}
// The camera ray of sample `sample` of every pixel — the ray a frame with that seed traces — and its closest hit: W*H hits in output
// order (row 0 = top); rays_out (optional) receives the rays.
inline std::vector<Hit> query_camera(Scene& s, const Camera& cam, uint32_t W, uint32_t H, uint32_t sample = 0, uint64_t seed = 0x5EED,
                                     std::vector<Ray>* rays_out = nullptr) {
    const size_t n = (size_t)W * H;
    std::vector<double> rec(n * 16), rays(rays_out ? n * 7 : 0);
    if (rt_query_camera(s.raw(), &cam.c, W, H, sample, seed, 0, rays_out ? rays.data() : nullptr, rec.data()) != 0) throw Error(rt_last_error());
    std::vector<Hit> out(n);
    for (size_t k = 0; k < n; k++) out[k] = Hit::from_record(&rec[k * 16]);
    if (rays_out) {
        rays_out->resize(n);
        for (size_t k = 0; k < n; k++) { Ray& r = (*rays_out)[k]; r.origin = Point3(rays[k * 7], rays[k * 7 + 1], rays[k * 7 + 2]); r.direction = Vec3(rays[k * 7 + 3], rays[k * 7 + 4], rays[k * 7 + 5]); r.time = rays[k * 7 + 6]; }
    }
    return out;
}

// The same query as the raw records rt_query_camera writes, 16 doubles per pixel: what `denoise` takes as its guide.
inline std::vector<double> query_camera_records(Scene& s, const Camera& cam, uint32_t W, uint32_t H, uint32_t sample = 0, uint64_t seed = 0x5EED) {
    std::vector<double> rec((size_t)W * H * 16);
    if (rt_query_camera(s.raw(), &cam.c, W, H, sample, seed, 0, nullptr, rec.data()) != 0) throw Error(rt_last_error());
    return rec;
}

// Denoising (rt_denoise*): an edge-avoiding a-trous wavelet filter over a frame of sums, guided by query_camera_records — K iterations of a
// 5x5 B3 kernel dilated by 2^i, with stops on colour (sigma_c), normal (sigma_n), plane distance relative to the hit distance (sigma_p) and
// hit / miss (with RT_DENOISE_SAME_MATERIAL: the material too).  The defaults are render.py's (DESIGN.md §14's error table).  Returns sums
// again (mean times samples): write_ppm takes them with the same sample count.
struct DenoiseSettings {
    uint32_t iterations = 2; double sigma[3] = {4.0, 0.5, 0.02}; uint32_t flags = 0;
};
inline std::vector<double> denoise(const std::vector<double>& rgb_sum, uint64_t samples, const std::vector<double>& hit_records, uint32_t W, uint32_t H,
                                   const DenoiseSettings& d = DenoiseSettings()) {
    if (rgb_sum.size() != (size_t)W * H * 3 || hit_records.size() != (size_t)W * H * 16) throw Error("denoise: frame or records of another size");
    std::vector<double> out(rgb_sum.size());
    if (rt_denoise(rgb_sum.data(), samples, hit_records.data(), W, H, d.iterations, d.sigma, d.flags, out.data()) != 0) throw Error(rt_last_error());
    return out;
}
// the host twin: the same words without a device
inline std::vector<double> denoise_host(const std::vector<double>& rgb_sum, uint64_t samples, const std::vector<double>& hit_records, uint32_t W, uint32_t H,
                                        const DenoiseSettings& d = DenoiseSettings()) {
    if (rgb_sum.size() != (size_t)W * H * 3 || hit_records.size() != (size_t)W * H * 16) throw Error("denoise_host: frame or records of another size");
    std::vector<double> out(rgb_sum.size());
    if (rt_denoise_host(rgb_sum.data(), samples, hit_records.data(), W, H, d.iterations, d.sigma, d.flags, out.data()) != 0) throw Error(rt_last_error());
    return out;
}

// Albedo queries (rt_query_albedo, rt_query_camera_albedo): the reflectance at the closest hit — the texture value under a Lambertian, PBR
// or ConstantMedium hit, a Metal's albedo, (1, 1, 1) for glass, emitters and misses.  query_albedo: n x 3 doubles for caller rays (hits_out,
// optional, receives the hits of query_hits for the same rays and seed).  query_camera_albedo: W*H*3 doubles in output order, per pixel the
// SUM over samples [first_sample, first_sample + n_samples) of the albedo under that sample's camera ray — what `denoise_albedo` divides by.
inline std::vector<double> query_albedo(Scene& s, const std::vector<Ray>& rays, double t_min = 0.00001, uint64_t seed = 0, std::vector<Hit>* hits_out = nullptr) {
    std::vector<double> in(rays.size() * 7), out(rays.size() * 3), rec(hits_out ? rays.size() * 16 : 0);
    for (size_t k = 0; k < rays.size(); k++) {
        for (int a = 0; a < 3; a++) { in[k * 7 + a] = rays[k].origin.e[a]; in[k * 7 + 3 + a] = rays[k].direction.e[a]; }
        in[k * 7 + 6] = rays[k].time;
    }
    if (rt_query_albedo(s.raw(), (uint32_t)rays.size(), in.data(), t_min, seed, 0, out.data(), hits_out ? rec.data() : nullptr) != 0) throw Error(rt_last_error());
    if (hits_out) { hits_out->resize(rays.size()); for (size_t k = 0; k < rays.size(); k++) (*hits_out)[k] = Hit::from_record(&rec[k * 16]); }
    return out;
}
inline std::vector<double> query_camera_albedo(Scene& s, const Camera& cam, uint32_t W, uint32_t H, uint32_t first_sample = 0, uint32_t n_samples = 1,
                                               uint64_t seed = 0x5EED) {
    std::vector<double> out((size_t)W * H * 3);
    if (rt_query_camera_albedo(s.raw(), &cam.c, W, H, first_sample, n_samples, seed, 0, out.data()) != 0) throw Error(rt_last_error());
    return out;
}
// `denoise` on rgb_sum / albedo, multiplied back (rt_denoise_albedo): textures are not colour the filter has to preserve.  albedo_sum as
// query_camera_albedo returns it, holding albedo_samples samples per pixel.
inline std::vector<double> denoise_albedo(const std::vector<double>& rgb_sum, uint64_t samples, const std::vector<double>& albedo_sum, uint64_t albedo_samples,
                                          const std::vector<double>& hit_records, uint32_t W, uint32_t H, const DenoiseSettings& d = DenoiseSettings()) {
    if (rgb_sum.size() != (size_t)W * H * 3 || albedo_sum.size() != rgb_sum.size() || hit_records.size() != (size_t)W * H * 16) throw Error("denoise_albedo: frame, albedo or records of another size");
    std::vector<double> out(rgb_sum.size());
    if (rt_denoise_albedo(rgb_sum.data(), samples, albedo_sum.data(), albedo_samples, hit_records.data(), W, H, d.iterations, d.sigma, d.flags, out.data()) != 0) throw Error(rt_last_error());
    return out;
}

// Averaged denoising guides (rt_query_camera_guide, csrc/rt_guide.h): the first-hit records of samples [first_sample, first_sample +
// n_samples) of every pixel reduced to one record in the 16-double layout of query_camera's — hit by majority, t / position / normal /
// front_face as means over the hitting samples, material / object where they agree (else -1), the coverage count in word [15] — which
// every `hit_records` parameter of the denoise family takes unchanged.  albedo_sum_out (optional) receives the W*H*3 sums of
// query_camera_albedo for the same samples, from the same searches.
inline std::vector<double> query_camera_guide(Scene& s, const Camera& cam, uint32_t W, uint32_t H, uint32_t first_sample = 0, uint32_t n_samples = 16,
                                              uint64_t seed = 0x5EED, std::vector<double>* albedo_sum_out = nullptr) {
    std::vector<double> out((size_t)W * H * 16);
    if (albedo_sum_out) albedo_sum_out->assign((size_t)W * H * 3, 0.0);
    if (rt_query_camera_guide(s.raw(), &cam.c, W, H, first_sample, n_samples, seed, 0, out.data(), albedo_sum_out ? albedo_sum_out->data() : nullptr) != 0) throw Error(rt_last_error());
    return out;
}
// Specular-chain guides (rt_query_chain, rt_query_camera_chain_guide, csrc/rt_chain.h): rays followed through mirrors (fuzz <= max_fuzz) and glass
// to the first non-specular surface, up to max_links (0 .. 64) links.  The records are in query_camera_records' layout with word [1] the path
// length in units of the first ray's parameter and word [15] the links followed; the albedo is that surface's times the mirrors' tints.
// max_links = 0 gives the first-hit queries' words.  The default max_fuzz follows perfect mirrors only: an untuned starting value.
struct ChainSettings { uint32_t max_links = 4; double max_fuzz = 0.0; };
// rays: n x 7 doubles (origin, direction, time) -> n x 16; albedo_out (optional): n x 3
inline std::vector<double> query_chain(Scene& s, const std::vector<double>& rays, const ChainSettings& c = ChainSettings(), double t_min = 1e-5, uint64_t seed = 0,
                                       std::vector<double>* albedo_out = nullptr) {
    if (rays.size() % 7u != 0u) throw Error("query_chain: rays are 7 doubles each");
    const uint32_t n = (uint32_t)(rays.size() / 7u);
    std::vector<double> out((size_t)n * 16);
    if (albedo_out) albedo_out->assign((size_t)n * 3, 0.0);
    if (rt_query_chain(s.raw(), n, rays.data(), t_min, seed, c.max_links, c.max_fuzz, 0, out.data(), albedo_out ? albedo_out->data() : nullptr) != 0) throw Error(rt_last_error());
    return out;
}
// query_camera_guide over chain records: what every `hit_records` parameter of the denoise family takes; albedo_sum_out (optional) W*H*3 sums of
// the chain albedos, links_out (optional) W*H counts of the links followed over all samples
inline std::vector<double> query_camera_chain_guide(Scene& s, const Camera& cam, uint32_t W, uint32_t H, const ChainSettings& c = ChainSettings(), uint32_t first_sample = 0,
                                                    uint32_t n_samples = 16, uint64_t seed = 0x5EED, std::vector<double>* albedo_sum_out = nullptr,
                                                    std::vector<uint32_t>* links_out = nullptr) {
    std::vector<double> out((size_t)W * H * 16);
    if (albedo_sum_out) albedo_sum_out->assign((size_t)W * H * 3, 0.0);
    if (links_out) links_out->assign((size_t)W * H, 0u);
    if (rt_query_camera_chain_guide(s.raw(), &cam.c, W, H, first_sample, n_samples, seed, c.max_links, c.max_fuzz, 0, out.data(),
                                    albedo_sum_out ? albedo_sum_out->data() : nullptr, links_out ? links_out->data() : nullptr) != 0) throw Error(rt_last_error());
    return out;
}
// the specification on the host (no device): hit_records = n_samples x n_px x 16 doubles, sample-major -> n_px x 16
inline std::vector<double> guide_from_hits(const std::vector<double>& hit_records, uint32_t n_samples, uint64_t n_px) {
    if (n_samples == 0 || hit_records.size() != (size_t)n_samples * n_px * 16) throw Error("guide_from_hits: records of another size");
    std::vector<double> out((size_t)n_px * 16);
    if (rt_guide_from_hits_host(hit_records.data(), n_samples, n_px, out.data()) != 0) throw Error(rt_last_error());
    return out;
}

// ray_color (src/main.rs:41-120) along rays the caller chooses (rt_query_radiance), samples_per_ray samples of each: per ray the SUM over
// its samples, n x 3, as render() returns per pixel — another projection than Camera's, a light probe, a baked light map.  Sample s of ray k
// draws from the stream of rt_rng_path(seed, k, s).  samples_out (optional) receives every sample, ray-major; nonfinite_out (optional) the
// number of samples with a non-finite component.
inline std::vector<double> query_radiance(Scene& s, const std::vector<Ray>& rays, uint32_t samples_per_ray, uint32_t max_depth,
                                          Color background = Color(0.0, 0.0, 0.0), uint64_t seed = 0x5EED, uint32_t flags = 0,
                                          std::vector<double>* samples_out = nullptr, uint64_t* nonfinite_out = nullptr) {
    std::vector<double> in(rays.size() * 7), sums(rays.size() * 3);
    for (size_t k = 0; k < rays.size(); k++) {
        for (int a = 0; a < 3; a++) { in[k * 7 + a] = rays[k].origin.e[a]; in[k * 7 + 3 + a] = rays[k].direction.e[a]; }
        in[k * 7 + 6] = rays[k].time;
    }
    if (samples_out) samples_out->assign(rays.size() * (size_t)samples_per_ray * 3, 0.0);
    if (rt_query_radiance(s.raw(), (uint32_t)rays.size(), in.data(), background.e, samples_per_ray, max_depth, seed, flags, sums.data(),
                          samples_out ? samples_out->data() : nullptr, nonfinite_out) != 0) throw Error(rt_last_error());
    return sums;
}
// The rays of a W x H equirectangular (360 x 180 degree) panorama seen from `origin`, in output order (row 0 = top): row r, column i looks
// along (sin t cos p, cos t, sin t sin p) with t = pi (r + 0.5) / H from +y, p = 2 pi (i + 0.5) / W.  No jitter.
inline std::vector<Ray> equirect_rays(Point3 origin, uint32_t W, uint32_t H, double time = 0.0) {
    const double pi = 3.141592653589793;
    std::vector<double> sp(W), cp(W);
    for (uint32_t i = 0; i < W; i++) { const double phi = 2.0 * pi * ((double)i + 0.5) / (double)W; sp[i] = std::sin(phi); cp[i] = std::cos(phi); }
    std::vector<Ray> rays((size_t)W * H);
    for (uint32_t r = 0; r < H; r++) {
        const double theta = pi * ((double)r + 0.5) / (double)H, st = std::sin(theta), ct = std::cos(theta);
        for (uint32_t i = 0; i < W; i++) { Ray& q = rays[(size_t)r * W + i]; q.origin = origin; q.direction = Vec3(st * cp[i], ct, st * sp[i]); q.time = time; }
    }
    return rays;
}

// The per-pixel error estimate of a frame of passes (rt_moments_*, csrc/rt_moments.h).  ErrorStats: the pixels whose standard error in display
// units (1/256 = one code value) is <= tau / > tau / not finite, and the largest finite e2 (a squared standard error).
struct ErrorStats {
    uint64_t converged = 0, unconverged = 0, nonfinite = 0; double max_e2 = 0.0;
    static ErrorStats from_words(const uint64_t w[4]) { ErrorStats s; s.converged = w[0]; s.unconverged = w[1]; s.nonfinite = w[2]; std::memcpy(&s.max_e2, &w[3], sizeof(double)); return s; }
};
// e2 of every pixel (W*H doubles, output order) from sums and second moments of `passes` passes holding `samples` samples per pixel — the host
// form: no device needed.  stats (optional) receives the statistics for tau.
inline std::vector<double> moments_error(const std::vector<double>& rgb_sum, const std::vector<double>& sq_sum, uint64_t samples, uint64_t passes,
                                         uint32_t W, uint32_t H, double tau = 1.0 / 256.0, ErrorStats* stats = nullptr) {
    if (rgb_sum.size() != (size_t)W * H * 3 || sq_sum.size() != rgb_sum.size()) throw Error("moments_error: frames of another size");
    std::vector<double> e2((size_t)W * H);
    if (rt_moments_error_host(rgb_sum.data(), sq_sum.data(), samples, passes, W, H, e2.data()) != 0) throw Error(rt_last_error());
    if (stats) { uint64_t w[4]; if (rt_moments_stats_host(e2.data(), e2.size(), tau, w) != 0) throw Error(rt_last_error()); *stats = ErrorStats::from_words(w); }
    return e2;
}
// The variance of the mean of every pixel and channel (W*H*3 doubles; rt_moments_variance_host, csrc/rt_moments.h (4)): the V that e2 is
// computed from, and what `denoise_variance` takes as its input.  The host form: no device needed.
inline std::vector<double> moments_variance(const std::vector<double>& rgb_sum, const std::vector<double>& sq_sum, uint64_t samples, uint64_t passes,
                                            uint32_t W, uint32_t H) {
    if (rgb_sum.size() != (size_t)W * H * 3 || sq_sum.size() != rgb_sum.size()) throw Error("moments_variance: frames of another size");
    std::vector<double> var(rgb_sum.size());
    if (rt_moments_variance_host(rgb_sum.data(), sq_sum.data(), samples, passes, W, H, var.data()) != 0) throw Error(rt_last_error());
    return var;
}
// Variance-guided denoising (rt_denoise_variance, csrc/rt_denoise_var.h): `denoise` with its colour stop measured in standard deviations of
// the two pixels a tap compares, from `var` (moments_variance, Progressive::variance).  sigma = {sigma_v, sigma_n, sigma_p}; the default
// sigma_v is render.py's.  var_out (optional): the filtered variance, W*H doubles.
struct DenoiseVarianceSettings {
    uint32_t iterations = 2; double sigma[3] = {3.0, 0.5, 0.02}; uint32_t flags = 0;
};
inline std::vector<double> denoise_variance(const std::vector<double>& rgb_sum, uint64_t samples, const std::vector<double>& var, const std::vector<double>& hit_records,
                                            uint32_t W, uint32_t H, const DenoiseVarianceSettings& d = DenoiseVarianceSettings(), std::vector<double>* var_out = nullptr) {
    if (rgb_sum.size() != (size_t)W * H * 3 || var.size() != rgb_sum.size() || hit_records.size() != (size_t)W * H * 16) throw Error("denoise_variance: frame, variance or records of another size");
    std::vector<double> out(rgb_sum.size());
    if (var_out) var_out->resize((size_t)W * H);
    if (rt_denoise_variance(rgb_sum.data(), samples, var.data(), hit_records.data(), W, H, d.iterations, d.sigma, d.flags, out.data(), var_out ? var_out->data() : nullptr) != 0) throw Error(rt_last_error());
    return out;
}
// The variance frame of a frame with per-pixel counts (rt_adaptive_variance_host, csrc/rt_denoise_frame.h (E)): `moments_variance` with
// every pixel's own sample and pass counts; +inf where a pixel has fewer than two passes.  The host form: no device needed.
inline std::vector<double> adaptive_variance(const std::vector<double>& rgb_sum, const std::vector<double>& sq_sum, const std::vector<uint32_t>& counts,
                                             const std::vector<uint32_t>& passes, uint32_t W, uint32_t H) {
    if (rgb_sum.size() != (size_t)W * H * 3 || sq_sum.size() != rgb_sum.size() || counts.size() != (size_t)W * H || passes.size() != counts.size())
        throw Error("adaptive_variance: frames of another size");
    std::vector<double> var(rgb_sum.size());
    if (rt_adaptive_variance_host(rgb_sum.data(), sq_sum.data(), counts.data(), passes.data(), W, H, var.data()) != 0) throw Error(rt_last_error());
    return var;
}
// Denoising a frame as it is (rt_denoise_frame, csrc/rt_denoise_frame.h): `denoise`, `denoise_albedo` and `denoise_variance` composed, for one
// sample count or a count per pixel.  counts: null, or W*H per-pixel sample counts (then `samples` is ignored); var: null (the colour stop,
// sigma[0] = sigma_c), or W*H*3 variances (the variance stop, sigma[0] = sigma_v); albedo_sum: null, or W*H*3 sums of albedo_samples samples.
struct DenoiseFrameSettings {
    bool variance = false; uint32_t albedo_samples = 0;          // what Progressive::rgb8_denoised_frame uses of the frame's own
    uint32_t iterations = 2; double sigma[3] = {4.0, 0.5, 0.02}; uint32_t flags = 0;
    static DenoiseFrameSettings with_variance(uint32_t albedo_samples = 0) { DenoiseFrameSettings d; d.variance = true; d.albedo_samples = albedo_samples; d.sigma[0] = 3.0; return d; }
};
inline std::vector<double> denoise_frame(const std::vector<double>& rgb_sum, const std::vector<uint32_t>* counts, uint64_t samples, const std::vector<double>* var,
                                         const std::vector<double>* albedo_sum, uint64_t albedo_samples, const std::vector<double>& hit_records, uint32_t W, uint32_t H,
                                         const DenoiseFrameSettings& d = DenoiseFrameSettings(), std::vector<double>* var_out = nullptr) {
    if (rgb_sum.size() != (size_t)W * H * 3 || hit_records.size() != (size_t)W * H * 16 || (counts && counts->size() != (size_t)W * H) || (var && var->size() != rgb_sum.size()) ||
        (albedo_sum && albedo_sum->size() != rgb_sum.size())) throw Error("denoise_frame: frame, counts, variance, albedo or records of another size");
    std::vector<double> out(rgb_sum.size());
    if (var_out) var_out->resize((size_t)W * H);
    if (rt_denoise_frame(rgb_sum.data(), counts ? counts->data() : nullptr, samples, var ? var->data() : nullptr, albedo_sum ? albedo_sum->data() : nullptr, albedo_samples,
                         hit_records.data(), W, H, d.iterations, d.sigma, d.flags, out.data(), var_out ? var_out->data() : nullptr) != 0) throw Error(rt_last_error());
    return out;
}

// Temporal accumulation (rt_reproject, csrc/rt_reproject.h): the previous view's frame — prev_sum with prev_counts (null: prev_samples in every
// pixel) — reprojected into a new view, from the query_camera / query_camera_guide records of the two views.  History: W*H*3 sums and W*H
// counts, 0 where a pixel has none.  The defaults are render.py's starting values, not tuned.  host = true: the plain-C++ twin, no device.
struct ReprojectSettings { uint32_t max_history = 64; double sigma[2] = {0.9, 0.01}; };      // sigma = {normal_min, sigma_p}
struct History { std::vector<double> sum; std::vector<uint32_t> counts; };
inline History reproject(const std::vector<double>& prev_sum, const std::vector<uint32_t>* prev_counts, uint64_t prev_samples, const std::vector<double>& prev_records,
                         const Camera& prev_cam, const std::vector<double>& cur_records, uint32_t W, uint32_t H, const ReprojectSettings& r = ReprojectSettings(),
                         bool host = false) {
    if (prev_sum.size() != (size_t)W * H * 3 || prev_records.size() != (size_t)W * H * 16 || cur_records.size() != prev_records.size() ||
        (prev_counts && prev_counts->size() != (size_t)W * H)) throw Error("reproject: frame, counts or records of another size");
    History h; h.sum.resize(prev_sum.size()); h.counts.resize((size_t)W * H);
    if ((host ? rt_reproject_host : rt_reproject)(prev_sum.data(), prev_counts ? prev_counts->data() : nullptr, prev_samples, prev_records.data(), &prev_cam.c, cur_records.data(),
                                                  W, H, r.max_history, r.sigma, 0, h.sum.data(), h.counts.data()) != 0) throw Error(rt_last_error());
    return h;
}
// The blend of a frame with a history (rt_temporal_blend_host; no device): sums added, counts added — a frame with counts, which
// denoise_frame(counts = ...) takes as it is.
inline History temporal_blend(const std::vector<double>& rgb_sum, const std::vector<uint32_t>* counts, uint64_t samples, const History& history, uint32_t W, uint32_t H) {
    if (rgb_sum.size() != (size_t)W * H * 3 || history.sum.size() != rgb_sum.size() || history.counts.size() != (size_t)W * H || (counts && counts->size() != (size_t)W * H))
        throw Error("temporal_blend: frame, counts or history of another size");
    History out; out.sum.resize(rgb_sum.size()); out.counts.resize((size_t)W * H);
    if (rt_temporal_blend_host(rgb_sum.data(), counts ? counts->data() : nullptr, samples, history.sum.data(), history.counts.data(), W, H, out.sum.data(), out.counts.data()) != 0)
        throw Error(rt_last_error());
    return out;
}

// Temporal variance (rt_reproject_variance, csrc/rt_reproject_var.h): `reproject` with prev_var — W*H*3 variances of the previous frame's per-pixel
// mean — carried along; the history's sums and counts are reproject's words, var is +inf where a pixel has history of unknown variance and +0.0
// where it has none.  host = true: the plain-C++ twin, no device.
struct HistoryVariance { History history; std::vector<double> var; };
inline HistoryVariance reproject_variance(const std::vector<double>& prev_sum, const std::vector<uint32_t>* prev_counts, uint64_t prev_samples, const std::vector<double>& prev_var,
                                          const std::vector<double>& prev_records, const Camera& prev_cam, const std::vector<double>& cur_records, uint32_t W, uint32_t H,
                                          const ReprojectSettings& r = ReprojectSettings(), bool host = false) {
    if (prev_sum.size() != (size_t)W * H * 3 || prev_var.size() != prev_sum.size() || prev_records.size() != (size_t)W * H * 16 || cur_records.size() != prev_records.size() ||
        (prev_counts && prev_counts->size() != (size_t)W * H)) throw Error("reproject_variance: frame, variance, counts or records of another size");
    HistoryVariance h; h.history.sum.resize(prev_sum.size()); h.history.counts.resize((size_t)W * H); h.var.resize(prev_sum.size());
    if ((host ? rt_reproject_variance_host : rt_reproject_variance)(prev_sum.data(), prev_counts ? prev_counts->data() : nullptr, prev_samples, prev_var.data(), prev_records.data(),
                                                                    &prev_cam.c, cur_records.data(), W, H, r.max_history, r.sigma, 0, h.history.sum.data(), h.history.counts.data(),
                                                                    h.var.data()) != 0) throw Error(rt_last_error());
    return h;
}
// The variance of the mean of temporal_blend's frame (rt_temporal_blend_variance_host; no device): var null = unknown everywhere (a frame with
// fewer than two passes); the result is what denoise_frame(counts = the blend's counts, var = ...) takes.
inline std::vector<double> temporal_blend_variance(const std::vector<double>* var, const std::vector<uint32_t>* counts, uint64_t samples, const std::vector<double>& hist_var,
                                                   const std::vector<uint32_t>& hist_counts) {
    if (hist_var.size() != hist_counts.size() * 3 || (var && var->size() != hist_var.size()) || (counts && counts->size() != hist_counts.size()))
        throw Error("temporal_blend_variance: variance, counts or history of another size");
    std::vector<double> out(hist_var.size());
    if (rt_temporal_blend_variance_host(var ? var->data() : nullptr, counts ? counts->data() : nullptr, samples, hist_var.data(), hist_counts.data(), hist_counts.size(),
                                        out.data()) != 0) throw Error(rt_last_error());
    return out;
}

// A progressive frame (rt_progressive_*): the same loop in passes of samples that accumulate on the device, with the reference's
// format_color (src/vec.rs:125-131) resolved there too — progress, preview, stop half-way, "another 1000 samples", save and resume.
class Progressive {
public:
    Progressive(Scene& s, const Camera& cam, Color background, uint32_t W, uint32_t H, uint32_t max_depth, uint64_t seed = 0x5EED, uint32_t flags = RT_F64)
        : p_(rt_progressive_create(s.raw(), &cam.c, background.e, W, H, max_depth, seed, flags)), n_px_((size_t)W * H) { if (!p_) throw Error(rt_last_error()); }
    ~Progressive() { rt_progressive_destroy(p_); }
    Progressive(const Progressive&) = delete; Progressive& operator=(const Progressive&) = delete;
    void* raw() const { return p_; }
    void add(uint32_t n_samples) { chk(rt_progressive_add(p_, n_samples, nullptr)); }                 // samples [done, done + n) of every pixel
    uint64_t samples() const { uint64_t n = 0; chk(rt_progressive_samples(p_, &n)); return n; }
    // format_color(samples()) of every pixel, W*H*3 bytes in output order; changed_px: pixels that differ from the previous resolve
    std::vector<uint8_t> rgb8(uint64_t* changed_px = nullptr) { std::vector<uint8_t> out(n_px_ * 3); chk(rt_progressive_resolve_rgb8(p_, out.data(), changed_px)); return out; }
    // the frame as it is now through `denoise` and format_color on the device (the frame builds and keeps its own guide); rgb8 and its count are untouched
    std::vector<uint8_t> rgb8_denoised(const DenoiseSettings& d = DenoiseSettings()) {
        std::vector<uint8_t> out(n_px_ * 3); chk(rt_progressive_resolve_denoised_rgb8(p_, d.iterations, d.sigma, d.flags, out.data())); return out;
    }
    // the same with albedo demodulation (`denoise_albedo`): the frame builds the albedo sums of samples [0, albedo_samples) itself and keeps them
    std::vector<uint8_t> rgb8_denoised_albedo(uint32_t albedo_samples = 16, const DenoiseSettings& d = DenoiseSettings()) {
        std::vector<uint8_t> out(n_px_ * 3); chk(rt_progressive_resolve_denoised_albedo_rgb8(p_, albedo_samples, d.iterations, d.sigma, d.flags, out.data())); return out;
    }
    // the guide of every denoised resolve: 1 (the default) the camera hits of sample 0, n > 1 `query_camera_guide` over samples [0, n); another
    // value drops the packed guide and the next denoised resolve builds it.  guide_info: the value in force and the guides built so far
    void set_guide_samples(uint32_t n_samples) { chk(rt_progressive_set_guide_samples(p_, n_samples)); }
    // max_links > 0: the guide AND the albedo sums of every denoised resolve come from `query_camera_chain_guide` over samples [0, guide_samples)
    // (the albedo resolves then divide by those sums over guide_samples); 0 (the default): first hits.  set_view reprojects with first hits always.
    void set_guide_chain(uint32_t max_links, double max_fuzz = 0.0) { chk(rt_progressive_set_guide_chain(p_, max_links, max_fuzz)); }
    ChainSettings guide_chain() const { ChainSettings c; chk(rt_progressive_guide_chain_info(p_, &c.max_links, &c.max_fuzz)); return c; }
    struct GuideInfo { uint32_t guide_samples; uint64_t builds; };
    GuideInfo guide_info() const { GuideInfo g{0u, 0u}; chk(rt_progressive_guide_info(p_, &g.guide_samples, &g.builds)); return g; }
    std::vector<double> sum() const { std::vector<double> out(n_px_ * 3); chk(rt_progressive_read_sum(p_, out.data())); return out; }
    void load(const std::vector<double>& rgb_sum, uint64_t samples_done) {
        if (rgb_sum.size() != n_px_ * 3) throw Error("checkpoint of another frame size");
        chk(rt_progressive_load_sum(p_, rgb_sum.data(), samples_done));
    }
    void reset() { chk(rt_progressive_reset(p_)); }                                                   // drops the history set_view keeps
    // Another view of the same scene WITH the frame's history (rt_progressive_set_view): the frame's sums blended with the history it holds are
    // reprojected into the new view; the frame then holds 0 samples of the new camera and seed.  Give every view a NEW seed (the random
    // streams are keyed by pixel and sample, so the same seed under a nearby camera repeats the history's noise).  max_history = 0: a plain
    // change of view.  Not on an adaptive frame.
    void set_view(const Camera& cam, uint64_t seed, const ReprojectSettings& r = ReprojectSettings()) { chk(rt_progressive_set_view(p_, &cam.c, seed, r.max_history, r.sigma)); }
    History history() const { History h; h.sum.resize(n_px_ * 3); h.counts.resize(n_px_); chk(rt_progressive_read_history(p_, h.sum.data(), h.counts.data())); return h; }
    // the resolve of the frame blended with its history, every pixel divided by its own count; iterations >= 1: denoise_frame with the blend's
    // counts in between.  Works with 0 samples once there is history: the preview right after a camera move
    std::vector<uint8_t> rgb8_temporal(uint32_t iterations = 0, const DenoiseSettings& d = DenoiseSettings()) {
        std::vector<uint8_t> out(n_px_ * 3); chk(rt_progressive_resolve_temporal_rgb8(p_, iterations, d.sigma, d.flags, out.data())); return out;
    }
    // ... on a frame with moments: the variance of the history's mean, which set_view carries along (+inf: unknown; all +0.0 without a history), and
    // the temporal resolve through the variance stop on the blend's own variance, d.sigma = {sigma_v, sigma_n, sigma_p}, iterations 1 .. 8
    std::vector<double> history_variance() const { std::vector<double> out(n_px_ * 3); chk(rt_progressive_read_history_variance(p_, out.data())); return out; }
    std::vector<uint8_t> rgb8_temporal_variance(const DenoiseVarianceSettings& d = DenoiseVarianceSettings(), uint32_t albedo_samples = 0) {
        std::vector<uint8_t> out(n_px_ * 3); chk(rt_progressive_resolve_temporal_variance_rgb8(p_, albedo_samples, d.iterations, d.sigma, d.flags, out.data())); return out;
    }
    // moments (rt_progressive_enable_moments): only while the frame holds 0 samples; from then on every pass is also merged into the second
    // moment of the pass sums, and once two passes are in error_map / error_stats estimate every pixel's standard error
    void enable_moments() { chk(rt_progressive_enable_moments(p_)); }
    uint64_t passes() const { uint64_t n = 0; chk(rt_progressive_passes(p_, &n)); return n; }
    std::vector<double> sq_sum() const { std::vector<double> out(n_px_ * 3); chk(rt_progressive_read_moments(p_, out.data())); return out; }
    void load(const std::vector<double>& rgb_sum, const std::vector<double>& sq_sum, uint64_t samples_done, uint64_t passes) {
        if (rgb_sum.size() != n_px_ * 3 || sq_sum.size() != n_px_ * 3) throw Error("checkpoint of another frame size");
        chk(rt_progressive_load_moments(p_, rgb_sum.data(), sq_sum.data(), samples_done, passes));
    }
    std::vector<double> error_map() { std::vector<double> out(n_px_); chk(rt_progressive_error_map(p_, out.data())); return out; }      // e2, W*H doubles
    ErrorStats error_stats(double tau) { uint64_t w[4]; chk(rt_progressive_error_stats(p_, tau, w)); return ErrorStats::from_words(w); }
    std::vector<double> variance() { std::vector<double> out(n_px_ * 3); chk(rt_progressive_variance(p_, out.data())); return out; }    // the variance of the mean, W*H*3 doubles
    // the frame as it is now through `denoise_variance`, guided by its own variance, and format_color, all on the device; needs moments and two passes
    std::vector<uint8_t> rgb8_denoised_variance(const DenoiseVarianceSettings& d = DenoiseVarianceSettings()) {
        std::vector<uint8_t> out(n_px_ * 3); chk(rt_progressive_resolve_denoised_variance_rgb8(p_, d.iterations, d.sigma, d.flags, out.data())); return out;
    }
    // adaptive sampling (rt_progressive_enable_adaptive): per-pixel sample counts on a frame with moments, only while it holds 0 samples.
    // add_adaptive: one pass of n_samples over the pixels whose estimated standard error exceeds tau (spread = 1: and their 8 neighbours)
    // and that stay within max_samples (0: 2^32 - 1); listed == 0 is the stop condition, nothing was rendered
    struct AdaptiveInfo { uint64_t listed, samples, total, kernel; };      // pixels sampled, samples rendered, the sum of all counts, 0 the frames' / 1 the list kernel
    void enable_adaptive() { chk(rt_progressive_enable_adaptive(p_)); }
    AdaptiveInfo add_adaptive(uint32_t n_samples, double tau, uint64_t max_samples = 0, uint32_t spread = 1) {
        uint64_t w[4]; chk(rt_progressive_add_adaptive(p_, n_samples, tau, max_samples, spread, w)); return AdaptiveInfo{w[0], w[1], w[2], w[3]};
    }
    std::vector<uint32_t> counts() const { std::vector<uint32_t> out(n_px_); chk(rt_progressive_read_counts(p_, out.data(), nullptr)); return out; }      // n[p], W*H
    // `variance` for any frame with moments: on an adaptive frame from every pixel's own counts (+inf where a pixel has fewer than two passes)
    std::vector<double> variance_counts() { std::vector<double> out(n_px_ * 3); chk(rt_progressive_variance_counts(p_, out.data())); return out; }
    // the denoised resolve of the frame as it is (`denoise_frame`): works on adaptive frames whose counts differ, and combines the variance stop
    // (d.variance; needs moments) with albedo demodulation (d.albedo_samples >= 1)
    std::vector<uint8_t> rgb8_denoised_frame(const DenoiseFrameSettings& d = DenoiseFrameSettings()) {
        std::vector<uint8_t> out(n_px_ * 3);
        chk(rt_progressive_resolve_denoised_frame_rgb8(p_, d.variance ? RT_DENOISE_STOP_VARIANCE : RT_DENOISE_STOP_COLOUR, d.albedo_samples, d.iterations, d.sigma, d.flags, out.data()));
        return out;
    }
private:
    static void chk(int rc) { if (rc != 0) throw Error(rt_last_error()); }
    void* p_; size_t n_px_;
};
// main.rs:767-769,832 from an image that is already format_color's output (Progressive::rgb8): the same bytes write_ppm emits
inline void write_ppm_rgb8(const char* path, const std::vector<uint8_t>& rgb8, uint32_t W, uint32_t H) {
    if (rgb8.size() != (size_t)W * H * 3) throw Error("write_ppm_rgb8: image of another size");
    FILE* f = (!path || std::strcmp(path, "-") == 0) ? stdout : std::fopen(path, "w");
    if (!f) throw Error(std::string("cannot open ") + path);
    std::fprintf(f, "P3\n%u %u\n255\n", W, H);
    for (size_t p = 0; p < (size_t)W * H; p++) std::fprintf(f, "%u %u %u\n", (unsigned)rgb8[p * 3], (unsigned)rgb8[p * 3 + 1], (unsigned)rgb8[p * 3 + 2]);
    if (f != stdout) std::fclose(f); else std::fflush(f);
}

} // namespace rtr

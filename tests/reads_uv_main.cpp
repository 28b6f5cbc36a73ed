// tests/reads_uv_main.cpp — which materials the flattener marks MAT_NEEDS_UV (rt_flatten.cpp), read from the flattened scene itself: the
// C-ABI shows no flattened material, so this program (built by tests/test_scene_forms_host.py against librt_amd.so and the library's own
// headers) looks behind the opaque handle.  Host only, no GPU.  Prints one line per material: "<name> <0|1>".
#include <cstdio>
#include <string>
#include <vector>
#include "../include/rt_amd.h"
#include "../raytracinginrust_amd/csrc/rt_scene.h"

static int chain(rt_scene* sc, int leaf, int n, int other, bool leaf_is_odd) {
    int t = leaf;
    for (int k = 0; k < n; k++) {
        const int o = other < 0 ? t : other;
        t = leaf_is_odd ? rt_texture_check(sc, t, o) : rt_texture_check(sc, o, t);
    }
    return t;
}

int main() {
    rt_scene* sc = rt_scene_create();
    const double grey[3] = {0.5, 0.5, 0.5};
    const uint8_t px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    const int constant = rt_texture_constant(sc, grey);
    const int image = rt_texture_image(sc, px, 2, 2);
    std::vector<std::pair<std::string, int>> mats;
    const int lengths[] = {0, 1, 63, 64, 65, 66, 70, 300, 5000};
    for (int n : lengths) {
        mats.push_back({"image_both_" + std::to_string(n), rt_material_lambertian(sc, chain(sc, image, n, -1, true))});
        mats.push_back({"image_odd_" + std::to_string(n), rt_material_diffuse_light(sc, chain(sc, image, n, constant, true))});
        mats.push_back({"image_even_" + std::to_string(n), rt_material_isotropic(sc, chain(sc, image, n, constant, false))});
        mats.push_back({"constant_" + std::to_string(n), rt_material_lambertian(sc, chain(sc, constant, n, -1, true))});
    }
    const double p[10] = {0.1, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.5, 0.0, 1.0};
    mats.push_back({"pbr_image_70", rt_material_pbr(sc, chain(sc, image, 70, constant, false), p)});
    const double c[3] = {0.0, 0.0, 0.0};
    const int world = rt_list_create(sc);
    for (const auto& m : mats) {
        if (m.second < 0) { std::fprintf(stderr, "material %s: %s\n", m.first.c_str(), rt_scene_error(sc)); return 1; }
        rt_list_push(sc, world, rt_sphere(sc, c, 1.0, m.second));
    }
    rt_scene_set_world(sc, world);
    if (rt_scene_flatten(sc, nullptr) != 0) { std::fprintf(stderr, "flatten: %s\n", rt_last_error()); return 1; }
    for (const auto& m : mats)
        std::printf("%s %d\n", m.first.c_str(), (sc->s.flat.materials[(size_t)m.second].kind & rt::MAT_NEEDS_UV) ? 1 : 0);
    rt_scene_destroy(sc);
    return 0;
}

// csrc/rt_chain_cpu.cpp — the link step of a specular chain on the host: rt_chain.h's chain_step over a table of (ray, record) pairs, and the
// argument checks of the chain queries.  Plain C++ (no HIP include; it is also compiled stand-alone under sanitizers by
// tests/test_chain_host.py).  rt_chain_step_host (rt_host.cpp) hands it the scene's materials.
#include <string>
#include "rt_chain.h"

namespace rt {

std::string chain_check(uint32_t max_links, double max_fuzz, uint32_t flags) {
    if (max_links > CHAIN_MAX_LINKS) return "max_links must be <= 64 (a chain's links are numbered in 8 bits of its streams' seeds, csrc/rt_chain.h)";
    if (!(max_fuzz >= 0.0)) return "max_fuzz must be >= 0 (a number or +inf; NaN and negative values: not supported)";
    if (flags != 0u) return "chain queries take flags = 0: they run in f64 and in the reference's traversal order (RT_F32 and every other flag: not supported)";
    return "";
}

// word [11] as an index into the table: -1 a medium's, -2 no material at all
static int64_t chain_material_word(double w, size_t n_materials) {
    if (w == -1.0) return -1;
    if (!(w >= 0.0 && w < (double)n_materials)) return -2;
    const int64_t m = (int64_t)w;
    return (double)m == w ? m : -2;
}

std::string chain_step_host(const ChainMaterial* materials, size_t n_materials, uint32_t n, const double* rays, const double* hits, double max_fuzz,
                            double* next_rays_out, double* weight_out, uint32_t* status_out) {
    for (uint32_t k = 0; k < n; k++) {                               // before any write
        const double* r = hits + (size_t)k * CHAIN_HIT_DOUBLES;
        if (r[0] != 0.0 && chain_material_word(r[11], n_materials) == -2)
            return "rt_chain_step_host: record " + std::to_string(k) + " names no material of this scene (word [11])";
    }
    for (uint32_t k = 0; k < n; k++) {
        const double* ray = rays + (size_t)k * CHAIN_RAY_DOUBLES;
        const double* r = hits + (size_t)k * CHAIN_HIT_DOUBLES;
        double* out = next_rays_out + (size_t)k * CHAIN_RAY_DOUBLES;
        double weight[3] = {1.0, 1.0, 1.0}, new_d[3] = {0.0, 0.0, 0.0};
        uint32_t status;
        if (!(r[0] != 0.0)) status = CHAIN_END_MISS;
        else {
            const int64_t m = chain_material_word(r[11], n_materials);
            if (m < 0) status = CHAIN_END_SURFACE;                   // a medium
            else {
                const ChainMaterial& mt = materials[(size_t)m];
                status = chain_step(ray + 3, r + 5, r[8] != 0.0, mt.kind, mt.param, mt.albedo, max_fuzz, new_d, weight);
            }
        }
        if (status == CHAIN_CONTINUE) {
            out[0] = r[2]; out[1] = r[3]; out[2] = r[4];
            out[3] = new_d[0]; out[4] = new_d[1]; out[5] = new_d[2];
            out[6] = ray[6];
        } else for (uint32_t j = 0; j < CHAIN_RAY_DOUBLES; j++) out[j] = ray[j];
        for (int j = 0; j < 3; j++) weight_out[(size_t)k * 3u + j] = weight[j];
        status_out[k] = status;
    }
    return "";
}

} // namespace rt

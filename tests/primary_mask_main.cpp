// tests/primary_mask_main.cpp — csrc/rt_primary.h alone (the host twin of the primary pass's pixel classifier) on hostile inputs, built
// with -fsanitize=address,undefined by tests/test_primary_pass_host.py.  Cameras with zero, huge and non-finite fields and frames with
// W or H of 1 must give a mask without undefined behaviour — and "candidate" wherever the arithmetic is not finite; a tame camera
// must still clear an object that lies behind it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "rt_primary.h"

using namespace rt;

static DCamera<double> tame() {
    DCamera<double> c{};
    const double o[3] = {278, 278, -800}, ll[3] = {274.36, 274.36, -790}, h[3] = {7.28, 0, 0}, v[3] = {0, 7.28, 0}, cu[3] = {1, 0, 0}, cv[3] = {0, 1, 0};
    for (int k = 0; k < 3; k++) { c.origin[k] = o[k]; c.lower_left_corner[k] = ll[k]; c.horizontal[k] = h[k]; c.vertical[k] = v[k]; c.cu[k] = cu[k]; c.cv[k] = cv[k]; }
    c.lens_radius = 0.025;
    return c;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // objects: a rect in front of the camera, one behind it, a rotated and translated cube, a sphere, a medium, a range past the table
    std::vector<DRect<double>> rects;
    auto rect = [&](uint32_t plane, double a0, double a1, double b0, double b1, double k) { DRect<double> r{}; r.a0 = a0; r.a1 = a1; r.b0 = b0; r.b1 = b1; r.k = k; r.plane = plane; rects.push_back(r); };
    rect(0, 0, 555, 0, 555, 555);                        // 0: in front (XY at z = 555)
    rect(0, 0, 555, 0, 555, -2000);                      // 1: behind
    for (int f = 0; f < 6; f++) rect((uint32_t)(f / 2), 0, 165, 0, 165, (f & 1) ? 165.0 : 0.0);       // 2..7: a cube's faces
    std::vector<DOp<double>> ops(3);
    ops[0].kind = OP_TRANSLATE; ops[0].axis = 0; ops[0].x = 130; ops[0].y = 0; ops[0].z = 65;
    ops[1].kind = OP_ROTATE; ops[1].axis = 1; ops[1].x = std::sin(-0.3); ops[1].y = std::cos(-0.3); ops[1].z = 0;
    ops[2].kind = OP_ROTATE; ops[2].axis = 0; ops[2].x = 0.6; ops[2].y = 0.8; ops[2].z = 0;         // an axis the classifier does not understand
    std::vector<DObject> obs(7);
    for (DObject& o : obs) { o = DObject{}; o.medium = -1; o.geom_kind = G_RECT; o.geom_count = 1; }
    obs[0].geom_first = 0;
    obs[1].geom_first = 1;
    obs[2].geom_first = 2; obs[2].geom_count = 6; obs[2].first_op = 0; obs[2].n_ops = 2; obs[2].is_cube = 1;
    obs[3].geom_kind = G_SPHERE;
    obs[4].geom_first = 1; obs[4].medium = 0;
    obs[5].geom_first = 7; obs[5].geom_count = 5;         // leaves the table
    obs[6].geom_first = 1; obs[6].first_op = 2; obs[6].n_ops = 1;
    const uint32_t n_rects = (uint32_t)rects.size();

    unsigned long long checksum = 0;
    // the tame camera: object 1 (behind) is cleared for every pixel, 0 is kept at the centre, 3..6 are never cleared
    for (uint32_t W : {2u, 7u, 64u}) for (uint32_t H : {2u, 5u, 64u}) for (uint32_t i = 0; i < W; i += (W > 8 ? 9 : 1)) for (uint32_t j = 0; j < H; j += (H > 8 ? 7 : 1)) {
        const uint32_t m = pm_mask(tame(), i, j, W, H, obs.data(), 7, ops.data(), rects.data(), n_rects);
        if (m & 2u) { std::printf("FAIL: the rect behind the camera was kept (W %u H %u i %u j %u mask %x)\n", W, H, i, j, m); return 1; }
        if ((m & 0x78u) != 0x78u) { std::printf("FAIL: an object the classifier does not understand was cleared (mask %x)\n", m); return 1; }
        checksum += m;
    }
    if (!(pm_mask(tame(), 32, 32, 64, 64, obs.data(), 7, ops.data(), rects.data(), n_rects) & 1u)) { std::printf("FAIL: the rect in front was cleared at the centre\n"); return 1; }
    // hostile cameras and frames: anything not finite must be all candidates
    const double bad[] = {0.0, -0.0, inf, -inf, nan, 1e308, -1e308, 5e-324, 1e-300};
    for (double x : bad) for (int field = 0; field < 19; field++) {
        DCamera<double> c = tame();
        double* fields[19] = {&c.origin[0], &c.origin[1], &c.origin[2], &c.lower_left_corner[0], &c.lower_left_corner[1], &c.lower_left_corner[2],
                              &c.horizontal[0], &c.horizontal[1], &c.horizontal[2], &c.vertical[0], &c.vertical[1], &c.vertical[2],
                              &c.cu[0], &c.cu[1], &c.cu[2], &c.cv[0], &c.cv[1], &c.cv[2], &c.lens_radius};
        *fields[field] = x;
        for (uint32_t W : {1u, 2u, 33u}) for (uint32_t H : {1u, 2u, 33u}) {
            const uint32_t m = pm_mask(c, W - 1u, H / 2u, W, H, obs.data(), 7, ops.data(), rects.data(), n_rects);
            if ((m & 0x78u) != 0x78u) { std::printf("FAIL: hostile camera cleared an object it cannot understand\n"); return 1; }
            if ((std::isnan(x) || W == 1u || H == 1u) && (m & 7u) != 7u) {
                // (a NaN field, or a division by W - 1 = 0, reaches every axis of the ray set: nothing may be cleared)
                std::printf("FAIL: non-finite arithmetic cleared an object (field %d value %g W %u H %u mask %x)\n", field, x, W, H, m); return 1;
            }
            checksum += m;
        }
    }
    // an all-zero camera, and a list of more than 32 objects
    DCamera<double> z{};
    checksum += pm_mask(z, 0, 0, 4, 4, obs.data(), 7, ops.data(), rects.data(), n_rects);
    std::vector<DObject> many(40, obs[1]);
    if (pm_mask(tame(), 0, 0, 4, 4, many.data(), 40, ops.data(), rects.data(), n_rects) != 0xFFFFFFFFu) { std::printf("FAIL: more than 32 objects must give all ones\n"); return 1; }
    std::printf("ok %llu\n", checksum);
    return 0;
}

// csrc/rt_primary.h — which top-level objects the camera rays of ONE pixel can hit (host + device).
//
// The lean f64 list-scene kernel runs the first level of the camera paths of a refill together (rt_kernel.hip: the primary pass) and
// does not search objects that every ray it can generate for their pixel provably misses.  pm_may_hit answers, for one pixel and one
// object of the flattened top-level list, "may some such ray be given a hit by this object?"; a false is a proof, a true is no claim.
//
// THE RAY SET of pixel (i, j) is every ray refill_queue's expressions can deliver for it, not the ones some seed happens to draw:
//     rd  = lens_radius * (da, db, 0)               da, db in [-1, 1]          (the unit disk, bounded by its square)
//     off = cu * rd.x + cv * rd.y
//     o   = origin + off
//     d   = lower_left + u * horizontal + v * vertical - (origin + off)
//     u   = (i + U01) / (W - 1) in [i, i + 1] / (W - 1),   v = (j + U01) / (H - 1) in [j, j + 1] / (H - 1)
// (U01 < 1, but i + U01 may round up to i + 1: the interval is closed).  Time plays no part: the lean kernel has no moving primitive.
//
// THE ARGUMENT is interval arithmetic over the kernel's OWN expressions, in their order.  Every quantity the kernel computes on the way
// to a hit — o, d, the ray after each wrapper, t = (k - o_k) / d_k, a = o_a + t d_a — is mirrored by an interval [lo, hi], and the
// invariant is:  for EVERY ray of the set, the f64 number the kernel computes lies in the interval.  It holds at the inputs (camera
// fields and table entries are the same numbers here and there; da, db, u, v by the ranges above) and each operation keeps it:
//   * the exact result of x (op) y with x, y in their intervals lies between the extremes of the endpoint combinations (op is monotone
//     in each argument on the ranges used; the divisor's interval excludes zero, see below);
//   * the kernel's result is the exact one rounded once, so it differs from it by at most 2^-53 of its magnitude (2^-1075 where it
//     underflows); our endpoints are such roundings too;
//   * pm_iv() then widens the interval OUTWARD by 2^-40 of its larger magnitude plus 2^-1000 — a thousand times more than both
//     roundings together — so the rounded result of the kernel is inside, not only the exact one.
// o and d share `off`; treating them as independent only enlarges the set.  The short forms of rt_short.h return the bits of the
// division they stand for, so u and v are covered as divisions.
//
// MISSED.  An object is understood when it is a range of axis-aligned rects (a rect, a Cube's six, a room's walls) behind a chain of
// Translate, Rotate-about-y and FlipNormal wrappers and without a medium.  Whichever form the kernel searches the range by (the six
// exact tests, cube_hit's division-only form, the room form), a hit it accepts is one that rect_test_axes accepts for some rect of the
// range — that is those forms' own contract, tested where they live — so it suffices that EVERY rect of the range rejects every ray:
//   * rect_test_axes accepts iff !(t < t_min || t > t_max) and !(a < a0 || a > a1 || b < b0 || b > b1).  With the invariant and numbers
//     that are not NaN, acceptance needs t >= t_min > 0 and a0 <= a <= a1 and b0 <= b <= b1.  So the rect rejects every ray when the
//     interval of t lies below zero, or the interval of a (computed with t clipped to t >= 0) lies outside [a0, a1], or b's outside
//     [b0, b1] — for any t_max, so the running closest hit, the room's tie rule and the list order play no part.
//   * NaN and infinity accept anything (0 / 0 on a ray that starts on the plane, inf * 0 on one parallel to it: rt_kernel.hip
//     world_hit_list).  They are excluded, not argued about: the object stays a candidate unless d_k's interval excludes zero for the
//     plane axis k of every rect and every endpoint of every interval involved is finite (then every kernel number is finite: it lies
//     between two finite numbers).
// Everything else is a candidate: another geometry kind, another wrapper or axis, a medium, a non-finite field, W or H of 1 (the
// division by zero makes u or v non-finite), an object index past the list.  The cap of 32 objects is the caller's (pm_mask).
// Rays the classifier never "sees" are not an issue: the statement is about the intervals, which contain every (u, v, da, db).
#pragma once
#include <stdint.h>
#include "rt_ir.h"

#if defined(__HIPCC__)
#define RT_PM __host__ __device__ inline
#else
#define RT_PM inline
#endif

namespace rt {

struct PmIv { double lo, hi; };
// [lo, hi] widened outward (above); a NaN endpoint stays NaN and is caught by pm_finite
RT_PM PmIv pm_iv(double lo, double hi) {
    const double al = lo < 0.0 ? -lo : lo, ah = hi < 0.0 ? -hi : hi;
    const double w = (al > ah ? al : ah) * 0x1.0p-40 + 0x1.0p-1000;
    PmIv r; r.lo = lo - w; r.hi = hi + w; return r;
}
RT_PM PmIv pm_pt(double x) { PmIv r; r.lo = x; r.hi = x; return r; }
RT_PM bool pm_finite(PmIv a) { return a.lo - a.lo == 0.0 && a.hi - a.hi == 0.0; }
RT_PM double pm_min(double a, double b) { return a < b ? a : b; }
RT_PM double pm_max(double a, double b) { return a > b ? a : b; }
RT_PM PmIv pm_add(PmIv a, PmIv b) { return pm_iv(a.lo + b.lo, a.hi + b.hi); }
RT_PM PmIv pm_sub(PmIv a, PmIv b) { return pm_iv(a.lo - b.hi, a.hi - b.lo); }
RT_PM PmIv pm_mul(PmIv a, PmIv b) {
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    return pm_iv(pm_min(pm_min(p0, p1), pm_min(p2, p3)), pm_max(pm_max(p0, p1), pm_max(p2, p3)));
}
// a / b; the caller has checked that b excludes zero
RT_PM PmIv pm_div(PmIv a, PmIv b) {
    const double q0 = a.lo / b.lo, q1 = a.lo / b.hi, q2 = a.hi / b.lo, q3 = a.hi / b.hi;
    return pm_iv(pm_min(pm_min(q0, q1), pm_min(q2, q3)), pm_max(pm_max(q0, q1), pm_max(q2, q3)));
}
RT_PM bool pm_excludes_zero(PmIv a) { return a.lo > 0.0 || a.hi < 0.0; }      // (false for NaN)

struct PmRay { PmIv o[3], d[3]; };

// The ray set of pixel (i, j): refill_queue's expressions, in its order
RT_PM PmRay pm_camera_rays(const DCamera<double>& cam, uint32_t i, uint32_t j, uint32_t W, uint32_t H) {
    PmIv unit; unit.lo = -1.0; unit.hi = 1.0;
    const PmIv rdx = pm_mul(pm_pt(cam.lens_radius), unit), rdy = rdx;                      // lens_radius * da, lens_radius * db
    const PmIv u = pm_div(pm_iv((double)i, (double)i + 1.0), pm_pt((double)(W - 1u)));      // (W = 1: a division by zero — not finite, a candidate)
    const PmIv v = pm_div(pm_iv((double)j, (double)j + 1.0), pm_pt((double)(H - 1u)));
    PmRay r;
    for (int k = 0; k < 3; k++) {
        const PmIv off = pm_add(pm_mul(pm_pt(cam.cu[k]), rdx), pm_mul(pm_pt(cam.cv[k]), rdy));
        r.o[k] = pm_add(pm_pt(cam.origin[k]), off);
        const PmIv target = pm_add(pm_add(pm_pt(cam.lower_left_corner[k]), pm_mul(u, pm_pt(cam.horizontal[k]))), pm_mul(v, pm_pt(cam.vertical[k])));
        r.d[k] = pm_sub(target, r.o[k]);
    }
    return r;
}

// One rect against the ray set in the rect's own space: true = it rejects every ray (above)
RT_PM bool pm_rect_rejects(const DRect<double>& rc, const PmRay& r) {
    int k, a, b;
    if (rc.plane == 2u) { k = 0; a = 1; b = 2; } else if (rc.plane == 1u) { k = 1; a = 0; b = 2; } else if (rc.plane == 0u) { k = 2; a = 0; b = 1; } else return false;
    if (!pm_excludes_zero(r.d[k])) return false;
    PmIv t = pm_div(pm_sub(pm_pt(rc.k), r.o[k]), r.d[k]);
    const PmIv pa0 = pm_mul(t, r.d[a]), pb0 = pm_mul(t, r.d[b]);
    if (!(pm_finite(t) && pm_finite(pa0) && pm_finite(pb0) && pm_finite(r.o[a]) && pm_finite(r.o[b]))) return false;
    if (!(rc.a0 - rc.a0 == 0.0 && rc.a1 - rc.a1 == 0.0 && rc.b0 - rc.b0 == 0.0 && rc.b1 - rc.b1 == 0.0)) return false;
    if (t.hi < 0.0) return true;                      // every t below t_min
    if (t.lo < 0.0) t.lo = 0.0;                       // an accepted t is >= t_min > 0
    const PmIv pa = pm_add(r.o[a], pm_mul(t, r.d[a])), pb = pm_add(r.o[b], pm_mul(t, r.d[b]));
    if (!(pm_finite(pa) && pm_finite(pb))) return false;
    return pa.lo > rc.a1 || pa.hi < rc.a0 || pb.lo > rc.b1 || pb.hi < rc.b0;
}

// May object `ob` give some camera ray of the set a hit?  ops / rects: the scene's f64 tables.  n_rects: how many rect records exist
// (a range that leaves the table is not understood).
RT_PM bool pm_may_hit(const PmRay& cam_rays, const DObject& ob, const DOp<double>* ops, const DRect<double>* rects, uint32_t n_rects) {
    if (ob.geom_kind != G_RECT || ob.medium >= 0 || ob.n_ops > (uint32_t)RT_SHORT_CHAIN) return true;
    if (ob.geom_count == 0u || ob.geom_count > 64u || (uint64_t)ob.geom_first + ob.geom_count > n_rects) return true;
    PmRay r = cam_rays;
    // a room (is_cube & 2) keeps a tie table in first_op and has no wrappers (rt_flatten.cpp form_room)
    const uint32_t n_ops = (ob.is_cube & 2u) ? 0u : ob.n_ops;
    for (uint32_t q = 0; q < n_ops; q++) {
        const DOp<double> op = ops[ob.first_op + q];
        if (op.kind == OP_FLIP) continue;                                                   // hit.rs:113-119: the record, not the ray
        if (op.kind == OP_TRANSLATE) {                                                      // translate.rs:23
            r.o[0] = pm_sub(r.o[0], pm_pt(op.x)); r.o[1] = pm_sub(r.o[1], pm_pt(op.y)); r.o[2] = pm_sub(r.o[2], pm_pt(op.z));
        } else if (op.kind == OP_ROTATE && op.axis == 1u) {                                 // rotate.rs:82-86: x' = cos x - sin z, z' = sin x + cos z
            const PmIv sn = pm_pt(op.x), cs = pm_pt(op.y);
            const PmIv ox = r.o[0], oz = r.o[2], dx = r.d[0], dz = r.d[2];
            r.o[0] = pm_sub(pm_mul(cs, ox), pm_mul(sn, oz)); r.o[2] = pm_add(pm_mul(sn, ox), pm_mul(cs, oz));
            r.d[0] = pm_sub(pm_mul(cs, dx), pm_mul(sn, dz)); r.d[2] = pm_add(pm_mul(sn, dx), pm_mul(cs, dz));
        } else return true;
    }
    for (uint32_t q = 0; q < ob.geom_count; q++) if (!pm_rect_rejects(rects[ob.geom_first + q], r)) return true;
    return false;
}

// The mask of one pixel: bit k set = object k of [0, n_objects) is a candidate.  More than 32 objects: all ones (no saving, no claim).
// (Host and device: rt_kernel.hip primary_mask_kernel runs it, one thread per pixel, before a frame's launch; rt_debug_primary_mask_host here.)
RT_PM uint32_t pm_mask(const DCamera<double>& cam, uint32_t i, uint32_t j, uint32_t W, uint32_t H, const DObject* objects, uint32_t n_objects,
                       const DOp<double>* ops, const DRect<double>* rects, uint32_t n_rects) {
    if (n_objects > 32u) return 0xFFFFFFFFu;
    const PmRay r = pm_camera_rays(cam, i, j, W, H);
    uint32_t m = 0u;
    for (uint32_t k = 0; k < n_objects; k++) if (pm_may_hit(r, objects[k], ops, rects, n_rects)) m |= 1u << k;
    return m;
}

} // namespace rt

"""Host-side mirror of the reference's render loop (src/main.rs:767-835) over the C-ABI.

`render()` is the single call that replaces the `for j / for i / into_par_iter().map().sum()` nest;
`render_tiles_device()` is the tile-sharded form used one-process-per-GPU (see dist.py).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._abi import c_u32_p
from .api import CameraParams, SceneBuilder

RT_F64, RT_F32, RT_STOP_ON_ZERO, RT_ISOTROPIC_SCATTER, RT_NEAR_FIRST_BVH = 0, 1, 2, 4, 8
RT_PERSISTENT_BVH, RT_LOCKSTEP_BVH = 16, 32
RT_MULTI_COLLECTIVE = 64
RT_SPECULATE_BVH, RT_NO_SPECULATE_BVH = 1024, 2048
FLATTEN_COUNT_NAMES = ("objects", "ops", "rects", "spheres", "moving_spheres", "triangles", "bvh_nodes",
                       "materials", "textures", "lights", "media", "perlins")


class RenderError(RuntimeError):
    pass


def _rt():
    """The loaded library, every rt_* function declared (_abi.SIGNATURES)."""
    return _lib.load().lib


def _err() -> str:
    return _rt().rt_last_error().decode()


def _check(rc) -> None:
    if rc != 0:
        raise RenderError(_err())


def device_count() -> int:
    return _rt().rt_device_count()


def flatten(b: SceneBuilder) -> dict:
    """Flatten the Hittable tree into the device scene (host only) and return the table sizes."""
    counts = (C.c_uint32 * 12)()
    _check(_rt().rt_scene_flatten(b.h, counts))
    return dict(zip(FLATTEN_COUNT_NAMES, [int(x) for x in counts]))


OBJECT_FIELDS = ("geom_kind", "geom_first", "geom_count", "first_op", "n_ops", "medium", "is_cube", "nest")


def debug_objects(b: SceneBuilder, top_only: bool = True) -> list:
    """The flattened object table (rt_debug_objects; host only): one dict per object, the world's top-level objects in the order the
    kernels search them.  is_cube: 1 = a Cube's six faces; 2 | map << 8 = a ROOM (bare AARects that are faces of one box, tested through
    the Cube fast path: rt_flatten.cpp form_room) — map: three bits per face in cube.rs:17-24 order, the wall's place in the room's run
    of rect records or 7 = no such wall; first_op then holds, five bits per wall, the tie-rule index."""
    rows, n_top = debug_object_rows(b)
    return [dict(zip(OBJECT_FIELDS, [int(x) for x in r])) for r in (rows[:n_top] if top_only else rows)]


def debug_object_rows(b: SceneBuilder):
    """The same table as it comes: ((n, 8) uint32, columns in OBJECT_FIELDS order; how many of the rows are top-level objects)."""
    n_top = C.c_uint32(0)
    n = _rt().rt_debug_objects(b.h, None, 0, C.byref(n_top))
    if n < 0:
        raise RenderError(_err())
    out = np.zeros((max(n, 1), 8), np.uint32)
    if _rt().rt_debug_objects(b.h, out.ctypes.data, n, C.byref(n_top)) != n:
        raise RenderError(_err())
    return out[:n], int(n_top.value)


ONB_MAG_INVALID = 0xFFFFFFFFFFFFFFFF


def debug_onb_table(b: SceneBuilder):
    """rt_debug_onb_table (host only): the per-face ONB memo of the lean f64 list-scene kernel as flattened, one entry per rect record:
    (mag (n, 3) uint64 — the bit patterns of |n| of the hit normal, ONB_MAG_INVALID in all three for an invalid entry —,
    slots (n, 8, 2, 3) float64 — [sign bits sx | sy << 1 | sz << 2][v, u] —, the number of valid entries)."""
    n_valid = C.c_uint32(0)
    n = _rt().rt_debug_onb_table(b.h, None, None, 0, C.byref(n_valid))
    if n < 0:
        raise RenderError(_err())
    mag = np.zeros((max(n, 1), 3), np.uint64)
    slots = np.zeros((max(n, 1), 8, 2, 3), np.float64)
    if _rt().rt_debug_onb_table(b.h, mag.ctypes.data, slots.ctypes.data, n, C.byref(n_valid)) != n:
        raise RenderError(_err())
    return mag[:n], slots[:n], int(n_valid.value)


def debug_ring_form(b: SceneBuilder, flags: int = 0) -> dict:
    """rt_debug_ring_form (host only): the first-hit ring this scene's frames get from the lean f64 kernels — compact (98 entries of 80 B)
    where every rect has a valid ONB-table entry, wide (76 of 104 B) otherwise; entries 0 where those kernels do not serve the scene."""
    n, nb = C.c_uint32(0), C.c_uint32(0)
    rc = _rt().rt_debug_ring_form(b.h, flags, C.byref(n), C.byref(nb))
    if rc < 0:
        raise RenderError(_err())
    return {"compact": rc == 1, "entries": int(n.value), "entry_bytes": int(nb.value)}


def debug_ring_normal(b: SceneBuilder, rays: np.ndarray, t_min: np.ndarray):
    """rt_debug_ring_normal (needs a GPU): for n rays (n, 6) the closest hit's normal as finalize_hit gives it and as the compact first-hit
    record carries it (three sign bits, rebuilt from the ONB table): (hit (n,) bool, rect (n,) int, normal (n, 3), rebuilt (n, 3))."""
    r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    t = np.ascontiguousarray(t_min, np.float64).reshape(-1)
    if len(r) != len(t):
        raise ValueError("rays and t_min differ in length")
    out = np.zeros((len(r), 8), np.float64)
    _check(_rt().rt_debug_ring_normal(b.h, len(r), r.ctypes.data, t.ctypes.data, out.ctypes.data))
    return out[:, 0] != 0.0, out[:, 1].astype(np.int64), out[:, 2:5].copy(), out[:, 5:8].copy()


def debug_onb_table_w(b: SceneBuilder):
    """rt_debug_onb_table_w (host only): the ONB table's companion records, (n, 3) uint64 — the bit patterns of |normalized(n)| per rect
    record, ONB_MAG_INVALID in all three exactly where debug_onb_table's entry is invalid."""
    n = _rt().rt_debug_onb_table_w(b.h, None, 0)
    if n < 0:
        raise RenderError(_err())
    wmag = np.zeros((max(n, 1), 3), np.uint64)
    if _rt().rt_debug_onb_table_w(b.h, wmag.ctypes.data, n) != n:
        raise RenderError(_err())
    return wmag[:n]


def debug_ring_w(b: SceneBuilder, rays: np.ndarray, t_min: np.ndarray):
    """rt_debug_ring_w (needs a GPU): for n rays (n, 6) the closest hit's normalized(normal) as the kernel's normalisation gives it and w as
    the compact lean f64 kernel takes it from the table: (hit (n,) bool, rect (n,) int, normalized (n, 3), from_table (n, 3))."""
    r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    t = np.ascontiguousarray(t_min, np.float64).reshape(-1)
    if len(r) != len(t):
        raise ValueError("rays and t_min differ in length")
    out = np.zeros((len(r), 8), np.float64)
    _check(_rt().rt_debug_ring_w(b.h, len(r), r.ctypes.data, t.ctypes.data, out.ctypes.data))
    return out[:, 0] != 0.0, out[:, 1].astype(np.int64), out[:, 2:5].copy(), out[:, 5:8].copy()


def debug_onb(b: SceneBuilder, rects: np.ndarray, normals: np.ndarray):
    """rt_debug_onb (needs a GPU): the memo as the kernel's Lambertian arm reads it, for n pairs of (rect index, normal):
    (hit (n,) bool, v (n, 3), u (n, 3)); v and u are zero on a miss."""
    r = np.ascontiguousarray(rects, np.float64).reshape(-1)
    nm = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    if len(r) != len(nm):
        raise ValueError("rects and normals differ in length")
    out = np.zeros((len(r), 7), np.float64)
    _check(_rt().rt_debug_onb(b.h, len(r), r.ctypes.data, nm.ctypes.data, out.ctypes.data))
    return out[:, 0] != 0.0, out[:, 1:4].copy(), out[:, 4:7].copy()


def debug_list_hit(b: SceneBuilder, rays: np.ndarray, t_min: float = 0.001, mask: int | None = None) -> np.ndarray:
    """rt_debug_list_hit / rt_debug_list_hit_masked (needs a GPU; list scenes): world.hit and the hit record for n rays (origin[3],
    direction[3]) through the lean kernels' own search -> (n, 12): hit, t, position[3], normal[3], front_face, object, primitive,
    material.  With a mask: the search as the primary pass runs it — objects whose bit is clear are left out, except by a wave (64
    consecutive rays) that takes the NaN-guard route."""
    r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    tm = np.full(len(r), float(t_min))
    out = np.zeros((len(r), 12), np.float64)
    if mask is None:
        _check(_rt().rt_debug_list_hit(b.h, len(r), r.ctypes.data, tm.ctypes.data, out.ctypes.data))
    else:
        _check(_rt().rt_debug_list_hit_masked(b.h, len(r), r.ctypes.data, tm.ctypes.data, int(mask), out.ctypes.data))
    return out


def debug_primary_mask(b: SceneBuilder, cam: CameraParams, W: int, H: int, pixels: np.ndarray, host: bool = False) -> np.ndarray:
    """rt_debug_primary_mask (needs a GPU) / rt_debug_primary_mask_host (host=True, no GPU): the primary pass's pixel classifier
    (csrc/rt_primary.h) for n pixels (i, j), j counted from the bottom row: per pixel a uint32 whose bit k is set when top-level object
    k may be hit by a camera ray of that pixel (a clear bit is a proof)."""
    px = np.ascontiguousarray(pixels, np.uint32).reshape(-1, 2)
    out = np.zeros(len(px), np.uint32)
    fn = _rt().rt_debug_primary_mask_host if host else _rt().rt_debug_primary_mask
    _check(fn(b.h, C.byref(cam), W, H, px.ctypes.data, len(px), out.ctypes.data))
    return out


def debug_short_forms(op: int, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
    """rt_debug_short_forms (needs a GPU): the lean f64 kernel's exact short forms (csrc/rt_short.h) on caller operands, one record per
    lane, waves of 64.  op 0: a (n,) cosines, b (n,) max(dot, 0) -> (n, 3) pdf, sc, wave took the short form; op 1: a (n,) numerators,
    b (n, 2) divisor and enabled reciprocal -> (n,) quotients; op 2: a (n,) uint64 words -> (n,) U01; op 3: a (n, 3) directions, b (n, 3)
    t, axis, area -> (n, 2) pdf, wave took the short form."""
    a_cols, b_cols, out_cols = ((1, 1, 3), (1, 2, 1), (1, 0, 1), (3, 3, 2))[op]
    a = np.ascontiguousarray(a, np.uint64 if op == 2 else np.float64).reshape(-1, a_cols)
    if b_cols:
        b = np.ascontiguousarray(b, np.float64).reshape(-1, b_cols)
        if len(a) != len(b):
            raise ValueError("a and b differ in length")
    out = np.zeros((len(a), out_cols), np.float64)
    _check(_rt().rt_debug_short_forms(op, len(a), a.ctypes.data, b.ctypes.data if b_cols else None, out.ctypes.data))
    return out[:, 0].copy() if out_cols == 1 else out


KAT_OPS = ("sincos_0_2pi", "sin", "cos", "tan", "atan", "atan2", "acos", "log", "log2", "pow", "div3", "onb_from_w",
           "GTR_1", "GTR_2_aniso", "smithG_GGX", "smithG_GGX_aniso", "schlick_fresnel")
KAT_RECORDS = ((1, 0, 2), (1, 0, 1), (1, 0, 1), (1, 0, 1), (1, 0, 1), (1, 1, 1), (1, 0, 1), (1, 0, 1), (1, 0, 1), (1, 1, 1),
               (3, 1, 4), (3, 0, 9), (1, 1, 1), (3, 2, 1), (1, 1, 1), (3, 2, 1), (1, 0, 1))
KAT_SHAPES = {"lean": 0, "rest": 0x100}


def debug_math(op: str, a: np.ndarray, b: np.ndarray | None = None, shape: str = "lean") -> np.ndarray:
    """rt_debug_math (needs a GPU): one shading-side device function of rt_kernel.hip per lane on caller operands, f64, under the code
    shape of the lean unit or of the rest (KAT_SHAPES).  op: a name of KAT_OPS; a, b: (n, cols) as KAT_RECORDS says; -> (n, out cols),
    or (n,) where the op gives one value.  div3: the three quotients, then 1.0 where the lane took the shared-denominator form."""
    k = KAT_OPS.index(op)
    a_cols, b_cols, out_cols = KAT_RECORDS[k]
    a = np.ascontiguousarray(a, np.float64).reshape(-1, a_cols)
    if b_cols:
        b = np.ascontiguousarray(b, np.float64).reshape(-1, b_cols)
        if len(a) != len(b):
            raise ValueError("a and b differ in length")
    out = np.zeros((len(a), out_cols), np.float64)
    _check(_rt().rt_debug_math(k | KAT_SHAPES[shape], len(a), a.ctypes.data, b.ctypes.data if b_cols else None, out.ctypes.data))
    return out[:, 0].copy() if out_cols == 1 else out


def debug_brdf(b: SceneBuilder, material: int, r_in: np.ndarray, r_out: np.ndarray, normal: np.ndarray, base: np.ndarray,
               shape: str = "lean") -> np.ndarray:
    """rt_debug_brdf (needs a GPU): Material::brdf and PDF::BRDF value of a PBR material of the scene on the device, for n records of
    (r_in, r_out, normal, base colour), each (n, 3) -> (n, 4): brdf[3], pdf value."""
    arrs = [np.ascontiguousarray(x, np.float64).reshape(-1, 3) for x in (r_in, r_out, normal, base)]
    if len({len(x) for x in arrs}) != 1:
        raise ValueError("r_in, r_out, normal and base differ in length")
    out = np.zeros((len(arrs[0]), 4), np.float64)
    _check(_rt().rt_debug_brdf(b.h, len(out), int(material), *[x.ctypes.data for x in arrs], out.ctypes.data, KAT_SHAPES[shape]))
    return out


RT_KAT_REST_SHAPE, RT_KAT_NO_ONB_TABLE, RT_KAT_TABLE_W = 0x100, 0x200, 0x400
SHADE_FIELDS = {"ray": slice(0, 7), "beta": slice(7, 10), "e": slice(10, 13), "done": 13, "depth_left": 14, "state": slice(15, 19)}


def debug_shade(b: SceneBuilder, records: np.ndarray, rays: np.ndarray, beta=(1.0, 1.0, 1.0), seed: int = 0, depth_left: int = 50,
                flags: int = 0, shape: str = "lean", onb_table: bool = True, table_w: bool = False) -> np.ndarray:
    """rt_debug_shade (needs a GPU): ONE call of the kernels' shade_hit per record — records (n, 16) as query_hits gives them, rays (n, 7),
    record k on the stream rt_rng_path(seed, k, 0) — under the lean instantiation and code shape (list scenes; onb_table=False: without
    the ONB memo; table_w=True: the call as the compact lean f64 kernel makes it, w, v and u from the ONB table — scenes with the compact
    ring, Lambertian and Metal records whose normals have their rects' magnitudes) or the all-features one (shape="rest").
    flags: RT_STOP_ON_ZERO, RT_ISOTROPIC_SCATTER.  -> (n, 19), columns SHADE_FIELDS.  The arguments are checked before any device call."""
    rec = np.ascontiguousarray(records, np.float64).reshape(-1, 16)
    ry = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
    if len(rec) != len(ry):
        raise ValueError("records and rays differ in length")
    bt = np.ascontiguousarray(beta, np.float64).reshape(3)
    out = np.zeros((len(rec), 19), np.float64)
    fl = int(flags) | KAT_SHAPES[shape] | (0 if onb_table else RT_KAT_NO_ONB_TABLE) | (RT_KAT_TABLE_W if table_w else 0)
    _check(_rt().rt_debug_shade(b.h, len(rec), rec.ctypes.data, ry.ctypes.data, bt.ctypes.data, int(seed), int(depth_left), fl, out.ctypes.data))
    return out


def debug_light_pdf(b: SceneBuilder, origins: np.ndarray, dirs: np.ndarray) -> np.ndarray:
    """rt_debug_light_pdf (needs a GPU): the scene's `lights` pdf_value (HittableList::pdf_value, nested lists included) for n
    (origin, direction) pairs, computed on the device by the function the all-features kernel with object leaves runs."""
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and dirs differ in shape")
    out = np.zeros(len(o), np.float64)
    _check(_rt().rt_debug_light_pdf(b.h, len(o), o.ctypes.data, d.ctypes.data, out.ctypes.data))
    return out


def debug_bvh_links(b: SceneBuilder):
    """rt_debug_bvh_links (host only): the flattened BVHs' link words, (n, 4) uint32 {a, b, c, skip} per node, and the root node of every
    BVH object of the world list (uint32)."""
    n_roots = C.c_uint32(0)
    n = _rt().rt_debug_bvh_links(b.h, None, 0, None, 0, C.byref(n_roots))
    if n < 0:
        raise RenderError(_err())
    links = np.zeros((n, 4), np.uint32); roots = np.zeros(n_roots.value, np.uint32)
    if _rt().rt_debug_bvh_links(b.h, links.ctypes.data_as(c_u32_p), n, roots.ctypes.data_as(c_u32_p), len(roots), None) != n:
        raise RenderError(_err())
    return links, roots


def debug_filter_nodes(b: SceneBuilder):
    """rt_debug_filter_nodes (host only): the filter tree the kernels' box steps walk, for the n nodes of debug_bvh_links: the f32 boxes
    (n, 6) {min.x, max.x, min.y, max.y, min.z, max.z}, the links (n, 2) uint32 {skip, info}, the exact f64 boxes (n, 6) {min[3], max[3]},
    and filter_m (0: filter off)."""
    n = _rt().rt_debug_filter_nodes(b.h, None, None, None, 0, None)
    if n < 0:
        raise RenderError(_err())
    boxes = np.zeros((n, 6), np.float32); links = np.zeros((n, 2), np.uint32); f64_boxes = np.zeros((n, 6)); filter_m = C.c_float(0)
    if _rt().rt_debug_filter_nodes(b.h, boxes.ctypes.data, links.ctypes.data, f64_boxes.ctypes.data, n, C.byref(filter_m)) != n:
        raise RenderError(_err())
    return boxes, links, f64_boxes, filter_m.value


def _hit_inputs(boxes, rays, tlim):
    """(n, 6) boxes {min[3], max[3]}, (n, 6) rays {origin[3], direction[3]}, (n, 2) [t_min, t_max] as contiguous f64 arrays."""
    boxes, rays, tlim = (np.ascontiguousarray(a, np.float64) for a in (boxes, rays, tlim))
    n = len(boxes)
    if boxes.shape != (n, 6) or rays.shape != (n, 6) or tlim.shape != (n, 2):
        raise ValueError(f"boxes {boxes.shape}, rays {rays.shape}, tlim {tlim.shape}: want (n, 6), (n, 6), (n, 2)")
    return n, boxes, rays, tlim


def debug_aabb_hit(boxes, rays, tlim) -> np.ndarray:
    """rt_debug_aabb_hit (needs a GPU): AABB::hit on the device for n (box, ray, [t_min, t_max]) triples -> (n,) int32 of verdict bits."""
    n, boxes, rays, tlim = _hit_inputs(boxes, rays, tlim)
    out = np.zeros(n, np.int32)
    _check(_rt().rt_debug_aabb_hit(n, boxes.ctypes.data, rays.ctypes.data, tlim.ctypes.data, out.ctypes.data))
    return out


def debug_cube_hit(boxes, rays, tlim, rect_m: float) -> np.ndarray:
    """rt_debug_cube_hit (needs a GPU): Cube::hit on the device by the six exact rect tests and by the fast path -> (n, 4) f64
    {exact t, exact face, fast t, 8 * clear + face + 1}."""
    n, boxes, rays, tlim = _hit_inputs(boxes, rays, tlim)
    out = np.zeros((n, 4))
    _check(_rt().rt_debug_cube_hit(n, rect_m, boxes.ctypes.data, rays.ctypes.data, tlim.ctypes.data, out.ctypes.data))
    return out


def debug_room_hit(boxes, rays, tlim, rect_m: float, masks) -> np.ndarray:
    """rt_debug_room_hit (needs a GPU): the same for the ROOM form; masks[i]: which of the six faces exist -> (n, 4) f64 as debug_cube_hit."""
    n, boxes, rays, tlim = _hit_inputs(boxes, rays, tlim)
    masks = np.ascontiguousarray(masks, np.uint32)
    if masks.shape != (n,):
        raise ValueError(f"masks {masks.shape}: want ({n},)")
    out = np.zeros((n, 4))
    _check(_rt().rt_debug_room_hit(n, rect_m, boxes.ctypes.data, rays.ctypes.data, tlim.ctypes.data, masks.ctypes.data, out.ctypes.data))
    return out


RT_BVH_MEDIAN, RT_BVH_SAH = 0, 1


def set_bvh_builder(b: SceneBuilder, mode: int) -> None:
    """RT_BVH_MEDIAN: the reference's BVH::new (default); RT_BVH_SAH: opt-in binned surface-area heuristic."""
    _check(_rt().rt_scene_set_bvh_builder(b.h, mode))


def set_traversal_schedule(b: SceneBuilder, start_at: int = 40, stop_below: int = 24, leaf_share64: int = 16) -> None:
    """Tuning knob of the persistent-traversal loop (scheduling only)."""
    _check(_rt().rt_scene_set_traversal_schedule(b.h, start_at, stop_below, leaf_share64))


def prepare(b: SceneBuilder, flags: int = RT_F64) -> None:
    """Flatten, upload and load the kernel now instead of inside the first render (no launch)."""
    _check(_rt().rt_scene_prepare(b.h, flags))


LOOP_SHAPES = ("list", "lock-step", "persistent")
LOOP_CHOSEN_BY = ("the scene leaves no choice", "size rule", "calibration of this view", "caller's flag", "rt_scene_set_loop_shape")


def calibrate(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, spp: int, max_depth: int,
              seed: int = 0x5EED, flags: int = RT_F64) -> None:
    """rt_scene_calibrate: mesh scenes measure now, synchronously, which loop shape is faster for this view (four small launches);
    a no-op for every other scene.  The asynchronous entry points (render_tiles_device, render_multi_device) never do it themselves."""
    bg = (C.c_double * 3)(*[float(x) for x in background])
    _check(_rt().rt_scene_calibrate(b.h, C.byref(cam), bg, W, H, spp, max_depth, seed, flags))


def set_loop_shape(b: SceneBuilder, shape: int) -> None:
    """rt_scene_set_loop_shape: 1 persistent traversal, 0 lock-step (every view, until the scene changes), -1 forget."""
    _check(_rt().rt_scene_set_loop_shape(b.h, shape))


def stored_loop_shape(b: SceneBuilder) -> int:
    """rt_scene_loop_shape: 1 persistent traversal, 0 lock-step, -1 nothing stored."""
    return int(_rt().rt_scene_loop_shape(b.h))


def last_loop_info(b: SceneBuilder) -> dict:
    """rt_last_loop_info: the loop shape and instantiation the most recent launch ran, how the shape was chosen, and the stored
    calibration's kernel times."""
    out = (C.c_int32 * 4)(); ms = (C.c_float * 2)()
    _check(_rt().rt_last_loop_info(b.h, out, ms))
    t = "float" if out[3] else "double"
    # (`kernel` is the symbol that ran, but for a list scene the lean f64 kernel serves with its WIDE first-hit ring: last_ring_info)
    return {"shape": LOOP_SHAPES[out[0]], "feats": int(out[1]), "kernel": f"rt::pathtrace_kernel<{t}, {int(out[1])}u>",
            "chosen_by": LOOP_CHOSEN_BY[out[2]],
            "calibration_ms": {"lock-step": float(ms[0]), "persistent": float(ms[1])} if ms[0] > 0 or ms[1] > 0 else None}


def last_ring_info(b: SceneBuilder) -> dict:
    """rt_last_ring_info: the first-hit ring of the most recent launch — entries per wave, bytes per entry, `form` "compact", "wide" or None
    (not one of the lean f64 kernels) — and `symbol`, the kernel that ran as a rocprofv3 trace names it: last_loop_info's `kernel`, but for
    the lean f64 kernel with the wide ring, which is a kernel of its own."""
    ring = (C.c_uint32 * 3)()
    _check(_rt().rt_last_ring_info(b.h, ring))
    return {"entries": int(ring[0]), "entry_bytes": int(ring[1]), "form": ("wide" if ring[2] else "compact") if ring[0] else None,
            "symbol": "rt::pathtrace_wide_ring_kernel<double>" if ring[2] else last_loop_info(b)["kernel"]}


def render(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, spp: int, max_depth: int,
           seed: int = 0x5EED, flags: int = RT_F64, want_samples: bool = False):
    """Per-pixel sums of ray_color over `spp` samples, shape (H, W, 3) f64, row 0 = top (what `.sum()`
    yields at src/main.rs:830, in the order the reference prints pixels).  With want_samples also returns
    the (H, W, spp, 3) per-sample radiance."""
    out = np.zeros((H, W, 3), dtype=np.float64)
    bg = (C.c_double * 3)(*[float(x) for x in background])
    if want_samples:
        samples = np.zeros((H, W, spp, 3), dtype=np.float64)
        rc = _rt().rt_render_samples(b.h, C.byref(cam), bg, W, H, spp, max_depth, seed, flags, out.ctypes.data, samples.ctypes.data)
    else:
        samples = None
        rc = _rt().rt_render(b.h, C.byref(cam), bg, W, H, spp, max_depth, seed, flags, out.ctypes.data)
    _check(rc)
    return (out, samples) if want_samples else out


class Progressive:
    """A progressive frame (rt_progressive_*): one fixed view of one scene, a device-resident f64 sum frame that passes of samples
    accumulate into, resolved to the reference's 8-bit output on the device at any time.  Pass k holds samples [done, done + n) of every
    pixel — the very samples `render` with spp >= done + n and the same seed holds at those indices.  A context manager:

        with Progressive(b, cam, bg, W, H, max_depth) as frame:
            while frame.samples < 1024:
                frame.add(64)
                image, changed = frame.rgb8()        # (H, W, 3) uint8 and the pixels that differ from the previous resolve

    moments=True (rt_progressive_enable_moments) also keeps the second moment of the pass sums, from which `error_map` and `error_stats`
    estimate every pixel's standard error in display units once two passes are in (csrc/rt_moments.h):

        with Progressive(b, cam, bg, W, H, max_depth, moments=True) as frame:
            while frame.passes < 2 or frame.error_stats(1 / 256)["unconverged"]:
                frame.add(64)
    """

    def __init__(self, b: SceneBuilder, cam: CameraParams, background, W: int, H: int, max_depth: int, seed: int = 0x5EED, flags: int = RT_F64,
                 moments: bool = False, adaptive: bool = False, guide_samples: int = 1, guide_chain=None):
        self._lib = _rt()
        self.W, self.H = int(W), int(H)
        bg = (C.c_double * 3)(*[float(x) for x in background])
        self._h = self._lib.rt_progressive_create(b.h, C.byref(cam), bg, W, H, max_depth, seed, flags)
        if not self._h:
            raise RenderError(_err())
        self._builder = b              # the scene stays alive at least as long as the frame
        self.has_moments = False
        self.is_adaptive = False
        if moments or adaptive:
            self.enable_moments()
        if adaptive:
            self.enable_adaptive()
        if guide_samples != 1:
            self.set_guide_samples(guide_samples)
        if guide_chain is not None:
            self.set_guide_chain(*guide_chain)

    def set_guide_chain(self, max_links: int, max_fuzz: float = 0.0) -> None:
        """rt_progressive_set_guide_chain: max_links > 0 builds the guide and the albedo sums of every denoised resolve from specular-chain
        records of samples [0, guide_samples) (`query_camera_chain_guide`); the albedo resolves then demodulate by those sums over
        guide_samples, whatever albedo_samples they are given.  0 (the default): first hits, as without this call.  Another value drops the
        packed guide and the albedo sums.  `set_view` reprojects with first-hit records whatever the setting."""
        _check(self._lib.rt_progressive_set_guide_chain(self._h, int(max_links), float(max_fuzz)))

    def guide_chain_info(self):
        """(max_links, max_fuzz) in force."""
        n, f = C.c_uint32(), C.c_double()
        _check(self._lib.rt_progressive_guide_chain_info(self._h, C.byref(n), C.byref(f)))
        return int(n.value), float(f.value)

    def set_guide_samples(self, n: int) -> None:
        """rt_progressive_set_guide_samples: the guide of every denoised resolve — 1 (the default): the camera hits of sample 0; n > 1: the
        averaged record of samples [0, n) (`query_camera_guide`).  Another value drops the packed guide; the next denoised resolve builds it."""
        _check(self._lib.rt_progressive_set_guide_samples(self._h, int(n)))

    def guide_info(self):
        """(the guide_samples in force, how many guides the frame has built so far)."""
        n, builds = C.c_uint32(), C.c_uint64()
        _check(self._lib.rt_progressive_guide_info(self._h, C.byref(n), C.byref(builds)))
        return int(n.value), int(builds.value)

    def enable_adaptive(self) -> None:
        """rt_progressive_enable_adaptive: per-pixel sample counts on a frame with moments, only while it holds 0 samples (csrc/rt_adaptive.h)."""
        _check(self._lib.rt_progressive_enable_adaptive(self._h))
        self.is_adaptive = True

    def add_adaptive(self, n: int, tau: float, max_samples=None, spread: int = 1) -> dict:
        """rt_progressive_add_adaptive: one pass of n samples over the pixels whose estimated standard error exceeds tau (display units; with
        spread=1 also their 8 neighbours) and that hold at most max_samples - n samples.  -> {"listed": pixels sampled, "samples": samples
        rendered by this pass, "total": the sum of all counts, "kernel": 0 the frames' kernel / 1 the pixel-list kernel}; listed == 0 is the
        stop condition: nothing was rendered."""
        info = (C.c_uint64 * 4)()
        _check(self._lib.rt_progressive_add_adaptive(self._h, int(n), float(tau), 0 if max_samples is None else int(max_samples), int(spread), info))
        return {"listed": int(info[0]), "samples": int(info[1]), "total": int(info[2]), "kernel": int(info[3])}

    def counts(self):
        """(n, b): the samples every pixel holds and the passes it took part in, (H, W) uint32 each (rt_progressive_read_counts)."""
        n = np.zeros((self.H, self.W), dtype=np.uint32); b = np.zeros((self.H, self.W), dtype=np.uint32)
        _check(self._lib.rt_progressive_read_counts(self._h, n.ctypes.data, b.ctypes.data))
        return n, b

    def enable_moments(self) -> None:
        """rt_progressive_enable_moments: only while the frame holds 0 samples; 48 more bytes per pixel."""
        _check(self._lib.rt_progressive_enable_moments(self._h))
        self.has_moments = True

    @property
    def passes(self) -> int:
        """Passes merged so far (0 on a frame without moments)."""
        n = C.c_uint64()
        _check(self._lib.rt_progressive_passes(self._h, C.byref(n)))
        return int(n.value)

    def sq_sum(self) -> np.ndarray:
        """The second moments of the pass sums, (H, W, 3) f64 (rt_progressive_read_moments)."""
        out = np.zeros((self.H, self.W, 3), dtype=np.float64)
        _check(self._lib.rt_progressive_read_moments(self._h, out.ctypes.data))
        return out

    def error_map(self) -> np.ndarray:
        """e2 of every pixel, (H, W) f64: the squared standard error of the displayed value sqrt(mean), the largest of the three channels
        (csrc/rt_moments.h); needs two passes."""
        out = np.zeros((self.H, self.W), dtype=np.float64)
        _check(self._lib.rt_progressive_error_map(self._h, out.ctypes.data))
        return out

    def error_map_device(self, stream: int = 0) -> int:
        """Enqueue the error kernel on a HIP stream; returns the DEVICE address of the W*H doubles (owned by the frame)."""
        ptr = C.c_void_p()
        _check(self._lib.rt_progressive_error_map_device(self._h, C.byref(ptr), C.c_void_p(stream)))
        return int(ptr.value or 0)

    def error_stats(self, tau: float) -> dict:
        """Pixels whose standard error is <= tau / > tau / not finite, and the largest finite e2 (see `moments_stats`)."""
        words = (C.c_uint64 * 4)()
        _check(self._lib.rt_progressive_error_stats(self._h, float(tau), words))
        return moments_stats(words, tau)

    def checkpoint(self) -> dict:
        """Everything `restore` needs: the sums, the sample count and — with moments — the second moments and the pass count."""
        ck = {"rgb_sum": self.sum(), "samples": self.samples, "passes": self.passes, "sq_sum": self.sq_sum() if self.has_moments else None}
        if self.is_adaptive:
            ck["counts"], ck["pixel_passes"] = self.counts()
        return ck

    def restore(self, ck: dict) -> None:
        """Resume from `checkpoint()`: with second moments into a frame with moments (rt_progressive_load_moments), with counts into an
        adaptive frame (rt_progressive_load_adaptive), else the sums alone."""
        if ck.get("counts") is not None:
            a = np.ascontiguousarray(ck["rgb_sum"], dtype=np.float64); q = np.ascontiguousarray(ck["sq_sum"], dtype=np.float64)
            n = np.ascontiguousarray(ck["counts"], dtype=np.uint32); nb = np.ascontiguousarray(ck["pixel_passes"], dtype=np.uint32)
            if a.shape != (self.H, self.W, 3) or q.shape != a.shape or n.shape != a.shape[:2] or nb.shape != n.shape:
                raise ValueError(f"checkpoint of shapes {a.shape}, {q.shape}, {n.shape}, {nb.shape} for a frame of {(self.H, self.W, 3)}")
            return _check(self._lib.rt_progressive_load_adaptive(self._h, a.ctypes.data, q.ctypes.data, n.ctypes.data, nb.ctypes.data))
        if ck.get("sq_sum") is None:
            return self.load(ck["rgb_sum"], ck["samples"])
        a = np.ascontiguousarray(ck["rgb_sum"], dtype=np.float64)
        q = np.ascontiguousarray(ck["sq_sum"], dtype=np.float64)
        if a.shape != (self.H, self.W, 3) or q.shape != a.shape:
            raise ValueError(f"checkpoint of shapes {a.shape}, {q.shape} for a frame of {(self.H, self.W, 3)}")
        _check(self._lib.rt_progressive_load_moments(self._h, a.ctypes.data, q.ctypes.data, int(ck["samples"]), int(ck["passes"])))

    def add(self, n: int, want_samples: bool = False):
        """One synchronous pass of n samples per pixel; with want_samples returns them, (H, W, n, 3) as `render` lays them out."""
        samples = np.zeros((self.H, self.W, n, 3), dtype=np.float64) if want_samples else None
        _check(self._lib.rt_progressive_add(self._h, n, samples.ctypes.data if want_samples else None))
        return samples

    def add_async(self, n: int, stream: int = 0) -> None:
        """The same pass enqueued on a HIP stream of the frame's device; never waits."""
        _check(self._lib.rt_progressive_add_async(self._h, n, C.c_void_p(stream)))

    @property
    def samples(self) -> int:
        done = C.c_uint64()
        _check(self._lib.rt_progressive_samples(self._h, C.byref(done)))
        return int(done.value)

    def rgb8(self):
        """format_color(samples) of every pixel, computed on the device: ((H, W, 3) uint8, pixels changed since the previous resolve)."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        changed = C.c_uint64()
        _check(self._lib.rt_progressive_resolve_rgb8(self._h, out.ctypes.data, C.byref(changed)))
        return out, int(changed.value)

    def rgb8_device(self, stream: int = 0) -> int:
        """Enqueue the resolve on a HIP stream; returns the DEVICE address of the W*H*3 bytes (valid until the next-but-one resolve)."""
        ptr = C.c_void_p()
        _check(self._lib.rt_progressive_resolve_rgb8_device(self._h, C.byref(ptr), C.c_void_p(stream)))
        return int(ptr.value or 0)

    def rgb8_copy(self):
        """Wait for the most recent resolve and fetch it with its changed-pixel count, without resolving again."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        changed = C.c_uint64()
        _check(self._lib.rt_progressive_copy_rgb8(self._h, out.ctypes.data, C.byref(changed)))
        return out, int(changed.value)

    def rgb8_denoised(self, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
        """rt_progressive_resolve_denoised_rgb8: the frame's sums as they are now through the edge-avoiding a-trous filter (`denoise`) and
        format_color, all on the device -> (H, W, 3) uint8.  The frame builds its guide (sample 0's camera hits, or the averaged record of
        `set_guide_samples`) at the first call and keeps it until reset; `sum`, `rgb8` and its changed-pixel count are untouched."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        k, sg = _denoise_settings(iterations, sigma)
        _check(self._lib.rt_progressive_resolve_denoised_rgb8(self._h, k, sg, flags, out.ctypes.data))
        return out

    def rgb8_denoised_albedo(self, albedo_samples: int = 16, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
        """rt_progressive_resolve_denoised_albedo_rgb8: `rgb8_denoised` on the frame divided by its first-hit albedo and multiplied back
        (`denoise_albedo`), so that textures are not smoothed -> (H, W, 3) uint8.  The frame builds the albedo sums of samples
        [0, albedo_samples) itself at the first call and keeps them until reset or another albedo_samples."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        k, sg = _denoise_settings(iterations, sigma)
        _check(self._lib.rt_progressive_resolve_denoised_albedo_rgb8(self._h, int(albedo_samples), k, sg, flags, out.ctypes.data))
        return out

    def variance(self) -> np.ndarray:
        """rt_progressive_variance: the variance of the mean of every pixel and channel, (H, W, 3) f64 (csrc/rt_moments.h (4)), computed on
        the device from the frame's sums and second moments; needs two passes."""
        out = np.zeros((self.H, self.W, 3), dtype=np.float64)
        _check(self._lib.rt_progressive_variance(self._h, out.ctypes.data))
        return out

    def rgb8_denoised_variance(self, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
        """rt_progressive_resolve_denoised_variance_rgb8: `rgb8_denoised` with the colour stop measured in standard deviations of the
        frame's own per-pixel variance (`denoise_variance`) -> (H, W, 3) uint8.  sigma = (sigma_v, sigma_n, sigma_p).  Needs moments and
        two passes; the variance, the filter and the resolve run on the device, and `sum`, `sq_sum`, `passes`, `rgb8` and its changed-pixel
        count are untouched."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        k, sg = _denoise_variance_settings(iterations, sigma)
        _check(self._lib.rt_progressive_resolve_denoised_variance_rgb8(self._h, k, sg, flags, out.ctypes.data))
        return out

    def variance_counts(self) -> np.ndarray:
        """rt_progressive_variance_counts: `variance` for any frame with moments, (H, W, 3) f64 — on an adaptive frame every pixel's variance
        from its own sample and pass counts (`adaptive_variance_host`; +inf where a pixel has fewer than two passes), whether the counts
        differ or not."""
        out = np.zeros((self.H, self.W, 3), dtype=np.float64)
        _check(self._lib.rt_progressive_variance_counts(self._h, out.ctypes.data))
        return out

    def rgb8_denoised_frame(self, iterations: int = None, sigma=None, flags: int = 0, variance: bool = False, albedo_samples: int = 0) -> np.ndarray:
        """rt_progressive_resolve_denoised_frame_rgb8: the denoised resolve of the frame as it is (`denoise_frame`) -> (H, W, 3) uint8.  Works
        on adaptive frames whose counts differ, which the three resolves above refuse, and combines the variance stop (variance=True:
        sigma = (sigma_v, sigma_n, sigma_p), default DENOISE_VARIANCE_SIGMA; needs moments) with albedo demodulation (albedo_samples >= 1).
        On a frame without counts the three modes `rgb8_denoised`, `rgb8_denoised_albedo` and `rgb8_denoised_variance` cover give their bytes.
        `sum`, `sq_sum`, `counts`, `rgb8` and its changed-pixel count are untouched."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        k, sg = _denoise_variance_settings(iterations, sigma) if variance else _denoise_settings(iterations, sigma)
        _check(self._lib.rt_progressive_resolve_denoised_frame_rgb8(self._h, DENOISE_STOP_VARIANCE if variance else DENOISE_STOP_COLOUR, int(albedo_samples), k, sg,
                                                                    flags, out.ctypes.data))
        return out

    def albedo_info(self):
        """(the albedo_samples the frame holds albedo sums for — 0: none —, how many times it has built them)."""
        n, builds = C.c_uint32(), C.c_uint64()
        _check(self._lib.rt_progressive_albedo_info(self._h, C.byref(n), C.byref(builds)))
        return int(n.value), int(builds.value)

    def sum(self) -> np.ndarray:
        """The accumulated per-pixel sums, (H, W, 3) f64 as `render` returns them; with `samples`, a checkpoint."""
        out = np.zeros((self.H, self.W, 3), dtype=np.float64)
        _check(self._lib.rt_progressive_read_sum(self._h, out.ctypes.data))
        return out

    def load(self, rgb_sum: np.ndarray, samples: int) -> None:
        """Resume from a checkpoint: the frame becomes `rgb_sum` holding `samples` samples per pixel."""
        a = np.ascontiguousarray(rgb_sum, dtype=np.float64)
        if a.shape != (self.H, self.W, 3):
            raise ValueError(f"checkpoint of shape {a.shape} for a frame of {(self.H, self.W, 3)}")
        _check(self._lib.rt_progressive_load_sum(self._h, a.ctypes.data, samples))

    def set_view(self, cam: CameraParams, seed: int, max_history: int = None, sigma=None) -> None:
        """rt_progressive_set_view: move the frame to another view of the same scene and keep what it knows — the frame's sums blended with
        the history it already holds are reprojected into the new view (`reproject`) and become the history; the frame itself then holds 0
        samples of the new camera and seed, exactly as after `reset`.  Give every view a NEW seed: the random streams are keyed by pixel and
        sample index, so the same seed under a nearby camera gives the new samples nearly the noise the history already has.  max_history
        (default REPROJECT_MAX_HISTORY) caps the samples a history pixel counts for; 0 is a plain change of view.  sigma = (normal_min,
        sigma_p), default REPROJECT_SIGMA.  Not on an adaptive frame."""
        cap, sg = _reproject_settings(max_history, sigma)
        _check(self._lib.rt_progressive_set_view(self._h, C.byref(cam), int(seed), cap, sg))

    def history(self):
        """rt_progressive_read_history -> (hist_sum (H, W, 3) f64, hist_counts (H, W) uint32); all zero without a history."""
        s = np.zeros((self.H, self.W, 3), dtype=np.float64); n = np.zeros((self.H, self.W), dtype=np.uint32)
        _check(self._lib.rt_progressive_read_history(self._h, s.ctypes.data, n.ctypes.data))
        return s, n

    def history_info(self) -> dict:
        """{"views": the views taken by `set_view` so far, "pixels": the pixels that hold history}."""
        out = (C.c_uint64 * 2)()
        _check(self._lib.rt_progressive_history_info(self._h, out))
        return {"views": int(out[0]), "pixels": int(out[1])}

    def history_variance(self) -> np.ndarray:
        """rt_progressive_read_history_variance -> hist_var (H, W, 3) f64: the variance of the history's per-pixel mean, which `set_view`
        carries along on a frame with moments (`reproject_variance`); +inf where it is unknown, all +0.0 without a history."""
        out = np.zeros((self.H, self.W, 3), dtype=np.float64)
        _check(self._lib.rt_progressive_read_history_variance(self._h, out.ctypes.data))
        return out

    def rgb8_temporal(self, iterations: int = 0, sigma=None, flags: int = 0, variance: bool = False, albedo_samples: int = 0) -> np.ndarray:
        """rt_progressive_resolve_temporal_rgb8: the resolve of the frame blended with its history -> (H, W, 3) uint8; every pixel is
        divided by its own count (`temporal_blend_host`, `adaptive_resolve_rgb8_host`).  iterations >= 1: `denoise_frame` with the blend's
        counts and the frame's guide in between (sigma: DENOISE_SIGMA).  Works with 0 samples once there is history: the preview right after a
        camera move.
        variance=True (rt_progressive_resolve_temporal_variance_rgb8; a frame with moments, iterations 1 .. 8): the filter's colour stop is
        measured in standard deviations of the blend's own variance (`temporal_blend_variance_host` of the frame's variance, when it has two
        passes, with `history_variance`); sigma = (sigma_v, sigma_n, sigma_p), default DENOISE_VARIANCE_SIGMA; albedo_samples >= 1
        demodulates as `rgb8_denoised_frame` does."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        if variance:
            k, sg = _denoise_variance_settings(int(iterations), sigma)
            _check(self._lib.rt_progressive_resolve_temporal_variance_rgb8(self._h, int(albedo_samples), k, sg, flags, out.ctypes.data))
            return out
        if albedo_samples:
            raise ValueError("rgb8_temporal: albedo_samples goes with variance=True")
        k, sg = _denoise_settings(int(iterations), sigma)
        _check(self._lib.rt_progressive_resolve_temporal_rgb8(self._h, k, sg, flags, out.ctypes.data))
        return out

    def reset(self) -> None:
        """rt_progressive_reset: 0 samples of the same view and seed; drops the history `set_view` keeps."""
        _check(self._lib.rt_progressive_reset(self._h))

    def close(self) -> None:
        if self._h:
            self._lib.rt_progressive_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


# Samples per pass `render_progressive` uses by default: every pass is one persistent launch that fills and drains the chip (~0.5 ms) and
# ends with a tail, so small passes cost throughput; DESIGN.md ("Progressive frames") has the measured cost by pass size.
DEFAULT_PASS_SPP = 64


def render_progressive(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, spp: int, max_depth: int, passes=None,
                       seed: int = 0x5EED, flags: int = RT_F64, until_error=None, min_passes: int = 2, max_samples=None, adaptive: bool = False,
                       spread: int = 1):
    """Generator: renders `spp` samples per pixel in passes and yields (samples_done, rgb8, changed_px) after each; the last item is the
    full frame — the image `format_image(render(..., spp), spp)` gives.  passes: None (passes of DEFAULT_PASS_SPP), an int (that many
    passes of equal size, the remainder in the first ones), or a sequence of pass sizes that sums to spp.

    until_error=tau: a frame with moments that stops at the first pass — not before min_passes (>= 2) — after which no pixel's estimated
    standard error exceeds tau (display units: 1/256 is one code value), at the latest after max_samples (default: spp, which `passes`
    then divides) samples.  Every item is then (samples_done, rgb8, changed_px, stats): the dict of `Progressive.error_stats(tau)`, None
    while the frame holds fewer than two passes.

    adaptive=True (with until_error): an adaptive frame — every pass samples only the pixels whose estimated standard error still exceeds tau
    (`Progressive.add_adaptive`, with `spread`), no pixel beyond max_samples, and the generator ends with the pass that lists no pixel.
    samples_done is then the LARGEST per-pixel count, and stats carries "listed", "samples" and "total" of the pass beside the error words."""
    if adaptive and until_error is None:
        raise ValueError("adaptive=True needs until_error: the pixels to sample are chosen by their estimated error")
    if until_error is not None:
        if min_passes < 2:
            raise ValueError("min_passes must be >= 2: the error is estimated from the spread between passes")
        spp = spp if max_samples is None else int(max_samples)
    if passes is None:
        sizes = [DEFAULT_PASS_SPP] * (spp // DEFAULT_PASS_SPP) + ([spp % DEFAULT_PASS_SPP] if spp % DEFAULT_PASS_SPP else [])
    elif isinstance(passes, int):
        if not 1 <= passes <= spp:
            raise ValueError("passes must be between 1 and spp")
        sizes = [spp // passes + (1 if k < spp % passes else 0) for k in range(passes)]
    else:
        sizes = [int(n) for n in passes]
        if sum(sizes) != spp or min(sizes, default=0) < 1:
            raise ValueError("pass sizes must be >= 1 and sum to spp")
    with Progressive(b, cam, background, W, H, max_depth, seed, flags, moments=until_error is not None, adaptive=adaptive) as frame:
        for n in sizes:
            if adaptive:
                info = frame.add_adaptive(n, until_error, max_samples=spp, spread=spread)
                if info["listed"] == 0:
                    return
                image, changed = frame.rgb8()
                stats = frame.error_stats(until_error) if frame.passes >= 2 else None
                yield frame.samples, image, changed, None if stats is None else {**stats, **info}
                continue
            frame.add(n)
            image, changed = frame.rgb8()
            if until_error is None:
                yield frame.samples, image, changed
                continue
            stats = frame.error_stats(until_error) if frame.passes >= 2 else None
            yield frame.samples, image, changed, stats
            if stats is not None and frame.passes >= min_passes and stats["unconverged"] == 0:
                return


def render_multi(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, spp: int, max_depth: int, device_mask: int = 0,
                 seed: int = 0x5EED, flags: int = RT_F64, tile_px: int = 0):
    """The whole frame on the GPUs of this node selected by `device_mask` (bit d = HIP device d; 0 = all visible) from ONE call:
    per-device replicas of the scene, tiles dealt round-robin, one RCCL gather to the first device, un-permuted there
    (rt_render_multi, csrc/rt_multi.cpp).  Returns the (H, W, 3) per-pixel sums like render()."""
    out = np.zeros((H, W, 3), dtype=np.float64)
    bg = (C.c_double * 3)(*[float(x) for x in background])
    _check(_rt().rt_render_multi(b.h, C.byref(cam), bg, W, H, spp, max_depth, seed, flags, device_mask, tile_px, out.ctypes.data))
    return out


def render_multi_device(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, spp: int, max_depth: int, device_mask: int = 0,
                        seed: int = 0x5EED, flags: int = RT_F64, tile_px: int = 0) -> int:
    """rt_render_multi_device: enqueue the frame on the selected devices and return the DEVICE address (first selected device) of
    its W*H*3 per-pixel sums; `multi_sync` waits for it, `multi_frame` fetches it."""
    bg = (C.c_double * 3)(*[float(x) for x in background])
    ptr = C.c_void_p()
    _check(_rt().rt_render_multi_device(b.h, C.byref(cam), bg, W, H, spp, max_depth, seed, flags, device_mask, tile_px, C.byref(ptr)))
    return int(ptr.value or 0)


def multi_sync(b: SceneBuilder) -> None:
    _check(_rt().rt_multi_sync(b.h))


def multi_frame(b: SceneBuilder, W: int, H: int) -> np.ndarray:
    """The last rt_render_multi_device frame as an (H, W, 3) host array (waits for it)."""
    out = np.zeros((H, W, 3), dtype=np.float64)
    _check(_rt().rt_multi_copy_frame(b.h, out.ctypes.data, out.size))
    return out


def last_multi_ms(b: SceneBuilder) -> dict:
    ms = (C.c_double * 4)()
    _check(_rt().rt_last_multi_ms(b.h, ms))
    return {"slowest_kernel_ms": ms[0], "gather_ms": ms[1], "unpermute_ms": ms[2], "call_ms": ms[3]}


def last_multi_ranks(b: SceneBuilder) -> dict:
    """rt_last_multi_ranks: HIP device and kernel ms of every rank of the last rt_render_multi* frame, and the rank count RCCL
    reports for the communicator its gather ran on (0: no collective ran)."""
    n, coll = C.c_uint32(), C.c_uint32()
    dev = (C.c_int * 64)(); ms = (C.c_double * 64)()
    _check(_rt().rt_last_multi_ranks(b.h, 64, C.byref(n), dev, ms, C.byref(coll)))
    k = min(int(n.value), 64)
    return {"n_ranks": int(n.value), "devices": [int(dev[i]) for i in range(k)], "kernel_ms": [float(ms[i]) for i in range(k)],
            "collective_ranks": int(coll.value)}


def local_tiles(W: int, H: int, tile_px: int, rank: int, world: int) -> int:
    return int(_rt().rt_local_tiles(W, H, tile_px, rank, world))


def render_tiles_device(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, spp: int, max_depth: int,
                        seed: int, flags: int, tile_px: int, rank: int, world: int, d_out_ptr: int, d_out_bytes: int,
                        stream: int = 0) -> None:
    """Asynchronously render tiles t ≡ rank (mod world) into device memory at d_out_ptr on `stream`."""
    bg = (C.c_double * 3)(*[float(x) for x in background])
    rc = _rt().rt_render_device(b.h, C.byref(cam), bg, W, H, spp, max_depth, seed, flags, tile_px, rank, world,
                                 C.c_void_p(d_out_ptr), d_out_bytes, C.c_void_p(stream))
    _check(rc)


# ---- ray queries (rt_query_*): world.hit (src/main.rs:48) for rays of the caller's, or for the camera rays of one sample of every pixel
DEFAULT_SEED = 0x5EED
# the hit record's 16 doubles by name (include/rt_amd.h): material = the handle the builder returned (-1: a ConstantMedium hit, or a miss),
# object = the index in the flattened object table (debug_objects), prim_kind 0 rect, 1 sphere, 2 moving sphere, 3 triangle, -1 medium
HIT_FIELDS = {"hit": slice(0, 1), "t": slice(1, 2), "position": slice(2, 5), "normal": slice(5, 8), "front_face": slice(8, 9),
              "u": slice(9, 10), "v": slice(10, 11), "material": slice(11, 12), "object": slice(12, 13), "prim_kind": slice(13, 14),
              "prim_index": slice(14, 15)}
RAY_DOUBLES, HIT_DOUBLES = 7, 16


def camera_ray(cam: CameraParams, W: int, H: int, i: int, j: int, seed: int = DEFAULT_SEED, sample: int = 0) -> np.ndarray:
    """rt_camera_ray (host only): Camera::get_ray for sample `sample` of pixel (i, j), j counted from the bottom row (main.rs:811-820) —
    the very ray a frame with that seed traces -> (7,) f64: origin, direction, time."""
    out = (C.c_double * RAY_DOUBLES)()
    _check(_rt().rt_camera_ray(C.byref(cam), W, H, i, j, seed, sample, out))
    return np.array(out, dtype=np.float64)


def query_hits(b: SceneBuilder, rays, t_min: float = 1e-5, seed: int = 0) -> np.ndarray:
    """rt_query_hits: world.hit(ray, t_min, +inf) for n rays, (n, 7) f64 {origin, direction, time} -> (n, 16) hit records (HIT_FIELDS).
    Ray k draws from the stream of Rng(seed, k) where a ConstantMedium needs a random number."""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != RAY_DOUBLES:
        raise ValueError(f"rays of shape {r.shape}: want (n, {RAY_DOUBLES})")
    out = np.zeros((len(r), HIT_DOUBLES), dtype=np.float64)
    _check(_rt().rt_query_hits(b.h, len(r), r.ctypes.data, float(t_min), seed, 0, out.ctypes.data))
    return out


def query_camera(b: SceneBuilder, cam: CameraParams, W: int, H: int, sample: int = 0, seed: int = DEFAULT_SEED, want_rays: bool = False):
    """rt_query_camera: the camera ray of sample `sample` of every pixel, generated on the device as a frame with that seed generates
    it, and its closest hit -> (H, W, 16) hit records, row 0 = top; with want_rays also the (H, W, 7) rays."""
    hits = np.zeros((H, W, HIT_DOUBLES), dtype=np.float64)
    rays = np.zeros((H, W, RAY_DOUBLES), dtype=np.float64) if want_rays else None
    _check(_rt().rt_query_camera(b.h, C.byref(cam), W, H, sample, seed, 0, rays.ctypes.data if want_rays else None, hits.ctypes.data))
    return (hits, rays) if want_rays else hits


def _device_buffer(x):
    """(address, bytes) of a device buffer given as a torch tensor, or (address, None) for a raw pointer."""
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr()), int(x.numel() * x.element_size())
    return int(x), None


def query_hits_device(b: SceneBuilder, n: int, d_rays, d_hits, t_min: float = 1e-5, seed: int = 0, stream: int = 0, d_hits_bytes=None) -> None:
    """rt_query_hits_device: the same for rays and records in device memory (torch tensors of f64, or raw pointers — then d_hits_bytes
    says how large the record buffer is), enqueued on `stream`; never waits.  Both buffers 16-byte aligned."""
    rays_ptr, _ = _device_buffer(d_rays)
    hits_ptr, nbytes = _device_buffer(d_hits)
    nbytes = nbytes if d_hits_bytes is None else int(d_hits_bytes)
    if nbytes is None:
        raise ValueError("d_hits_bytes is needed with a raw pointer")
    _check(_rt().rt_query_hits_device(b.h, n, C.c_void_p(rays_ptr), float(t_min), seed, 0, C.c_void_p(hits_ptr), nbytes, C.c_void_p(stream)))


def query_camera_device(b: SceneBuilder, cam: CameraParams, W: int, H: int, d_hits, sample: int = 0, seed: int = DEFAULT_SEED,
                        d_rays_out=None, stream: int = 0, d_hits_bytes=None) -> None:
    """rt_query_camera_device: W*H records (and, with d_rays_out, rays) into device memory, enqueued on `stream`; never waits."""
    hits_ptr, nbytes = _device_buffer(d_hits)
    nbytes = nbytes if d_hits_bytes is None else int(d_hits_bytes)
    if nbytes is None:
        raise ValueError("d_hits_bytes is needed with a raw pointer")
    rays_ptr = None if d_rays_out is None else _device_buffer(d_rays_out)[0]
    _check(_rt().rt_query_camera_device(b.h, C.byref(cam), W, H, sample, seed, 0, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr), nbytes,
                                        C.c_void_p(stream)))


def query_radiance(b: SceneBuilder, rays, spp: int, max_depth: int, background=(0.0, 0.0, 0.0), seed: int = DEFAULT_SEED, flags: int = 0,
                   want_samples: bool = False):
    """rt_query_radiance: ray_color (main.rs:41-120) along n caller rays, (n, 7) f64 {origin, direction, time}, spp samples of each; sample s
    of ray k draws from the stream of rng_path(seed, k, s) -> (sums (n, 3)[, samples (n, spp, 3)], nonfinite): per ray the SUM over its
    samples, as render() returns per pixel; nonfinite = the samples with a non-finite component."""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != RAY_DOUBLES:
        raise ValueError(f"rays of shape {r.shape}: want (n, {RAY_DOUBLES})")
    bg = (C.c_double * 3)(*[float(x) for x in background])
    sums = np.zeros((len(r), 3), dtype=np.float64)
    samples = np.zeros((len(r), spp, 3), dtype=np.float64) if want_samples else None
    nonfinite = C.c_uint64(0)
    _check(_rt().rt_query_radiance(b.h, len(r), r.ctypes.data, bg, spp, max_depth, seed, flags, sums.ctypes.data,
                                   samples.ctypes.data if want_samples else None, C.byref(nonfinite)))
    return (sums, samples, int(nonfinite.value)) if want_samples else (sums, int(nonfinite.value))


def query_radiance_device(b: SceneBuilder, n: int, d_rays, d_rgb_sum, spp: int, max_depth: int, background=(0.0, 0.0, 0.0),
                          seed: int = DEFAULT_SEED, flags: int = 0, first_sample: int = 0, accumulate: bool = False, d_samples=None,
                          d_nonfinite=None, stream: int = 0, d_rgb_sum_bytes=None) -> None:
    """rt_query_radiance_device: the same for rays and sums in device memory (torch tensors of f64, or raw pointers — then d_rgb_sum_bytes
    says how large the sum buffer is), samples [first_sample, first_sample + spp) of every ray, enqueued on `stream`; never waits.
    accumulate: added to what d_rgb_sum holds instead of overwriting it.  d_samples (n * spp * 3 f64) and d_nonfinite (one 64-bit word,
    only ever added to: the caller zeroes it) are optional."""
    rays_ptr, _ = _device_buffer(d_rays)
    sum_ptr, nbytes = _device_buffer(d_rgb_sum)
    nbytes = nbytes if d_rgb_sum_bytes is None else int(d_rgb_sum_bytes)
    if nbytes is None:
        raise ValueError("d_rgb_sum_bytes is needed with a raw pointer")
    samples_ptr = None if d_samples is None else _device_buffer(d_samples)[0]
    nonfinite_ptr = None if d_nonfinite is None else _device_buffer(d_nonfinite)[0]
    bg = (C.c_double * 3)(*[float(x) for x in background])
    _check(_rt().rt_query_radiance_device(b.h, n, C.c_void_p(rays_ptr), bg, spp, max_depth, seed, flags, first_sample, 1 if accumulate else 0,
                                          C.c_void_p(sum_ptr), nbytes, C.c_void_p(samples_ptr), C.c_void_p(nonfinite_ptr), C.c_void_p(stream)))


def equirect_rays(origin, W: int, H: int, time: float = 0.0) -> np.ndarray:
    """The rays of a W x H equirectangular (360 x 180 degree) panorama seen from `origin` -> (H * W, 7) in output order, row 0 = top:
    row r, column i looks along (sin t cos p, cos t, sin t sin p) with t = pi (r + 0.5) / H from +y, p = 2 pi (i + 0.5) / W.  No jitter."""
    # (sines and cosines from libm, one row / column at a time: the very doubles include/raytracinginrust.hpp's equirect_rays computes)
    theta = [math.pi * (r + 0.5) / H for r in range(H)]
    phi = [2.0 * math.pi * (i + 0.5) / W for i in range(W)]
    st, ct = np.array([math.sin(t) for t in theta]), np.array([math.cos(t) for t in theta])
    sp, cp = np.array([math.sin(p) for p in phi]), np.array([math.cos(p) for p in phi])
    rays = np.empty((H, W, RAY_DOUBLES), dtype=np.float64)
    rays[..., 0:3] = np.asarray(origin, dtype=np.float64)
    rays[..., 3] = st[:, None] * cp[None, :]
    rays[..., 4] = ct[:, None]
    rays[..., 5] = st[:, None] * sp[None, :]
    rays[..., 6] = float(time)
    return rays.reshape(H * W, RAY_DOUBLES)


# ---- albedo queries (rt_query_albedo*, rt_query_camera_albedo*): the reflectance at the closest hit, csrc/rt_albedo.h
MATERIAL_KINDS = ("lambertian", "metal", "dielectric", "diffuse_light", "isotropic", "pbr")


def query_albedo(b: SceneBuilder, rays, t_min: float = 1e-5, seed: int = 0, want_hits: bool = False):
    """rt_query_albedo: the albedo at the closest hit of n rays, (n, 7) f64 -> (n, 3); with want_hits also the (n, 16) records, the words
    `query_hits` returns for the same rays and seed.  Misses, emitters and dielectrics are (1, 1, 1)."""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != RAY_DOUBLES:
        raise ValueError(f"rays of shape {r.shape}: want (n, {RAY_DOUBLES})")
    out = np.zeros((len(r), 3), dtype=np.float64)
    hits = np.zeros((len(r), HIT_DOUBLES), dtype=np.float64) if want_hits else None
    _check(_rt().rt_query_albedo(b.h, len(r), r.ctypes.data, float(t_min), seed, 0, out.ctypes.data, hits.ctypes.data if want_hits else None))
    return (out, hits) if want_hits else out


def query_albedo_device(b: SceneBuilder, n: int, d_rays, d_albedo, d_hits=None, t_min: float = 1e-5, seed: int = 0, stream: int = 0,
                        d_albedo_bytes=None, d_hits_bytes=None) -> None:
    """rt_query_albedo_device: the same for buffers in device memory (torch tensors of f64, or raw pointers with their sizes), enqueued on
    `stream`; never waits.  d_rays and d_hits 16-byte aligned."""
    rays_ptr, _ = _device_buffer(d_rays)
    alb_ptr, abytes = _device_buffer(d_albedo)
    abytes = abytes if d_albedo_bytes is None else int(d_albedo_bytes)
    hits_ptr, hbytes = (None, 0) if d_hits is None else _device_buffer(d_hits)
    hbytes = hbytes if d_hits_bytes is None else int(d_hits_bytes)
    if abytes is None or hbytes is None:
        raise ValueError("d_albedo_bytes / d_hits_bytes are needed with raw pointers")
    _check(_rt().rt_query_albedo_device(b.h, n, C.c_void_p(rays_ptr), float(t_min), seed, 0, C.c_void_p(alb_ptr), abytes, C.c_void_p(hits_ptr), hbytes,
                                        C.c_void_p(stream)))


def query_camera_albedo(b: SceneBuilder, cam: CameraParams, W: int, H: int, first_sample: int = 0, n_samples: int = 1,
                        seed: int = DEFAULT_SEED) -> np.ndarray:
    """rt_query_camera_albedo: per pixel the sum over samples [first_sample, first_sample + n_samples) of the albedo under that sample's
    camera ray -> (H, W, 3) f64, row 0 = top; divide by n_samples for the mean."""
    out = np.zeros((H, W, 3), dtype=np.float64)
    _check(_rt().rt_query_camera_albedo(b.h, C.byref(cam), W, H, first_sample, n_samples, seed, 0, out.ctypes.data))
    return out


def query_camera_albedo_device(b: SceneBuilder, cam: CameraParams, W: int, H: int, d_albedo_sum, first_sample: int = 0, n_samples: int = 1,
                               seed: int = DEFAULT_SEED, stream: int = 0, d_albedo_sum_bytes=None) -> None:
    """rt_query_camera_albedo_device: the W*H*3 sums into device memory, enqueued on `stream`; never waits."""
    ptr, nbytes = _device_buffer(d_albedo_sum)
    nbytes = nbytes if d_albedo_sum_bytes is None else int(d_albedo_sum_bytes)
    if nbytes is None:
        raise ValueError("d_albedo_sum_bytes is needed with a raw pointer")
    _check(_rt().rt_query_camera_albedo_device(b.h, C.byref(cam), W, H, first_sample, n_samples, seed, 0, C.c_void_p(ptr), nbytes, C.c_void_p(stream)))


# ---- averaged denoising guides (rt_query_camera_guide*, rt_guide_from_hits_host): csrc/rt_guide.h
# the guide record's 16 doubles by name: HIT_FIELDS (t, position, normal, front_face are means over the hitting samples, u, v, prim_kind and
# prim_index carry nothing) and the coverage count in the last word
GUIDE_FIELDS = dict(HIT_FIELDS, hits=slice(15, 16))


def query_camera_guide(b: SceneBuilder, cam: CameraParams, W: int, H: int, first_sample: int = 0, n_samples: int = 16,
                       seed: int = DEFAULT_SEED, want_albedo: bool = False):
    """rt_query_camera_guide: per pixel the first-hit records of samples [first_sample, first_sample + n_samples) reduced to one record
    every denoiser takes as `hits` -> (H, W, 16) (GUIDE_FIELDS); with want_albedo also (H, W, 3), the words `query_camera_albedo` gives for
    the same samples, from the same searches."""
    out = np.zeros((H, W, HIT_DOUBLES), dtype=np.float64)
    alb = np.zeros((H, W, 3), dtype=np.float64) if want_albedo else None
    _check(_rt().rt_query_camera_guide(b.h, C.byref(cam), W, H, first_sample, n_samples, seed, 0, out.ctypes.data,
                                       alb.ctypes.data if want_albedo else None))
    return (out, alb) if want_albedo else out


def query_camera_guide_device(b: SceneBuilder, cam: CameraParams, W: int, H: int, d_guide, d_albedo_sum=None, first_sample: int = 0,
                              n_samples: int = 16, seed: int = DEFAULT_SEED, stream: int = 0, d_guide_bytes=None, d_albedo_sum_bytes=None) -> None:
    """rt_query_camera_guide_device: the W*H*16 records (and, with d_albedo_sum, the W*H*3 albedo sums) into device memory (torch tensors of
    f64, or raw pointers with their sizes), enqueued on `stream`; never waits."""
    g_ptr, gbytes = _device_buffer(d_guide)
    gbytes = gbytes if d_guide_bytes is None else int(d_guide_bytes)
    a_ptr, abytes = _device_buffer(d_albedo_sum) if d_albedo_sum is not None else (None, 0)
    abytes = abytes if d_albedo_sum_bytes is None else int(d_albedo_sum_bytes)
    if gbytes is None or abytes is None:
        raise ValueError("d_guide_bytes / d_albedo_sum_bytes are needed with raw pointers")
    _check(_rt().rt_query_camera_guide_device(b.h, C.byref(cam), W, H, first_sample, n_samples, seed, 0, C.c_void_p(g_ptr), gbytes,
                                              C.c_void_p(a_ptr), abytes, C.c_void_p(stream)))


# ---- specular-chain guides (rt_query_chain*, rt_query_camera_chain_guide*, rt_chain_step_host): csrc/rt_chain.h
# the Metal fuzz up to which a chain follows a mirror: 0.0 follows perfect mirrors only.  An untuned starting value, not a measured optimum.
CHAIN_MAX_FUZZ = 0.0
CHAIN_MAX_LINKS = 64
CHAIN_STATUS = ("continue", "non_specular", "miss", "absorbed", "non_finite", "fuzz")
# the chain record's 16 doubles by name: HIT_FIELDS with t the path length in units of the first ray's parameter, and the links followed
CHAIN_FIELDS = dict(HIT_FIELDS, links=slice(15, 16))


def query_chain(b: SceneBuilder, rays, max_links: int, max_fuzz: float = CHAIN_MAX_FUZZ, t_min: float = 1e-5, seed: int = 0, want_albedo: bool = False):
    """rt_query_chain: n rays followed through mirrors and glass to the first non-specular surface, (n, 7) f64 -> (n, 16) (CHAIN_FIELDS);
    with want_albedo also (n, 3), the albedo there times the mirrors' tints.  max_links = 0 gives `query_hits`' and `query_albedo`'s words."""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != RAY_DOUBLES:
        raise ValueError(f"rays of shape {r.shape}: want (n, {RAY_DOUBLES})")
    hits = np.zeros((len(r), HIT_DOUBLES), dtype=np.float64)
    alb = np.zeros((len(r), 3), dtype=np.float64) if want_albedo else None
    _check(_rt().rt_query_chain(b.h, len(r), r.ctypes.data, float(t_min), seed, int(max_links), float(max_fuzz), 0, hits.ctypes.data,
                                alb.ctypes.data if want_albedo else None))
    return (hits, alb) if want_albedo else hits


def query_chain_device(b: SceneBuilder, n: int, d_rays, d_hits, max_links: int, max_fuzz: float = CHAIN_MAX_FUZZ, d_albedo=None, t_min: float = 1e-5,
                       seed: int = 0, stream: int = 0, d_hits_bytes=None, d_albedo_bytes=None) -> None:
    """rt_query_chain_device: the same for buffers in device memory (torch tensors of f64, or raw pointers with their sizes), enqueued on
    `stream`; never waits.  d_rays and d_hits 16-byte aligned."""
    rays_ptr, _ = _device_buffer(d_rays)
    hits_ptr, hbytes = _device_buffer(d_hits)
    hbytes = hbytes if d_hits_bytes is None else int(d_hits_bytes)
    alb_ptr, abytes = (None, 0) if d_albedo is None else _device_buffer(d_albedo)
    abytes = abytes if d_albedo_bytes is None else int(d_albedo_bytes)
    if abytes is None or hbytes is None:
        raise ValueError("d_hits_bytes / d_albedo_bytes are needed with raw pointers")
    _check(_rt().rt_query_chain_device(b.h, n, C.c_void_p(rays_ptr), float(t_min), seed, int(max_links), float(max_fuzz), 0, C.c_void_p(hits_ptr), hbytes,
                                       C.c_void_p(alb_ptr), abytes, C.c_void_p(stream)))


def query_camera_chain_guide(b: SceneBuilder, cam: CameraParams, W: int, H: int, max_links: int, max_fuzz: float = CHAIN_MAX_FUZZ, first_sample: int = 0,
                             n_samples: int = 16, seed: int = DEFAULT_SEED, want_albedo: bool = False, want_links: bool = False):
    """rt_query_camera_chain_guide: per pixel the chain records of samples [first_sample, first_sample + n_samples) reduced as
    `query_camera_guide` reduces first hits -> (H, W, 16) (GUIDE_FIELDS); with want_albedo also the (H, W, 3) sums of the chain albedos, with
    want_links also (H, W) uint32, the links followed over all samples.  Returns the guide, or a tuple in that order."""
    out = np.zeros((H, W, HIT_DOUBLES), dtype=np.float64)
    alb = np.zeros((H, W, 3), dtype=np.float64) if want_albedo else None
    links = np.zeros((H, W), dtype=np.uint32) if want_links else None
    _check(_rt().rt_query_camera_chain_guide(b.h, C.byref(cam), W, H, first_sample, n_samples, seed, int(max_links), float(max_fuzz), 0, out.ctypes.data,
                                             alb.ctypes.data if want_albedo else None, links.ctypes.data if want_links else None))
    res = (out,) + ((alb,) if want_albedo else ()) + ((links,) if want_links else ())
    return res if len(res) > 1 else out


def query_camera_chain_guide_device(b: SceneBuilder, cam: CameraParams, W: int, H: int, d_guide, max_links: int, max_fuzz: float = CHAIN_MAX_FUZZ,
                                    d_albedo_sum=None, d_links=None, first_sample: int = 0, n_samples: int = 16, seed: int = DEFAULT_SEED, stream: int = 0,
                                    d_guide_bytes=None, d_albedo_sum_bytes=None, d_links_bytes=None) -> None:
    """rt_query_camera_chain_guide_device: the W*H*16 records (and, when given, the W*H*3 albedo sums and the W*H uint32 link counts) into
    device memory (torch tensors, or raw pointers with their sizes), enqueued on `stream`; never waits."""
    g_ptr, gbytes = _device_buffer(d_guide)
    gbytes = gbytes if d_guide_bytes is None else int(d_guide_bytes)
    a_ptr, abytes = _device_buffer(d_albedo_sum) if d_albedo_sum is not None else (None, 0)
    abytes = abytes if d_albedo_sum_bytes is None else int(d_albedo_sum_bytes)
    l_ptr, lbytes = _device_buffer(d_links) if d_links is not None else (None, 0)
    lbytes = lbytes if d_links_bytes is None else int(d_links_bytes)
    if gbytes is None or abytes is None or lbytes is None:
        raise ValueError("d_guide_bytes / d_albedo_sum_bytes / d_links_bytes are needed with raw pointers")
    _check(_rt().rt_query_camera_chain_guide_device(b.h, C.byref(cam), W, H, first_sample, n_samples, seed, int(max_links), float(max_fuzz), 0,
                                                    C.c_void_p(g_ptr), gbytes, C.c_void_p(a_ptr), abytes, C.c_void_p(l_ptr), lbytes, C.c_void_p(stream)))


def chain_step_host(b: SceneBuilder, rays, hits, max_fuzz: float = CHAIN_MAX_FUZZ):
    """rt_chain_step_host (no GPU): one link of a chain on n (ray, record) pairs, (n, 7) and (n, 16) -> the next rays (n, 7), this link's
    weight factors (n, 3) and the status words (n,) uint32 (CHAIN_STATUS)."""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    h = np.ascontiguousarray(hits, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != RAY_DOUBLES or h.shape != (len(r), HIT_DOUBLES):
        raise ValueError(f"rays of shape {r.shape} and hits of shape {h.shape}: want (n, {RAY_DOUBLES}) and (n, {HIT_DOUBLES})")
    nxt = np.zeros_like(r)
    weight = np.zeros((len(r), 3), dtype=np.float64)
    status = np.zeros(len(r), dtype=np.uint32)
    _check(_rt().rt_chain_step_host(b.h, len(r), r.ctypes.data, h.ctypes.data, float(max_fuzz), nxt.ctypes.data, weight.ctypes.data, status.ctypes.data))
    return nxt, weight, status


def guide_from_hits(hits) -> np.ndarray:
    """rt_guide_from_hits_host (no GPU): the guide's specification as plain C++ on stacked records, (n_samples, H, W, 16) or
    (n_samples, n, 16) as n_samples calls of `query_camera` / `query_hits` return them -> (H, W, 16) or (n, 16)."""
    h = np.ascontiguousarray(hits, dtype=np.float64)
    if h.ndim not in (3, 4) or h.shape[-1] != HIT_DOUBLES:
        raise ValueError(f"hits of shape {h.shape}: (n_samples, H, W, 16) or (n_samples, n, 16) is needed")
    out = np.zeros(h.shape[1:], dtype=np.float64)
    _check(_rt().rt_guide_from_hits_host(h.ctypes.data, h.shape[0], int(np.prod(h.shape[1:-1])), out.ctypes.data))
    return out


def material_info(b: SceneBuilder, material: int) -> dict:
    """rt_material_info (host only): {"kind": index into MATERIAL_KINDS, "texture": handle or -1, "albedo": (3,) — Metal's, else zeros}."""
    kt = (C.c_int32 * 2)()
    alb = (C.c_double * 3)()
    _check(_rt().rt_material_info(b.h, int(material), kt, alb))
    return {"kind": int(kt[0]), "texture": int(kt[1]), "albedo": np.array(alb, dtype=np.float64)}


def albedo_image(albedo_sum: np.ndarray, n_samples: int) -> np.ndarray:
    """An (H, W, 3) 8-bit image of an albedo frame, as `rtrender --aov albedo` writes it: the mean held to [0, 1], times 255.999, truncated
    (no gamma: an albedo is data, not radiance)."""
    a = np.asarray(albedo_sum, dtype=np.float64) / float(n_samples)
    return (np.clip(np.nan_to_num(a, nan=0.0), 0.0, 1.0) * 255.999).astype(np.uint8)


def last_query_ms(b: SceneBuilder) -> float:
    """Milliseconds of the most recent query kernel of this scene (HIP events; waits for it)."""
    ms = C.c_float()
    _check(_rt().rt_last_query_ms(b.h, C.byref(ms)))
    return float(ms.value)


def last_query_launch(b: SceneBuilder) -> dict:
    """rt_last_query_launch: the launch geometry of the most recent query kernel of this scene (ray, albedo or radiance query, pixel-list
    pass) as the host computed it — workgroups, threads per workgroup, waves (workgroups x threads / 64), and paths per chunk / chunks
    of a radiance query or pixel-list pass (0 / 0 for a ray or albedo query).  Waits for nothing; an error before the first query."""
    out = (C.c_uint32 * 4)()
    _check(_rt().rt_last_query_launch(b.h, out))
    wg, th, chunk, n_chunks = (int(x) for x in out)
    return {"workgroups": wg, "threads": th, "waves": wg * (th // 64), "chunk": chunk, "chunks": n_chunks}


LOOP_LIMITS = ("denoise_frame_max_blocks", "denoise_frame_threads", "variance_max_blocks", "variance_threads", "compaction_block_px",
               "scan_threads", "adaptive_error_max_blocks", "adaptive_threads", "adaptive_max_blocks", "resolve_max_blocks", "resolve_threads",
               "resolve_px_per_lane", "query_threads", "radiance_threads", "radiance_chunk", "pixels_threads", "pixels_chunk")


def debug_loop_limits() -> dict:
    """rt_debug_loop_limits (host only): the compiled-in launch limits of the element-wise kernels and the workgroup and chunk sizes of the
    query kernels, by name (include/rt_amd.h has the slots)."""
    n = _rt().rt_debug_loop_limits(None, 0)
    if n != len(LOOP_LIMITS):
        raise RenderError(f"rt_debug_loop_limits reports {n} words, this binding knows {len(LOOP_LIMITS)}")
    out = (C.c_uint32 * n)()
    if _rt().rt_debug_loop_limits(out, n) != n:
        raise RenderError(_err())
    return dict(zip(LOOP_LIMITS, (int(x) for x in out)))


def aov_image(hits: np.ndarray, which: str) -> np.ndarray:
    """An (H, W, 3) 8-bit image of one field of (H, W, 16) hit records, as `rtrender --aov` writes it: "normal" = 0.5 (n + 1) * 255.999
    truncated (a miss: the zero normal, 127); "depth" = t linear between the frame's smallest (255) and largest (0) finite hit t, a miss 0;
    "material" = the handle mod 256 in all channels (a miss or a medium, -1: 255)."""
    H, W, _ = hits.shape

    def level(x):                                   # one channel value: truncated, held to 0 .. 255, a NaN gives 0
        x = np.asarray(x, dtype=np.float64)
        return np.where(x >= 0.0, np.minimum(np.nan_to_num(x, nan=0.0), 255.0), 0.0).astype(np.int64)

    if which == "normal":
        return level(0.5 * (hits[..., 5:8] + 1.0) * 255.999).astype(np.uint8)
    if which == "depth":
        t = hits[..., 1]
        ok = (hits[..., 0] != 0.0) & np.isfinite(t)
        out = np.zeros((H, W), dtype=np.int64)
        if ok.any():
            lo, hi = t[ok].min(), t[ok].max()
            out[ok] = level((hi - t[ok]) / (hi - lo) * 255.999) if hi > lo else 255
        return np.repeat(out[..., None], 3, axis=2).astype(np.uint8)
    if which == "material":
        m = hits[..., 11].astype(np.int64) & 255
        return np.repeat(m[..., None], 3, axis=2).astype(np.uint8)
    raise KeyError(which)


# ---- denoising (rt_denoise*): the edge-avoiding a-trous filter of csrc/rt_denoise.h over a frame of sums, guided by query_camera's records
RT_DENOISE_SAME_MATERIAL = 1
# Defaults of the Python layer (the C entry points take them explicitly), read off DESIGN.md §14's error table (profiles/denoise.log): with
# sigma = (colour 4, normal 0.5, plane 0.02) — the setting of that table and of tests/test_denoise_host.py's quality check — two iterations
# (a 9 x 9 footprint) have the lowest or second-lowest error at 16 and at 64 samples per pixel on the two untextured preview scenes (Cornell
# box 0.20 / 0.17 of the raw error, teapot room 0.09 / 0.20), and every further iteration raises the error on the two textured ones.
DENOISE_ITERATIONS = 2
DENOISE_SIGMA = (4.0, 0.5, 0.02)


def _denoise_settings(iterations, sigma):
    k = DENOISE_ITERATIONS if iterations is None else int(iterations)
    sg = DENOISE_SIGMA if sigma is None else tuple(float(x) for x in sigma)
    if len(sg) != 3:
        raise ValueError("sigma = (sigma_c, sigma_n, sigma_p)")
    return k, (C.c_double * 3)(*sg)


def _denoise_frames(rgb_sum, hits):
    a = np.ascontiguousarray(rgb_sum, dtype=np.float64)
    g = np.ascontiguousarray(hits, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or g.shape != a.shape[:2] + (HIT_DOUBLES,):
        raise ValueError(f"rgb_sum of shape {a.shape} and hits of shape {g.shape}: want (H, W, 3) and (H, W, {HIT_DOUBLES})")
    return a, g


def _denoise_call(fn, rgb_sum, samples, hits, iterations, sigma, flags):
    a, g = _denoise_frames(rgb_sum, hits)
    k, sg = _denoise_settings(iterations, sigma)
    out = np.zeros_like(a)
    _check(fn(a.ctypes.data, int(samples), g.ctypes.data, a.shape[1], a.shape[0], k, sg, flags, out.ctypes.data))
    return out


def denoise_host(rgb_sum, samples: int, hits, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
    """rt_denoise_host (no GPU): the filter's specification as plain C++.  rgb_sum (H, W, 3) sums holding `samples` samples per pixel, hits
    (H, W, 16) records of query_camera -> the filtered frame, (H, W, 3), in sum units (hand it to format_image / write_ppm with `samples`)."""
    return _denoise_call(_rt().rt_denoise_host, rgb_sum, samples, hits, iterations, sigma, flags)


def denoise(rgb_sum, samples: int, hits, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
    """rt_denoise: the same call computed by the HIP kernels on the current device — the same words as denoise_host."""
    return _denoise_call(_rt().rt_denoise, rgb_sum, samples, hits, iterations, sigma, flags)


def denoise_workspace_bytes(W: int, H: int) -> int:
    return int(_rt().rt_denoise_workspace_bytes(W, H))


def denoise_device(d_rgb_sum, samples: int, d_hits, W: int, H: int, d_rgb_sum_out=None, d_workspace=None, iterations: int = None, sigma=None,
                   flags: int = 0, stream: int = 0, workspace_bytes=None):
    """rt_denoise_device: the filter for sums and records in device memory (torch tensors of f64, or raw pointers), enqueued on `stream`;
    never waits.  d_rgb_sum_out: None filters in place.  d_workspace: a tensor (or a raw pointer with workspace_bytes) of at least
    denoise_workspace_bytes(W, H) bytes; None allocates a torch tensor on d_rgb_sum's device, which is returned so that the caller keeps it
    alive until the stream has run."""
    sum_ptr, _ = _device_buffer(d_rgb_sum)
    hits_ptr, _ = _device_buffer(d_hits)
    out_ptr = sum_ptr if d_rgb_sum_out is None else _device_buffer(d_rgb_sum_out)[0]
    if d_workspace is None:
        import torch
        d_workspace = torch.empty(denoise_workspace_bytes(W, H), dtype=torch.uint8, device=d_rgb_sum.device)
    ws_ptr, nbytes = _device_buffer(d_workspace)
    nbytes = nbytes if workspace_bytes is None else int(workspace_bytes)
    if nbytes is None:
        raise ValueError("workspace_bytes is needed with a raw pointer")
    k, sg = _denoise_settings(iterations, sigma)
    _check(_rt().rt_denoise_device(C.c_void_p(sum_ptr), int(samples), C.c_void_p(hits_ptr), W, H, k, sg, flags, C.c_void_p(out_ptr),
                                   C.c_void_p(ws_ptr), nbytes, C.c_void_p(stream)))
    return d_workspace


# ---- albedo-demodulated denoising (rt_denoise_albedo*, csrc/rt_albedo.h): the same filter on rgb_sum / albedo, multiplied back
def _denoise_albedo_call(fn, rgb_sum, samples, albedo_sum, albedo_samples, hits, iterations, sigma, flags):
    a, g = _denoise_frames(rgb_sum, hits)
    al = np.ascontiguousarray(albedo_sum, dtype=np.float64)
    if al.shape != a.shape:
        raise ValueError(f"albedo_sum of shape {al.shape} for a frame of {a.shape}")
    k, sg = _denoise_settings(iterations, sigma)
    out = np.zeros_like(a)
    _check(fn(a.ctypes.data, int(samples), al.ctypes.data, int(albedo_samples), g.ctypes.data, a.shape[1], a.shape[0], k, sg, flags, out.ctypes.data))
    return out


def denoise_albedo_host(rgb_sum, samples: int, albedo_sum, albedo_samples: int, hits, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
    """rt_denoise_albedo_host (no GPU): the demodulated filter's specification as plain C++.  albedo_sum (H, W, 3) as query_camera_albedo
    returns it, holding albedo_samples samples per pixel; the rest as `denoise_host`."""
    return _denoise_albedo_call(_rt().rt_denoise_albedo_host, rgb_sum, samples, albedo_sum, albedo_samples, hits, iterations, sigma, flags)


def denoise_albedo(rgb_sum, samples: int, albedo_sum, albedo_samples: int, hits, iterations: int = None, sigma=None, flags: int = 0) -> np.ndarray:
    """rt_denoise_albedo: the same call computed by the HIP kernels on the current device — the same words as denoise_albedo_host."""
    return _denoise_albedo_call(_rt().rt_denoise_albedo, rgb_sum, samples, albedo_sum, albedo_samples, hits, iterations, sigma, flags)


def denoise_albedo_workspace_bytes(W: int, H: int) -> int:
    return int(_rt().rt_denoise_albedo_workspace_bytes(W, H))


def denoise_albedo_device(d_rgb_sum, samples: int, d_albedo_sum, albedo_samples: int, d_hits, W: int, H: int, d_rgb_sum_out=None, d_workspace=None,
                          iterations: int = None, sigma=None, flags: int = 0, stream: int = 0, workspace_bytes=None):
    """rt_denoise_albedo_device: `denoise_device` with demodulation; the workspace is denoise_albedo_workspace_bytes(W, H) bytes."""
    sum_ptr, _ = _device_buffer(d_rgb_sum)
    alb_ptr, _ = _device_buffer(d_albedo_sum)
    hits_ptr, _ = _device_buffer(d_hits)
    out_ptr = sum_ptr if d_rgb_sum_out is None else _device_buffer(d_rgb_sum_out)[0]
    if d_workspace is None:
        import torch
        d_workspace = torch.empty(denoise_albedo_workspace_bytes(W, H), dtype=torch.uint8, device=d_rgb_sum.device)
    ws_ptr, nbytes = _device_buffer(d_workspace)
    nbytes = nbytes if workspace_bytes is None else int(workspace_bytes)
    if nbytes is None:
        raise ValueError("workspace_bytes is needed with a raw pointer")
    k, sg = _denoise_settings(iterations, sigma)
    _check(_rt().rt_denoise_albedo_device(C.c_void_p(sum_ptr), int(samples), C.c_void_p(alb_ptr), int(albedo_samples), C.c_void_p(hits_ptr), W, H, k, sg,
                                          flags, C.c_void_p(out_ptr), C.c_void_p(ws_ptr), nbytes, C.c_void_p(stream)))
    return d_workspace


# ---- variance-guided denoising (rt_denoise_variance*, csrc/rt_denoise_var.h): the colour stop in standard deviations of the frame's own noise.
# The default sigma_v: DESIGN.md ("Variance-guided denoising") has the errors by sigma_v and K that it was chosen from.
DENOISE_VARIANCE_SIGMA = (3.0, 0.5, 0.02)


def _denoise_variance_settings(iterations, sigma):
    return _denoise_settings(iterations, DENOISE_VARIANCE_SIGMA if sigma is None else sigma)


def _denoise_variance_call(fn, rgb_sum, samples, var, hits, iterations, sigma, flags, want_var):
    a, g = _denoise_frames(rgb_sum, hits)
    v = np.ascontiguousarray(var, dtype=np.float64)
    if v.shape != a.shape:
        raise ValueError(f"var of shape {v.shape} for a frame of {a.shape}: the variance of the mean per pixel and channel")
    k, sg = _denoise_variance_settings(iterations, sigma)
    out = np.zeros_like(a)
    v_out = np.zeros(a.shape[:2], dtype=np.float64) if want_var else None
    _check(fn(a.ctypes.data, int(samples), v.ctypes.data, g.ctypes.data, a.shape[1], a.shape[0], k, sg, flags, out.ctypes.data,
              v_out.ctypes.data if want_var else None))
    return (out, v_out) if want_var else out


def denoise_variance_host(rgb_sum, samples: int, var, hits, iterations: int = None, sigma=None, flags: int = 0, want_var: bool = False):
    """rt_denoise_variance_host (no GPU): the variance-guided filter's specification as plain C++.  var (H, W, 3): the variance of the mean
    of every pixel and channel, as `moments_variance_host` / `Progressive.variance` return it; sigma = (sigma_v, sigma_n, sigma_p), sigma_v
    in standard deviations; the rest as `denoise_host`.  want_var: also the filtered variance, (H, W)."""
    return _denoise_variance_call(_rt().rt_denoise_variance_host, rgb_sum, samples, var, hits, iterations, sigma, flags, want_var)


def denoise_variance(rgb_sum, samples: int, var, hits, iterations: int = None, sigma=None, flags: int = 0, want_var: bool = False):
    """rt_denoise_variance: the same call computed by the HIP kernels on the current device — the same words as denoise_variance_host."""
    return _denoise_variance_call(_rt().rt_denoise_variance, rgb_sum, samples, var, hits, iterations, sigma, flags, want_var)


def denoise_variance_workspace_bytes(W: int, H: int) -> int:
    return int(_rt().rt_denoise_variance_workspace_bytes(W, H))


def denoise_variance_device(d_rgb_sum, samples: int, d_var, d_hits, W: int, H: int, d_rgb_sum_out=None, d_var_out=None, d_workspace=None,
                            iterations: int = None, sigma=None, flags: int = 0, stream: int = 0, workspace_bytes=None):
    """rt_denoise_variance_device: `denoise_device` with the per-channel variance frame d_var (W*H*3 f64 in device memory); d_var_out: None,
    or W*H f64 that receive the filtered variance.  The workspace is denoise_variance_workspace_bytes(W, H) bytes."""
    sum_ptr, _ = _device_buffer(d_rgb_sum)
    var_ptr, _ = _device_buffer(d_var)
    hits_ptr, _ = _device_buffer(d_hits)
    out_ptr = sum_ptr if d_rgb_sum_out is None else _device_buffer(d_rgb_sum_out)[0]
    vout_ptr = None if d_var_out is None else _device_buffer(d_var_out)[0]
    if d_workspace is None:
        import torch
        d_workspace = torch.empty(denoise_variance_workspace_bytes(W, H), dtype=torch.uint8, device=d_rgb_sum.device)
    ws_ptr, nbytes = _device_buffer(d_workspace)
    nbytes = nbytes if workspace_bytes is None else int(workspace_bytes)
    if nbytes is None:
        raise ValueError("workspace_bytes is needed with a raw pointer")
    k, sg = _denoise_variance_settings(iterations, sigma)
    _check(_rt().rt_denoise_variance_device(C.c_void_p(sum_ptr), int(samples), C.c_void_p(var_ptr), C.c_void_p(hits_ptr), W, H, k, sg, flags,
                                            C.c_void_p(out_ptr), C.c_void_p(vout_ptr), C.c_void_p(ws_ptr), nbytes, C.c_void_p(stream)))
    return d_workspace


# ---- moments (rt_moments_*, csrc/rt_moments.h): the second moment of pass sums and the per-pixel error estimate of a frame of passes
def moments_stats(words, tau: float) -> dict:
    """The four words of rt_moments_stats_host / rt_moments_error_device / rt_progressive_error_stats as a dict: the three pixel counts,
    max_e2 (the largest finite e2, a float), max_error = sqrt(max_e2) in display units, and tau."""
    w = [int(x) for x in words]
    max_e2 = float(np.array([w[3]], dtype=np.uint64).view(np.float64)[0])
    return {"converged": w[0], "unconverged": w[1], "nonfinite": w[2], "max_e2": max_e2, "max_error": math.sqrt(max_e2), "tau": float(tau)}


def moments_merge_host(pass_sum, n_samples: int, rgb_sum: np.ndarray, sq_sum: np.ndarray) -> None:
    """rt_moments_merge_host (no GPU): merges the pass frame `pass_sum` of n_samples samples per pixel into rgb_sum and sq_sum IN PLACE
    (C-contiguous f64 arrays of pass_sum's size): S += p, Q += p * p / n_samples."""
    p = np.ascontiguousarray(pass_sum, dtype=np.float64)
    for a in (rgb_sum, sq_sum):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.size == p.size):
            raise ValueError("rgb_sum and sq_sum are merged in place: C-contiguous float64 arrays of pass_sum's size")
    _check(_rt().rt_moments_merge_host(p.ctypes.data, int(n_samples), rgb_sum.ctypes.data, sq_sum.ctypes.data, p.size))


def _moments_frames(rgb_sum, sq_sum):
    s = np.ascontiguousarray(rgb_sum, dtype=np.float64)
    q = np.ascontiguousarray(sq_sum, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 3 or q.shape != s.shape:
        raise ValueError(f"rgb_sum of shape {s.shape} and sq_sum of shape {q.shape}: want (H, W, 3) twice")
    return s, q


def moments_error_host(rgb_sum, sq_sum, samples: int, passes: int) -> np.ndarray:
    """rt_moments_error_host (no GPU): e2 of every pixel, (H, W), from (H, W, 3) sums and second moments of `passes` passes holding
    `samples` samples per pixel."""
    s, q = _moments_frames(rgb_sum, sq_sum)
    out = np.zeros(s.shape[:2], dtype=np.float64)
    _check(_rt().rt_moments_error_host(s.ctypes.data, q.ctypes.data, int(samples), int(passes), s.shape[1], s.shape[0], out.ctypes.data))
    return out


def moments_variance_host(rgb_sum, sq_sum, samples: int, passes: int) -> np.ndarray:
    """rt_moments_variance_host (no GPU): the variance of the mean of every pixel and channel, (H, W, 3) — the V that e2 is computed from
    (csrc/rt_moments.h (4)), and the input of `denoise_variance`."""
    s, q = _moments_frames(rgb_sum, sq_sum)
    out = np.zeros_like(s)
    _check(_rt().rt_moments_variance_host(s.ctypes.data, q.ctypes.data, int(samples), int(passes), s.shape[1], s.shape[0], out.ctypes.data))
    return out


def moments_variance(rgb_sum, sq_sum, samples: int, passes: int) -> np.ndarray:
    """`moments_variance_host`'s words computed by the HIP kernel on the current device (through torch tensors)."""
    import torch
    s, q = _moments_frames(rgb_sum, sq_sum)
    d_s, d_q = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(q.copy()).cuda()      # (a copy: the caller's arrays may be read-only)
    d_v = torch.empty_like(d_s)
    moments_variance_device(d_s, d_q, samples, passes, s.shape[1], s.shape[0], d_v, stream=torch.cuda.current_stream().cuda_stream)
    return d_v.cpu().numpy()


def moments_variance_device(d_rgb_sum, d_sq_sum, samples: int, passes: int, W: int, H: int, d_var_out, stream: int = 0) -> None:
    """rt_moments_variance_device: the variance frame (d_var_out, W*H*3 f64) for frames in device memory, enqueued on `stream`; never waits."""
    _check(_rt().rt_moments_variance_device(C.c_void_p(_device_buffer(d_rgb_sum)[0]), C.c_void_p(_device_buffer(d_sq_sum)[0]), int(samples), int(passes),
                                            W, H, C.c_void_p(_device_buffer(d_var_out)[0]), C.c_void_p(stream)))


def moments_stats_host(e2, tau: float) -> dict:
    """rt_moments_stats_host (no GPU): `moments_stats` of an error map for the threshold tau."""
    e = np.ascontiguousarray(e2, dtype=np.float64)
    words = (C.c_uint64 * 4)()
    _check(_rt().rt_moments_stats_host(e.ctypes.data, e.size, float(tau), words))
    return moments_stats(words, tau)


def moments_merge_device(d_pass_sum, n_samples: int, d_rgb_sum, d_sq_sum, n_doubles=None, stream: int = 0) -> None:
    """rt_moments_merge_device: the merge for frames in device memory (torch tensors of f64, or raw pointers with n_doubles), enqueued on
    `stream`; never waits; d_pass_sum is all +0.0 afterwards."""
    p_ptr, nbytes = _device_buffer(d_pass_sum)
    n = nbytes // 8 if n_doubles is None and nbytes is not None else n_doubles
    if n is None:
        raise ValueError("n_doubles is needed with a raw pointer")
    _check(_rt().rt_moments_merge_device(C.c_void_p(p_ptr), int(n_samples), C.c_void_p(_device_buffer(d_rgb_sum)[0]),
                                         C.c_void_p(_device_buffer(d_sq_sum)[0]), int(n), C.c_void_p(stream)))


def moments_error_device(d_rgb_sum, d_sq_sum, samples: int, passes: int, W: int, H: int, d_e2_out=None, tau: float = 0.0, d_stats_out=None,
                         stream: int = 0) -> None:
    """rt_moments_error_device: the error map (d_e2_out, W*H f64) and / or the four statistics words for tau (d_stats_out, 4 x int64 /
    uint64; read them with `moments_stats`), for frames in device memory, enqueued on `stream`; never waits."""
    e2_ptr = None if d_e2_out is None else _device_buffer(d_e2_out)[0]
    st_ptr = None if d_stats_out is None else _device_buffer(d_stats_out)[0]
    _check(_rt().rt_moments_error_device(C.c_void_p(_device_buffer(d_rgb_sum)[0]), C.c_void_p(_device_buffer(d_sq_sum)[0]), int(samples), int(passes),
                                         W, H, C.c_void_p(e2_ptr), float(tau), C.c_void_p(st_ptr), C.c_void_p(stream)))


# ---- adaptive frames (rt_adaptive_*, rt_render_pixels_device; csrc/rt_adaptive.h): per-pixel sample counts through error, selection, merge, resolve
ADAPTIVE_MAX_SAMPLES = 2 ** 32 - 1


def _adaptive_state(rgb_sum, sq_sum, counts, passes):
    s, q = _moments_frames(rgb_sum, sq_sum)
    n = np.ascontiguousarray(counts, dtype=np.uint32); b = np.ascontiguousarray(passes, dtype=np.uint32)
    if n.shape != s.shape[:2] or b.shape != n.shape:
        raise ValueError(f"counts of shape {n.shape} and passes of shape {b.shape} for frames of shape {s.shape}: want (H, W) twice")
    return s, q, n, b


def adaptive_error_host(rgb_sum, sq_sum, counts, passes, tau=None):
    """rt_adaptive_error_host (no GPU): e2 of every pixel, (H, W), from (H, W, 3) sums and second moments and (H, W) uint32 per-pixel sample
    and pass counts; +inf where a pixel has fewer than two passes.  With tau: (e2, `moments_stats` of the map)."""
    s, q, n, b = _adaptive_state(rgb_sum, sq_sum, counts, passes)
    out = np.zeros(n.shape, dtype=np.float64)
    words = (C.c_uint64 * 4)()
    _check(_rt().rt_adaptive_error_host(s.ctypes.data, q.ctypes.data, n.ctypes.data, b.ctypes.data, s.shape[1], s.shape[0], out.ctypes.data,
                                        0.0 if tau is None else float(tau), None if tau is None else words))
    return out if tau is None else (out, moments_stats(words, tau))


def adaptive_select_host(rgb_sum, sq_sum, counts, passes, n_samples: int, tau: float, max_samples: int = ADAPTIVE_MAX_SAMPLES, spread: int = 1) -> np.ndarray:
    """rt_adaptive_select_host (no GPU): the ascending output-order indices (uint32) of the pixels a pass of n_samples would sample."""
    s, q, n, b = _adaptive_state(rgb_sum, sq_sum, counts, passes)
    out = np.zeros(n.size, dtype=np.uint32)
    count = C.c_uint32()
    _check(_rt().rt_adaptive_select_host(s.ctypes.data, q.ctypes.data, n.ctypes.data, b.ctypes.data, s.shape[1], s.shape[0], int(n_samples), float(tau),
                                         int(max_samples), int(spread), out.ctypes.data, C.byref(count)))
    return out[:count.value].copy()


def adaptive_merge_host(pass_sum: np.ndarray, n_samples: int, rgb_sum: np.ndarray, sq_sum: np.ndarray, counts: np.ndarray, passes: np.ndarray, pixels) -> None:
    """rt_adaptive_merge_host (no GPU): merges the listed pixels of the pass frame IN PLACE into rgb_sum, sq_sum, counts and passes and zeroes
    them in pass_sum; every other pixel is left alone.  All five are C-contiguous arrays, (H, W, 3) float64 / (H, W) uint32."""
    for a, dt in ((pass_sum, np.float64), (rgb_sum, np.float64), (sq_sum, np.float64), (counts, np.uint32), (passes, np.uint32)):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("the frames are merged in place: writeable C-contiguous float64 (frames) and uint32 (counts) arrays")
    if rgb_sum.ndim != 3 or rgb_sum.shape[2] != 3 or pass_sum.shape != rgb_sum.shape or sq_sum.shape != rgb_sum.shape or counts.shape != rgb_sum.shape[:2] or passes.shape != counts.shape:
        raise ValueError("want (H, W, 3) frames and (H, W) counts of one size")
    px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
    _check(_rt().rt_adaptive_merge_host(pass_sum.ctypes.data, int(n_samples), rgb_sum.ctypes.data, sq_sum.ctypes.data, counts.ctypes.data, passes.ctypes.data,
                                        px.ctypes.data if px.size else None, px.size, rgb_sum.shape[1], rgb_sum.shape[0]))


def adaptive_resolve_rgb8_host(rgb_sum, counts, rgb8_prev=None):
    """rt_adaptive_resolve_rgb8_host (no GPU): format_color with every pixel's own count -> ((H, W, 3) uint8, pixels that differ from rgb8_prev)."""
    s = np.ascontiguousarray(rgb_sum, dtype=np.float64); n = np.ascontiguousarray(counts, dtype=np.uint32)
    if s.ndim != 3 or s.shape[2] != 3 or n.shape != s.shape[:2]:
        raise ValueError(f"rgb_sum of shape {s.shape} and counts of shape {n.shape}: want (H, W, 3) and (H, W)")
    prev = None if rgb8_prev is None else np.ascontiguousarray(rgb8_prev, dtype=np.uint8)
    if prev is not None and prev.shape != s.shape:
        raise ValueError("rgb8_prev must have the frame's shape")
    out = np.zeros(s.shape, dtype=np.uint8)
    changed = C.c_uint64()
    _check(_rt().rt_adaptive_resolve_rgb8_host(s.ctypes.data, n.ctypes.data, s.shape[1], s.shape[0], None if prev is None else prev.ctypes.data, out.ctypes.data,
                                               C.byref(changed)))
    return out, int(changed.value)


def _ptr_or_none(x):
    return C.c_void_p(None if x is None else _device_buffer(x)[0])


def adaptive_error_device(d_rgb_sum, d_sq_sum, d_counts, d_passes, W: int, H: int, d_e2_out=None, tau: float = 0.0, d_stats_out=None, stream: int = 0) -> None:
    """rt_adaptive_error_device: `adaptive_error_host` for frames in device memory, enqueued on `stream`; never waits."""
    _check(_rt().rt_adaptive_error_device(_ptr_or_none(d_rgb_sum), _ptr_or_none(d_sq_sum), _ptr_or_none(d_counts), _ptr_or_none(d_passes), W, H,
                                          _ptr_or_none(d_e2_out), float(tau), _ptr_or_none(d_stats_out), C.c_void_p(stream)))


def adaptive_select_workspace_bytes(W: int, H: int) -> int:
    return int(_rt().rt_adaptive_select_workspace_bytes(W, H))


def adaptive_select_device(d_rgb_sum, d_sq_sum, d_counts, d_passes, W: int, H: int, n_samples: int, tau: float, d_list_out, d_n_list_out, d_workspace,
                           max_samples: int = ADAPTIVE_MAX_SAMPLES, spread: int = 1, stream: int = 0, workspace_bytes=None) -> None:
    """rt_adaptive_select_device: the list (room for W*H uint32 / int32) and its length (one word) in device memory; the workspace is
    `adaptive_select_workspace_bytes(W, H)` bytes, 16-byte aligned.  Enqueued on `stream`; never waits."""
    ws_ptr, nbytes = _device_buffer(d_workspace)
    nbytes = nbytes if workspace_bytes is None else int(workspace_bytes)
    if nbytes is None:
        raise ValueError("workspace_bytes is needed with a raw pointer")
    _check(_rt().rt_adaptive_select_device(_ptr_or_none(d_rgb_sum), _ptr_or_none(d_sq_sum), _ptr_or_none(d_counts), _ptr_or_none(d_passes), W, H, int(n_samples),
                                           float(tau), int(max_samples), int(spread), _ptr_or_none(d_list_out), _ptr_or_none(d_n_list_out), C.c_void_p(ws_ptr), nbytes,
                                           C.c_void_p(stream)))


def adaptive_merge_device(d_pass_sum, n_samples: int, d_rgb_sum, d_sq_sum, d_counts, d_passes, d_list, n_list: int, stream: int = 0) -> None:
    """rt_adaptive_merge_device: the list merge for frames in device memory, enqueued on `stream`; never waits."""
    _check(_rt().rt_adaptive_merge_device(_ptr_or_none(d_pass_sum), int(n_samples), _ptr_or_none(d_rgb_sum), _ptr_or_none(d_sq_sum), _ptr_or_none(d_counts),
                                          _ptr_or_none(d_passes), _ptr_or_none(d_list), int(n_list), C.c_void_p(stream)))


def adaptive_resolve_rgb8_device(d_rgb_sum, d_counts, W: int, H: int, d_rgb8_out, d_rgb8_prev=None, d_changed=None, stream: int = 0) -> None:
    """rt_adaptive_resolve_rgb8_device: the resolve with counts for frames in device memory; the changed-pixel count is ADDED to d_changed."""
    _check(_rt().rt_adaptive_resolve_rgb8_device(_ptr_or_none(d_rgb_sum), _ptr_or_none(d_counts), W, H, _ptr_or_none(d_rgb8_prev), _ptr_or_none(d_rgb8_out),
                                                 _ptr_or_none(d_changed), C.c_void_p(stream)))


def render_pixels_device(b: SceneBuilder, cam: CameraParams, background, W: int, H: int, n_samples: int, max_depth: int, d_list, n_list: int, d_out,
                         d_counts=None, seed: int = DEFAULT_SEED, flags: int = 0, stream: int = 0, d_out_bytes=None) -> None:
    """rt_render_pixels_device: n_samples samples of every pixel of d_list (n_list ascending output-order indices, uint32 / int32 in device
    memory) ADDED to the W*H*3 f64 frame d_out; pixel p receives samples [d_counts[p], d_counts[p] + n_samples) of the frame `render` with
    the same view and seed would hold (d_counts None: from sample 0).  Enqueued on `stream`; never waits."""
    out_ptr, nbytes = _device_buffer(d_out)
    nbytes = nbytes if d_out_bytes is None else int(d_out_bytes)
    if nbytes is None:
        raise ValueError("d_out_bytes is needed with a raw pointer")
    bg = (C.c_double * 3)(*[float(x) for x in background])
    _check(_rt().rt_render_pixels_device(b.h, C.byref(cam), bg, W, H, int(n_samples), max_depth, seed, flags, _ptr_or_none(d_list), int(n_list),
                                         _ptr_or_none(d_counts), C.c_void_p(out_ptr), nbytes, C.c_void_p(stream)))


# ---- denoising a frame as it is (rt_adaptive_variance*, rt_denoise_frame*; csrc/rt_denoise_frame.h): one sample count or a count per pixel,
# with or without a variance frame, with or without albedo sums, around the unchanged filters
DENOISE_STOP_COLOUR = 0
DENOISE_STOP_VARIANCE = 1


def adaptive_variance_host(rgb_sum, sq_sum, counts, passes) -> np.ndarray:
    """rt_adaptive_variance_host (no GPU): the variance of the mean of every pixel and channel, (H, W, 3), from every pixel's own sample and
    pass counts ((H, W) uint32); +inf where a pixel has fewer than two passes.  With equal counts: `moments_variance_host`."""
    s, q, n, b = _adaptive_state(rgb_sum, sq_sum, counts, passes)
    out = np.zeros(s.shape, dtype=np.float64)
    _check(_rt().rt_adaptive_variance_host(s.ctypes.data, q.ctypes.data, n.ctypes.data, b.ctypes.data, s.shape[1], s.shape[0], out.ctypes.data))
    return out


def adaptive_variance(rgb_sum, sq_sum, counts, passes) -> np.ndarray:
    """The same frame computed by the HIP kernel on the current device (rt_adaptive_variance_device on torch tensors) — the same words."""
    import torch
    s, q, n, b = _adaptive_state(rgb_sum, sq_sum, counts, passes)
    d_s, d_q = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(q.copy()).cuda()
    d_n, d_b = torch.from_numpy(n.view(np.int32).copy()).cuda(), torch.from_numpy(b.view(np.int32).copy()).cuda()
    d_v = torch.empty_like(d_s)
    adaptive_variance_device(d_s, d_q, d_n, d_b, s.shape[1], s.shape[0], d_v)
    torch.cuda.synchronize()
    return d_v.cpu().numpy()


def adaptive_variance_device(d_rgb_sum, d_sq_sum, d_counts, d_passes, W: int, H: int, d_var_out, stream: int = 0) -> None:
    """rt_adaptive_variance_device: `adaptive_variance_host` for frames in device memory, enqueued on `stream`; never waits."""
    _check(_rt().rt_adaptive_variance_device(_ptr_or_none(d_rgb_sum), _ptr_or_none(d_sq_sum), _ptr_or_none(d_counts), _ptr_or_none(d_passes), W, H,
                                             _ptr_or_none(d_var_out), C.c_void_p(stream)))


def _denoise_frame_call(fn, rgb_sum, hits, counts, samples, var, albedo_sum, albedo_samples, iterations, sigma, flags, want_var):
    a, g = _denoise_frames(rgb_sum, hits)
    n = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    if n is not None and n.shape != a.shape[:2]:
        raise ValueError(f"counts of shape {n.shape} for a frame of {a.shape}: want (H, W)")
    v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    al = None if albedo_sum is None else np.ascontiguousarray(albedo_sum, dtype=np.float64)
    for name, x in (("var", v), ("albedo_sum", al)):
        if x is not None and x.shape != a.shape:
            raise ValueError(f"{name} of shape {x.shape} for a frame of {a.shape}")
    k, sg = _denoise_settings(iterations, sigma) if v is None else _denoise_variance_settings(iterations, sigma)
    out = np.zeros_like(a)
    v_out = np.zeros(a.shape[:2], dtype=np.float64) if want_var else None
    _check(fn(a.ctypes.data, None if n is None else n.ctypes.data, int(samples), None if v is None else v.ctypes.data,
              None if al is None else al.ctypes.data, int(albedo_samples), g.ctypes.data, a.shape[1], a.shape[0], k, sg, flags, out.ctypes.data,
              v_out.ctypes.data if want_var else None))
    return (out, v_out) if want_var else out


def denoise_frame_host(rgb_sum, hits, counts=None, samples: int = 1, var=None, albedo_sum=None, albedo_samples: int = 1, iterations: int = None, sigma=None,
                       flags: int = 0, want_var: bool = False):
    """rt_denoise_frame_host (no GPU): the frame denoise of csrc/rt_denoise_frame.h as plain C++.  counts (H, W) uint32 or None (then `samples`
    is the frame's count); var (H, W, 3) or None (None: the colour stop of `denoise_host`, else the variance stop of `denoise_variance_host`
    and its default sigma); albedo_sum (H, W, 3) holding albedo_samples samples, or None.  -> the filtered frame in sum units, (H, W, 3);
    want_var (needs var): also the filtered variance, (H, W) — of the demodulated frame when albedo_sum is given."""
    return _denoise_frame_call(_rt().rt_denoise_frame_host, rgb_sum, hits, counts, samples, var, albedo_sum, albedo_samples, iterations, sigma, flags, want_var)


def denoise_frame(rgb_sum, hits, counts=None, samples: int = 1, var=None, albedo_sum=None, albedo_samples: int = 1, iterations: int = None, sigma=None,
                  flags: int = 0, want_var: bool = False):
    """rt_denoise_frame: the same call computed by the HIP kernels on the current device — the same words as denoise_frame_host."""
    return _denoise_frame_call(_rt().rt_denoise_frame, rgb_sum, hits, counts, samples, var, albedo_sum, albedo_samples, iterations, sigma, flags, want_var)


def denoise_frame_workspace_bytes(W: int, H: int) -> int:
    return int(_rt().rt_denoise_frame_workspace_bytes(W, H))


def denoise_frame_device(d_rgb_sum, d_hits, W: int, H: int, d_counts=None, samples: int = 1, d_var=None, d_albedo_sum=None, albedo_samples: int = 1,
                         d_rgb_sum_out=None, d_var_out=None, d_workspace=None, iterations: int = None, sigma=None, flags: int = 0, stream: int = 0,
                         workspace_bytes=None):
    """rt_denoise_frame_device: `denoise_device` for a frame as it is — d_counts (W*H uint32 / int32), d_var and d_albedo_sum (W*H*3 f64) in
    device memory, each optional; d_var_out: None, or W*H f64.  The workspace is denoise_frame_workspace_bytes(W, H) bytes."""
    sum_ptr, _ = _device_buffer(d_rgb_sum)
    out_ptr = sum_ptr if d_rgb_sum_out is None else _device_buffer(d_rgb_sum_out)[0]
    if d_workspace is None:
        import torch
        d_workspace = torch.empty(denoise_frame_workspace_bytes(W, H), dtype=torch.uint8, device=d_rgb_sum.device)
    ws_ptr, nbytes = _device_buffer(d_workspace)
    nbytes = nbytes if workspace_bytes is None else int(workspace_bytes)
    if nbytes is None:
        raise ValueError("workspace_bytes is needed with a raw pointer")
    k, sg = _denoise_settings(iterations, sigma) if d_var is None else _denoise_variance_settings(iterations, sigma)
    _check(_rt().rt_denoise_frame_device(C.c_void_p(sum_ptr), _ptr_or_none(d_counts), int(samples), _ptr_or_none(d_var), _ptr_or_none(d_albedo_sum),
                                         int(albedo_samples), _ptr_or_none(d_hits), W, H, k, sg, flags, C.c_void_p(out_ptr), _ptr_or_none(d_var_out),
                                         C.c_void_p(ws_ptr), nbytes, C.c_void_p(stream)))
    return d_workspace


# ---- temporal accumulation (rt_reproject*, rt_temporal_blend*; csrc/rt_reproject.h): a frame's history reprojected into a new view, and the
# blend of a frame with such a history.  The two defaults are starting values, NOT tuned: normal_min 0.9 (about 26 degrees) and sigma_p 0.01 (a
# plane distance of 1 % of the distance from the previous camera) follow the usual SVGF-style tests, and 64 is a cap after which new samples
# still weigh 1 / 5 at 16 samples per view.
REPROJECT_SIGMA = (0.9, 0.01)
REPROJECT_MAX_HISTORY = 64


def _reproject_settings(max_history, sigma):
    cap = REPROJECT_MAX_HISTORY if max_history is None else int(max_history)
    sg = REPROJECT_SIGMA if sigma is None else tuple(float(x) for x in sigma)
    if len(sg) != 2:
        raise ValueError("sigma = (normal_min, sigma_p)")
    return cap, (C.c_double * 2)(*sg)


def _reproject_frames(prev_sum, prev_counts, prev_hits, cur_hits):
    s = np.ascontiguousarray(prev_sum, dtype=np.float64)
    g0 = np.ascontiguousarray(prev_hits, dtype=np.float64); g1 = np.ascontiguousarray(cur_hits, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 3 or g0.shape != s.shape[:2] + (HIT_DOUBLES,) or g1.shape != g0.shape:
        raise ValueError(f"prev_sum of shape {s.shape}, prev_hits {g0.shape}, cur_hits {g1.shape}: want (H, W, 3), (H, W, {HIT_DOUBLES}) twice")
    n = None if prev_counts is None else np.ascontiguousarray(prev_counts, dtype=np.uint32)
    if n is not None and n.shape != s.shape[:2]:
        raise ValueError(f"prev_counts of shape {n.shape} for a frame of {s.shape}: want (H, W)")
    return s, n, g0, g1


def _reproject_call(fn, prev_sum, prev_hits, prev_cam, cur_hits, prev_counts, prev_samples, max_history, sigma, flags):
    s, n, g0, g1 = _reproject_frames(prev_sum, prev_counts, prev_hits, cur_hits)
    cap, sg = _reproject_settings(max_history, sigma)
    hs = np.zeros_like(s); hn = np.zeros(s.shape[:2], dtype=np.uint32)
    _check(fn(s.ctypes.data, None if n is None else n.ctypes.data, int(prev_samples), g0.ctypes.data, C.byref(prev_cam), g1.ctypes.data, s.shape[1], s.shape[0],
              cap, sg, flags, hs.ctypes.data, hn.ctypes.data))
    return hs, hn


def reproject_host(prev_sum, prev_hits, prev_cam: CameraParams, cur_hits, prev_counts=None, prev_samples: int = 1, max_history: int = None, sigma=None,
                   flags: int = 0):
    """rt_reproject_host (no GPU): the history of the previous view's frame in the new view, csrc/rt_reproject.h as plain C++.  prev_sum
    (H, W, 3) sums with prev_counts (H, W) uint32 or, when None, prev_samples samples in every pixel; prev_hits / cur_hits (H, W, 16): the
    `query_camera` or `query_camera_guide` records of the previous view (camera prev_cam) and of the new one.  -> (hist_sum (H, W, 3),
    hist_counts (H, W) uint32): a frame with counts, 0 where a pixel has no history."""
    return _reproject_call(_rt().rt_reproject_host, prev_sum, prev_hits, prev_cam, cur_hits, prev_counts, prev_samples, max_history, sigma, flags)


def reproject(prev_sum, prev_hits, prev_cam: CameraParams, cur_hits, prev_counts=None, prev_samples: int = 1, max_history: int = None, sigma=None,
              flags: int = 0):
    """rt_reproject: the same call computed by the HIP kernel on the current device — the same words as reproject_host."""
    return _reproject_call(_rt().rt_reproject, prev_sum, prev_hits, prev_cam, cur_hits, prev_counts, prev_samples, max_history, sigma, flags)


def reproject_device(d_prev_sum, d_prev_hits, prev_cam: CameraParams, d_cur_hits, W: int, H: int, d_hist_sum_out, d_hist_counts_out, d_prev_counts=None,
                     prev_samples: int = 1, max_history: int = None, sigma=None, flags: int = 0, stream: int = 0) -> None:
    """rt_reproject_device: `reproject` for frames in device memory (torch tensors or raw pointers; records 16-byte aligned), enqueued on
    `stream`; never waits, never allocates.  The outputs may overlap no input."""
    cap, sg = _reproject_settings(max_history, sigma)
    _check(_rt().rt_reproject_device(_ptr_or_none(d_prev_sum), _ptr_or_none(d_prev_counts), int(prev_samples), _ptr_or_none(d_prev_hits), C.byref(prev_cam),
                                     _ptr_or_none(d_cur_hits), W, H, cap, sg, flags, _ptr_or_none(d_hist_sum_out), _ptr_or_none(d_hist_counts_out), C.c_void_p(stream)))


def temporal_blend_host(rgb_sum, hist_sum, hist_counts, counts=None, samples: int = 0):
    """rt_temporal_blend_host (no GPU): a frame — rgb_sum (H, W, 3) with counts (H, W) uint32 or, when None, `samples` samples in every
    pixel — blended with a history -> (sum (H, W, 3), counts (H, W) uint32): the sums added, the counts added and held at 2^32 - 1.  The
    result goes to `adaptive_resolve_rgb8_host` and `denoise_frame_host(counts=...)` as it is."""
    s = np.ascontiguousarray(rgb_sum, dtype=np.float64); hs = np.ascontiguousarray(hist_sum, dtype=np.float64)
    hn = np.ascontiguousarray(hist_counts, dtype=np.uint32)
    n = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    if s.ndim != 3 or s.shape[2] != 3 or hs.shape != s.shape or hn.shape != s.shape[:2] or (n is not None and n.shape != hn.shape):
        raise ValueError(f"rgb_sum of shape {s.shape}, hist_sum {hs.shape}, hist_counts {hn.shape}: want (H, W, 3) twice and (H, W)")
    out = np.zeros_like(s); out_n = np.zeros_like(hn)
    _check(_rt().rt_temporal_blend_host(s.ctypes.data, None if n is None else n.ctypes.data, int(samples), hs.ctypes.data, hn.ctypes.data, s.shape[1], s.shape[0],
                                        out.ctypes.data, out_n.ctypes.data))
    return out, out_n


def temporal_blend_device(d_rgb_sum, d_hist_sum, d_hist_counts, W: int, H: int, d_sum_out=None, d_counts_out=None, d_counts=None, samples: int = 0,
                          stream: int = 0) -> None:
    """rt_temporal_blend_device: `temporal_blend_host` for frames in device memory, enqueued on `stream`; never waits.  d_sum_out None: in
    place in d_rgb_sum; d_counts_out None: in place in d_counts (which must then be given)."""
    _check(_rt().rt_temporal_blend_device(_ptr_or_none(d_rgb_sum), _ptr_or_none(d_counts), int(samples), _ptr_or_none(d_hist_sum), _ptr_or_none(d_hist_counts), W, H,
                                          _ptr_or_none(d_rgb_sum if d_sum_out is None else d_sum_out), _ptr_or_none(d_counts if d_counts_out is None else d_counts_out),
                                          C.c_void_p(stream)))


# ---- temporal variance (rt_reproject_variance*, rt_temporal_blend_variance*; csrc/rt_reproject_var.h): the variance of a frame's per-pixel mean
# carried through a camera move beside the history.  A variance is known when it is finite and >= 0; unknown is +inf.
def _reproject_variance_call(fn, prev_sum, prev_var, prev_hits, prev_cam, cur_hits, prev_counts, prev_samples, max_history, sigma, flags):
    s, n, g0, g1 = _reproject_frames(prev_sum, prev_counts, prev_hits, cur_hits)
    v = np.ascontiguousarray(prev_var, dtype=np.float64)
    if v.shape != s.shape:
        raise ValueError(f"prev_var of shape {v.shape} for a frame of {s.shape}: the variance of the mean per pixel and channel")
    cap, sg = _reproject_settings(max_history, sigma)
    hs = np.zeros_like(s); hn = np.zeros(s.shape[:2], dtype=np.uint32); hv = np.zeros_like(s)
    _check(fn(s.ctypes.data, None if n is None else n.ctypes.data, int(prev_samples), v.ctypes.data, g0.ctypes.data, C.byref(prev_cam), g1.ctypes.data, s.shape[1],
              s.shape[0], cap, sg, flags, hs.ctypes.data, hn.ctypes.data, hv.ctypes.data))
    return hs, hn, hv


def reproject_variance_host(prev_sum, prev_var, prev_hits, prev_cam: CameraParams, cur_hits, prev_counts=None, prev_samples: int = 1, max_history: int = None,
                            sigma=None, flags: int = 0):
    """rt_reproject_variance_host (no GPU): `reproject_host` with prev_var (H, W, 3), the variance of the previous frame's per-pixel mean
    (`Progressive.variance`, `adaptive_variance_host` or an earlier `temporal_blend_variance_host`), carried along -> (hist_sum, hist_counts,
    hist_var (H, W, 3)).  The first two are `reproject_host`'s words; hist_var is +inf where a pixel has history of unknown variance and +0.0
    where it has none."""
    return _reproject_variance_call(_rt().rt_reproject_variance_host, prev_sum, prev_var, prev_hits, prev_cam, cur_hits, prev_counts, prev_samples, max_history, sigma, flags)


def reproject_variance(prev_sum, prev_var, prev_hits, prev_cam: CameraParams, cur_hits, prev_counts=None, prev_samples: int = 1, max_history: int = None,
                       sigma=None, flags: int = 0):
    """rt_reproject_variance: the same call computed by the fused HIP kernel on the current device — the same words as reproject_variance_host."""
    return _reproject_variance_call(_rt().rt_reproject_variance, prev_sum, prev_var, prev_hits, prev_cam, cur_hits, prev_counts, prev_samples, max_history, sigma, flags)


def reproject_variance_device(d_prev_sum, d_prev_var, d_prev_hits, prev_cam: CameraParams, d_cur_hits, W: int, H: int, d_hist_sum_out, d_hist_counts_out,
                              d_hist_var_out, d_prev_counts=None, prev_samples: int = 1, max_history: int = None, sigma=None, flags: int = 0, stream: int = 0) -> None:
    """rt_reproject_variance_device: `reproject_variance` for frames in device memory (torch tensors or raw pointers; records 16-byte
    aligned), one launch enqueued on `stream`; never waits, never allocates.  The outputs may overlap no input."""
    cap, sg = _reproject_settings(max_history, sigma)
    _check(_rt().rt_reproject_variance_device(_ptr_or_none(d_prev_sum), _ptr_or_none(d_prev_counts), int(prev_samples), _ptr_or_none(d_prev_var),
                                              _ptr_or_none(d_prev_hits), C.byref(prev_cam), _ptr_or_none(d_cur_hits), W, H, cap, sg, flags,
                                              _ptr_or_none(d_hist_sum_out), _ptr_or_none(d_hist_counts_out), _ptr_or_none(d_hist_var_out), C.c_void_p(stream)))


def temporal_blend_variance_host(var, hist_var, hist_counts, counts=None, samples: int = 0):
    """rt_temporal_blend_variance_host (no GPU): the variance of the mean of `temporal_blend_host`'s frame -> (H, W, 3).  var (H, W, 3) or
    None (unknown everywhere: a frame with fewer than two passes) with counts (H, W) uint32 or `samples`; hist_var / hist_counts from
    `reproject_variance`.  The result goes to `denoise_frame_host(counts=the blend's counts, var=...)` as it is."""
    hv = np.ascontiguousarray(hist_var, dtype=np.float64); hn = np.ascontiguousarray(hist_counts, dtype=np.uint32)
    v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    n = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    if hv.ndim != 3 or hv.shape[2] != 3 or hn.shape != hv.shape[:2] or (v is not None and v.shape != hv.shape) or (n is not None and n.shape != hn.shape):
        raise ValueError(f"hist_var of shape {hv.shape}, hist_counts {hn.shape}: want (H, W, 3) and (H, W), var and counts alike")
    out = np.zeros_like(hv)
    _check(_rt().rt_temporal_blend_variance_host(None if v is None else v.ctypes.data, None if n is None else n.ctypes.data, int(samples), hv.ctypes.data,
                                                 hn.ctypes.data, hn.size, out.ctypes.data))
    return out


def temporal_blend_variance_device(d_var, d_hist_var, d_hist_counts, n_px: int, d_var_out=None, d_counts=None, samples: int = 0, stream: int = 0) -> None:
    """rt_temporal_blend_variance_device: `temporal_blend_variance_host` for frames in device memory, enqueued on `stream`; never waits.
    d_var may be None; d_var_out None: in place in d_var (which must then be given)."""
    _check(_rt().rt_temporal_blend_variance_device(_ptr_or_none(d_var), _ptr_or_none(d_counts), int(samples), _ptr_or_none(d_hist_var), _ptr_or_none(d_hist_counts),
                                                   int(n_px), _ptr_or_none(d_var if d_var_out is None else d_var_out), C.c_void_p(stream)))


def kernel_time_total(b: SceneBuilder, reset: bool = False):
    """(total ms, launches) of this scene's kernels since the last reset; waits for launches in flight."""
    ms, n = C.c_double(), C.c_ulonglong()
    _check(_rt().rt_kernel_time_total(b.h, C.byref(ms), C.byref(n), 1 if reset else 0))
    return float(ms.value), int(n.value)


def last_flush_count(b: SceneBuilder) -> int:
    """Accumulator flushes of the last launch (three f64 atomics to the frame each)."""
    out = C.c_ulonglong()
    _check(_rt().rt_last_flush_count(b.h, C.byref(out)))
    return int(out.value)


def last_traversal_stats(b: SceneBuilder) -> dict:
    """BVH scenes: advance passes / traversal steps of the last launch and the lanes busy in each (summed over wavefronts)."""
    out = (C.c_ulonglong * 4)()
    _check(_rt().rt_last_traversal_stats(b.h, out))
    leaf = (C.c_ulonglong * 2)()
    _check(_rt().rt_last_leaf_steps(b.h, leaf))
    return {"advance_passes": out[0], "advance_lanes": out[1], "traversal_steps": out[2], "traversal_lanes": out[3],
            "leaf_steps": leaf[0], "leaf_lanes": leaf[1]}          # of the traversal steps: the primitive-test steps (the rest test boxes)


def last_launch_info(b: SceneBuilder) -> dict:
    """Geometry of the most recent launch (workgroups, threads, LDS bytes, BVH nodes staged in LDS / in the scene, workgroups per CU)."""
    out = (C.c_uint32 * 6)()
    _check(_rt().rt_last_launch_info(b.h, out))
    return dict(zip(("workgroups", "threads", "lds_bytes", "bvh_nodes_in_lds", "bvh_nodes", "workgroups_per_cu"), [int(x) for x in out]))


def last_kernel_ms(b: SceneBuilder) -> float:
    ms = C.c_float()
    _check(_rt().rt_last_kernel_ms(b.h, C.byref(ms)))
    return float(ms.value)


def last_stats(b: SceneBuilder) -> dict:
    st = (C.c_ulonglong * 3)()
    _check(_rt().rt_last_stats(b.h, st))
    return {"nonfinite_samples": int(st[0]), "wave_iterations": int(st[1]), "live_lane_iterations": int(st[2])}


def format_image(rgb_sum: np.ndarray, spp: int) -> np.ndarray:
    """Vec3::format_color (src/vec.rs:125-131) over a whole frame -> (H, W, 3) uint8-range ints."""
    H, W, _ = rgb_sum.shape
    out = np.zeros((H, W, 3), dtype=np.uint64)
    flat = np.ascontiguousarray(rgb_sum, dtype=np.float64).reshape(-1, 3)
    o = out.reshape(-1, 3)
    fn = _lib.load().fn("format_color")
    buf = (C.c_uint64 * 3)()
    for p in range(flat.shape[0]):
        fn(flat[p].ctypes.data_as(C.POINTER(C.c_double)), spp, buf)
        o[p, 0], o[p, 1], o[p, 2] = buf[0], buf[1], buf[2]
    return out


def write_ppm(path: str, rgb_sum: np.ndarray, spp: int) -> None:
    """The reference's P3 emitter (src/main.rs:767-769,832)."""
    H, W, _ = rgb_sum.shape
    a = np.ascontiguousarray(rgb_sum, dtype=np.float64)
    _check(_rt().rt_write_ppm(path.encode(), a.ctypes.data, W, H, spp))

"""The ctypes signature of every function of include/rt_amd.h: the one place where `restype` / `argtypes` of an `rt_*` function are set.

A call through ctypes without a declaration treats every integer argument and the return value as `c_int`: a 64-bit pointer, a
`uint64_t` seed or a `size_t` is then truncated silently.  So every function is declared when its library is loaded (`_lib.load_path`
declares all of them, `api.Backend` the builder subset under its prefix), and tests/test_python_binding.py compares this table with the
header, function by function.  The table is written by hand: where an argument is `c_void_p` (callers pass `array.ctypes.data` or None)
and where it is a typed pointer (callers pass a ctypes array or `byref`) is a choice made per call site.
"""
from __future__ import annotations

import ctypes as C

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_u32_p = C.POINTER(C.c_uint32)
c_u64_p = C.POINTER(C.c_uint64)
c_ull_p = C.POINTER(C.c_ulonglong)
c_void_pp = C.POINTER(C.c_void_p)
_int, _u32, _u64, _f64, _ptr = C.c_int, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p


class CameraParams(C.Structure):
    """rt_camera: the arguments of Camera::new (src/camera.rs:19)."""
    _fields_ = [("lookfrom", C.c_double * 3), ("lookat", C.c_double * 3), ("vup", C.c_double * 3),
                ("vfov", C.c_double), ("aspect", C.c_double), ("aperture", C.c_double),
                ("focus_dist", C.c_double), ("time0", C.c_double), ("time1", C.c_double)]


_cam_p = C.POINTER(CameraParams)
# scene, camera, background, W, H, samples_per_pixel, max_depth, seed, flags: how every entry point that takes a frame begins
_FRAME = [_ptr, _cam_p, c_double_p, _u32, _u32, _u32, _u32, _u64, _u32]
_HITS = [_u32, _f64, _ptr, _ptr, _ptr]          # n, rect_m, boxes, rays, tlim of the cube / room test hooks

# The builder entry points, which the CPU oracle exports too (under `orc_`): what `api.Backend` declares.  name -> (restype, argtypes)
_BUILDER = {
    "scene_create": (_ptr, []),
    "scene_destroy": (None, [_ptr]),
    "scene_error": (C.c_char_p, [_ptr]),
    "rng_create": (_ptr, [_u64, _u32]),
    "rng_destroy": (None, [_ptr]),
    "rng_f64": (_f64, [_ptr]),
    "rng_range": (_f64, [_ptr, _f64, _f64]),
    "rng_bool": (_int, [_ptr]),
    "rng_index": (_u32, [_ptr, _u32]),
    "rng_u32": (_u32, [_ptr]),
    "rng_path": (None, [_u64, _u32, _u32, c_u32_p]),
    "texture_constant": (_int, [_ptr, c_double_p]),
    "texture_check": (_int, [_ptr, _int, _int]),
    "texture_noise": (_int, [_ptr, _f64, _ptr]),
    "texture_image": (_int, [_ptr, C.c_char_p, _u32, _u32]),
    "material_lambertian": (_int, [_ptr, _int]),
    "material_metal": (_int, [_ptr, c_double_p, _f64]),
    "material_dielectric": (_int, [_ptr, _f64]),
    "material_diffuse_light": (_int, [_ptr, _int]),
    "material_isotropic": (_int, [_ptr, _int]),
    "material_pbr": (_int, [_ptr, _int, c_double_p]),
    "sphere": (_int, [_ptr, c_double_p, _f64, _int]),
    "moving_sphere": (_int, [_ptr, c_double_p, c_double_p, _f64, _f64, _f64, _int]),
    "aarect": (_int, [_ptr, _int] + [_f64] * 5 + [_int]),
    "cube": (_int, [_ptr, c_double_p, c_double_p, _int]),
    "triangle": (_int, [_ptr, c_double_p, _int]),
    "list_create": (_int, [_ptr]),
    "list_push": (_int, [_ptr, _int, _int]),
    "mesh": (_int, [_ptr, c_double_p, _u32, c_u32_p, _u32, _int]),
    "flip_normal": (_int, [_ptr, _int]),
    "translate": (_int, [_ptr, _int, c_double_p]),
    "rotate": (_int, [_ptr, _int, _int, _f64]),
    "constant_medium": (_int, [_ptr, _int, _f64, _int]),
    "bvh": (_int, [_ptr, c_int_p, _u32, _f64, _f64]),
    "bvh_of_list": (_int, [_ptr, _int, _f64, _f64]),
    "scene_set_world": (_int, [_ptr, _int]),
    "lights_push": (_int, [_ptr, _int]),
    "camera_fields": (None, [_cam_p, c_double_p]),
    "format_color": (None, [c_double_p, _u64, c_u64_p]),
}
BUILDER_NAMES = tuple(_BUILDER)

SIGNATURES = {
    **_BUILDER,
    "last_error": (C.c_char_p, []),
    "device_count": (_int, []),
    # host asset ingest
    "mesh_load_obj": (_int, [_ptr, C.c_char_p, c_double_p, _f64, _int]),
    "parse_obj": (_int, [C.c_char_p, C.c_size_t, c_double_p, _f64, C.POINTER(c_double_p), c_u32_p, C.POINTER(c_u32_p), c_u32_p]),
    "decode_jpeg_rgb8": (_ptr, [C.c_char_p, C.c_size_t, c_u32_p, c_u32_p]),
    "free": (None, [_ptr]),
    "write_ppm": (_int, [C.c_char_p, _ptr, _u32, _u32, _u64]),
    # frames
    "scene_flatten": (_int, [_ptr, c_u32_p]),
    "render": (_int, _FRAME + [_ptr]),
    "render_samples": (_int, _FRAME + [_ptr, _ptr]),
    "local_tiles": (_u32, [_u32] * 5),
    "render_device": (_int, _FRAME + [_u32, _u32, _u32, _ptr, C.c_size_t, _ptr]),
    "render_device_pass": (_int, _FRAME + [_u32, _int, _u32, _u32, _u32, _ptr, C.c_size_t, _ptr]),
    "progressive_create": (_ptr, [_ptr, _cam_p, c_double_p, _u32, _u32, _u32, _u64, _u32]),
    "progressive_add": (_int, [_ptr, _u32, _ptr]),
    "progressive_add_async": (_int, [_ptr, _u32, _ptr]),
    "progressive_samples": (_int, [_ptr, c_u64_p]),
    "progressive_resolve_rgb8": (_int, [_ptr, _ptr, c_u64_p]),
    "progressive_resolve_rgb8_device": (_int, [_ptr, c_void_pp, _ptr]),
    "progressive_copy_rgb8": (_int, [_ptr, _ptr, c_u64_p]),
    "progressive_read_sum": (_int, [_ptr, _ptr]),
    "progressive_load_sum": (_int, [_ptr, _ptr, _u64]),
    "progressive_reset": (_int, [_ptr]),
    "progressive_destroy": (None, [_ptr]),
    # moments: the per-pixel error estimate of a progressive frame
    "moments_merge_host": (_int, [_ptr, _u64, _ptr, _ptr, _u64]),
    "moments_merge_device": (_int, [_ptr, _u64, _ptr, _ptr, _u64, _ptr]),
    "moments_error_host": (_int, [_ptr, _ptr, _u64, _u64, _u32, _u32, _ptr]),
    "moments_stats_host": (_int, [_ptr, _u64, _f64, c_u64_p]),
    "moments_error_device": (_int, [_ptr, _ptr, _u64, _u64, _u32, _u32, _ptr, _f64, _ptr, _ptr]),
    "progressive_enable_moments": (_int, [_ptr]),
    "progressive_passes": (_int, [_ptr, c_u64_p]),
    "progressive_read_moments": (_int, [_ptr, _ptr]),
    "progressive_load_moments": (_int, [_ptr, _ptr, _ptr, _u64, _u64]),
    "progressive_error_map": (_int, [_ptr, _ptr]),
    "progressive_error_map_device": (_int, [_ptr, c_void_pp, _ptr]),
    "progressive_error_stats": (_int, [_ptr, _f64, c_u64_p]),
    "moments_variance_host": (_int, [_ptr, _ptr, _u64, _u64, _u32, _u32, _ptr]),
    "moments_variance_device": (_int, [_ptr, _ptr, _u64, _u64, _u32, _u32, _ptr, _ptr]),
    "progressive_variance": (_int, [_ptr, _ptr]),
    # adaptive frames: per-pixel sample counts, the pixel-list kernel
    "render_pixels_device": (_int, _FRAME + [_ptr, _u32, _ptr, _ptr, C.c_size_t, _ptr]),
    "adaptive_error_host": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _f64, c_u64_p]),
    "adaptive_error_device": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _f64, _ptr, _ptr]),
    "adaptive_select_host": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _f64, _u64, _u32, _ptr, c_u32_p]),
    "adaptive_select_workspace_bytes": (C.c_size_t, [_u32, _u32]),
    "adaptive_select_device": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _f64, _u64, _u32, _ptr, _ptr, _ptr, C.c_size_t, _ptr]),
    "adaptive_merge_host": (_int, [_ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32]),
    "adaptive_merge_device": (_int, [_ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr]),
    "adaptive_resolve_rgb8_host": (_int, [_ptr, _ptr, _u32, _u32, _ptr, _ptr, c_u64_p]),
    "adaptive_resolve_rgb8_device": (_int, [_ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr, _ptr]),
    "progressive_enable_adaptive": (_int, [_ptr]),
    "progressive_add_adaptive": (_int, [_ptr, _u32, _f64, _u64, _u32, c_u64_p]),
    "progressive_read_counts": (_int, [_ptr, _ptr, _ptr]),
    "progressive_load_adaptive": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr]),
    # ray queries
    "camera_ray": (_int, [_cam_p, _u32, _u32, _u32, _u32, _u64, _u32, c_double_p]),
    "query_hits": (_int, [_ptr, _u32, _ptr, _f64, _u64, _u32, _ptr]),
    "query_hits_device": (_int, [_ptr, _u32, _ptr, _f64, _u64, _u32, _ptr, C.c_size_t, _ptr]),
    "query_camera": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u64, _u32, _ptr, _ptr]),
    "query_camera_device": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u64, _u32, _ptr, _ptr, C.c_size_t, _ptr]),
    "last_query_ms": (_int, [_ptr, c_float_p]),
    "last_query_launch": (_int, [_ptr, c_u32_p]),
    # albedo queries
    "query_albedo": (_int, [_ptr, _u32, _ptr, _f64, _u64, _u32, _ptr, _ptr]),
    "query_albedo_device": (_int, [_ptr, _u32, _ptr, _f64, _u64, _u32, _ptr, C.c_size_t, _ptr, C.c_size_t, _ptr]),
    "query_camera_albedo": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u32, _u64, _u32, _ptr]),
    "query_camera_albedo_device": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u32, _u64, _u32, _ptr, C.c_size_t, _ptr]),
    # averaged denoising guides
    "query_camera_guide": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u32, _u64, _u32, _ptr, _ptr]),
    "query_camera_guide_device": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u32, _u64, _u32, _ptr, C.c_size_t, _ptr, C.c_size_t, _ptr]),
    "guide_from_hits_host": (_int, [_ptr, _u32, _u64, _ptr]),
    "progressive_set_guide_samples": (_int, [_ptr, _u32]),
    "progressive_guide_info": (_int, [_ptr, c_u32_p, c_u64_p]),
    # specular-chain guides
    "query_chain": (_int, [_ptr, _u32, _ptr, _f64, _u64, _u32, _f64, _u32, _ptr, _ptr]),
    "query_chain_device": (_int, [_ptr, _u32, _ptr, _f64, _u64, _u32, _f64, _u32, _ptr, C.c_size_t, _ptr, C.c_size_t, _ptr]),
    "query_camera_chain_guide": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u32, _u64, _u32, _f64, _u32, _ptr, _ptr, _ptr]),
    "query_camera_chain_guide_device": (_int, [_ptr, _cam_p, _u32, _u32, _u32, _u32, _u64, _u32, _f64, _u32, _ptr, C.c_size_t, _ptr, C.c_size_t,
                                               _ptr, C.c_size_t, _ptr]),
    "chain_step_host": (_int, [_ptr, _u32, _ptr, _ptr, _f64, _ptr, _ptr, _ptr]),
    "progressive_set_guide_chain": (_int, [_ptr, _u32, _f64]),
    "progressive_guide_chain_info": (_int, [_ptr, c_u32_p, c_double_p]),
    "material_info": (_int, [_ptr, _int, C.POINTER(C.c_int32), c_double_p]),
    # denoising
    "denoise_host": (_int, [_ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr]),
    "denoise": (_int, [_ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr]),
    "denoise_workspace_bytes": (C.c_size_t, [_u32, _u32]),
    "denoise_device": (_int, [_ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, C.c_size_t, _ptr]),
    "progressive_resolve_denoised_rgb8": (_int, [_ptr, _u32, c_double_p, _u32, _ptr]),
    "denoise_albedo_host": (_int, [_ptr, _u64, _ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr]),
    "denoise_albedo": (_int, [_ptr, _u64, _ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr]),
    "denoise_albedo_workspace_bytes": (C.c_size_t, [_u32, _u32]),
    "denoise_albedo_device": (_int, [_ptr, _u64, _ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, C.c_size_t, _ptr]),
    "progressive_resolve_denoised_albedo_rgb8": (_int, [_ptr, _u32, _u32, c_double_p, _u32, _ptr]),
    "progressive_albedo_info": (_int, [_ptr, c_u32_p, c_u64_p]),
    "denoise_variance_host": (_int, [_ptr, _u64, _ptr, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr]),
    "denoise_variance": (_int, [_ptr, _u64, _ptr, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr]),
    "denoise_variance_workspace_bytes": (C.c_size_t, [_u32, _u32]),
    "denoise_variance_device": (_int, [_ptr, _u64, _ptr, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, _ptr, C.c_size_t, _ptr]),
    "progressive_resolve_denoised_variance_rgb8": (_int, [_ptr, _u32, c_double_p, _u32, _ptr]),
    # denoising a frame as it is: per-pixel counts, variance and albedo around the same filters
    "adaptive_variance_host": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr]),
    "adaptive_variance_device": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr]),
    "denoise_frame_host": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr]),
    "denoise_frame": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr]),
    "denoise_frame_workspace_bytes": (C.c_size_t, [_u32, _u32]),
    "denoise_frame_device": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, _ptr, C.c_size_t, _ptr]),
    "progressive_variance_counts": (_int, [_ptr, _ptr]),
    "progressive_resolve_denoised_frame_rgb8": (_int, [_ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr]),
    # temporal accumulation: a frame's history reprojected into a new view, and the blend with it
    "reproject_host": (_int, [_ptr, _ptr, _u64, _ptr, _cam_p, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr]),
    "reproject": (_int, [_ptr, _ptr, _u64, _ptr, _cam_p, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr]),
    "reproject_device": (_int, [_ptr, _ptr, _u64, _ptr, _cam_p, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, _ptr]),
    "temporal_blend_host": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u32, _u32, _ptr, _ptr]),
    "temporal_blend_device": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr]),
    "progressive_set_view": (_int, [_ptr, _cam_p, _u64, _u32, c_double_p]),
    "progressive_read_history": (_int, [_ptr, _ptr, _ptr]),
    "progressive_history_info": (_int, [_ptr, c_u64_p]),
    "progressive_resolve_temporal_rgb8": (_int, [_ptr, _u32, c_double_p, _u32, _ptr]),
    # temporal variance: the variance of a frame's mean carried through a camera move, and its blend with a history's
    "reproject_variance_host": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _cam_p, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, _ptr]),
    "reproject_variance": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _cam_p, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, _ptr]),
    "reproject_variance_device": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _cam_p, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, _ptr, _ptr]),
    "temporal_blend_variance_host": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u64, _ptr]),
    "temporal_blend_variance_device": (_int, [_ptr, _ptr, _u64, _ptr, _ptr, _u64, _ptr, _ptr]),
    "progressive_read_history_variance": (_int, [_ptr, _ptr]),
    "progressive_resolve_temporal_variance_rgb8": (_int, [_ptr, _u32, _u32, c_double_p, _u32, _ptr]),
    # radiance queries
    "query_radiance":(_int, [_ptr, _u32, _ptr, c_double_p, _u32, _u32, _u64, _u32, _ptr, _ptr, c_u64_p]),
    "query_radiance_device": (_int, [_ptr, _u32, _ptr, c_double_p, _u32, _u32, _u64, _u32, _u32, _int, _ptr, C.c_size_t, _ptr, _ptr, _ptr]),
    "render_multi": (_int, _FRAME + [_u32, _u32, _ptr]),
    "render_multi_device": (_int, _FRAME + [_u32, _u32, c_void_pp]),
    "multi_sync": (_int, [_ptr]),
    "multi_copy_frame": (_int, [_ptr, _ptr, C.c_size_t]),
    "last_multi_ms": (_int, [_ptr, c_double_p]),
    "last_multi_ranks": (_int, [_ptr, _u32, c_u32_p, c_int_p, c_double_p, c_u32_p]),
    # scene settings
    "scene_set_traversal_schedule": (_int, [_ptr, _u32, _u32, _u32]),
    "scene_set_bvh_builder": (_int, [_ptr, _int]),
    "scene_prepare": (_int, [_ptr, _u32]),
    "scene_calibrate": (_int, _FRAME),
    "scene_set_loop_shape": (_int, [_ptr, _int]),
    "scene_loop_shape": (_int, [_ptr]),
    # what the most recent launch did
    "last_loop_info": (_int, [_ptr, C.POINTER(C.c_int32), c_float_p]),
    "last_kernel_ms": (_int, [_ptr, c_float_p]),
    "kernel_time_total": (_int, [_ptr, c_double_p, c_ull_p, _int]),
    "last_stats": (_int, [_ptr, c_ull_p]),
    "last_launch_info": (_int, [_ptr, c_u32_p]),
    "last_ring_info": (_int, [_ptr, c_u32_p]),
    "last_flush_count": (_int, [_ptr, c_ull_p]),
    "last_traversal_stats": (_int, [_ptr, c_ull_p]),
    "last_leaf_steps": (_int, [_ptr, c_ull_p]),
    # test and diagnostic hooks
    "debug_denoise_ms": (_int, [_ptr, _u64, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, C.c_size_t, c_float_p]),
    "debug_denoise_variance_ms": (_int, [_ptr, _u64, _ptr, _ptr, _u32, _u32, _u32, c_double_p, _u32, _ptr, _ptr, C.c_size_t, c_float_p]),
    "debug_albedo_modulate_ms": (_int, [_ptr, _ptr, _u64, _ptr, _u64, c_float_p]),
    "debug_section_cycles": (_int, [_ptr, c_ull_p]),
    "debug_loop_limits": (_int, [c_u32_p, _u32]),
    "debug_tune_filter": (_int, [_ptr, _ptr]),
    "debug_objects": (_int, [_ptr, _ptr, _u32, c_u32_p]),
    "debug_bvh_links": (_int, [_ptr, c_u32_p, _u32, c_u32_p, _u32, c_u32_p]),
    "debug_filter_nodes": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, c_float_p]),
    "debug_aabb_hit": (_int, [_u32, _ptr, _ptr, _ptr, _ptr]),
    "debug_cube_hit": (_int, _HITS + [_ptr]),
    "debug_room_hit": (_int, _HITS + [_ptr, _ptr]),
    "debug_list_hit": (_int, [_ptr, _u32, _ptr, _ptr, _ptr]),
    "debug_list_hit_masked": (_int, [_ptr, _u32, _ptr, _ptr, _u32, _ptr]),
    "debug_light_pdf": (_int, [_ptr, _u32, _ptr, _ptr, _ptr]),
    "debug_onb": (_int, [_ptr, _u32, _ptr, _ptr, _ptr]),
    "debug_onb_table": (_int, [_ptr, _ptr, _ptr, _u32, c_u32_p]),
    "debug_ring_form": (_int, [_ptr, _u32, c_u32_p, c_u32_p]),
    "debug_ring_normal": (_int, [_ptr, _u32, _ptr, _ptr, _ptr]),
    "debug_onb_table_w": (_int, [_ptr, _ptr, _u32]),
    "debug_ring_w": (_int, [_ptr, _u32, _ptr, _ptr, _ptr]),
    "debug_short_forms": (_int, [_u32, _u32, _ptr, _ptr, _ptr]),
    "debug_math": (_int, [_u32, _u32, _ptr, _ptr, _ptr]),
    "debug_brdf": (_int, [_ptr, _u32, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _u32]),
    "debug_shade": (_int, [_ptr, _u32, _ptr, _ptr, _ptr, _u64, _u32, _u32, _ptr]),
    "debug_primary_mask": (_int, [_ptr, _cam_p, _u32, _u32, _ptr, _u32, _ptr]),
    "debug_primary_mask_host": (_int, [_ptr, _cam_p, _u32, _u32, _ptr, _u32, _ptr]),
    "debug_trace_path": (_int, [_ptr, C.c_longlong, C.c_longlong]),
    "debug_get_trace": (_int, [_ptr, _ptr, _u32]),
}


def declare(lib, prefix: str, names, allow_missing: bool = False) -> None:
    """Set restype and argtypes of `prefix + name` on `lib` for every name.  A symbol the library lacks is an error that names every
    missing one — a stale or partial build — unless allow_missing (tools that load builds of other revisions)."""
    missing = []
    for name in names:
        fn = getattr(lib, prefix + name, None)
        if fn is None:
            missing.append(prefix + name)
            continue
        fn.restype, fn.argtypes = SIGNATURES[name]
    if missing and not allow_missing:
        raise AttributeError(f"{getattr(lib, '_name', lib)} lacks {len(missing)} declared symbol(s): {', '.join(missing)}")

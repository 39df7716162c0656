"""ctypes binding of the C ABI (include/srt_abi.h) and a `Tracer` with the reference's
class shape (/root/reference/include/tracer.hpp:26-88): ctor(width, height), public
`options` / `scene_data`, update_scene(shapes, triangles, materials), clear_canvas(),
render(ticks_stopped, output).

There is NO CPU fallback here: if lib/libsrt_hip.so is missing or no GPU is present the
calls raise. The oracle is never imported from this package.
"""
import ctypes as C
from pathlib import Path

import numpy as np

from . import build as B
from . import records as R

PKG = Path(__file__).resolve().parent
import os  # noqa: E402

# SRT_LIB selects an alternative build of the SAME library (A/B experiments); there is
# still no non-HIP path.
LIB_PATH = Path(os.environ["SRT_LIB"]) if os.environ.get("SRT_LIB") else PKG / "lib" / "libsrt_hip.so"

# every symbol include/srt_abi.h declares
ABI_SYMBOLS = [
    "srt_create", "srt_destroy", "srt_last_error", "srt_set_skybox", "srt_update_scene", "srt_clear_canvas",
    "srt_render", "srt_render_async", "srt_trace", "srt_set_radiance_budget", "srt_resolve", "srt_resolve_external", "srt_synchronize", "srt_read_canvas", "srt_read_argb",
    "srt_get_counters", "srt_set_count_triangles", "srt_reset_counters", "srt_last_kernel_ms", "srt_set_kernel_timers", "srt_last_trace_kernel_ms", "srt_last_trace_launches",
    "srt_device_buffers", "srt_bind_canvas", "srt_bind_stream", "srt_set_partition",
    "srt_partition_owned_rows", "srt_partition_padded_rows", "srt_partition_global_row",
    "srt_partition_unpermute", "srt_selftest_math", "srt_selftest_rare_lanes", "srt_version", "srt_set_acceleration", "srt_acceleration_info", "srt_bvh_build_host", "srt_bvh_wide_host", "srt_debug_counters", "srt_debug_region_counters",
    "srt_comm_unique_id", "srt_comm_init", "srt_gather", "srt_resolve_gathered", "srt_gathered_buffers", "srt_read_gathered",
    "srt_group_create", "srt_group_destroy", "srt_group_last_error", "srt_group_size", "srt_group_tracer", "srt_group_set_skybox",
    "srt_group_set_acceleration", "srt_group_update_scene", "srt_group_clear_canvas", "srt_group_trace_and_gather", "srt_group_render",
    "srt_group_read_canvas", "srt_group_get_counters", "srt_render_pipelined", "srt_pipeline_flush", "srt_unpermute_device",
    "srt_denoise_defaults", "srt_set_denoise", "srt_resolve_denoised", "srt_read_denoised", "srt_read_denoise_inputs",
    "srt_temporal_defaults", "srt_set_denoise_temporal", "srt_reset_denoise_history", "srt_read_denoise_history",
    "srt_set_denoise_object_motion", "srt_read_denoise_shape_ids", "srt_read_denoise_motion", "srt_motion_table_host",
    "srt_set_denoise_vertex_motion", "srt_read_denoise_triangle_ids", "srt_read_denoise_vertex_tables", "srt_motion_table_deform_host",
    "srt_set_textures", "srt_set_material_textures", "srt_set_triangle_uvs", "srt_last_trace_textured", "srt_plane_frame_host",
    "srt_texture_check_host", "srt_group_set_textures", "srt_group_set_material_textures", "srt_group_set_triangle_uvs",
    "srt_last_trace_class", "srt_bernoulli_threshold_host",
    "srt_last_trace_plane_form", "srt_plane_axis_code_host", "srt_selftest_plane_forms", "srt_selftest_diffuse_bounce",
    "srt_set_triangle_materials", "srt_group_set_triangle_materials", "srt_triangle_materials_check_host",
    "srt_group_set_denoise", "srt_group_set_denoise_temporal", "srt_group_reset_denoise_history", "srt_group_resolve_denoised",
    "srt_group_read_denoised", "srt_group_read_denoise_inputs", "srt_group_read_denoise_history", "srt_partition_planes_floats",
    "srt_unpermute_planes_device",
    "srt_set_denoise_demodulation", "srt_group_set_denoise_demodulation", "srt_last_filter_demodulated",
    "srt_group_last_filter_demodulated",
    "srt_set_denoise_spatial_variance", "srt_group_set_denoise_spatial_variance", "srt_last_filter_spatial_variance",
    "srt_group_last_filter_spatial_variance",
    "srt_set_denoise_history_illumination", "srt_group_set_denoise_history_illumination", "srt_last_setup_history_illumination",
    "srt_group_last_setup_history_illumination",
    "srt_set_denoise_history_clamp", "srt_group_set_denoise_history_clamp", "srt_last_setup_history_clamp",
    "srt_group_last_setup_history_clamp", "srt_read_denoise_history_bounds",
    "srt_set_denoise_history_feedback", "srt_group_set_denoise_history_feedback", "srt_last_filter_history_feedback",
    "srt_group_last_filter_history_feedback",
    "srt_bvh_refit_wide_host", "srt_set_acceleration_refit", "srt_group_set_acceleration_refit", "srt_acceleration_refit_info",
    "srt_last_refit_kernel_ms", "srt_read_bvh_blocks", "srt_bvh_wide_order_host",
    "srt_set_acceleration_deform", "srt_group_set_acceleration_deform", "srt_acceleration_deform_info",
    "srt_bvh_refit_deformed_wide_host", "srt_bvh_wide_cost_host",
    "srt_set_acceleration_build", "srt_group_set_acceleration_build", "srt_acceleration_build_info", "srt_last_build_kernel_ms",
    "srt_bvh_morton_order_host", "srt_bvh_morton_wide_host",
    "srt_set_acceleration_build_order", "srt_group_set_acceleration_build_order", "srt_bvh_median_order_host", "srt_bvh_median_wide_host",
    "srt_exposure_defaults", "srt_exposure_check_host", "srt_set_exposure", "srt_group_set_exposure", "srt_reset_exposure",
    "srt_group_reset_exposure", "srt_read_exposure", "srt_group_read_exposure", "srt_last_resolve_exposed",
    "srt_group_last_resolve_exposed",
    "srt_bloom_defaults", "srt_bloom_check_host", "srt_set_bloom", "srt_group_set_bloom", "srt_read_bloom", "srt_group_read_bloom",
    "srt_last_resolve_bloomed", "srt_group_last_resolve_bloomed",
    "srt_noise_defaults", "srt_noise_check_host", "srt_noise_evaluate_host", "srt_set_noise_meter", "srt_group_set_noise_meter",
    "srt_meter_noise", "srt_group_meter_noise", "srt_poll_noise", "srt_group_poll_noise", "srt_read_noise", "srt_group_read_noise",
    "srt_resolve_noise_view", "srt_group_resolve_noise_view", "srt_group_read_noise_view", "srt_render_until", "srt_last_meter_ran",
    "srt_selftest_noise_meter",
    "srt_cast_rays", "srt_cast_rays_device", "srt_pick", "srt_group_cast_rays", "srt_group_pick", "srt_last_ray_query_ms",
    "srt_ray_query_sizes",
    "srt_occluded_rays", "srt_occluded_rays_device", "srt_occluded_segments", "srt_segment_rays", "srt_group_occluded_rays",
    "srt_group_occluded_segments", "srt_group_segment_rays", "srt_occlusion_sizes",
    "srt_selection_defaults", "srt_selection_check_host", "srt_selection_sizes", "srt_selection_alpha_table_host", "srt_set_selection",
    "srt_group_set_selection", "srt_render_ids", "srt_read_id_pass", "srt_group_read_id_pass", "srt_read_selection_alpha",
    "srt_last_resolve_selected", "srt_group_last_resolve_selected",
    "srt_ao_defaults", "srt_ao_check_host", "srt_ao_sizes", "srt_ao_table_host", "srt_render_ao", "srt_read_ao", "srt_ao_rays",
    "srt_resolve_ao_view", "srt_group_render_ao", "srt_group_read_ao", "srt_group_ao_rays", "srt_group_resolve_ao_view",
    "srt_group_read_ao_view",
    "srt_nearest_points", "srt_nearest_points_device", "srt_group_nearest_points", "srt_nearest_triangle_host", "srt_nearest_sphere_host",
    "srt_nearest_plane_host", "srt_nearest_sizes",
    "srt_area_sizes", "srt_area_check_host", "srt_area_mask_host", "srt_area_coverage", "srt_area_triangle_coverage",
    "srt_area_coverage_device", "srt_select_area", "srt_read_selection", "srt_group_area_coverage", "srt_group_area_triangle_coverage",
    "srt_group_select_area", "srt_group_read_selection", "srt_last_area_ms", "srt_last_area_id_pass",
    "srt_cast_rays_multi", "srt_cast_rays_multi_device", "srt_pick_through", "srt_group_cast_rays_multi", "srt_group_pick_through",
    "srt_multi_hit_check_host", "srt_multi_hit_sizes",
    "srt_area_coverage_through", "srt_area_triangle_coverage_through", "srt_area_coverage_through_device", "srt_select_area_through",
    "srt_group_area_coverage_through", "srt_group_area_triangle_coverage_through", "srt_group_select_area_through", "srt_pick_rays", "srt_group_pick_rays",
]

ACCEL_NONE, ACCEL_BVH = 0, 1
REFIT_HOST, REFIT_DEVICE = 0, 1
DEFORM_REBUILD, DEFORM_REFIT = 0, 1
BUILD_HOST, BUILD_DEVICE = 0, 1
BUILD_ORDER_MORTON, BUILD_ORDER_MEDIAN = 0, 1
BUILD_LOCAL = 1024  # csrc/device_types.h SRT_BUILD_LOCAL: the largest range the median order's local launch takes
MOTION_STATIC, MOTION_MOVED, MOTION_NO_HISTORY, MOTION_DEFORMED = 0, 1, 2, 3
MOTION_WORDS = 22
NO_SHAPE = 0xFFFFFFFF
FILTER_LINEAR, FILTER_NEAREST = 0, 1
MAX_TEXTURES = 64


class TextureDesc(C.Structure):
    """srt_texture_desc"""
    _fields_ = [("rgba", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


def _texture_descs(images):
    """images: (H, W, 4) float32 arrays, row 0 = bottom -> (the contiguous arrays to keep alive, a TextureDesc array)."""
    keep = [np.ascontiguousarray(im, np.float32) for im in images]
    for im in keep:
        assert im.ndim == 3 and im.shape[2] == 4
    descs = (TextureDesc * max(len(keep), 1))()
    for k, im in enumerate(keep):
        descs[k].rgba, descs[k].width, descs[k].height = im.ctypes.data, im.shape[1], im.shape[0]
    return keep, descs


def _uv_array(uv):
    if uv is None:
        return None, 0
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 3, 2)
    return uv, len(uv)


def _tm_array(tm):
    if tm is None:
        return None
    tm = np.ascontiguousarray(tm, np.int32).reshape(-1)
    return tm if len(tm) else None


def triangle_materials_check_host(materials, scene_triangles, n_materials):
    """srt_triangle_materials_check_host (host only): the return code for a table (None: no table) meeting a scene."""
    lib = load_library()
    tm = None if materials is None else np.ascontiguousarray(materials, np.int32).reshape(-1)
    return lib.srt_triangle_materials_check_host(_ptr(tm) if tm is not None else None, 0 if tm is None else len(tm), int(scene_triangles), int(n_materials))


def plane_frame_host(normal):
    """srt_plane_frame_host (host only): (T, B) float32 (3,) each, or None for a plane without a frame."""
    lib = load_library()
    n = np.ascontiguousarray(normal, np.float32).reshape(3)
    T, B = np.zeros(3, np.float32), np.zeros(3, np.float32)
    return (T, B) if lib.srt_plane_frame_host(_ptr(n), _ptr(T), _ptr(B)) else None


def plane_axis_code_host(normal, position=(0.0, 0.0, 0.0)):
    """srt_plane_axis_code_host (host only): 1, 2, 3 for a plane srt_update_scene takes for an axis plane (normal +-e_x, +-e_y,
    +-e_z exactly, position at most 2^100 in every component), else 0."""
    n = np.ascontiguousarray(normal, np.float32).reshape(3)
    q = np.ascontiguousarray(position, np.float32).reshape(3)
    out = C.c_int(-1)
    if load_library().srt_plane_axis_code_host(_ptr(n), _ptr(q), C.byref(out)):
        raise SrtError("srt_plane_axis_code_host failed")
    return int(out.value)


def bernoulli_threshold_host(p):
    """srt_bernoulli_threshold_host (host only): the integer T in [0, 2^32] that srt_update_scene makes of a material
    probability p (a float32): the kernel's draw `r < T` is `p > float32(r) * 2^-32` for every generator output r."""
    out = C.c_uint64(0)
    if load_library().srt_bernoulli_threshold_host(C.c_float(float(np.float32(p))), C.byref(out)):
        raise SrtError("srt_bernoulli_threshold_host failed")
    return int(out.value)


def texture_check_host(n_textures, bindings=None, uv_triangles=None, scene_triangles=0, images=None):
    """srt_texture_check_host (host only): the setters' checks; returns the status (0 = SRT_OK, 1 = SRT_ERR_INVALID).
    images: (rgba pointer or None, width, height) triples, checked as srt_set_textures checks its descriptors."""
    lib = load_library()
    descs, keep = None, None
    if images is not None:
        keep = np.zeros(4, np.float32)
        descs = (TextureDesc * max(len(images), 1))()
        for k, (has_texels, w, h) in enumerate(images):
            descs[k].rgba, descs[k].width, descs[k].height = (keep.ctypes.data if has_texels else None), w, h
    b = R.as_records(bindings if bindings is not None else [], R.MATERIAL_TEXTURE)
    return lib.srt_texture_check_host(descs, n_textures, _ptr(b) if len(b) else None, len(b),
                                      -1 if uv_triangles is None else int(uv_triangles), scene_triangles)


def _motion_rows(table):
    """(n, 22) uint32 rows -> dict state (n,) int, A (n, 3, 4), B (n, 3, 3) float32."""
    table = np.ascontiguousarray(table, np.uint32).reshape(-1, MOTION_WORDS)
    f = table[:, 1:].copy().view(np.float32)
    return {"state": table[:, 0].astype(np.int64), "A": f[:, :12].reshape(-1, 3, 4), "B": f[:, 12:].reshape(-1, 3, 3)}


def motion_table_host(history, current, deform=False):
    """srt_motion_table_host (host only, no GPU needed). history / current: (shapes, triangles, materials, scene_data) of
    the two scenes. None when the history would be dropped, else dict state (n,), A (n, 3, 4) current world -> history
    world, B (n, 3, 3) current normal -> history normal. deform: srt_motion_table_deform_host, the keep rule of per-triangle
    motion; the dict then also holds first_row (n,) = word 1 of each row (a DEFORMED shape's first row in the vertex
    tables)."""
    lib = load_library()
    args, keep = [], []
    for shapes, triangles, materials, sd in (history, current):
        recs = [R.as_records(shapes, R.SHAPE), R.as_records(triangles, R.TRIANGLE), R.as_records(materials, R.MATERIAL)]
        sd = R.as_records(sd, R.SCENE_DATA)
        keep += recs + [sd]
        for r in recs:
            args += [_ptr(r) if len(r) else None, len(r)]
        args.append(_ptr(sd))
    n = len(keep[4])
    table = np.zeros((max(n, 1), MOTION_WORDS), np.uint32)
    kept = C.c_int(0)
    fn = lib.srt_motion_table_deform_host if deform else lib.srt_motion_table_host
    rc = fn(*args, _ptr(table), C.byref(kept))
    if rc:
        raise SrtError(f"srt_motion_table_host failed ({rc})")
    if not kept.value:
        return None
    out = _motion_rows(table[:n])
    if deform:
        out["first_row"] = table[:n, 1].astype(np.int64)
    return out


BVH_NODE = np.dtype({"names": ["lo", "skip", "hi", "leaf"], "formats": [(np.float32, (3,)), np.uint32, (np.float32, (3,)), np.uint32],
                     "offsets": [0, 12, 16, 28], "itemsize": 32})
BVH_END = 0xFFFFFFFF


def bvh_build_host(model_shape, triangles):
    """(nodes, order) of the BVH the library builds for one model shape record. Host only: no GPU needed."""
    lib = load_library()
    shape = np.zeros(1, R.SHAPE)
    shape[0] = model_shape
    tris = R.as_records(triangles, R.TRIANGLE)
    n = C.c_size_t(0)
    rc = lib.srt_bvh_build_host(_ptr(shape), _ptr(tris), len(tris), None, 0, None, 0, C.byref(n))
    if rc:
        raise SrtError(f"srt_bvh_build_host failed ({rc})")
    nodes = np.zeros(n.value, BVH_NODE)
    order = np.zeros(int(shape[0]["num_triangles"]), np.uint32)
    rc = lib.srt_bvh_build_host(_ptr(shape), _ptr(tris), len(tris), _ptr(nodes), len(nodes), _ptr(order), len(order), C.byref(n))
    if rc:
        raise SrtError(f"srt_bvh_build_host failed ({rc})")
    return nodes, order


BVH_NONE = 0xFFFFFFFF
BVH_LEAF_BIT = 0x80000000
BVH_INDEX_MASK = 0x0FFFFFFF
BVH_STACK_CAP = 64


def bvh_wide_host(model_shape, triangles, force_balanced=False):
    """The four-wide hierarchy the kernel walks for one model shape record (csrc/device_types.h): dict with
    blocks (n x 32 uint32; an inner block: origin, grid exponents + count, boxes as bytes, tags, first), dest (per record:
    leaf block << 2 | slot), root, stack_need, balanced. Host only: no GPU needed; leaf blocks come back empty (the device
    writes the triangles)."""
    lib = load_library()
    lib.srt_bvh_wide_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    shape = np.zeros(1, R.SHAPE)
    shape[0] = model_shape
    tris = R.as_records(triangles, R.TRIANGLE)
    n, root, need, bal = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    flags = int(bool(force_balanced))
    rc = lib.srt_bvh_wide_host(_ptr(shape), _ptr(tris), len(tris), flags, None, 0, None, 0, C.byref(n), None, None, None)
    if rc:
        raise SrtError(f"srt_bvh_wide_host failed ({rc})")
    blocks = np.zeros((n.value, 32), np.uint32)
    dest = np.zeros(int(shape[0]["num_triangles"]), np.uint32)
    rc = lib.srt_bvh_wide_host(_ptr(shape), _ptr(tris), len(tris), flags, _ptr(blocks), len(blocks), _ptr(dest), len(dest),
                               C.byref(n), C.byref(root), C.byref(need), C.byref(bal))
    if rc:
        raise SrtError(f"srt_bvh_wide_host failed ({rc})")
    return {"blocks": blocks, "dest": dest, "root": root.value, "stack_need": need.value, "balanced": bool(bal.value)}


def bvh_wide_order_host(model_shape, triangles, force_balanced=False):
    """srt_bvh_wide_order_host (host only): order[record] = triangle inside the model, of the hierarchy bvh_wide_host gives
    for the same arguments."""
    shape = np.zeros(1, R.SHAPE)
    shape[0] = model_shape
    tris = R.as_records(triangles, R.TRIANGLE)
    order = np.zeros(int(shape[0]["num_triangles"]), np.uint32)
    rc = load_library().srt_bvh_wide_order_host(_ptr(shape), _ptr(tris), len(tris), int(bool(force_balanced)), _ptr(order), len(order))
    if rc:
        raise SrtError(f"srt_bvh_wide_order_host failed ({rc})")
    return order


def bvh_refit_wide_host(built_shape, moved_shape, triangles, force_balanced=False):
    """srt_bvh_refit_wide_host (host only): the wide hierarchy of built_shape (bvh_wide_host's) refitted in place for
    moved_shape, which may differ in its transform only: dict with blocks (n x 32 uint32, relative to the model, leaf
    blocks zero) and root. What REFIT_DEVICE computes on the device."""
    lib = load_library()
    shapes = np.zeros(2, R.SHAPE)
    shapes[0], shapes[1] = built_shape, moved_shape
    tris = R.as_records(triangles, R.TRIANGLE)
    n, root = C.c_size_t(0), C.c_uint32(0)
    flags = int(bool(force_balanced))
    args = (_ptr(shapes[0:1]), _ptr(shapes[1:2]), _ptr(tris), len(tris), flags)
    rc = lib.srt_bvh_refit_wide_host(*args, None, 0, C.byref(n), None)
    if rc:
        raise SrtError(f"srt_bvh_refit_wide_host failed ({rc})")
    blocks = np.zeros((n.value, 32), np.uint32)
    rc = lib.srt_bvh_refit_wide_host(*args, _ptr(blocks), len(blocks), C.byref(n), C.byref(root))
    if rc:
        raise SrtError(f"srt_bvh_refit_wide_host failed ({rc})")
    return {"blocks": blocks, "root": root.value}


def _deformed_args(built_shape, built_triangles, now_shape, now_triangles, force_balanced):
    shapes = np.zeros(2, R.SHAPE)
    shapes[0], shapes[1] = built_shape, now_shape
    bt, nt = R.as_records(built_triangles, R.TRIANGLE), R.as_records(now_triangles, R.TRIANGLE)
    if len(bt) != len(nt):
        raise SrtError("the two triangle arrays differ in length")
    return (shapes, bt, nt), (_ptr(shapes[0:1]), _ptr(bt), _ptr(shapes[1:2]), _ptr(nt), len(bt), int(bool(force_balanced)))


def bvh_refit_deformed_wide_host(built_shape, built_triangles, now_shape, now_triangles, force_balanced=False):
    """srt_bvh_refit_deformed_wide_host (host only): bvh_refit_wide_host for a model whose triangles changed too -- the
    hierarchy of built_shape over built_triangles refitted in place around now_shape over now_triangles: dict with blocks
    and root. What DEFORM_REFIT with REFIT_DEVICE leaves on the device."""
    lib = load_library()
    keep, args = _deformed_args(built_shape, built_triangles, now_shape, now_triangles, force_balanced)
    n, root = C.c_size_t(0), C.c_uint32(0)
    rc = lib.srt_bvh_refit_deformed_wide_host(*args, None, 0, C.byref(n), None)
    if rc:
        raise SrtError(f"srt_bvh_refit_deformed_wide_host failed ({rc})")
    blocks = np.zeros((n.value, 32), np.uint32)
    rc = lib.srt_bvh_refit_deformed_wide_host(*args, _ptr(blocks), len(blocks), C.byref(n), C.byref(root))
    if rc:
        raise SrtError(f"srt_bvh_refit_deformed_wide_host failed ({rc})")
    return {"blocks": blocks, "root": root.value}


def bvh_wide_cost_host(built_shape, built_triangles, now_shape, now_triangles, force_balanced=False):
    """srt_bvh_wide_cost_host (host only): (cost_built, cost_now), the surface-area cost of that hierarchy as built and as
    refitted in place; 0.0 = unknown."""
    lib = load_library()
    keep, args = _deformed_args(built_shape, built_triangles, now_shape, now_triangles, force_balanced)
    built, now = C.c_double(0), C.c_double(0)
    rc = lib.srt_bvh_wide_cost_host(*args, C.byref(built), C.byref(now))
    if rc:
        raise SrtError(f"srt_bvh_wide_cost_host failed ({rc})")
    return built.value, now.value


def bvh_morton_order_host(model_shape, triangles, _call="srt_bvh_morton_order_host"):
    """srt_bvh_morton_order_host (host only): order[record] = triangle inside the model, by ascending (Morton code, index):
    what BUILD_DEVICE sorts on the device."""
    lib = load_library()
    shape = np.zeros(1, R.SHAPE)
    shape[0] = model_shape
    tris = R.as_records(triangles, R.TRIANGLE)
    order = np.zeros(int(shape[0]["num_triangles"]), np.uint32)
    rc = getattr(lib, _call)(_ptr(shape), _ptr(tris), len(tris), _ptr(order), len(order))
    if rc:
        raise SrtError(f"{_call} failed ({rc})")
    return order


def bvh_median_order_host(model_shape, triangles):
    """srt_bvh_median_order_host (host only): order[record] = triangle inside the model in the median-split order: what
    BUILD_DEVICE computes on the device under BUILD_ORDER_MEDIAN."""
    return bvh_morton_order_host(model_shape, triangles, _call="srt_bvh_median_order_host")


def bvh_morton_wide_host(model_shape, triangles, _call="srt_bvh_morton_wide_host"):
    """srt_bvh_morton_wide_host (host only): the hierarchy BUILD_DEVICE leaves on the device -- the balanced topology of the
    model's count over the Morton order, boxes of the in-place refit: dict with blocks (relative to the model, leaf blocks
    zero), dest, root, stack_need and cost (0.0: unknown)."""
    lib = load_library()
    shape = np.zeros(1, R.SHAPE)
    shape[0] = model_shape
    tris = R.as_records(triangles, R.TRIANGLE)
    n, root, need, cost = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0)
    call = getattr(lib, _call)
    rc = call(_ptr(shape), _ptr(tris), len(tris), None, 0, None, 0, C.byref(n), None, None, None)
    if rc:
        raise SrtError(f"{_call} failed ({rc})")
    blocks = np.zeros((n.value, 32), np.uint32)
    dest = np.zeros(int(shape[0]["num_triangles"]), np.uint32)
    rc = call(_ptr(shape), _ptr(tris), len(tris), _ptr(blocks), len(blocks), _ptr(dest), len(dest), C.byref(n), C.byref(root), C.byref(need), C.byref(cost))
    if rc:
        raise SrtError(f"{_call} failed ({rc})")
    return {"blocks": blocks, "dest": dest, "root": root.value, "stack_need": need.value, "cost": cost.value}


def bvh_median_wide_host(model_shape, triangles):
    """srt_bvh_median_wide_host (host only): bvh_morton_wide_host for BUILD_ORDER_MEDIAN -- the same topology over the
    median-split order."""
    return bvh_morton_wide_host(model_shape, triangles, _call="srt_bvh_median_wide_host")


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("paths", "rays", "sky", "tri_tests", "tri_pass_u", "nan_pixels", "watchdog")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DenoiseParams(C.Structure):
    """include/srt_types.h srt_denoise_params"""
    _fields_ = [("enable", C.c_int32), ("iterations", C.c_int32), ("feature_samples", C.c_int32), ("sigma_luminance", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(DenoiseParams) == 32


class TemporalParams(C.Structure):
    """include/srt_types.h srt_temporal_params"""
    _fields_ = [("enable", C.c_int32), ("history_limit", C.c_int32), ("normal_threshold", C.c_float), ("depth_threshold", C.c_float),
                ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "reserved" else getattr(self, n)) for n, _ in self._fields_}


assert C.sizeof(TemporalParams) == 32


EXPOSURE_MANUAL, EXPOSURE_AUTO = 0, 1


class ExposureParams(C.Structure):
    """include/srt_types.h srt_exposure_params"""
    _fields_ = [("enable", C.c_int32), ("mode", C.c_int32), ("ev", C.c_float), ("key", C.c_float), ("low_permille", C.c_int32),
                ("high_permille", C.c_int32), ("adapt", C.c_float), ("min_ev", C.c_float), ("max_ev", C.c_float), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "reserved" else getattr(self, n)) for n, _ in self._fields_}


assert C.sizeof(ExposureParams) == 48


def _exposure_params(kw, who):
    """srt_exposure_defaults() overridden by kw; mode may be "manual" / "auto"."""
    d = ExposureParams()
    if load_library().srt_exposure_defaults(C.byref(d)):
        raise SrtError("srt_exposure_defaults failed")
    for k, v in kw.items():
        if k not in d.as_dict():
            raise TypeError(f"{who}: unknown parameter {k}")
        if k == "mode" and isinstance(v, str):
            v = {"manual": EXPOSURE_MANUAL, "auto": EXPOSURE_AUTO}[v]
        if k == "reserved":
            v = (C.c_int32 * 3)(*v)
        setattr(d, k, v)
    return d


def exposure_defaults():
    """srt_exposure_defaults (host only, no GPU needed) as a dict."""
    return _exposure_params({}, "exposure_defaults").as_dict()


def exposure_check_host(**kw):
    """srt_exposure_check_host of the defaults overridden by kw (host only): True when srt_set_exposure would accept them."""
    return load_library().srt_exposure_check_host(C.byref(_exposure_params(kw, "exposure_check_host"))) == 0


BLOOM_MAX_LEVELS = 8


class BloomParams(C.Structure):
    """include/srt_types.h srt_bloom_params"""
    _fields_ = [("enable", C.c_int32), ("threshold", C.c_float), ("knee", C.c_float), ("intensity", C.c_float), ("scatter", C.c_float),
                ("clamp", C.c_float), ("levels", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(BloomParams) == 32


def _bloom_params(kw, who):
    """srt_bloom_defaults() overridden by kw."""
    d = BloomParams()
    if load_library().srt_bloom_defaults(C.byref(d)):
        raise SrtError("srt_bloom_defaults failed")
    for k, v in kw.items():
        if k not in d.as_dict():
            raise TypeError(f"{who}: unknown parameter {k}")
        setattr(d, k, v)
    return d


def bloom_defaults():
    """srt_bloom_defaults (host only, no GPU needed) as a dict."""
    return _bloom_params({}, "bloom_defaults").as_dict()


def bloom_check_host(**kw):
    """srt_bloom_check_host of the defaults overridden by kw (host only): True when srt_set_bloom would accept them."""
    return load_library().srt_bloom_check_host(C.byref(_bloom_params(kw, "bloom_check_host"))) == 0


def _selection_params(kw, who):
    """srt_selection_defaults() overridden by kw -> a records.SELECTION_PARAMS record. width: outline_width; outline / fill: (A, R, G, B)."""
    d = np.zeros((), R.SELECTION_PARAMS)
    if load_library().srt_selection_defaults(_ptr(d)):
        raise SrtError("srt_selection_defaults failed")
    for k, v in kw.items():
        k = {"width": "outline_width", "outline": "outline_argb", "fill": "fill_argb"}.get(k, k)
        if k not in R.SELECTION_PARAMS.names:
            raise TypeError(f"{who}: unknown parameter {k}")
        d[k] = v
    return d


def selection_defaults():
    """srt_selection_defaults (host only, no GPU needed) as a records.SELECTION_PARAMS record."""
    return _selection_params({}, "selection_defaults")


def selection_check_host(**kw):
    """srt_selection_check_host of the defaults overridden by kw (host only): True when srt_set_selection would accept them."""
    return load_library().srt_selection_check_host(_ptr(_selection_params(kw, "selection_check_host"))) == 0


def selection_alpha_table_host(**kw):
    """srt_selection_alpha_table_host of the defaults overridden by kw (host only) -> (table of 2 R^2 + 1 uint8, R)."""
    table, radius = np.zeros(R.SELECTION_TABLE_MAX, np.uint8), C.c_int(0)
    if load_library().srt_selection_alpha_table_host(_ptr(_selection_params(kw, "selection_alpha_table_host")), _ptr(table), table.size, C.byref(radius)):
        raise SrtError("srt_selection_alpha_table_host refused the parameters")
    return table[:2 * radius.value ** 2 + 1].copy(), radius.value


def area_record(rect, lasso=None):
    """(records.AREA record, (n, 2) int32 vertex array or None) of rect = (x0, y0, x1, y1) and an optional lasso: n pixel-corner
    vertices (x, y). Nothing is checked here: the library does that."""
    a = np.zeros((), R.AREA)
    a["x0"], a["y0"], a["x1"], a["y1"] = (int(v) for v in rect)
    if lasso is None or len(lasso) == 0:
        return a, None
    v = np.ascontiguousarray(np.asarray(lasso, np.int64).reshape(-1, 2).astype(np.int32))
    a["n_vertices"] = len(v)
    return a, v


def area_check_host(rect, lasso=None, **fields):
    """srt_area_check_host (host only): True when the coverage calls would accept the area. fields: overrides of the record's
    fields (flags, reserved, n_vertices), for the tests."""
    a, v = area_record(rect, lasso)
    for k, val in fields.items():
        a[k] = val
    return load_library().srt_area_check_host(_ptr(a), _ptr(v) if v is not None else None) == 0


def area_mask(rect, lasso=None, width=0, height=0):
    """srt_area_mask_host (host only): M(p) of a width x height frame -> (height, width) bool, the rule the device counts by."""
    a, v = area_record(rect, lasso)
    mask = np.zeros((max(height, 0), max(width, 0)), np.uint8)
    if load_library().srt_area_mask_host(_ptr(a), _ptr(v) if v is not None else None, width, height, _ptr(mask) if mask.size else None, mask.size):
        raise SrtError("srt_area_mask_host refused the area or the frame")
    return mask.astype(bool)


def _ao_params(kw, who):
    """srt_ao_defaults() overridden by kw (samples, radius, bias, seed, background = 0xAARRGGBB) -> a records.AO_PARAMS record."""
    d = np.zeros((), R.AO_PARAMS)
    if load_library().srt_ao_defaults(_ptr(d)):
        raise SrtError("srt_ao_defaults failed")
    for k, v in kw.items():
        if k not in R.AO_PARAMS.names:
            raise TypeError(f"{who}: unknown parameter {k}")
        d[k] = v
    return d


def ao_defaults():
    """srt_ao_defaults (host only, no GPU needed) as a records.AO_PARAMS record."""
    return _ao_params({}, "ao_defaults")


def ao_check_host(width, height, **kw):
    """srt_ao_check_host of the defaults overridden by kw for a frame of width x height (host only): True when srt_render_ao
    would accept them."""
    return load_library().srt_ao_check_host(_ptr(_ao_params(kw, "ao_check_host")), int(width), int(height)) == 0


def ao_table(**kw):
    """srt_ao_table_host of the defaults overridden by kw (host only) -> the samples + 1 grey levels of the view, uint8."""
    p, table = _ao_params(kw, "ao_table"), np.zeros(R.AO_MAX_SAMPLES + 1, np.uint8)
    if load_library().srt_ao_table_host(_ptr(p), _ptr(table)):
        raise SrtError("srt_ao_table_host refused the parameters")
    return table[:int(p["samples"]) + 1].copy()


class NoiseParams(C.Structure):
    """include/srt_types.h srt_noise_params"""
    _fields_ = [("enable", C.c_int32), ("threshold", C.c_float), ("luminance_floor", C.c_float), ("permille", C.c_int32),
                ("min_samples", C.c_uint32), ("check_every", C.c_int32), ("reserved", C.c_int32 * 2)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n == "reserved" else getattr(self, n)) for n, _ in self._fields_}


class NoiseResult(C.Structure):
    """include/srt_types.h srt_noise_result"""
    _fields_ = [("metered", C.c_uint32), ("left_out", C.c_uint32), ("below", C.c_uint32), ("converged", C.c_int32),
                ("dispatches", C.c_uint32), ("samples", C.c_uint32), ("level_bin", C.c_int32), ("level", C.c_float)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["level"] = np.float32(d["level"])
        return d


assert C.sizeof(NoiseParams) == 32 and C.sizeof(NoiseResult) == 32


def _noise_params(kw, who):
    """srt_noise_defaults() overridden by kw."""
    d = NoiseParams()
    if load_library().srt_noise_defaults(C.byref(d)):
        raise SrtError("srt_noise_defaults failed")
    for k, v in kw.items():
        if k not in d.as_dict():
            raise TypeError(f"{who}: unknown parameter {k}")
        if k == "reserved":
            v = (C.c_int32 * 2)(*v)
        setattr(d, k, v)
    return d


def noise_defaults():
    """srt_noise_defaults (host only, no GPU needed) as a dict."""
    return _noise_params({}, "noise_defaults").as_dict()


def noise_check_host(**kw):
    """srt_noise_check_host of the defaults overridden by kw (host only): True when srt_set_noise_meter would accept them."""
    return load_library().srt_noise_check_host(C.byref(_noise_params(kw, "noise_check_host"))) == 0


def noise_evaluate_host(hist, counts, T, P, **kw):
    """srt_noise_evaluate_host (host only): the result dict of a record hist (256), counts (metered, left_out, below) metered
    at T dispatches and P samples under the defaults overridden by kw."""
    hist = np.ascontiguousarray(hist, np.uint32).reshape(256)
    c = (C.c_uint32 * 3)(*[int(v) for v in counts])
    out = NoiseResult()
    if load_library().srt_noise_evaluate_host(hist.ctypes.data_as(C.POINTER(C.c_uint32)), c, int(T), int(P),
                                              C.byref(_noise_params(kw, "noise_evaluate_host")), C.byref(out)):
        raise SrtError("srt_noise_evaluate_host: bad arguments")
    return out.as_dict()


def temporal_defaults():
    """srt_temporal_defaults (host only, no GPU needed) as a dict."""
    d = TemporalParams()
    if load_library().srt_temporal_defaults(C.byref(d)):
        raise SrtError("srt_temporal_defaults failed")
    return d.as_dict()


def denoise_defaults():
    """srt_denoise_defaults (host only, no GPU needed) as a dict."""
    d = DenoiseParams()
    if load_library().srt_denoise_defaults(C.byref(d)):
        raise SrtError("srt_denoise_defaults failed")
    return d.as_dict()


class SrtError(RuntimeError):
    """Raised where the reference would throw a boost::compute exception."""


_lib = None


def load_library():
    """dlopen lib/libsrt_hip.so. Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SrtError(f"{LIB_PATH} not built: run `python __graft_entry__.py` / simple-raytracer_amd/build.py (needs hipcc)")
    _lib = _bind(C.CDLL(str(LIB_PATH)))
    return _lib


_variants = {}


def load_dev_library():
    """The -DSRT_DEV_KNOBS build (lib/variants/dev/, build.py build_dev()): the same library, which additionally reads the
    development knobs SRT_WAVES_PER_CU / SRT_SCAN_PAIRS / SRT_JOB_CAP_SUBS / SRT_POOL_BLOCKS / SRT_NO_SCAN_POOL from the
    environment. Tests that force rare paths pass it to Tracer(lib=...); the product library ignores those variables."""
    path = B.DEV_LIB
    if str(path) not in _variants:
        if not path.exists():
            raise SrtError(f"{path} not built: simple_raytracer_amd.build.build_dev()")
        lib = _bind(C.CDLL(str(path)))
        assert b"dev knobs" in lib.srt_version(), lib.srt_version()
        _variants[str(path)] = lib
    return _variants[str(path)]


def _bind(lib):
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.srt_create.argtypes = [i, i, i, C.POINTER(vp)]
    lib.srt_destroy.argtypes = [vp]
    lib.srt_destroy.restype = None
    lib.srt_last_error.argtypes = [vp]
    lib.srt_last_error.restype = C.c_char_p
    lib.srt_set_skybox.argtypes = [vp, vp, i, i]
    lib.srt_update_scene.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
    lib.srt_clear_canvas.argtypes = [vp]
    lib.srt_render.argtypes = [vp, vp, C.c_uint32, vp]
    lib.srt_trace.argtypes = [vp, vp]
    if hasattr(lib, "srt_render_async"):
        lib.srt_render_async.argtypes = [vp, vp, C.c_uint32, vp]
    lib.srt_resolve.argtypes = [vp, C.c_uint32]
    if hasattr(lib, "srt_set_radiance_budget"):
        lib.srt_set_radiance_budget.argtypes = [vp, sz]
    lib.srt_synchronize.argtypes = [vp]
    lib.srt_resolve_external.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp]
    lib.srt_read_canvas.argtypes = [vp, vp]
    lib.srt_read_argb.argtypes = [vp, vp]
    lib.srt_get_counters.argtypes = [vp, C.POINTER(Counters)]
    lib.srt_set_count_triangles.argtypes = [vp, i]
    lib.srt_reset_counters.argtypes = [vp]
    lib.srt_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    if hasattr(lib, "srt_set_kernel_timers"):
        lib.srt_set_kernel_timers.argtypes = [vp, i]
    if hasattr(lib, "srt_last_trace_kernel_ms"):
        lib.srt_last_trace_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.srt_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
    lib.srt_bind_canvas.argtypes = [vp, vp, sz]
    lib.srt_bind_stream.argtypes = [vp, vp]
    lib.srt_set_partition.argtypes = [vp, i, i, i]
    lib.srt_partition_owned_rows.argtypes = [i, i, i, i]
    lib.srt_partition_padded_rows.argtypes = [i, i, i]
    lib.srt_partition_global_row.argtypes = [i, i, i, i, i]
    lib.srt_partition_unpermute.argtypes = [vp, vp, i, i, i, sz]
    if hasattr(lib, "srt_selftest_math"):  # absent only in older A/B builds selected through SRT_LIB
        lib.srt_selftest_math.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64)]
    if hasattr(lib, "srt_selftest_rare_lanes"):  # (the same)
        lib.srt_selftest_rare_lanes.argtypes = [vp, i, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.srt_version.restype = C.c_char_p
    if hasattr(lib, "srt_set_acceleration"):
        lib.srt_set_acceleration.argtypes = [vp, i]
        lib.srt_acceleration_info.argtypes = [vp, C.POINTER(C.c_uint64)]
        lib.srt_bvh_build_host.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.POINTER(sz)]
    if hasattr(lib, "srt_set_acceleration_refit"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_bvh_refit_wide_host.argtypes = [vp, vp, vp, sz, i, vp, sz, C.POINTER(sz), C.POINTER(C.c_uint32)]
        lib.srt_bvh_wide_order_host.argtypes = [vp, vp, sz, i, vp, sz]
        lib.srt_set_acceleration_refit.argtypes = [vp, i]
        lib.srt_group_set_acceleration_refit.argtypes = [vp, i]
        lib.srt_acceleration_refit_info.argtypes = [vp, C.POINTER(C.c_uint64)]
        lib.srt_last_refit_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    if hasattr(lib, "srt_set_acceleration_deform"):  # (likewise)
        lib.srt_set_acceleration_deform.argtypes = [vp, i, C.c_float]
        lib.srt_group_set_acceleration_deform.argtypes = [vp, i, C.c_float]
        lib.srt_acceleration_deform_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        lib.srt_bvh_refit_deformed_wide_host.argtypes = [vp, vp, vp, vp, sz, i, vp, sz, C.POINTER(sz), C.POINTER(C.c_uint32)]
        lib.srt_bvh_wide_cost_host.argtypes = [vp, vp, vp, vp, sz, i, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(lib, "srt_set_acceleration_build"):  # (likewise)
        lib.srt_set_acceleration_build.argtypes = [vp, i, C.c_uint32]
        lib.srt_group_set_acceleration_build.argtypes = [vp, i, C.c_uint32]
        lib.srt_acceleration_build_info.argtypes = [vp, C.POINTER(C.c_uint64)]
        lib.srt_last_build_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.srt_bvh_morton_order_host.argtypes = [vp, vp, sz, vp, sz]
        lib.srt_bvh_morton_wide_host.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        lib.srt_read_bvh_blocks.argtypes = [vp, vp, sz, C.POINTER(sz)]
    if hasattr(lib, "srt_set_acceleration_build_order"):  # (likewise)
        lib.srt_set_acceleration_build_order.argtypes = [vp, i]
        lib.srt_group_set_acceleration_build_order.argtypes = [vp, i]
        lib.srt_bvh_median_order_host.argtypes = lib.srt_bvh_morton_order_host.argtypes
        lib.srt_bvh_median_wide_host.argtypes = lib.srt_bvh_morton_wide_host.argtypes
    if hasattr(lib, "srt_gather"):
        lib.srt_comm_unique_id.argtypes = [vp]
        lib.srt_comm_init.argtypes = [vp, vp, i, i]
        lib.srt_gather.argtypes = [vp, i]
        lib.srt_resolve_gathered.argtypes = [vp, C.c_uint32]
        lib.srt_gathered_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        lib.srt_read_gathered.argtypes = [vp, vp, vp]
        lib.srt_group_create.argtypes = [i, i, i, vp, i, C.POINTER(vp)]
        lib.srt_group_destroy.argtypes = [vp]
        lib.srt_group_destroy.restype = None
        lib.srt_group_last_error.argtypes = [vp]
        lib.srt_group_last_error.restype = C.c_char_p
        lib.srt_group_size.argtypes = [vp]
        lib.srt_group_tracer.argtypes = [vp, i]
        lib.srt_group_tracer.restype = vp
        lib.srt_group_set_skybox.argtypes = [vp, vp, i, i]
        lib.srt_group_set_acceleration.argtypes = [vp, i]
        lib.srt_group_update_scene.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp]
        lib.srt_group_clear_canvas.argtypes = [vp]
        lib.srt_group_trace_and_gather.argtypes = [vp, vp]
        lib.srt_group_render.argtypes = [vp, vp, C.c_uint32, vp]
        lib.srt_group_read_canvas.argtypes = [vp, vp]
        lib.srt_group_get_counters.argtypes = [vp, C.POINTER(Counters)]
        if hasattr(lib, "srt_group_set_denoise"):  # (an older library, SRT_LIB, in an A/B run)
            lib.srt_group_set_denoise.argtypes = [vp, C.POINTER(DenoiseParams)]
            lib.srt_group_set_denoise_temporal.argtypes = [vp, C.POINTER(TemporalParams)]
            lib.srt_group_reset_denoise_history.argtypes = [vp]
            lib.srt_group_resolve_denoised.argtypes = [vp, C.c_uint32]
            lib.srt_group_read_denoised.argtypes = [vp, vp]
            lib.srt_group_read_denoise_inputs.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_uint32)]
            lib.srt_group_read_denoise_history.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
            lib.srt_partition_planes_floats.argtypes = [i, i, i, i]
            lib.srt_partition_planes_floats.restype = C.c_longlong
            lib.srt_unpermute_planes_device.argtypes = [vp, vp, vp, vp, vp, i, i, i, i]
        lib.srt_render_pipelined.argtypes = [vp, vp, C.c_uint32, vp, C.POINTER(C.c_longlong)]
        lib.srt_pipeline_flush.argtypes = [vp, vp, C.POINTER(C.c_longlong)]
    if hasattr(lib, "srt_set_denoise"):
        lib.srt_denoise_defaults.argtypes = [C.POINTER(DenoiseParams)]
        lib.srt_set_denoise.argtypes = [vp, C.POINTER(DenoiseParams)]
        lib.srt_resolve_denoised.argtypes = [vp, C.c_uint32]
        lib.srt_read_denoised.argtypes = [vp, vp]
        lib.srt_read_denoise_inputs.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_uint32)]
    if hasattr(lib, "srt_set_denoise_temporal"):
        lib.srt_temporal_defaults.argtypes = [C.POINTER(TemporalParams)]
        lib.srt_set_denoise_temporal.argtypes = [vp, C.POINTER(TemporalParams)]
        lib.srt_reset_denoise_history.argtypes = [vp]
        lib.srt_read_denoise_history.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_set_denoise_object_motion"):
        lib.srt_set_denoise_object_motion.argtypes = [vp, C.c_int]
        lib.srt_read_denoise_shape_ids.argtypes = [vp, vp, vp]
        lib.srt_read_denoise_motion.argtypes = [vp, vp, sz, C.POINTER(sz), C.POINTER(C.c_int)]
        lib.srt_motion_table_host.argtypes = [vp, sz, vp, sz, vp, sz, vp] * 2 + [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_set_denoise_vertex_motion"):
        lib.srt_set_denoise_vertex_motion.argtypes = [vp, C.c_int]
        lib.srt_read_denoise_triangle_ids.argtypes = [vp, vp, vp]
        lib.srt_read_denoise_vertex_tables.argtypes = [vp, vp, vp, sz, C.POINTER(sz)]
        lib.srt_motion_table_deform_host.argtypes = [vp, sz, vp, sz, vp, sz, vp] * 2 + [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_set_denoise_demodulation"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_set_denoise_demodulation.argtypes = [vp, C.c_int]
        lib.srt_group_set_denoise_demodulation.argtypes = [vp, C.c_int]
        lib.srt_last_filter_demodulated.argtypes = [vp, C.POINTER(C.c_int)]
        lib.srt_group_last_filter_demodulated.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_set_denoise_spatial_variance"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_set_denoise_spatial_variance.argtypes = [vp, C.c_uint32]
        lib.srt_group_set_denoise_spatial_variance.argtypes = [vp, C.c_uint32]
        lib.srt_last_filter_spatial_variance.argtypes = [vp, C.POINTER(C.c_int)]
        lib.srt_group_last_filter_spatial_variance.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_set_denoise_history_illumination"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_set_denoise_history_illumination.argtypes = [vp, C.c_int]
        lib.srt_group_set_denoise_history_illumination.argtypes = [vp, C.c_int]
        lib.srt_last_setup_history_illumination.argtypes = [vp]
        lib.srt_group_last_setup_history_illumination.argtypes = [vp]
    if hasattr(lib, "srt_set_denoise_history_clamp"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_set_denoise_history_clamp.argtypes = [vp, C.c_float]
        lib.srt_group_set_denoise_history_clamp.argtypes = [vp, C.c_float]
        lib.srt_last_setup_history_clamp.argtypes = [vp]
        lib.srt_group_last_setup_history_clamp.argtypes = [vp]
        lib.srt_read_denoise_history_bounds.argtypes = [vp, vp, vp]
    if hasattr(lib, "srt_set_denoise_history_feedback"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_set_denoise_history_feedback.argtypes = [vp, C.c_int]
        lib.srt_group_set_denoise_history_feedback.argtypes = [vp, C.c_int]
        lib.srt_last_filter_history_feedback.argtypes = [vp]
        lib.srt_group_last_filter_history_feedback.argtypes = [vp]
    if hasattr(lib, "srt_set_textures"):
        lib.srt_set_textures.argtypes = [vp, vp, sz]
        lib.srt_set_material_textures.argtypes = [vp, vp, sz]
        lib.srt_set_triangle_uvs.argtypes = [vp, vp, sz]
        lib.srt_last_trace_textured.argtypes = [vp, C.POINTER(C.c_int)]
        lib.srt_plane_frame_host.argtypes = [vp, vp, vp]
        lib.srt_texture_check_host.argtypes = [vp, sz, vp, sz, C.c_longlong, sz]
        lib.srt_group_set_textures.argtypes = [vp, vp, sz]
        lib.srt_group_set_material_textures.argtypes = [vp, vp, sz]
        lib.srt_group_set_triangle_uvs.argtypes = [vp, vp, sz]
    if hasattr(lib, "srt_set_triangle_materials"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_set_triangle_materials.argtypes = [vp, vp, sz]
        lib.srt_group_set_triangle_materials.argtypes = [vp, vp, sz]
        lib.srt_triangle_materials_check_host.argtypes = [vp, sz, sz, sz]
    if hasattr(lib, "srt_last_trace_class"):  # (an older library, SRT_LIB, in an A/B run)
        lib.srt_last_trace_class.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_last_trace_plane_form"):  # (the same)
        lib.srt_last_trace_plane_form.argtypes = [vp, C.POINTER(C.c_int)]
        lib.srt_plane_axis_code_host.argtypes = [vp, vp, C.POINTER(C.c_int)]
        u32p = C.POINTER(C.c_uint32)
        lib.srt_selftest_plane_forms.argtypes = [vp, i, vp, vp, u32p, C.c_uint32, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
    if hasattr(lib, "srt_selftest_diffuse_bounce"):  # (the same)
        u32p = C.POINTER(C.c_uint32)
        lib.srt_selftest_diffuse_bounce.argtypes = [vp, u32p, C.c_uint32, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
    if hasattr(lib, "srt_bernoulli_threshold_host"):
        lib.srt_bernoulli_threshold_host.argtypes = [C.c_float, C.POINTER(C.c_uint64)]
    if hasattr(lib, "srt_set_exposure"):  # (an older library, SRT_LIB, in an A/B run)
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        lib.srt_exposure_defaults.argtypes = [C.POINTER(ExposureParams)]
        lib.srt_exposure_check_host.argtypes = [C.POINTER(ExposureParams)]
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "set_exposure").argtypes = [vp, C.POINTER(ExposureParams)]
            getattr(lib, pre + "reset_exposure").argtypes = [vp]
            getattr(lib, pre + "read_exposure").argtypes = [vp, fp, fp, u32p, u32p]
            getattr(lib, pre + "last_resolve_exposed").argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "srt_set_bloom"):  # (likewise)
        ip = C.POINTER(C.c_int)
        lib.srt_bloom_defaults.argtypes = [C.POINTER(BloomParams)]
        lib.srt_bloom_check_host.argtypes = [C.POINTER(BloomParams)]
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "set_bloom").argtypes = [vp, C.POINTER(BloomParams)]
            getattr(lib, pre + "read_bloom").argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_size_t, ip, ip]
            getattr(lib, pre + "last_resolve_bloomed").argtypes = [vp, ip]
    if hasattr(lib, "srt_set_noise_meter"):  # (likewise)
        ip, u32p, fp = C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        npp, nrp = C.POINTER(NoiseParams), C.POINTER(NoiseResult)
        lib.srt_noise_defaults.argtypes = [npp]
        lib.srt_noise_check_host.argtypes = [npp]
        lib.srt_noise_evaluate_host.argtypes = [u32p, u32p, C.c_uint32, C.c_uint32, npp, nrp]
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "set_noise_meter").argtypes = [vp, npp]
            getattr(lib, pre + "meter_noise").argtypes = [vp]
            getattr(lib, pre + "poll_noise").argtypes = [vp, nrp, u32p, ip]
            getattr(lib, pre + "read_noise").argtypes = [vp, nrp, u32p]
            getattr(lib, pre + "resolve_noise_view").argtypes = [vp]
        lib.srt_group_read_noise_view.argtypes = [vp, vp]
        lib.srt_render_until.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, nrp, u32p]
        lib.srt_last_meter_ran.argtypes = [vp, ip]
        lib.srt_selftest_noise_meter.argtypes = [vp, fp, fp, C.c_uint32, C.c_uint32, C.c_uint32, npp, u32p, u32p, vp]
    if hasattr(lib, "srt_cast_rays"):  # (likewise)
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "cast_rays").argtypes = [vp, vp, sz, C.c_uint32, vp]
            getattr(lib, pre + "pick").argtypes = [vp, vp, vp, sz, vp]
        lib.srt_cast_rays_device.argtypes = [vp, vp, sz, C.c_uint32, vp]
        lib.srt_last_ray_query_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.srt_ray_query_sizes.argtypes = [C.POINTER(sz)]
        sizes = (sz * 2)()
        assert lib.srt_ray_query_sizes(sizes) == 0 and (sizes[0], sizes[1]) == (R.RAY.itemsize, R.RAY_HIT.itemsize), tuple(sizes)
    if hasattr(lib, "srt_occluded_rays"):  # (likewise)
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "occluded_rays").argtypes = [vp, vp, sz, C.c_uint32, vp, vp]
            getattr(lib, pre + "occluded_segments").argtypes = [vp, vp, sz, vp, vp]
            getattr(lib, pre + "segment_rays").argtypes = [vp, vp, sz, vp]
        lib.srt_occluded_rays_device.argtypes = [vp, vp, sz, C.c_uint32, vp, vp]
        lib.srt_occlusion_sizes.argtypes = [C.POINTER(sz)]
        sizes = (sz * 2)()
        assert lib.srt_occlusion_sizes(sizes) == 0 and (sizes[0], sizes[1]) == (R.SEGMENT.itemsize, 8), tuple(sizes)
    if hasattr(lib, "srt_nearest_points"):  # (likewise)
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "nearest_points").argtypes = [vp, vp, sz, C.c_uint32, vp]
        lib.srt_nearest_points_device.argtypes = [vp, vp, sz, C.c_uint32, vp]
        lib.srt_nearest_triangle_host.argtypes = [vp, vp, vp, vp, vp]
        lib.srt_nearest_sphere_host.argtypes = [vp, C.c_float, vp, vp, vp, vp]
        lib.srt_nearest_plane_host.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.srt_nearest_sizes.argtypes = [C.POINTER(sz)]
        sizes = (sz * 2)()
        assert lib.srt_nearest_sizes(sizes) == 0 and (sizes[0], sizes[1]) == (R.POINT_QUERY.itemsize, R.NEAREST.itemsize), tuple(sizes)
    if hasattr(lib, "srt_set_selection"):  # (likewise)
        ip = C.POINTER(C.c_int)
        lib.srt_selection_defaults.argtypes = [vp]
        lib.srt_selection_check_host.argtypes = [vp]
        lib.srt_selection_alpha_table_host.argtypes = [vp, vp, sz, ip]
        lib.srt_selection_sizes.argtypes = [C.POINTER(sz)]
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "set_selection").argtypes = [vp, vp, vp, sz]
            getattr(lib, pre + "read_id_pass").argtypes = [vp, vp, vp, vp, sz, ip, ip]
            getattr(lib, pre + "last_resolve_selected").argtypes = [vp, ip, ip]
        lib.srt_render_ids.argtypes = [vp, vp]
        lib.srt_read_selection_alpha.argtypes = [vp, vp, sz]
        sizes = (sz * 1)()
        assert lib.srt_selection_sizes(sizes) == 0 and sizes[0] == R.SELECTION_PARAMS.itemsize, tuple(sizes)
    if hasattr(lib, "srt_render_ao"):  # (likewise)
        ip = C.POINTER(C.c_int)
        lib.srt_ao_defaults.argtypes = [vp]
        lib.srt_ao_check_host.argtypes = [vp, C.c_int, C.c_int]
        lib.srt_ao_table_host.argtypes = [vp, vp]
        lib.srt_ao_sizes.argtypes = [C.POINTER(sz)]
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "render_ao").argtypes = [vp, vp, vp]
            getattr(lib, pre + "read_ao").argtypes = [vp, vp, sz, ip, ip, ip]
            getattr(lib, pre + "ao_rays").argtypes = [vp, vp, vp, sz, sz, vp]
            getattr(lib, pre + "resolve_ao_view").argtypes = [vp]
        lib.srt_group_read_ao_view.argtypes = [vp, vp]
        sizes = (sz * 1)()
        assert lib.srt_ao_sizes(sizes) == 0 and sizes[0] == R.AO_PARAMS.itemsize, tuple(sizes)
    if hasattr(lib, "srt_area_coverage"):  # (likewise)
        ip, szp = C.POINTER(C.c_int), C.POINTER(sz)
        lib.srt_area_sizes.argtypes = [szp]
        lib.srt_area_check_host.argtypes = [vp, vp]
        lib.srt_area_mask_host.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz]
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "area_coverage").argtypes = [vp, vp, vp, vp, vp, sz, vp]
            getattr(lib, pre + "area_triangle_coverage").argtypes = [vp, vp, vp, vp, C.c_uint32, vp, sz, vp]
            getattr(lib, pre + "select_area").argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, szp]
            getattr(lib, pre + "read_selection").argtypes = [vp, vp, sz, szp]
        lib.srt_area_coverage_device.argtypes = [vp, vp, vp, vp, vp, sz, vp]
        lib.srt_last_area_ms.argtypes = [vp, C.POINTER(C.c_float)]
        lib.srt_last_area_id_pass.argtypes = [vp, ip]
        sizes = (sz * 2)()
        assert lib.srt_area_sizes(sizes) == 0 and (sizes[0], sizes[1]) == (R.AREA.itemsize, R.AREA_SUMMARY.itemsize), tuple(sizes)
    if hasattr(lib, "srt_cast_rays_multi"):  # (likewise)
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "cast_rays_multi").argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, vp]
            getattr(lib, pre + "pick_through").argtypes = [vp, vp, vp, sz, C.c_uint32, vp, vp]
        lib.srt_cast_rays_multi_device.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint32, vp, vp]
        lib.srt_multi_hit_check_host.argtypes = [C.c_uint32, C.c_uint32]
        lib.srt_multi_hit_sizes.argtypes = [C.POINTER(sz)]
        sizes = (sz * 3)()
        assert lib.srt_multi_hit_sizes(sizes) == 0 and tuple(sizes) == (R.RAY.itemsize, R.RAY_HIT.itemsize, R.MULTI_HIT_MAX), tuple(sizes)
    if hasattr(lib, "srt_area_coverage_through"):  # (likewise)
        for pre in ("srt_", "srt_group_"):
            getattr(lib, pre + "area_coverage_through").argtypes = [vp, vp, vp, vp, vp, sz, vp]
            getattr(lib, pre + "area_triangle_coverage_through").argtypes = [vp, vp, vp, vp, C.c_uint32, vp, sz, vp]
            getattr(lib, pre + "select_area_through").argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint32, C.POINTER(sz)]
            getattr(lib, pre + "pick_rays").argtypes = [vp, vp, vp, sz, vp]
        lib.srt_area_coverage_through_device.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class _Denoise:
    """The denoiser's calls, shared by Tracer (srt_*) and TracerGroup (srt_group_*: the same semantics on a device group).
    self._dn(name, *args) calls the class's entry point of that name on its handle."""

    def set_denoise(self, enable=True, **kw):
        """Turn the denoiser on with srt_denoise_defaults() overridden by kw (iterations, feature_samples, sigma_luminance,
        sigma_normal, sigma_depth, sigma_albedo), or off with enable=False."""
        if not enable:
            self._check(self._dn("set_denoise", None))
            return
        d = DenoiseParams()
        self._check(self.lib.srt_denoise_defaults(C.byref(d)))
        for k, v in kw.items():
            if k not in d.as_dict() or k == "enable":
                raise TypeError(f"set_denoise: unknown parameter {k}")
            setattr(d, k, v)
        self._check(self._dn("set_denoise", C.byref(d)))

    def resolve_denoised(self, ticks_stopped):
        """The filter over the current canvas into the handle's ARGB image (read_argb); asynchronous."""
        self._check(self._dn("resolve_denoised", ticks_stopped))

    def read_denoised(self):
        """(height, width, 4) float32: the last filter result before tonemapping (r, g, b, variance)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._dn("read_denoised", _ptr(out)))
        return out

    def read_denoise_inputs(self):
        """dict: normal_depth (h, w, 4), albedo_hits (h, w, 4), moments (h, w), T, P."""
        nd = np.zeros((self.height, self.width, 4), np.float32)
        ah = np.zeros((self.height, self.width, 4), np.float32)
        m = np.zeros((self.height, self.width), np.float32)
        counts = (C.c_uint32 * 2)()
        self._check(self._dn("read_denoise_inputs", _ptr(nd), _ptr(ah), _ptr(m), counts))
        return {"normal_depth": nd, "albedo_hits": ah, "moments": m, "T": int(counts[0]), "P": int(counts[1])}

    def set_denoise_temporal(self, enable=True, **kw):
        """Turn the denoiser's temporal reprojection on with srt_temporal_defaults() overridden by kw (history_limit,
        normal_threshold, depth_threshold), or off with enable=False. Needs the denoiser on (set_denoise)."""
        if not enable:
            self._check(self._dn("set_denoise_temporal", None))
            return
        d = TemporalParams()
        self._check(self.lib.srt_temporal_defaults(C.byref(d)))
        for k, v in kw.items():
            if k not in ("history_limit", "normal_threshold", "depth_threshold"):
                raise TypeError(f"set_denoise_temporal: unknown parameter {k}")
            setattr(d, k, v)
        self._check(self._dn("set_denoise_temporal", C.byref(d)))

    def set_denoise_demodulation(self, enable=True):
        """Filter illumination (colour / first-hit albedo) and multiply the albedo back in the last pass
        (srt_set_denoise_demodulation). Needs the denoiser on; clears nothing, keeps the temporal history."""
        self._check(self._dn("set_denoise_demodulation", 1 if enable else 0))

    def last_filter_demodulated(self):
        """True when the last filter ran the demodulated passes (the switch on and iterations >= 1)."""
        out = C.c_int(0)
        self._check(self._dn("last_filter_demodulated", C.byref(out)))
        return bool(out.value)

    def set_denoise_spatial_variance(self, min_samples=8):
        """Pixels with fewer than min_samples samples get their variance from the moments of their 7x7 neighbourhood
        (srt_set_denoise_spatial_variance); 0: off. Needs the denoiser on; clears nothing, keeps the temporal history."""
        self._check(self._dn("set_denoise_spatial_variance", int(min_samples)))

    def last_filter_spatial_variance(self):
        """True when the last filter enqueued the spatial variance estimate (the switch on and iterations >= 1)."""
        out = C.c_int(0)
        self._check(self._dn("last_filter_spatial_variance", C.byref(out)))
        return bool(out.value)

    def set_denoise_history_illumination(self, enable=True):
        """Reproject the temporal history as illumination: a history tap is rescaled from its own first-hit albedo to the
        pixel's (srt_set_denoise_history_illumination). Needs temporal reprojection on; clears nothing, keeps the history."""
        self._check(self._dn("set_denoise_history_illumination", 1 if enable else 0))

    def last_setup_history_illumination(self):
        """True when the last temporal set-up (a filter's or a clear's) launched an illumination kernel."""
        return bool(self._dn("last_setup_history_illumination"))

    def set_denoise_history_clamp(self, gamma=1.0):
        """Clamp the reprojected history colour of a pixel into mean +- gamma sigma of the current frame's 7x7 neighbourhood
        before it is blended in (srt_set_denoise_history_clamp), so that lighting a moved shape left behind (its shadow, its
        reflection) is corrected within a frame or two. 0 turns it off; 0 < gamma <= 64. Needs temporal reprojection on; clears
        nothing, keeps the history."""
        self._check(self._dn("set_denoise_history_clamp", float(gamma)))

    def last_setup_history_clamp(self):
        """True when the last temporal set-up (a filter's or a clear's) ran the bounds launch and a clamping set-up."""
        return bool(self._dn("last_setup_history_clamp"))

    def set_denoise_history_feedback(self, enable=True):
        """Feed the first a-trous pass back into the temporal history: with iterations >= 1 the colour a clear commits is pass 1's
        output instead of the integrated samples (srt_set_denoise_history_feedback). Needs temporal reprojection on; clears
        nothing, keeps the history. After a clear that had to run the pass itself read_denoised() fails until the next filter."""
        self._check(self._dn("set_denoise_history_feedback", 1 if enable else 0))

    def last_filter_history_feedback(self):
        """True when the last pass 1 (a filter's or a clear's) was a feedback instantiation."""
        return bool(self._dn("last_filter_history_feedback"))

    def reset_denoise_history(self):
        """Drop the temporal history: the next frame is filtered as by the spatial denoiser alone."""
        self._check(self._dn("reset_denoise_history"))

    def read_denoise_history(self):
        """dict: valid, colour (h, w, 3), count (h, w), m1, m2 (h, w), guide (h, w, 2, 4) {N, Z}, {A, cov}, camera (the history
        frame's records.RENDER_DATA). Without a history every array is zero and valid is False."""
        cc = np.zeros((self.height, self.width, 4), np.float32)
        m = np.zeros((self.height, self.width, 2), np.float32)
        g = np.zeros((self.height, self.width, 2, 4), np.float32)
        cam = np.zeros((), R.RENDER_DATA)
        valid = C.c_int(0)
        self._check(self._dn("read_denoise_history", _ptr(cc), _ptr(m), _ptr(g), _ptr(cam), C.byref(valid)))
        return {"valid": bool(valid.value), "colour": cc[..., :3], "count": cc[..., 3], "m1": m[..., 0], "m2": m[..., 1], "guide": g,
                "camera": cam}


class _Exposure:
    """Exposure for the resolve (srt_set_exposure), shared by Tracer and TracerGroup the way _Denoise is."""

    def set_exposure(self, enable=True, **kw):
        """Turn exposure on with srt_exposure_defaults() overridden by kw (mode "manual" / "auto" or EXPOSURE_*, ev, key,
        low_permille, high_permille, adapt, min_ev, max_ev), or off with enable=False (forgets the adaptation state)."""
        if not enable:
            self._check(self._dn("set_exposure", None))
            return
        self._check(self._dn("set_exposure", C.byref(_exposure_params(kw, "set_exposure"))))

    def reset_exposure(self):
        """Forget the adaptation state: the next metered frame adopts its target."""
        self._check(self._dn("reset_exposure"))

    def read_exposure(self):
        """dict: log2_exposure, exposure (numpy float32), hist (256 uint32), metered, left_out. Waits for the stream."""
        l2, e = C.c_float(0), C.c_float(0)
        hist, counts = np.zeros(256, np.uint32), (C.c_uint32 * 2)()
        self._check(self._dn("read_exposure", C.byref(l2), C.byref(e), hist.ctypes.data_as(C.POINTER(C.c_uint32)), counts))
        return {"log2_exposure": np.float32(l2.value), "exposure": np.float32(e.value), "hist": hist, "metered": int(counts[0]),
                "left_out": int(counts[1])}

    def last_resolve_exposed(self):
        """True when the last resolving call ran the exposed resolve."""
        out = C.c_int(0)
        self._check(self._dn("last_resolve_exposed", C.byref(out)))
        return bool(out.value)


class _Bloom:
    """Bloom for the resolve (srt_set_bloom), shared by Tracer and TracerGroup the way _Denoise is."""

    def set_bloom(self, enable=True, **kw):
        """Turn bloom on with srt_bloom_defaults() overridden by kw (threshold, knee, intensity, scatter, clamp, levels), or off
        with enable=False."""
        if not enable:
            self._check(self._dn("set_bloom", None))
            return
        self._check(self._dn("set_bloom", C.byref(_bloom_params(kw, "set_bloom"))))

    def read_bloom(self, level):
        """up_level of the last bloomed frame: (h_level, w_level, 4) float32 (r, g, b, 0). Waits for the stream."""
        w, h = C.c_int(0), C.c_int(0)
        self._check(self._dn("read_bloom", int(level), None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value, 4), np.float32)
        self._check(self._dn("read_bloom", int(level), out.ctypes.data_as(C.POINTER(C.c_float)), out.size // 4, C.byref(w), C.byref(h)))
        return out

    def last_resolve_bloomed(self):
        """True when the last resolving call ran the bloom composite."""
        out = C.c_int(0)
        self._check(self._dn("last_resolve_bloomed", C.byref(out)))
        return bool(out.value)


class _Noise:
    """Noise metering (srt_set_noise_meter), shared by Tracer and TracerGroup the way _Denoise is. A result is a dict: metered,
    left_out, below, converged, dispatches, samples, level_bin, level (numpy float32) and hist (256 uint32)."""

    def set_noise_meter(self, enable=True, **kw):
        """Turn the meter on with srt_noise_defaults() overridden by kw (threshold, luminance_floor, permille, min_samples,
        check_every), or off with enable=False. Needs the denoiser on (set_denoise; iterations=0 is enough)."""
        if not enable:
            self._check(self._dn("set_noise_meter", None))
            return
        self._check(self._dn("set_noise_meter", C.byref(_noise_params(kw, "set_noise_meter"))))

    def meter_noise(self):
        """Enqueue one metering of the current accumulation; asynchronous (then poll_noise / read_noise)."""
        self._check(self._dn("meter_noise"))

    @staticmethod
    def _noise_dict(res, hist):
        d = res.as_dict()
        d["hist"] = hist
        return d

    def poll_noise(self):
        """The newest metering's result, or None while its copy is in flight. Never blocks."""
        res, hist, ready = NoiseResult(), np.zeros(256, np.uint32), C.c_int(0)
        self._check(self._dn("poll_noise", C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ready)))
        return self._noise_dict(res, hist) if ready.value else None

    def read_noise(self):
        """The newest metering's result; waits for its copy only."""
        res, hist = NoiseResult(), np.zeros(256, np.uint32)
        self._check(self._dn("read_noise", C.byref(res), hist.ctypes.data_as(C.POINTER(C.c_uint32))))
        return self._noise_dict(res, hist)

    def resolve_noise_view(self):
        """Meter and overwrite the ARGB image with the heat map; asynchronous (Tracer: read_argb; a group: read_noise_view)."""
        self._check(self._dn("resolve_noise_view"))


class _RayQuery:
    """Ray queries (include/srt_abi.h "ray queries"), shared by Tracer (srt_*) and TracerGroup (srt_group_*: answered by the
    first member). self._dn(name, *args) calls the class's entry point of that name on its handle."""

    def cast_rays(self, origins, directions=None, tmax=np.inf, unit=False):
        """The closest hit of each ray -> records.RAY_HIT array. origins / directions: (n, 3) or (3,), broadcast against each
        other; tmax a scalar or (n,); or pass a records.RAY array as `origins` alone. unit=True: the directions are unit
        length already and are used bit for bit (SRT_RAYS_UNIT_DIRECTIONS). Blocking."""
        rays = R.as_records(origins, R.RAY) if directions is None else R.rays(origins, directions, tmax)
        hits = np.zeros(len(rays), R.RAY_HIT)
        self._check(self._dn("cast_rays", _ptr(rays) if len(rays) else None, len(rays), R.RAYS_UNIT_DIRECTIONS if unit else 0,
                             _ptr(hits) if len(rays) else None))
        return hits

    def pick(self, xy, options=None):
        """The hits under image points -> records.RAY_HIT array. xy: (n, 2) or (2,) continuous pixel coordinates (a pixel's
        centre is (px + 0.5, py + 0.5)); options: the camera and frame size (default: self.options). Blocking."""
        xy = np.ascontiguousarray(np.atleast_2d(np.asarray(xy, np.float32)))
        assert xy.ndim == 2 and xy.shape[1] == 2, xy.shape
        rd = R.as_records(self.options if options is None else options, R.RENDER_DATA)
        hits = np.zeros(len(xy), R.RAY_HIT)
        self._check(self._dn("pick", _ptr(rd), _ptr(xy) if len(xy) else None, len(xy), _ptr(hits) if len(xy) else None))
        return hits

    # ---- multi-hit ray queries (include/srt_abi.h "multi-hit ray queries") ----
    def cast_rays_multi(self, origins, directions=None, k=1, tmax=np.inf, unit=False, count_all=False):
        """The first k hits along each ray in order -> (hits, counts): a records.RAY_HIT array of shape (n, k), the slots past
        a ray's last hit holding the miss record, and counts (n,) uint32 -- the records written, or with count_all=True the
        size of the ray's whole candidate set, which may exceed k. Rays as cast_rays takes them; k in 1 .. MULTI_HIT_MAX.
        Blocking."""
        rays = R.as_records(origins, R.RAY) if directions is None else R.rays(origins, directions, tmax)
        n, k = len(rays), int(k)
        hits, counts = np.zeros((n, max(k, 0)), R.RAY_HIT), np.zeros(n, np.uint32)
        self._check(self._dn("cast_rays_multi", _ptr(rays) if n else None, n, k, self._multi_flags(unit, count_all), _ptr(hits) if n else None,
                             _ptr(counts) if n else None))
        return hits, counts

    def pick_through(self, xy, k, options=None):
        """The first k hits under image points -> (hits (n, k), counts (n,)), as cast_rays_multi; xy and options as pick.
        Blocking."""
        xy = np.ascontiguousarray(np.atleast_2d(np.asarray(xy, np.float32)))
        assert xy.ndim == 2 and xy.shape[1] == 2, xy.shape
        rd = R.as_records(self.options if options is None else options, R.RENDER_DATA)
        n, k = len(xy), int(k)
        hits, counts = np.zeros((n, max(k, 0)), R.RAY_HIT), np.zeros(n, np.uint32)
        self._check(self._dn("pick_through", _ptr(rd), _ptr(xy) if n else None, n, k, _ptr(hits) if n else None, _ptr(counts) if n else None))
        return hits, counts

    def pick_rays(self, xy, options=None):
        """The rays pick would cast for image points -> records.RAY array (unit directions, tmax = +inf: cast them with
        unit=True); xy and options as pick. Blocking."""
        xy = np.ascontiguousarray(np.atleast_2d(np.asarray(xy, np.float32)))
        assert xy.ndim == 2 and xy.shape[1] == 2, xy.shape
        rd = R.as_records(self.options if options is None else options, R.RENDER_DATA)
        rays = np.zeros(len(xy), R.RAY)
        self._check(self._dn("pick_rays", _ptr(rd), _ptr(xy) if len(xy) else None, len(xy), _ptr(rays) if len(xy) else None))
        return rays

    @staticmethod
    def _multi_flags(unit, count_all):
        return (R.RAYS_UNIT_DIRECTIONS if unit else 0) | (R.RAYS_COUNT_ALL if count_all else 0)

    # ---- nearest-surface queries (include/srt_abi.h "nearest-surface queries") ----
    def nearest_points(self, points, max_distance=np.inf, skip_shape=None):
        """The closest scene point to each point -> records.NEAREST array. points: (n, 3) or (3,) with a scalar or (n,)
        max_distance, or a records.POINT_QUERY array alone; skip_shape: a shape index left out of the search. Blocking."""
        pts = np.asarray(points)
        qs = R.as_records(pts, R.POINT_QUERY) if pts.dtype.names else R.point_queries(pts, max_distance)
        out = np.zeros(len(qs), R.NEAREST)
        self._check(self._dn("nearest_points", _ptr(qs) if len(qs) else None, len(qs), R.HIT_NONE if skip_shape is None else int(skip_shape),
                             _ptr(out) if len(qs) else None))
        return out

    # ---- occlusion queries (include/srt_abi.h "occlusion queries") ----
    def occluded_rays(self, origins, directions=None, tmax=np.inf, unit=False, with_invalid=False):
        """Is anything closer than tmax along each ray -> bool array of length n: True exactly where cast_rays of the same
        ray would set HIT_HIT. Arguments as cast_rays. with_invalid=True: (occluded, invalid), the second True for the rays
        the device refused (they are not occluded). Blocking."""
        rays = R.as_records(origins, R.RAY) if directions is None else R.rays(origins, directions, tmax)
        return self._masks("occluded_rays", rays, (R.RAYS_UNIT_DIRECTIONS if unit else 0,), with_invalid)

    def occluded_segments(self, segments, to=None, end_gap=0.0, with_invalid=False):
        """Is anything between `from` and the point end_gap short of `to` -> bool array. segments: a records.SEGMENT array,
        or (n, 3) / (3,) start points with `to` and `end_gap` (records.segments). Blocking."""
        segs = R.as_records(segments, R.SEGMENT) if to is None else R.segments(segments, to, end_gap)
        return self._masks("occluded_segments", segs, (), with_invalid)

    def segment_rays(self, segments, to=None, end_gap=0.0):
        """The rays occluded_segments casts -> records.RAY array (unit directions: pass unit=True with them). Blocking."""
        segs = R.as_records(segments, R.SEGMENT) if to is None else R.segments(segments, to, end_gap)
        rays = np.zeros(len(segs), R.RAY)
        self._check(self._dn("segment_rays", _ptr(segs) if len(segs) else None, len(segs), _ptr(rays) if len(segs) else None))
        return rays

    def _masks(self, name, recs, flags, with_invalid):
        n = len(recs)
        occ, inv = np.zeros((n + 63) // 64, np.uint64), np.zeros((n + 63) // 64, np.uint64)
        self._check(self._dn(name, _ptr(recs) if n else None, n, *flags, _ptr(occ) if n else None, _ptr(inv) if n and with_invalid else None))
        return (R.mask_bits(occ, n), R.mask_bits(inv, n)) if with_invalid else R.mask_bits(occ, n)


class _Selection:
    """Selection overlay and ID pass (include/srt_abi.h "selection overlay and the ID pass"), shared by Tracer and TracerGroup
    (the group: its first member's state and scene)."""

    def set_selection(self, shapes=(), **kw):
        """Outline and tint the shapes (indices into update_scene's array) in every picture the handle resolves, with
        srt_selection_defaults() overridden by kw (width, outline=(A, R, G, B), fill=(A, R, G, B)); no shapes, None or
        enabled=0: off."""
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray([] if shapes is None else shapes, np.int64)).astype(np.uint32))
        self._check(self._dn("set_selection", _ptr(_selection_params(kw, "set_selection")), _ptr(idx) if len(idx) else None, len(idx)))

    def read_id_pass(self):
        """The planes of the last ID pass (render_ids, or the overlay's) -> dict shape, triangle (h, w) uint32 and material
        (h, w) int32. Waits for the stream."""
        w, h = C.c_int(0), C.c_int(0)
        self._check(self._dn("read_id_pass", None, None, None, 0, C.byref(w), C.byref(h)))
        out = dict(shape=np.zeros((h.value, w.value), np.uint32), triangle=np.zeros((h.value, w.value), np.uint32),
                   material=np.zeros((h.value, w.value), np.int32))
        self._check(self._dn("read_id_pass", _ptr(out["shape"]), _ptr(out["triangle"]), _ptr(out["material"]), w.value * h.value, C.byref(w), C.byref(h)))
        return out

    def last_resolve_selected(self):
        """(applied, id_pass_ran) of the last picture-producing resolve."""
        a, r = C.c_int(0), C.c_int(0)
        self._check(self._dn("last_resolve_selected", C.byref(a), C.byref(r)))
        return bool(a.value), bool(r.value)


class _Area:
    """Area selection (include/srt_abi.h "area selection"), shared by Tracer and TracerGroup (the group: its first member's planes,
    scene and selection). rect = (x0, y0, x1, y1), half open, clipped to the frame; lasso: pixel-corner vertices (x, y) or None;
    options: the camera and frame the ID planes are brought up to date for (default: self.options), False: the planes the handle
    holds. through=True (include/srt_abi.h "area selection, through"): X-ray coverage -- the shapes and faces hidden behind
    others count too, over each pixel ray's whole candidate set; no ID planes are used, so options=False is refused."""

    def _area_args(self, rect, lasso, options):
        a, v = area_record(rect, lasso)
        rd = None if options is False else R.as_records(self.options if options is None else options, R.RENDER_DATA)
        self._area_keep = (a, v, rd)
        return (_ptr(rd) if rd is not None else None), _ptr(a), (_ptr(v) if v is not None else None)

    def area_coverage(self, rect, lasso=None, options=None, n_shapes=None, through=False):
        """Visible pixels per shape inside the area -> (counts (n_shapes,) uint32, summary dict). n_shapes: the scene's shape
        count (default: self.scene_data's). through=True: pixels whose ray meets the shape at all, visible or not. Blocking."""
        n = int(self.scene_data["num_shapes"]) if n_shapes is None else int(n_shapes)
        counts, summary = np.zeros(n, np.uint32), np.zeros((), R.AREA_SUMMARY)
        self._check(self._dn("area_coverage_through" if through else "area_coverage", *self._area_args(rect, lasso, options), _ptr(counts) if n else None, n, _ptr(summary)))
        return counts, {k: int(summary[k]) for k in R.AREA_SUMMARY.names[:5]}

    def area_triangle_coverage(self, shape, n_triangles, rect, lasso=None, options=None, through=False):
        """Visible pixels per triangle of the model shape inside the area -> (counts (n_triangles,) uint32, summary dict).
        n_triangles: at least the model's triangle count. through=True: pixels whose ray crosses the triangle, back-facing and
        hidden ones included. Blocking."""
        counts, summary = np.zeros(int(n_triangles), np.uint32), np.zeros((), R.AREA_SUMMARY)
        self._check(self._dn("area_triangle_coverage_through" if through else "area_triangle_coverage", *self._area_args(rect, lasso, options), int(shape), _ptr(counts) if len(counts) else None,
                             len(counts), _ptr(summary)))
        return counts, {k: int(summary[k]) for k in R.AREA_SUMMARY.names[:5]}

    def select_area(self, rect, lasso=None, mode=R.SELECT_REPLACE, min_pixels=1, options=None, through=False):
        """Combine the shapes with at least min_pixels visible pixels inside the area with the current selection (mode:
        records.SELECT_REPLACE, SELECT_ADD, SELECT_SUBTRACT, SELECT_TOGGLE) and overlay the result -> its length. through=True:
        by the through counts (an infinite plane the frame faces is met by most pixels: filter it with min_pixels or by type).
        Blocking."""
        n = C.c_size_t(0)
        self._check(self._dn("select_area_through" if through else "select_area", *self._area_args(rect, lasso, options), int(mode), int(min_pixels), C.byref(n)))
        return n.value

    def read_selection(self):
        """The current selection -> (n,) uint32, ascending and unique; empty while the overlay is off."""
        n = C.c_size_t(0)
        self._check(self._dn("read_selection", None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        self._check(self._dn("read_selection", _ptr(out) if n.value else None, n.value, C.byref(n)))
        return out

    area_mask = staticmethod(area_mask)


class _AmbientOcclusion:
    """The ambient-occlusion pass (include/srt_abi.h "ambient-occlusion pass"), shared by Tracer and TracerGroup (the group: on
    its first member, which holds the whole scene). kw: srt_ao_defaults() overridden (samples, radius, bias, seed, background)."""

    def render_ao(self, options=None, **kw):
        """The pass for the camera and frame size of options (default: self.options), asynchronous; then read_ao()."""
        rd = R.as_records(self.options if options is None else options, R.RENDER_DATA)
        self._check(self._dn("render_ao", _ptr(rd), _ptr(_ao_params(kw, "render_ao"))))

    def read_ao(self):
        """The last pass's plane -> ((h, w) uint32: occluded rays per pixel, records.HIT_NONE without a surface; samples).
        Waits for the stream."""
        w, h, s = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._dn("read_ao", None, 0, C.byref(w), C.byref(h), C.byref(s)))
        out = np.zeros((h.value, w.value), np.uint32)
        self._check(self._dn("read_ao", _ptr(out), out.size, C.byref(w), C.byref(h), C.byref(s)))
        return out, s.value

    def ao_rays(self, options=None, first=0, n=None, **kw):
        """The rays the pass casts for pixels first .. first + n of the frame (default: all of it) -> records.RAY array of
        n * samples, ray (q, s) at (q - first) * samples + s; tmax = NaN where the pixel has no surface. Blocking."""
        rd = R.as_records(self.options if options is None else options, R.RENDER_DATA)
        p = _ao_params(kw, "ao_rays")
        n = int(rd["width"]) * int(rd["height"]) - first if n is None else n
        rays = np.zeros(max(n, 0) * int(p["samples"]), R.RAY)
        self._check(self._dn("ao_rays", _ptr(rd), _ptr(p), first, n, _ptr(rays) if len(rays) else None))
        return rays

    def resolve_ao_view(self):
        """Overwrite the ARGB image with the last pass's grey picture; asynchronous (Tracer: read_argb; a group: read_ao_view)."""
        self._check(self._dn("resolve_ao_view"))

    ao_table = staticmethod(ao_table)


class Tracer(_Denoise, _Exposure, _Bloom, _Noise, _RayQuery, _Selection, _Area, _AmbientOcclusion):
    """Mirror of the reference's `class Tracer`. Field and method names are the
    reference's; records are numpy scalars of records.RENDER_DATA / SCENE_DATA."""

    def __init__(self, width, height, device=0, lib=None):
        self.lib = lib if lib is not None else load_library()
        self._h = C.c_void_p()
        rc = self.lib.srt_create(width, height, device, C.byref(self._h))
        if rc:
            raise SrtError(self.lib.srt_last_error(None).decode())
        self.width, self.height = width, height
        # RenderData(width, height): num_samples = 4, num_bounces = 10 (tracer.hpp:61-66)
        self.options = R.render_data(width, height, num_samples=4, num_bounces=10)
        self.scene_data = R.scene_data(0)
        self.owned_rows = height

    # -- plumbing --
    def _check(self, rc):
        if rc:
            e = SrtError(self.lib.srt_last_error(self._h).decode())
            e.code = rc  # SRT_ERR_*
            raise e

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.srt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the reference's interface --
    def set_skybox(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32)
        assert rgba.ndim == 3 and rgba.shape[2] == 4
        self._check(self.lib.srt_set_skybox(self._h, _ptr(rgba), rgba.shape[1], rgba.shape[0]))

    # -- albedo textures (include/srt_abi.h) --
    def set_textures(self, images):
        """images: list of (H, W, 4) float32, row 0 = bottom; [] removes them all."""
        keep, descs = _texture_descs(images)
        self._check(self.lib.srt_set_textures(self._h, descs if keep else None, len(keep)))

    def set_material_textures(self, bindings):
        """bindings: records.MATERIAL_TEXTURE records (records.material_texture), one per material; None / [] unbinds all."""
        b = R.as_records(bindings if bindings is not None else [], R.MATERIAL_TEXTURE)
        self._check(self.lib.srt_set_material_textures(self._h, _ptr(b) if len(b) else None, len(b)))

    def set_triangle_uvs(self, uv):
        """uv: (n_triangles, 3, 2) float32 parallel to the triangle array, or None."""
        uv, n = _uv_array(uv)
        self._check(self.lib.srt_set_triangle_uvs(self._h, _ptr(uv) if uv is not None else None, n))

    def set_triangle_materials(self, materials):
        """materials: n_triangles int32 parallel to the triangle array (-1: the shape's material, m >= 0: materials[m]), or None
        (include/srt_abi.h "per-triangle materials")."""
        tm = _tm_array(materials)
        self._check(self.lib.srt_set_triangle_materials(self._h, _ptr(tm) if tm is not None else None, 0 if tm is None else len(tm)))

    def last_trace_textured(self):
        out = C.c_int(0)
        self._check(self.lib.srt_last_trace_textured(self._h, C.byref(out)))
        return bool(out.value)

    def last_trace_plane_form(self):
        """0: the last trace ran its class's own kernel (or a general one); else the scene's plane form, whose axis twin ran
        (srt_last_trace_plane_form)"""
        out = C.c_int(-1)
        self._check(self.lib.srt_last_trace_plane_form(self._h, C.byref(out)))
        return int(out.value)

    def last_trace_class(self):
        """0: the last trace ran a general kernel; 1..: the kernel of the scene's class (srt_last_trace_class)"""
        out = C.c_int(0)
        self._check(self.lib.srt_last_trace_class(self._h, C.byref(out)))
        return out.value

    def update_scene(self, shapes, triangles, materials):
        shapes = R.as_records(shapes, R.SHAPE)
        triangles = R.as_records(triangles, R.TRIANGLE)
        materials = R.as_records(materials, R.MATERIAL)
        sd = R.as_records(self.scene_data, R.SCENE_DATA)
        self._check(self.lib.srt_update_scene(self._h, _ptr(shapes), len(shapes), _ptr(triangles), len(triangles),
                                              _ptr(materials), len(materials), _ptr(sd)))
        self.scene_data["num_shapes"] = len(shapes)  # src/tracer.cpp:94

    def clear_canvas(self):
        self._check(self.lib.srt_clear_canvas(self._h))

    def render(self, ticks_stopped, output=None):
        """Tracer::render: trace + resolve + blocking read-back into `output`
        (uint8, owned_rows*width*4, bytes A,R,G,B)."""
        if output is None:
            output = np.zeros(self.owned_rows * self.width * 4, np.uint8)
        assert output.dtype == np.uint8 and output.size >= self.owned_rows * self.width * 4
        rd = R.as_records(self.options, R.RENDER_DATA)
        self._check(self.lib.srt_render(self._h, _ptr(rd), ticks_stopped, _ptr(output)))
        return output

    # -- extras --
    def render_async(self, ticks_stopped, output):
        """Enqueue trace + resolve + copy into `output`; valid after synchronize()."""
        assert output.dtype == np.uint8 and output.size >= self.owned_rows * self.width * 4
        rd = R.as_records(self.options, R.RENDER_DATA)
        self._check(self.lib.srt_render_async(self._h, _ptr(rd), ticks_stopped, _ptr(output)))

    def trace(self):
        rd = R.as_records(self.options, R.RENDER_DATA)
        self._check(self.lib.srt_trace(self._h, _ptr(rd)))

    def set_radiance_budget(self, nbytes):
        self._check(self.lib.srt_set_radiance_budget(self._h, nbytes))

    def resolve(self, ticks_stopped):
        self._check(self.lib.srt_resolve(self._h, ticks_stopped))

    def resolve_external(self, canvas_ptr, num_pixels, ticks_stopped, argb_ptr):
        self._check(self.lib.srt_resolve_external(self._h, C.c_void_p(canvas_ptr), num_pixels, ticks_stopped, C.c_void_p(argb_ptr)))

    def synchronize(self):
        self._check(self.lib.srt_synchronize(self._h))

    def read_canvas(self):
        out = np.zeros((self.owned_rows, self.width, 4), np.float32)
        self._check(self.lib.srt_read_canvas(self._h, _ptr(out)))
        return out

    def read_argb(self):
        out = np.zeros((self.owned_rows, self.width, 4), np.uint8)
        self._check(self.lib.srt_read_argb(self._h, _ptr(out)))
        return out

    def counters(self):
        c = Counters()
        self._check(self.lib.srt_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def debug_counters(self):
        out = (C.c_uint64 * 18)()
        self.lib.srt_debug_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(self.lib.srt_debug_counters(self._h, out))
        v = [int(x) for x in out]
        return {"rays": v[0], "sky": v[1], "paths": v[2], "orphans": 0, "evictions": 0,  # (rounds 1-3; the scripts still print them)
                # scene-class kernels: EXTEND phases of fresh camera rays only (they run the camera forms), and the rays in them
                "camera_phases": v[5] >> 36, "camera_phase_rays": v[5] & ((1 << 36) - 1),
                "iterations": v[6], "shade_phases": v[7], "waves_per_cu": v[8], "grid": v[9],
                "phase_cycles": dict(zip(("extend", "ring", "shade", "park", "deliver", "refill", "head", "kernel"), v[10:18])),
                # array-scan kernels without -DSRT_PHASE_CLOCK reuse the first two clock slots: big-model scans and the lanes in them
                "scans": v[10], "scan_lanes": v[11],
                # ... as do the scene classes' axis twins: their EXTEND phases, and those among them that failed the twin's guard
                "axis_phases": v[10], "axis_failed": v[11],
                # ... and the NO_SPEC classes (which count shade_phases in the product build, too): SHADE phases in which no lane ran the
                # per-lane bounce, and those whose lanes were all plain diffuse but failed the operand guard
                "diffuse_short": v[12], "diffuse_failed": v[13],
                # ... and the next four: the launch-end ray pool (blocks taken, records handed in, sum of squares of the blocks a wave took, blocks the last wave took)
                "pool_taken": v[12], "pool_given": v[13], "pool_taken_sq": v[14], "pool_last_taken": v[15]}

    def debug_region_counters(self):
        """[(waves, lanes)] per region of SRT_REGION_LIST for a -DSRT_REGION_COUNT build; [] for the product build."""
        out = (C.c_uint64 * 128)()
        n = C.c_int(0)
        self.lib.srt_debug_region_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]
        self._check(self.lib.srt_debug_region_counters(self._h, out, 128, C.byref(n)))
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value // 2)]

    def reset_counters(self):
        self._check(self.lib.srt_reset_counters(self._h))

    def count_triangles(self, enable=True):
        self._check(self.lib.srt_set_count_triangles(self._h, 1 if enable else 0))

    def set_acceleration(self, mode):
        """ACCEL_NONE (array-order triangle scan, the parity mode) or ACCEL_BVH; applies at the next update_scene."""
        self._check(self.lib.srt_set_acceleration(self._h, int(mode)))

    def acceleration_info(self):
        out = (C.c_uint64 * 7)()
        self._check(self.lib.srt_acceleration_info(self._h, out))
        return dict(zip(("nodes", "leaves", "depth", "build_us", "models_built", "models_reused", "models_refitted"), (int(v) for v in out)))

    def set_acceleration_refit(self, mode):
        """REFIT_HOST (the default) or REFIT_DEVICE: who refits the hierarchy of a model that only moved; applies at the next
        update_scene."""
        self._check(self.lib.srt_set_acceleration_refit(self._h, int(mode)))

    def set_acceleration_deform(self, mode, rebuild_ratio=0.0):
        """DEFORM_REBUILD (the default) or DEFORM_REFIT: a model whose vertices changed is built anew / keeps its tree with
        new boxes until its cost ratio passes rebuild_ratio (0: never); applies at the next update_scene."""
        self._check(self.lib.srt_set_acceleration_deform(self._h, int(mode), float(rebuild_ratio)))

    def acceleration_deform_info(self):
        """Of the last update_scene: models kept across a change of triangle bytes, models rebuilt on their cost ratio, cost
        launches, and the largest known cost ratio (0.0: none known). Waits for the cost read-back only."""
        out, worst = (C.c_uint64 * 4)(), C.c_double(0)
        self._check(self.lib.srt_acceleration_deform_info(self._h, out, C.byref(worst)))
        return {"models_kept": int(out[0]), "models_rebuilt": int(out[1]), "cost_launches": int(out[2]), "worst_ratio": worst.value}

    def set_acceleration_build(self, mode, min_triangles=0):
        """BUILD_HOST (the default) or BUILD_DEVICE: a model of at least min_triangles triangles that has no hierarchy to keep
        gets the balanced topology over its Morton order, sorted on the device; applies at the next update_scene."""
        self._check(self.lib.srt_set_acceleration_build(self._h, int(mode), int(min_triangles)))

    def set_acceleration_build_order(self, order):
        """BUILD_ORDER_MORTON (the default) or BUILD_ORDER_MEDIAN: the order BUILD_DEVICE lays the balanced topology over -- the
        30-bit Morton order, or every range of the topology sorted along its widest centroid axis, top-down (more launches, a
        tree close to the host's balanced one); applies at the next update_scene, without effect under BUILD_HOST."""
        self._check(self.lib.srt_set_acceleration_build_order(self._h, int(order)))

    def acceleration_build_info(self):
        """Of the last update_scene: models built on the device, records sorted, build launches. Waits for the sorted order's
        read-back only."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.srt_acceleration_build_info(self._h, out))
        return dict(zip(("models", "records", "launches"), (int(v) for v in out)))

    def last_build_kernel_ms(self):
        """Device time from the first build launch of the last update_scene to the end of the refit behind it (needs
        set_kernel_timers); blocking."""
        a = C.c_float()
        self._check(self.lib.srt_last_build_kernel_ms(self._h, C.byref(a)))
        return a.value

    def acceleration_refit_info(self):
        """Of the last update_scene: models refitted on the device, inner blocks they requantised, refit launches."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.srt_acceleration_refit_info(self._h, out))
        return dict(zip(("models", "inner_blocks", "launches"), (int(v) for v in out)))

    def last_refit_kernel_ms(self):
        """Device time of the last update_scene's refit launches (needs set_kernel_timers); blocking."""
        a = C.c_float()
        self._check(self.lib.srt_last_refit_kernel_ms(self._h, C.byref(a)))
        return a.value

    def read_bvh_blocks(self):
        """(n, 32) uint32: the device's block array as the kernel walks it (absolute indices); blocking."""
        n = C.c_size_t(0)
        self._check(self.lib.srt_read_bvh_blocks(self._h, None, 0, C.byref(n)))
        blocks = np.zeros((n.value, 32), np.uint32)
        self._check(self.lib.srt_read_bvh_blocks(self._h, _ptr(blocks), len(blocks), C.byref(n)))
        return blocks

    def selftest_math(self, stride=1):
        out = (C.c_uint64 * 16)()
        self._check(self.lib.srt_selftest_math(self._h, stride, out))
        return [int(v) for v in out]

    def selftest_rare_lanes(self, what, words):
        """words: uint32 [lanes, 8], lanes a multiple of 64 (one wave each) -> (new [lanes, 4], per-lane reference [lanes, 4], mismatching words)"""
        words = np.ascontiguousarray(words, np.uint32)
        assert words.ndim == 2 and words.shape[1] == 8 and words.shape[0] % 64 == 0
        new, ref, bad = np.zeros((words.shape[0], 4), np.uint32), np.zeros((words.shape[0], 4), np.uint32), C.c_uint64()
        u32p = C.POINTER(C.c_uint32)
        self._check(self.lib.srt_selftest_rare_lanes(self._h, int(what), words.ctypes.data_as(u32p), words.shape[0] // 64,
                                                     new.ctypes.data_as(u32p), ref.ctypes.data_as(u32p), C.byref(bad)))
        return new, ref, int(bad.value)

    def selftest_plane_forms(self, what, planes, cam_org, words):
        """planes: float32 [32] (the two staged plane blocks of the layout planes y, x | plane z); words: uint32 [lanes, 8], lanes a
        multiple of 64 -> (new [lanes, 2] = {tmin bits, best}, test_planes2's [lanes, 2], fast [waves], mismatching words)"""
        words = np.ascontiguousarray(words, np.uint32)
        planes = np.ascontiguousarray(planes, np.float32).reshape(32)
        cam_org = np.ascontiguousarray(cam_org, np.float32).reshape(3)
        assert words.ndim == 2 and words.shape[1] == 8 and words.shape[0] % 64 == 0
        waves = words.shape[0] // 64
        new, ref = np.zeros((words.shape[0], 2), np.uint32), np.zeros((words.shape[0], 2), np.uint32)
        fast, bad = np.zeros(waves, np.uint32), C.c_uint64()
        u32p = C.POINTER(C.c_uint32)
        self._check(self.lib.srt_selftest_plane_forms(self._h, int(what), _ptr(planes), _ptr(cam_org), words.ctypes.data_as(u32p), waves,
                                                      new.ctypes.data_as(u32p), ref.ctypes.data_as(u32p), fast.ctypes.data_as(u32p), C.byref(bad)))
        return new, ref, fast, int(bad.value)

    def selftest_diffuse_bounce(self, words):
        """words: uint32 [lanes, 20] = {random_dir, dir, nrm, metallic threshold, transmittance threshold, smoothness, mask, colour,
        seed, -}, lanes a multiple of 64 -> (wave form [lanes, 8] = {dir, mask, seed, drew transparent}, the per-lane form's
        [lanes, 8], fast [waves], mismatching words)"""
        words = np.ascontiguousarray(words, np.uint32)
        assert words.ndim == 2 and words.shape[1] == 20 and words.shape[0] % 64 == 0
        waves = words.shape[0] // 64
        new, ref = np.zeros((words.shape[0], 8), np.uint32), np.zeros((words.shape[0], 8), np.uint32)
        fast, bad = np.zeros(waves, np.uint32), C.c_uint64()
        u32p = C.POINTER(C.c_uint32)
        self._check(self.lib.srt_selftest_diffuse_bounce(self._h, words.ctypes.data_as(u32p), waves, new.ctypes.data_as(u32p),
                                                         ref.ctypes.data_as(u32p), fast.ctypes.data_as(u32p), C.byref(bad)))
        return new, ref, fast, int(bad.value)

    def set_kernel_timers(self, enable=True):
        """the render calls record the kernel timers' events too (default: only trace() does)"""
        self._check(self.lib.srt_set_kernel_timers(self._h, int(bool(enable))))

    def last_kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        self._check(self.lib.srt_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_trace_launches(self):
        """(srt_trace_kernel launches of the last trace = its sample batches, whether they overlapped on two streams)"""
        n, o = C.c_int(0), C.c_int(0)
        self.lib.srt_last_trace_launches.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._check(self.lib.srt_last_trace_launches(self._h, C.byref(n), C.byref(o)))
        return n.value, bool(o.value)

    def last_trace_kernel_ms(self):
        a = C.c_float()
        self._check(self.lib.srt_last_trace_kernel_ms(self._h, C.byref(a)))
        return a.value

    def device_buffers(self):
        cp, cb, ap, ab = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        self._check(self.lib.srt_device_buffers(self._h, C.byref(cp), C.byref(cb), C.byref(ap), C.byref(ab)))
        return cp.value, cb.value, ap.value, ab.value

    def bind_canvas(self, device_ptr, nbytes):
        self._check(self.lib.srt_bind_canvas(self._h, C.c_void_p(device_ptr), nbytes))

    def bind_stream(self, hip_stream):
        self._check(self.lib.srt_bind_stream(self._h, C.c_void_p(hip_stream)))

    # -- collecting a partitioned frame over RCCL (one process per GPU) --
    @staticmethod
    def comm_unique_id():
        """128 bytes for srt_comm_init; made by ONE rank and shipped to all others by the caller."""
        buf = C.create_string_buffer(128)
        if load_library().srt_comm_unique_id(buf):
            raise SrtError(load_library().srt_last_error(None).decode())
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        self._check(self.lib.srt_comm_init(self._h, C.c_char_p(unique_id), rank, world))

    def gather(self, root=0):
        """ONE ncclGather of the packed canvases to `root` + unpermute there (asynchronous, collective)."""
        self._check(self.lib.srt_gather(self._h, root))

    def resolve_gathered(self, ticks_stopped):
        self._check(self.lib.srt_resolve_gathered(self._h, ticks_stopped))

    def gathered_buffers(self):
        cp, ap = C.c_void_p(), C.c_void_p()
        self._check(self.lib.srt_gathered_buffers(self._h, C.byref(cp), C.byref(ap)))
        return cp.value, ap.value

    def read_gathered(self, canvas=True, argb=False):
        c = np.zeros((self.height, self.width, 4), np.float32) if canvas else None
        a = np.zeros((self.height, self.width, 4), np.uint8) if argb else None
        self._check(self.lib.srt_read_gathered(self._h, _ptr(c) if canvas else None, _ptr(a) if argb else None))
        return c, a

    # -- frame pipeline --
    def render_pipelined(self, ticks_stopped, output):
        """Enqueue this frame, receive the previous one in `output`; returns its index or -1."""
        assert output.dtype == np.uint8 and output.size >= self.owned_rows * self.width * 4
        rd = R.as_records(self.options, R.RENDER_DATA)
        n = C.c_longlong(-1)
        self._check(self.lib.srt_render_pipelined(self._h, _ptr(rd), ticks_stopped, _ptr(output), C.byref(n)))
        return n.value

    def pipeline_flush(self, output):
        n = C.c_longlong(-1)
        self._check(self.lib.srt_pipeline_flush(self._h, _ptr(output), C.byref(n)))
        return n.value

    # -- noise metering (srt_set_noise_meter): set_noise_meter ... resolve_noise_view are _Noise's --
    def render_until(self, max_dispatches, time_stride=7919, output=None):
        """srt_render_until: trace self.options (time + i * time_stride) until a check converges or max_dispatches are done,
        resolve, blocking read-back -> (output, the deciding check's result dict without hist, dispatches done)."""
        if output is None:
            output = np.zeros(self.owned_rows * self.width * 4, np.uint8)
        assert output.dtype == np.uint8 and output.size >= self.owned_rows * self.width * 4
        rd = R.as_records(self.options, R.RENDER_DATA)
        res, done = NoiseResult(), C.c_uint32(0)
        self._check(self.lib.srt_render_until(self._h, _ptr(rd), int(time_stride), int(max_dispatches), _ptr(output), C.byref(res), C.byref(done)))
        return output, res.as_dict(), int(done.value)

    def last_meter_ran(self):
        """True when the last render / render_async / render_pipelined metered its frame."""
        out = C.c_int(0)
        self._check(self.lib.srt_last_meter_ran(self._h, C.byref(out)))
        return bool(out.value)

    def selftest_noise_meter(self, canvas, moments, T, P, view=False, **kw):
        """srt_selftest_noise_meter: the meter kernel over canvas (n, 4) and moments (n) float32 as a metering at T, P under the
        defaults overridden by kw -> hist (256 uint32), (metered, left_out, below), view bytes (n, 4) uint8 or None."""
        canvas = np.ascontiguousarray(canvas, np.float32).reshape(-1, 4)
        moments = np.ascontiguousarray(moments, np.float32).reshape(-1)
        assert len(canvas) == len(moments)
        hist, counts = np.zeros(256, np.uint32), (C.c_uint32 * 3)()
        out = np.zeros((len(canvas), 4), np.uint8) if view else None
        fp = C.POINTER(C.c_float)
        self._check(self.lib.srt_selftest_noise_meter(self._h, canvas.ctypes.data_as(fp), moments.ctypes.data_as(fp), len(canvas), int(T), int(P),
                                                      C.byref(_noise_params(kw, "selftest_noise_meter")), hist.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      counts, _ptr(out) if view else None))
        return hist, tuple(int(v) for v in counts), out

    # -- edge-aware denoiser (srt_set_denoise): set_denoise ... read_denoise_history are _Denoise's --
    def _dn(self, name, *args):
        return getattr(self.lib, "srt_" + name)(self._h, *args)

    def set_denoise_object_motion(self, enable=True):
        """Keep the temporal history across an update_scene that only moves shapes (srt_set_denoise_object_motion). Needs
        temporal reprojection on; every change of the switch drops the history."""
        self._check(self.lib.srt_set_denoise_object_motion(self._h, 1 if enable else 0))

    def read_denoise_history_bounds(self):
        """The history clamp's two planes of the last bounds launch (srt_read_denoise_history_bounds): dict mu (h, w, 3),
        weight (h, w) (0: do not clamp), sigma (h, w, 3), taps (h, w) (the counting taps, as floats)."""
        b0 = np.zeros((self.height, self.width, 4), np.float32)
        b1 = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self.lib.srt_read_denoise_history_bounds(self._h, _ptr(b0), _ptr(b1)))
        return {"mu": b0[..., :3], "weight": b0[..., 3], "sigma": b1[..., :3], "taps": b1[..., 3]}

    def read_denoise_shape_ids(self):
        """(current, history): (h, w) uint32 shape index of each pixel's first hit (feature sample 0 of the latest dispatch;
        NO_SHAPE: none), for the frame since the clear and for the history frame (all NO_SHAPE without a history)."""
        cur = np.zeros((self.height, self.width), np.uint32)
        hist = np.zeros((self.height, self.width), np.uint32)
        self._check(self.lib.srt_read_denoise_shape_ids(self._h, _ptr(cur), _ptr(hist)))
        return cur, hist

    def read_denoise_motion(self):
        """The per-shape table the next filter would use: dict state (n,), A (n, 3, 4), B (n, 3, 3), any_moved."""
        n, any_moved = C.c_size_t(0), C.c_int(0)
        self._check(self.lib.srt_read_denoise_motion(self._h, None, 0, C.byref(n), C.byref(any_moved)))
        table = np.zeros((max(n.value, 1), MOTION_WORDS), np.uint32)
        self._check(self.lib.srt_read_denoise_motion(self._h, _ptr(table), n.value, C.byref(n), C.byref(any_moved)))
        out = _motion_rows(table[:n.value])
        out["any_moved"] = bool(any_moved.value)
        out["first_row"] = table[:n.value, 1].astype(np.int64)  # (a DEFORMED row's word 1; the bits of A[0][0] otherwise)
        return out

    def set_denoise_vertex_motion(self, enable=True):
        """Keep the temporal history across an update_scene that changes a model's vertices and keeps its topology
        (srt_set_denoise_vertex_motion). Needs object motion on; every change of the switch drops the history."""
        self._check(self.lib.srt_set_denoise_vertex_motion(self._h, 1 if enable else 0))

    def read_denoise_triangle_ids(self):
        """(current, history): (h, w) uint32 index inside its model of the triangle each pixel's first hit lies on (feature
        sample 0 of the latest dispatch; NO_SHAPE: no hit, no material, or not a model), as read_denoise_shape_ids."""
        cur = np.zeros((self.height, self.width), np.uint32)
        hist = np.zeros((self.height, self.width), np.uint32)
        self._check(self.lib.srt_read_denoise_triangle_ids(self._h, _ptr(cur), _ptr(hist)))
        return cur, hist

    def read_denoise_vertex_tables(self):
        """(current, history): (rows, 3, 3) float32 world vertices P0, P1, P2 per instance triangle (model shapes in shape
        order), of the frame since the clear and of the history frame (zeros without a history)."""
        n = C.c_size_t(0)
        self._check(self.lib.srt_read_denoise_vertex_tables(self._h, None, None, 0, C.byref(n)))
        cur, hist = np.zeros((max(n.value, 1), 3, 3), np.float32), np.zeros((max(n.value, 1), 3, 3), np.float32)
        self._check(self.lib.srt_read_denoise_vertex_tables(self._h, _ptr(cur), _ptr(hist), n.value, C.byref(n)))
        return cur[:n.value], hist[:n.value]

    def cast_rays_device(self, rays_ptr, n, hits_ptr, unit=False):
        """cast_rays over device arrays (n records.RAY at rays_ptr, n records.RAY_HIT at hits_ptr, 16-byte aligned), enqueued
        on the handle's stream: synchronize() before the hits are read."""
        self._check(self.lib.srt_cast_rays_device(self._h, C.c_void_p(rays_ptr), n, R.RAYS_UNIT_DIRECTIONS if unit else 0, C.c_void_p(hits_ptr)))

    def cast_rays_multi_device(self, rays_ptr, n, k, hits_ptr, counts_ptr=None, unit=False, count_all=False):
        """cast_rays_multi over device arrays (n records.RAY at rays_ptr, n * k records.RAY_HIT at hits_ptr, 16-byte aligned;
        if given, n uint32 at counts_ptr), enqueued on the handle's stream: synchronize() before they are read."""
        self._check(self.lib.srt_cast_rays_multi_device(self._h, C.c_void_p(rays_ptr), n, int(k), self._multi_flags(unit, count_all), C.c_void_p(hits_ptr),
                                                        C.c_void_p(counts_ptr) if counts_ptr else None))

    def nearest_points_device(self, queries_ptr, n, out_ptr, skip_shape=None):
        """nearest_points over device arrays (n records.POINT_QUERY at queries_ptr, n records.NEAREST at out_ptr, 16-byte
        aligned), enqueued on the handle's stream: synchronize() before the records are read."""
        self._check(self.lib.srt_nearest_points_device(self._h, C.c_void_p(queries_ptr), n, R.HIT_NONE if skip_shape is None else int(skip_shape),
                                                       C.c_void_p(out_ptr)))

    def occluded_rays_device(self, rays_ptr, n, occluded_ptr, invalid_ptr=None, unit=False):
        """occluded_rays over device arrays (n records.RAY at rays_ptr, 16-byte aligned; ceil(n / 64) 64-bit words at
        occluded_ptr and, if given, at invalid_ptr, 8-byte aligned: ray q is bit q & 63 of word q >> 6, see records.mask_bits),
        enqueued on the handle's stream: synchronize() before the words are read."""
        self._check(self.lib.srt_occluded_rays_device(self._h, C.c_void_p(rays_ptr), n, R.RAYS_UNIT_DIRECTIONS if unit else 0, C.c_void_p(occluded_ptr),
                                                      C.c_void_p(invalid_ptr) if invalid_ptr else None))

    def render_ids(self, options=None):
        """The ID pass alone for the camera and frame size of options (default: self.options), asynchronous; then read_id_pass()."""
        rd = R.as_records(self.options if options is None else options, R.RENDER_DATA)
        self._check(self.lib.srt_render_ids(self._h, _ptr(rd)))

    def read_selection_alpha(self):
        """alpha(p) of the last overlaid frame -> (h, w) uint8. Waits for the stream."""
        out = np.zeros((self.owned_rows, self.width), np.uint8)
        self._check(self.lib.srt_read_selection_alpha(self._h, _ptr(out), out.size))
        return out

    def area_coverage_device(self, counts_ptr, n, summary_ptr, rect, lasso=None, options=None, through=False):
        """area_coverage left in device memory (n >= the scene's shape count uint32 at counts_ptr, 8 uint32 laid out as
        records.AREA_SUMMARY at summary_ptr), enqueued on the handle's stream: synchronize() before they are read."""
        fn = self.lib.srt_area_coverage_through_device if through else self.lib.srt_area_coverage_device
        self._check(fn(self._h, *self._area_args(rect, lasso, options), C.c_void_p(counts_ptr), n, C.c_void_p(summary_ptr)))

    def last_area_ms(self):
        """Device time of the last coverage call's clear and counting launches under set_kernel_timers (0 without)."""
        ms = C.c_float(0)
        self._check(self.lib.srt_last_area_ms(self._h, C.byref(ms)))
        return ms.value

    def last_area_id_pass(self):
        """Whether the last coverage call had to make the ID planes first."""
        ran = C.c_int(0)
        self._check(self.lib.srt_last_area_id_pass(self._h, C.byref(ran)))
        return bool(ran.value)

    def last_ray_query_ms(self):
        """Device time of the last query's launches under set_kernel_timers (0 without)."""
        ms = C.c_float(0)
        self._check(self.lib.srt_last_ray_query_ms(self._h, C.byref(ms)))
        return ms.value

    def set_partition(self, rank, world, rows_per_block=8):
        self._check(self.lib.srt_set_partition(self._h, rank, world, rows_per_block))
        self.owned_rows = self.lib.srt_partition_owned_rows(self.height, rank, world, rows_per_block)


class TracerGroup(_Denoise, _Exposure, _Bloom, _Noise, _RayQuery, _Selection, _Area, _AmbientOcclusion):
    """One process driving several GPUs (srt_group_*): the reference's Tracer interface over a row partition,
    collected with one ncclGather per frame."""

    def __init__(self, width, height, n_devices=1, devices=None, rows_per_block=8):
        self.lib = load_library()
        self._g = C.c_void_p()
        devs = (C.c_int * n_devices)(*devices) if devices is not None else None
        rc = self.lib.srt_group_create(width, height, n_devices, devs, rows_per_block, C.byref(self._g))
        if rc:
            raise SrtError(self.lib.srt_last_error(None).decode())
        self.width, self.height, self.n_devices = width, height, n_devices
        self.options = R.render_data(width, height, num_samples=4, num_bounces=10)
        self.scene_data = R.scene_data(0)

    def _check(self, rc):
        if rc:
            e = SrtError(self.lib.srt_group_last_error(self._g).decode())
            e.code = rc
            raise e

    def close(self):
        if getattr(self, "_g", None) is not None and self._g.value:
            self.lib.srt_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_skybox(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32)
        self._check(self.lib.srt_group_set_skybox(self._g, _ptr(rgba), rgba.shape[1], rgba.shape[0]))

    def set_acceleration(self, mode):
        self._check(self.lib.srt_group_set_acceleration(self._g, int(mode)))

    def set_acceleration_refit(self, mode):
        """Tracer.set_acceleration_refit on every member."""
        self._check(self.lib.srt_group_set_acceleration_refit(self._g, int(mode)))

    def set_acceleration_deform(self, mode, rebuild_ratio=0.0):
        """Tracer.set_acceleration_deform on every member."""
        self._check(self.lib.srt_group_set_acceleration_deform(self._g, int(mode), float(rebuild_ratio)))

    def set_acceleration_build(self, mode, min_triangles=0):
        """Tracer.set_acceleration_build on every member."""
        self._check(self.lib.srt_group_set_acceleration_build(self._g, int(mode), int(min_triangles)))

    def set_acceleration_build_order(self, order):
        """Tracer.set_acceleration_build_order on every member."""
        self._check(self.lib.srt_group_set_acceleration_build_order(self._g, int(order)))

    def member_build_info(self, i):
        """Tracer.acceleration_build_info of member i."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.srt_acceleration_build_info(self.member(i), out))
        return dict(zip(("models", "records", "launches"), (int(v) for v in out)))

    def member_deform_info(self, i):
        """Tracer.acceleration_deform_info of member i."""
        out, worst = (C.c_uint64 * 4)(), C.c_double(0)
        self._check(self.lib.srt_acceleration_deform_info(self.member(i), out, C.byref(worst)))
        return {"models_kept": int(out[0]), "models_rebuilt": int(out[1]), "cost_launches": int(out[2]), "worst_ratio": worst.value}

    def set_textures(self, images):
        keep, descs = _texture_descs(images)
        self._check(self.lib.srt_group_set_textures(self._g, descs if keep else None, len(keep)))

    def set_material_textures(self, bindings):
        b = R.as_records(bindings if bindings is not None else [], R.MATERIAL_TEXTURE)
        self._check(self.lib.srt_group_set_material_textures(self._g, _ptr(b) if len(b) else None, len(b)))

    def set_triangle_uvs(self, uv):
        uv, n = _uv_array(uv)
        self._check(self.lib.srt_group_set_triangle_uvs(self._g, _ptr(uv) if uv is not None else None, n))

    def set_triangle_materials(self, materials):
        tm = _tm_array(materials)
        self._check(self.lib.srt_group_set_triangle_materials(self._g, _ptr(tm) if tm is not None else None, 0 if tm is None else len(tm)))

    def update_scene(self, shapes, triangles, materials):
        shapes = R.as_records(shapes, R.SHAPE)
        triangles = R.as_records(triangles, R.TRIANGLE)
        materials = R.as_records(materials, R.MATERIAL)
        sd = R.as_records(self.scene_data, R.SCENE_DATA)
        self._check(self.lib.srt_group_update_scene(self._g, _ptr(shapes), len(shapes), _ptr(triangles), len(triangles), _ptr(materials),
                                                    len(materials), _ptr(sd)))
        self.scene_data["num_shapes"] = len(shapes)

    def clear_canvas(self):
        self._check(self.lib.srt_group_clear_canvas(self._g))

    def render(self, ticks_stopped, output=None):
        if output is None:
            output = np.zeros(self.height * self.width * 4, np.uint8)
        rd = R.as_records(self.options, R.RENDER_DATA)
        self._check(self.lib.srt_group_render(self._g, _ptr(rd), ticks_stopped, _ptr(output)))
        return output

    def read_canvas(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self.lib.srt_group_read_canvas(self._g, _ptr(out)))
        return out

    def counters(self):
        c = Counters()
        self._check(self.lib.srt_group_get_counters(self._g, C.byref(c)))
        return c.as_dict()

    # -- the denoiser on the group (srt_group_set_denoise): set_denoise, set_denoise_temporal, reset_denoise_history,
    # resolve_denoised, read_denoised, read_denoise_inputs, read_denoise_history are _Denoise's, on the whole frame --
    def _dn(self, name, *args):
        return getattr(self.lib, "srt_group_" + name)(self._g, *args)

    def trace_and_gather(self):
        """Trace on every member, collect and unpermute on the first device; asynchronous (then resolve_denoised)."""
        rd = R.as_records(self.options, R.RENDER_DATA)
        self._check(self.lib.srt_group_trace_and_gather(self._g, _ptr(rd)))

    def read_ao_view(self):
        """(height, width, 4) uint8: the grey picture resolve_ao_view wrote on the first device. Waits for its stream."""
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(self.lib.srt_group_read_ao_view(self._g, _ptr(out)))
        return out

    def read_noise_view(self):
        """(height, width, 4) uint8: the heat map resolve_noise_view wrote on the first device. Waits for its stream."""
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(self.lib.srt_group_read_noise_view(self._g, _ptr(out)))
        return out

    def member(self, i):
        """The srt_tracer handle of member i (ctypes void pointer; owned by the group)."""
        return C.c_void_p(self.lib.srt_group_tracer(self._g, i))


# ---- pure-host partition helpers (no GPU) ------------------------------------------
def owned_rows(height, rank, world, rows_per_block):
    return load_library().srt_partition_owned_rows(height, rank, world, rows_per_block)


def padded_rows(height, world, rows_per_block):
    return load_library().srt_partition_padded_rows(height, world, rows_per_block)


def global_row(height, rank, world, rows_per_block, local_row):
    return load_library().srt_partition_global_row(height, rank, world, rows_per_block, local_row)


def unpermute(gathered, height, world, rows_per_block):
    """gathered: (world*padded_rows, ...) array, rank-major -> (height, ...) image."""
    g = np.ascontiguousarray(gathered)
    row_bytes = g.strides[0]
    out = np.zeros((height,) + g.shape[1:], g.dtype)
    rc = load_library().srt_partition_unpermute(_ptr(g), _ptr(out), height, world, rows_per_block, row_bytes)
    if rc:
        raise SrtError("srt_partition_unpermute failed")
    return out

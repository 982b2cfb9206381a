"""The C-ABI of include/gmupt.h as ctypes sees it: constants, structures, numpy views of the records, GmuptError and the SYMBOLS table."""
import ctypes as C

import numpy as np

MAX_LIGHTS = 128
PATHCOUNT = 1 << 21
REF_GRID_THREADS = 34 * 8 * 256
STATE_BYTES = 248

(BUFFER_BVH_NODES, BUFFER_TRIANGLES, BUFFER_VERTICES, BUFFER_LIGHTS, BUFFER_TRI_PROPS, BUFFER_MATERIALS, BUFFER_TEXTURE_ARRAY) = range(7)
STAGE_SHADE, STAGE_EXTEND, STAGE_SHADOW, STAGE_RAYCASTS = range(4)
MATERIAL_UE4, MATERIAL_GLASS = 0, 1

# numpy views of the reference PODs (sizes asserted below)
bvh_node_dtype = np.dtype([("min", "<f4", 3), ("pad0", "<f4"), ("max", "<f4", 3), ("pad1", "<f4"),
                           ("left", "<i4"), ("right", "<i4"), ("isLeaf", "<i4"), ("pad2", "<f4")])
triangle_dtype = np.dtype([("v", "<i4", 3), ("materialID", "<u4")])
tri_props_dtype = np.dtype([("normal", "<f4", 3), ("pad0", "<f4"), ("uv", "<f4", 2), ("materialID", "<u4"), ("pad1", "<f4")])
light_dtype = np.dtype([("position", "<f4", 3), ("falloff", "<f4"), ("emission", "<f4", 3), ("radius", "<f4")])
material_dtype = np.dtype([("color", "<f4", 4), ("metallic", "<f4"), ("roughness", "<f4"), ("refractIndex", "<f4"),
                           ("transmittance", "<f4"), ("textureIndices", "<i4", 3), ("materialType", "<u4")])
assert bvh_node_dtype.itemsize == 48 and triangle_dtype.itemsize == 16 and tri_props_dtype.itemsize == 32
assert light_dtype.itemsize == 32 and material_dtype.itemsize == 48


def _info_dict(s):
    """The fields of an info structure, but its padding, as a dict of Python values (an array field as a list)."""
    out = {}
    for n, _ in s._fields_:
        if n != "pad":
            v = getattr(s, n)
            out[n] = list(v) if hasattr(v, "__len__") else v
    return out


class _AsDict:   # as_dict() of the info structures that have one (no docstring: a structure without one would inherit it)
    def as_dict(self):
        return _info_dict(self)


class CameraBuffer(C.Structure):
    _fields_ = [("position", C.c_float * 4), ("upperLeftCorner", C.c_float * 4), ("horizontal", C.c_float * 4),
                ("vertical", C.c_float * 4), ("pixelSize", C.c_float * 2), ("randomSeed", C.c_float * 2),
                ("envColor", C.c_float * 4), ("iterationCounter", C.c_int32), ("lightCount", C.c_uint32),
                ("sampleLights", C.c_uint32), ("pad_", C.c_uint32)]


assert C.sizeof(CameraBuffer) == 112


class RendererDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("pool_paths", C.c_uint32), ("live_paths", C.c_uint32),
                ("tile_enabled", C.c_uint32), ("tile_x0", C.c_uint32), ("tile_y0", C.c_uint32),
                ("path_budget", C.c_uint32), ("max_depth", C.c_uint32), ("collect_stats", C.c_uint32)]


STAT_STACK_OVERFLOW, STAT_FUSED_CAST, STAT_CAST_FETCH, STAT_STACK_SPILL, STAT_CAST_ABORTED, STAT_CAST_WIDE = 1, 2, 4, 8, 16, 32


class Stats(_AsDict, C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("paths_generated", C.c_uint64), ("paths_completed", C.c_uint64),
                ("segments", C.c_uint64), ("active_paths", C.c_uint32), ("flags", C.c_uint32),
                ("ext_rays", C.c_uint64), ("ext_inner", C.c_uint64), ("ext_leaves", C.c_uint64), ("ext_tris", C.c_uint64),
                ("sh_rays", C.c_uint64), ("sh_inner", C.c_uint64), ("sh_leaves", C.c_uint64), ("sh_tris", C.c_uint64),
                ("ms_logic", C.c_double), ("ms_scan", C.c_double), ("ms_accumulate", C.c_double), ("ms_material", C.c_double),
                ("ms_extend", C.c_double), ("ms_shadow", C.c_double), ("timed_iterations", C.c_uint64),
                ("ext_wave_inner", C.c_uint64), ("ext_wave_tris", C.c_uint64), ("sh_wave_inner", C.c_uint64), ("sh_wave_tris", C.c_uint64), ("ext_depth_hist", C.c_uint64 * 32),
                ("lane_census", C.c_uint64 * 4), ("cast_waves", C.c_uint64), ("cast_wave_ticks", C.c_uint64), ("cast_wave_ticks_max", C.c_uint64),
                ("cast_drain_ticks", C.c_uint64), ("cast_drain_iters", C.c_uint64), ("cast_drain_busy_lanes", C.c_uint64),
                ("cast_wave_end_hist", C.c_uint64 * 32), ("ray_inner_hist", C.c_uint64 * 32),
                ("ext_top_inner", C.c_uint64), ("sh_top_inner", C.c_uint64), ("cast_helper_subtrees", C.c_uint64),
                ("cast_nested_helpers", C.c_uint64), ("cast_redo_rays", C.c_uint64), ("wide_nodes", C.c_uint64), ("wide_top_nodes", C.c_uint64), ("wide_stack_bound", C.c_uint64), ("wide_pairs", C.c_uint64), ("wide_pair_fetches", C.c_uint64), ("wide_box_tests", C.c_uint64),
                ("wide_iterations", C.c_uint64), ("wide_general_iterations", C.c_uint64)]


class SbvhParams(C.Structure):
    _fields_ = [("split_alpha", C.c_float), ("max_depth", C.c_int32), ("max_spatial_depth", C.c_int32),
                ("min_leaf_size", C.c_int32), ("max_leaf_size", C.c_int32), ("node_cost", C.c_float), ("tri_cost", C.c_float)]


ERR_INVALID_ARGUMENT, ERR_HIP, ERR_OUT_OF_MEMORY, ERR_NOT_BOUND, ERR_UNSUPPORTED, ERR_IO, ERR_CAST_FAULT = -1, -2, -3, -4, -5, -6, -7
MAX_TRACE_BATCH = 1 << 26   # rays per batch of gmupt_trace_rays


class Ray(C.Structure):
    """gmupt_ray: 32 bytes; a (N, 8) float32 tensor holds N of them (origin xyz, tmax, direction xyz, pad)."""
    _fields_ = [("origin", C.c_float * 3), ("tmax", C.c_float), ("direction", C.c_float * 3), ("pad", C.c_uint32)]


class Hit(C.Structure):
    """gmupt_hit: 32 bytes (t, u, v, triangle, light, material, pad[2])."""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle", C.c_int32), ("light", C.c_uint32),
                ("material", C.c_uint32), ("pad", C.c_uint32 * 2)]


class TraceInfo(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("pad_", C.c_uint32), ("redo_rays", C.c_uint64), ("ms", C.c_double)]


class Aov(C.Structure):
    """gmupt_aov: 64 bytes per pixel (albedo, depth, normal, roughness, position, metallic, triangle, material, light, coverage)."""
    _fields_ = [("albedo", C.c_float * 3), ("depth", C.c_float), ("normal", C.c_float * 3), ("roughness", C.c_float),
                ("position", C.c_float * 3), ("metallic", C.c_float), ("triangle", C.c_int32), ("material", C.c_uint32),
                ("light", C.c_uint32), ("coverage", C.c_uint32)]


AOV_MAX_SAMPLES = 8
AOV_CHUNK_RAYS = 1 << 21   # rays per chunk of gmupt_render_aovs
assert C.sizeof(Ray) == 32 and C.sizeof(Hit) == 32 and C.sizeof(TraceInfo) == 24 and C.sizeof(Aov) == 64
ray_dtype = np.dtype([("origin", "<f4", 3), ("tmax", "<f4"), ("direction", "<f4", 3), ("pad", "<u4")])
hit_dtype = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("triangle", "<i4"), ("light", "<u4"), ("material", "<u4"), ("pad", "<u4", 2)])
aov_dtype = np.dtype([("albedo", "<f4", 3), ("depth", "<f4"), ("normal", "<f4", 3), ("roughness", "<f4"), ("position", "<f4", 3),
                      ("metallic", "<f4"), ("triangle", "<i4"), ("material", "<u4"), ("light", "<u4"), ("coverage", "<u4")])
assert ray_dtype.itemsize == 32 and hit_dtype.itemsize == 32 and aov_dtype.itemsize == 64


class DenoiseParams(C.Structure):
    """gmupt_denoise_params: 20 bytes (passes 1..5; every sigma finite and > 0)."""
    _fields_ = [("passes", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("sigma_albedo", C.c_float)]


DENOISE_MAX_PASSES = 5
assert C.sizeof(DenoiseParams) == 20


class TemporalParams(C.Structure):
    """gmupt_temporal_params: 32 bytes (the spatial filter's parameters, then history_cap, min_normal_cos, plane_dist)."""
    _fields_ = [("spatial", DenoiseParams), ("history_cap", C.c_float), ("min_normal_cos", C.c_float), ("plane_dist", C.c_float)]


TEMPORAL_MAX_CAP = 65536.0
assert C.sizeof(TemporalParams) == 32


class InfillParams(C.Structure):
    """gmupt_infill_params: 16 bytes (passes 1..8; every sigma finite and > 0)."""
    _fields_ = [("passes", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("sigma_albedo", C.c_float)]


class InfillInfo(_AsDict, C.Structure):
    """gmupt_infill_info: 24 bytes (surface pixels with / without a sample, holes filled / left open, device time)."""
    _fields_ = [("sources", C.c_uint32), ("holes", C.c_uint32), ("filled", C.c_uint32), ("open_left", C.c_uint32), ("ms", C.c_double)]


INFILL_MAX_PASSES = 8
PREVIEW_MOTION = 1
assert C.sizeof(InfillParams) == 16 and C.sizeof(InfillInfo) == 24
# gmupt_history: the integrated unfiltered colour, its effective sample count and the guides of one pixel (48 bytes)
history_dtype = np.dtype([("color", "<f4", 3), ("count", "<f4"), ("normal", "<f4", 3), ("material", "<u4"), ("position", "<f4", 3),
                          ("valid", "<u4")])
assert history_dtype.itemsize == 48
# gmupt_motion: where the pixel's surface point was in the previous vertex pose; flags = 1 on a triangle hit without a nearer light (16 bytes)
motion_dtype = np.dtype([("prev_position", "<f4", 3), ("flags", "<u4")])
assert motion_dtype.itemsize == 16


class RefitInfo(C.Structure):
    """gmupt_refit_info: 24 bytes."""
    _fields_ = [("rebuilt", C.c_uint32), ("reason", C.c_uint32), ("levels", C.c_uint32), ("opened_nodes", C.c_uint32), ("ms", C.c_double)]


REFIT_FLAT_CHILD, REFIT_VARIANTS_BUILD = 1, 2
assert C.sizeof(RefitInfo) == 24


class LbvhParams(C.Structure):
    """gmupt_lbvh_params."""
    _fields_ = [("max_leaf_size", C.c_uint32)]


class LbvhInfo(C.Structure):
    """gmupt_lbvh_info: 48 bytes."""
    _fields_ = [("num_nodes", C.c_uint32), ("num_leaves", C.c_uint32), ("depth", C.c_uint32), ("num_tris", C.c_uint32),
                ("root_min", C.c_float * 3), ("root_max", C.c_float * 3), ("ms", C.c_double)]

    def as_dict(self):
        out = _info_dict(self)
        out["root_min"], out["root_max"] = np.array(self.root_min[:], np.float32), np.array(self.root_max[:], np.float32)
        return out


assert C.sizeof(LbvhInfo) == 48


class NormalsInfo(C.Structure):
    """gmupt_normals_info: 24 bytes."""
    _fields_ = [("num_verts", C.c_uint32), ("num_tris", C.c_uint32), ("max_valence", C.c_uint32), ("pad", C.c_uint32), ("ms", C.c_double)]


assert C.sizeof(NormalsInfo) == 24


class PoseInfo(C.Structure):
    """gmupt_pose_info: 16 bytes."""
    _fields_ = [("num_verts", C.c_uint32), ("active_targets", C.c_uint32), ("ms", C.c_double)]


assert C.sizeof(PoseInfo) == 16


class TreeCostInfo(_AsDict, C.Structure):
    """gmupt_tree_cost_info: 64 bytes."""
    _fields_ = [("sum_inner", C.c_double), ("sum_leaf", C.c_double), ("num_inner", C.c_uint32), ("num_leaves", C.c_uint32),
                ("num_refs", C.c_uint64), ("max_leaf_refs", C.c_uint32), ("pad", C.c_uint32), ("root_half_area", C.c_double),
                ("sah", C.c_double), ("ms", C.c_double)]


assert C.sizeof(TreeCostInfo) == 64


class TreeoptParams(C.Structure):
    """gmupt_treeopt_params."""
    _fields_ = [("passes", C.c_uint32)]


class TreeoptInfo(_AsDict, C.Structure):
    """gmupt_treeopt_info: 40 bytes."""
    _fields_ = [("num_nodes", C.c_uint32), ("depth_before", C.c_uint32), ("depth_after", C.c_uint32), ("treelets_rewritten", C.c_uint32),
                ("cost_before", C.c_double), ("cost_after", C.c_double), ("ms", C.c_double)]


assert C.sizeof(TreeoptInfo) == 40


class ConvergeParams(C.Structure):
    """gmupt_converge_params: 12 bytes (threshold not a NaN; min_batches >= 2)."""
    _fields_ = [("threshold", C.c_float), ("min_batches", C.c_uint32), ("allow_pixels", C.c_uint32)]


class ConvergeInfo(C.Structure):
    """gmupt_converge_info: 56 bytes."""
    _fields_ = [("pixels", C.c_uint32), ("unsampled", C.c_uint32), ("known", C.c_uint32), ("nonfinite", C.c_uint32), ("below", C.c_uint32),
                ("converged", C.c_uint32), ("max_error", C.c_float), ("pad", C.c_uint32), ("sum_error", C.c_double), ("mean_error", C.c_double),
                ("ms", C.c_double)]

    def as_dict(self):
        out = _info_dict(self)
        out["converged"] = bool(self.converged)
        return out


converge_pixel_dtype = np.dtype([("n", "<u4"), ("k", "<u4"), ("w", "<u4"), ("pad", "<u4"), ("s", "<f8"), ("mean", "<f8"), ("m2", "<f8")])
assert C.sizeof(ConvergeParams) == 12 and C.sizeof(ConvergeInfo) == 56 and converge_pixel_dtype.itemsize == 40

# Prototypes of the feature modules that keep their own part of the ABI (adaptive.py): name -> (restype, argtypes), bound by _lib with
# SYMBOLS on every load.  A module adds its entries when it is imported, which the package does before any library is loaded.
_EXTRA_SYMBOLS = {}

# the `which` of gmupt_debug_travtables_data / gmupt_debug_read_travtable, in order
TRAVTABLE_KINDS = ("node64", "tri48", "tripair", "pair_ref", "wnode", "rec64", "scalars", "level_nodes", "level_off", "node_map", "wide_map", "opened")


class GmuptError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


# every symbol include/gmupt.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "gmupt_device_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "gmupt_device_destroy": (None, [_P]),
    "gmupt_last_error": (C.c_char_p, []),
    "gmupt_device_count": (C.c_int, []),
    "gmupt_buffer_create": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.POINTER(_P)]),
    "gmupt_buffer_update": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_buffer_read": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_buffer_destroy": (None, [_P]),
    "gmupt_buffer_size": (C.c_size_t, [_P]),
    "gmupt_texture_array_create": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "gmupt_image_decode_png": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_P)]),
    "gmupt_image_free": (None, [_P]),
    "gmupt_image_resize_square": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "gmupt_texture_common_size": (C.c_uint32, [C.POINTER(C.c_size_t), C.c_uint32]),
    "gmupt_renderer_create": (C.c_int, [_P, C.POINTER(RendererDesc), C.POINTER(_P)]),
    "gmupt_renderer_destroy": (None, [_P]),
    "gmupt_renderer_bind_scene": (C.c_int, [_P] * 7),
    "gmupt_renderer_bind_textures": (C.c_int, [_P, _P, _P, _P]),
    "gmupt_set_camera": (C.c_int, [_P, C.POINTER(CameraBuffer)]),
    "gmupt_iterate": (C.c_int, [_P]),
    "gmupt_resize": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "gmupt_read_framebuffer": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_copy_framebuffer_to_device": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_get_counters": (C.c_int, [_P, C.POINTER(C.c_uint32 * 8)]),
    "gmupt_synchronize": (C.c_int, [_P]),
    "gmupt_get_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "gmupt_reset_stats": (C.c_int, [_P]),
    "gmupt_enable_timing": (C.c_int, [_P, C.c_int]),
    "gmupt_render_budget": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gmupt_trace_rays": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(TraceInfo)]),
    "gmupt_camera_pick_ray": (C.c_int, [C.POINTER(CameraBuffer), C.c_float, C.c_float, C.POINTER(Ray)]),
    "gmupt_pick": (C.c_int, [_P, C.c_float, C.c_float, C.c_uint32, C.POINTER(Ray), C.POINTER(Hit)]),
    "gmupt_render_aovs": (C.c_int, [_P, C.c_uint32, _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_aov_ray": (C.c_int, [C.POINTER(CameraBuffer), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Ray)]),
    "gmupt_denoise_default_params": (None, [C.POINTER(DenoiseParams)]),
    "gmupt_denoise_image": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), _P, C.c_size_t, C.POINTER(C.c_float)]),
    "gmupt_render_denoised": (C.c_int, [_P, C.c_uint32, C.POINTER(DenoiseParams), _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_denoise_host": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), _P, C.c_size_t, C.c_uint32]),
    "gmupt_infill_default_params": (None, [C.POINTER(InfillParams)]),
    "gmupt_infill_image": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.POINTER(InfillParams), _P, C.c_size_t, C.POINTER(InfillInfo)]),
    "gmupt_infill_host": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(InfillParams), _P, C.c_size_t, C.POINTER(InfillInfo), C.c_uint32]),
    "gmupt_temporal_preview_image": (C.c_int, [_P, _P, _P, _P, C.POINTER(CameraBuffer), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                               C.POINTER(TemporalParams), C.POINTER(InfillParams), _P, C.c_size_t, C.POINTER(C.c_float)]),
    "gmupt_render_preview": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), C.POINTER(InfillParams), _P, C.c_size_t,
                                       C.POINTER(TraceInfo)]),
    "gmupt_temporal_default_params": (None, [C.POINTER(TemporalParams)]),
    "gmupt_temporal_create": (C.c_int, [_P, C.POINTER(_P)]),
    "gmupt_temporal_destroy": (None, [_P]),
    "gmupt_temporal_reset": (C.c_int, [_P]),
    "gmupt_temporal_denoise_image": (C.c_int, [_P, _P, _P, C.POINTER(CameraBuffer), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                               C.POINTER(TemporalParams), _P, C.c_size_t, C.POINTER(C.c_float)]),
    "gmupt_render_denoised_temporal": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(TemporalParams), _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_temporal_integrate_host": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.POINTER(CameraBuffer), C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), _P, _P, C.c_uint32]),
    "gmupt_bvh_refit_host": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32]),
    "gmupt_renderer_refit": (C.c_int, [_P, C.POINTER(RefitInfo)]),
    "gmupt_render_aovs_motion": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_motion_host": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32, _P, _P, C.c_uint32, _P]),
    "gmupt_temporal_integrate_motion_host": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, C.POINTER(CameraBuffer), C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), _P, _P, C.c_uint32]),
    "gmupt_temporal_denoise_image_motion": (C.c_int, [_P, _P, _P, _P, C.POINTER(CameraBuffer), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                                      C.POINTER(TemporalParams), _P, C.c_size_t, C.POINTER(C.c_float)]),
    "gmupt_render_denoised_temporal_motion": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(TemporalParams), _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_lbvh_default_params": (None, [C.POINTER(LbvhParams)]),
    "gmupt_lbvh_build_host": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.POINTER(LbvhParams), _P, _P, _P, C.POINTER(LbvhInfo)]),
    "gmupt_lbvh_create": (C.c_int, [_P, C.POINTER(_P)]),
    "gmupt_lbvh_destroy": (None, [_P]),
    "gmupt_lbvh_build": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.POINTER(LbvhParams), C.POINTER(_P), C.POINTER(_P), _P, C.POINTER(LbvhInfo)]),
    "gmupt_vertex_normals_host": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32]),
    "gmupt_normals_create": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "gmupt_normals_update": (C.c_int, [_P, C.POINTER(NormalsInfo)]),
    "gmupt_normals_destroy": (None, [_P]),
    "gmupt_buffer_update_device": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_tree_cost_host": (C.c_int, [_P, C.c_uint32, C.POINTER(TreeCostInfo), C.c_uint32]),
    "gmupt_renderer_tree_cost": (C.c_int, [_P, _P, C.POINTER(TreeCostInfo)]),
    "gmupt_treeopt_default_params": (None, [C.POINTER(TreeoptParams)]),
    "gmupt_tree_optimize_host": (C.c_int, [_P, C.c_uint32, C.POINTER(TreeoptParams), _P, C.POINTER(TreeoptInfo)]),
    "gmupt_treeopt_create": (C.c_int, [_P, C.POINTER(_P)]),
    "gmupt_treeopt_destroy": (None, [_P]),
    "gmupt_treeopt_run": (C.c_int, [_P, _P, C.POINTER(TreeoptParams), C.POINTER(_P), C.POINTER(TreeoptInfo)]),
    "gmupt_pose_host": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32]),
    "gmupt_pose_create": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(_P)]),
    "gmupt_pose_update": (C.c_int, [_P, _P, _P, C.POINTER(PoseInfo)]),
    "gmupt_pose_update_device": (C.c_int, [_P, _P, _P, C.POINTER(PoseInfo)]),
    "gmupt_pose_destroy": (None, [_P]),
    "gmupt_converge_default_params": (None, [C.POINTER(ConvergeParams)]),
    "gmupt_converge_host": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(ConvergeParams), _P, C.POINTER(ConvergeInfo)]),
    "gmupt_converge_create": (C.c_int, [_P, C.POINTER(_P)]),
    "gmupt_converge_destroy": (None, [_P]),
    "gmupt_converge_reset": (C.c_int, [_P]),
    "gmupt_converge_update": (C.c_int, [_P, C.POINTER(ConvergeParams), _P, C.POINTER(ConvergeInfo)]),
    "gmupt_converge_update_image": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(ConvergeParams), _P, C.POINTER(ConvergeInfo)]),
    "gmupt_converge_read_state": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_render_until": (C.c_int, [_P, _P, _P, C.POINTER(ConvergeParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(ConvergeInfo)]),
    "gmupt_debug_read_path_state": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_debug_write_path_state": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_debug_read_queues": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_debug_write_queues": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_debug_write_counters": (C.c_int, [_P, C.POINTER(C.c_uint32 * 8)]),
    "gmupt_debug_write_framebuffer": (C.c_int, [_P, _P, C.c_size_t]),
    "gmupt_debug_run_stage": (C.c_int, [_P, C.c_int]),
    "gmupt_debug_detmath": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_uint32]),
    "gmupt_debug_travtables_build": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "gmupt_debug_travtables_data": (_P, [_P, C.c_int, C.POINTER(C.c_size_t)]),
    "gmupt_debug_travtables_destroy": (None, [_P]),
    "gmupt_debug_read_travtable": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "gmupt_debug_wide_tables_addressable": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "gmupt_sbvh_default_params": (None, [C.POINTER(SbvhParams)]),
    "gmupt_sbvh_build": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(SbvhParams), C.POINTER(_P)]),
    "gmupt_sbvh_num_nodes": (C.c_uint32, [_P]),
    "gmupt_sbvh_num_references": (C.c_uint32, [_P]),
    "gmupt_sbvh_sah": (C.c_float, [_P]),
    "gmupt_sbvh_depth": (C.c_uint32, [_P]),
    "gmupt_sbvh_flatten": (C.c_int, [_P, _P, _P, _P, _P]),
    "gmupt_sbvh_destroy": (None, [_P]),
    "gmupt_camera_create": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "gmupt_camera_destroy": (None, [_P]),
    "gmupt_camera_update_resolution": (None, [_P, C.c_uint32, C.c_uint32]),
    "gmupt_camera_set_pose": (None, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "gmupt_camera_update": (None, [_P, C.c_float]),
    "gmupt_camera_set_input": (None, [_P, C.c_float, C.c_float, C.c_uint32]),
    "gmupt_camera_reset_accumulation": (None, [_P]),
    "gmupt_camera_get_buffer": (C.POINTER(CameraBuffer), [_P]),
    "gmupt_version": (C.c_char_p, []),
}

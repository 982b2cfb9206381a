"""ctypes binding of libgmupt.so -- the binding a Python host would add on top of include/gmupt.h.

This is plumbing only: every call goes straight to the C-ABI, there is no CPU fallback.  If the HIP
library is missing or a HIP call fails, GmuptError is raised with gmupt_last_error().
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

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


class Stats(C.Structure):
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

    def as_dict(self):
        return {n: (list(getattr(self, n)) if hasattr(getattr(self, n), "__len__") else getattr(self, n)) for n, _ in self._fields_}


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


class InfillInfo(C.Structure):
    """gmupt_infill_info: 24 bytes (surface pixels with / without a sample, holes filled / left open, device time)."""
    _fields_ = [("sources", C.c_uint32), ("holes", C.c_uint32), ("filled", C.c_uint32), ("open_left", C.c_uint32), ("ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


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
        return {"num_nodes": int(self.num_nodes), "num_leaves": int(self.num_leaves), "depth": int(self.depth), "num_tris": int(self.num_tris),
                "root_min": np.array(self.root_min[:], np.float32), "root_max": np.array(self.root_max[:], np.float32), "ms": float(self.ms)}


assert C.sizeof(LbvhInfo) == 48


class NormalsInfo(C.Structure):
    """gmupt_normals_info: 24 bytes."""
    _fields_ = [("num_verts", C.c_uint32), ("num_tris", C.c_uint32), ("max_valence", C.c_uint32), ("pad", C.c_uint32), ("ms", C.c_double)]


assert C.sizeof(NormalsInfo) == 24


class PoseInfo(C.Structure):
    """gmupt_pose_info: 16 bytes."""
    _fields_ = [("num_verts", C.c_uint32), ("active_targets", C.c_uint32), ("ms", C.c_double)]


assert C.sizeof(PoseInfo) == 16


class TreeCostInfo(C.Structure):
    """gmupt_tree_cost_info: 64 bytes."""
    _fields_ = [("sum_inner", C.c_double), ("sum_leaf", C.c_double), ("num_inner", C.c_uint32), ("num_leaves", C.c_uint32),
                ("num_refs", C.c_uint64), ("max_leaf_refs", C.c_uint32), ("pad", C.c_uint32), ("root_half_area", C.c_double),
                ("sah", C.c_double), ("ms", C.c_double)]

    def as_dict(self):
        return {"sum_inner": float(self.sum_inner), "sum_leaf": float(self.sum_leaf), "num_inner": int(self.num_inner),
                "num_leaves": int(self.num_leaves), "num_refs": int(self.num_refs), "max_leaf_refs": int(self.max_leaf_refs),
                "root_half_area": float(self.root_half_area), "sah": float(self.sah), "ms": float(self.ms)}


assert C.sizeof(TreeCostInfo) == 64


class TreeoptParams(C.Structure):
    """gmupt_treeopt_params."""
    _fields_ = [("passes", C.c_uint32)]


class TreeoptInfo(C.Structure):
    """gmupt_treeopt_info: 40 bytes."""
    _fields_ = [("num_nodes", C.c_uint32), ("depth_before", C.c_uint32), ("depth_after", C.c_uint32), ("treelets_rewritten", C.c_uint32),
                ("cost_before", C.c_double), ("cost_after", C.c_double), ("ms", C.c_double)]

    def as_dict(self):
        return {"num_nodes": int(self.num_nodes), "depth_before": int(self.depth_before), "depth_after": int(self.depth_after),
                "treelets_rewritten": int(self.treelets_rewritten), "cost_before": float(self.cost_before), "cost_after": float(self.cost_after),
                "ms": float(self.ms)}


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
        return {"pixels": int(self.pixels), "unsampled": int(self.unsampled), "known": int(self.known), "nonfinite": int(self.nonfinite),
                "below": int(self.below), "converged": bool(self.converged), "max_error": float(self.max_error),
                "sum_error": float(self.sum_error), "mean_error": float(self.mean_error), "ms": float(self.ms)}


converge_pixel_dtype = np.dtype([("n", "<u4"), ("k", "<u4"), ("w", "<u4"), ("pad", "<u4"), ("s", "<f8"), ("mean", "<f8"), ("m2", "<f8")])
assert C.sizeof(ConvergeParams) == 12 and C.sizeof(ConvergeInfo) == 56 and converge_pixel_dtype.itemsize == 40


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

_lib = None
_libs = {}
_devices_created = 0   # gmupt_device_create calls of this process (a process that uses the GPU must not spawn a compiler)


def _load(path):
    if path not in _libs:
        handle = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _libs[path] = handle
    return _libs[path]


def lib():
    """Loads libgmupt.so (building it first if the sources are newer).  Fails loudly when it cannot."""
    global _lib
    if _lib is None:
        path = os.environ.get("GMUPT_LIB") or _build.LIB   # GMUPT_LIB: A/B timing of differently configured builds
        if not os.environ.get("GMUPT_LIB") and (not os.path.exists(path) or (os.path.exists("/opt/rocm/bin/hipcc") and _build.needs_build())):
            path = _build.build()
        _lib = _load(path)
    return _lib


class use_build:
    """Context manager: inside the block every call of this module goes to a test build of the same sources (build.TEST_BUILDS,
    e.g. "variants" = the library with the whole traversal ladder).  Objects created inside must be closed inside."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _lib
        path = _build.lib_path(self.name)
        if not os.path.exists(path) or (os.path.exists("/opt/rocm/bin/hipcc") and _build.needs_build(self.name)):
            if _devices_created:
                # a process that has initialised the GPU must not start hipcc (fork + exec): the GPU box refuses it.  __graft_entry__.build()
                # prebuilds every test build; a stale one is an error here, not something to repair on the fly
                raise GmuptError("test build %r is missing or older than its sources and this process already uses the GPU: run __graft_entry__.build() first" % self.name)
            path = _build.build(name=self.name)
        self.saved = lib()
        _lib = _load(path)
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.saved
        return False


def _check(rc):
    if rc != 0:
        raise GmuptError("gmupt error %d: %s" % (rc, lib().gmupt_last_error().decode(errors="replace")), rc)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Device:
    def __init__(self, index=0):
        global _devices_created
        self.h = _P()
        _check(lib().gmupt_device_create(index, C.byref(self.h)))
        _devices_created += 1
        self.index = index

    def close(self):
        if self.h:
            lib().gmupt_device_destroy(self.h)
            self.h = _P()

    def detmath(self, fn, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float32)
        out = np.empty_like(x)
        _check(lib().gmupt_debug_detmath(self.h, fn, _ptr(x), _ptr(y), _ptr(out), x.size))
        return out


class Buffer:
    def __init__(self, dev, kind, array):
        array = np.ascontiguousarray(array)
        self.h = _P()
        self.dev = dev
        _check(lib().gmupt_buffer_create(dev.h, kind, _ptr(array), array.nbytes, C.byref(self.h)))

    @classmethod
    def wrap(cls, dev, handle):
        """A Buffer around a gmupt_buffer the library created (gmupt_lbvh_build); close() destroys it like any other."""
        self = cls.__new__(cls)
        self.h, self.dev = handle, dev
        return self

    def update(self, array):
        array = np.ascontiguousarray(array)
        _check(lib().gmupt_buffer_update(self.h, _ptr(array), array.nbytes))

    def update_from_device(self, tensor):
        """gmupt_buffer_update_device: the buffer's first bytes from a torch tensor on this buffer's GPU (e.g. a pose computed there),
        without a trip through the host.  torch's current stream is synchronised first."""
        import torch
        device = torch.device("cuda", getattr(self.dev, "index", 0))
        if not isinstance(tensor, torch.Tensor) or tensor.device != device or not tensor.is_contiguous():
            raise GmuptError("update_from_device: a contiguous tensor on %s" % device, ERR_INVALID_ARGUMENT)
        nbytes = tensor.numel() * tensor.element_size()
        if nbytes > int(lib().gmupt_buffer_size(self.h)):
            raise GmuptError("update_from_device: %d bytes into a %d-byte buffer" % (nbytes, int(lib().gmupt_buffer_size(self.h))), ERR_INVALID_ARGUMENT)
        torch.cuda.current_stream(device).synchronize()
        _check(lib().gmupt_buffer_update_device(self.h, C.c_void_p(tensor.data_ptr()), nbytes))

    def read(self, dtype=np.uint8):
        """The buffer's bytes as a new array of `dtype` (gmupt_buffer_read: synchronous)."""
        dtype = np.dtype(dtype)
        nbytes = int(lib().gmupt_buffer_size(self.h))
        out = np.empty(nbytes // dtype.itemsize, dtype=dtype)
        _check(lib().gmupt_buffer_read(self.h, _ptr(out), out.nbytes))
        return out

    def close(self):
        if self.h:
            lib().gmupt_buffer_destroy(self.h)
            self.h = _P()


class TextureArray:
    """R8G8B8A8_UNORM Texture2DArray: (layers, size, size, 4) uint8."""

    def __init__(self, dev, array):
        array = np.ascontiguousarray(array, dtype=np.uint8)
        assert array.ndim == 4 and array.shape[1] == array.shape[2] and array.shape[3] == 4
        self.h = _P()
        _check(lib().gmupt_texture_array_create(dev.h, _ptr(array), array.shape[1], array.shape[0], C.byref(self.h)))

    def close(self):
        if self.h:
            lib().gmupt_buffer_destroy(self.h)
            self.h = _P()


def decode_png(data):
    """PNG file bytes -> (h, w, 4) uint8 through gmupt_image_decode_png (the reference's lodepng::decode call, Scene.cpp:226)."""
    w, h, mem = C.c_uint32(), C.c_uint32(), _P()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    _check(lib().gmupt_image_decode_png(buf, len(data), C.byref(w), C.byref(h), C.byref(mem)))
    try:
        out = np.ctypeslib.as_array(C.cast(mem, C.POINTER(C.c_uint8)), shape=(h.value, w.value, 4)).copy()
    finally:
        lib().gmupt_image_free(mem)
    return out


def resize_square(rgba, new_size):
    """Square RGBA8 resize: the bytes of the reference's avir call (Scene.cpp:276-279; host/AvirResize.cpp restates avir's pipeline for it)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    assert rgba.ndim == 3 and rgba.shape[0] == rgba.shape[1] and rgba.shape[2] == 4
    out = np.empty((new_size, new_size, 4), dtype=np.uint8)
    _check(lib().gmupt_image_resize_square(_ptr(rgba), rgba.shape[0], new_size, _ptr(out)))
    return out


def texture_common_size(layer_bytes):
    arr = (C.c_size_t * len(layer_bytes))(*layer_bytes)
    return int(lib().gmupt_texture_common_size(arr, len(layer_bytes)))


def texture_array_from_png(files):
    """Layers from encoded PNG files in material order, as Scene::loadSpecificTexture + createTextures: decode, pick the common size by
    the median rule, resize the layers that differ.  Returns (layers, size, size, 4) uint8."""
    layers = [decode_png(f) for f in files]
    for l in layers:
        if l.shape[0] != l.shape[1]:
            raise GmuptError("texture is not square")
    size = texture_common_size([l.size for l in layers])
    return np.stack([l if l.shape[0] == size else resize_square(l, size) for l in layers])


class SceneBuffers:
    """The six scene resources of Renderer::draw (t0-t4, b1) uploaded through gmupt_buffer_create."""

    def __init__(self, dev, scene):
        self.nodes = Buffer(dev, BUFFER_BVH_NODES, scene["nodes"])
        self.tris = Buffer(dev, BUFFER_TRIANGLES, scene["tris"])
        self.verts = Buffer(dev, BUFFER_VERTICES, scene["verts"])
        self.lights = Buffer(dev, BUFFER_LIGHTS, scene["lights"])
        self.props = Buffer(dev, BUFFER_TRI_PROPS, scene["props"])
        self.materials = Buffer(dev, BUFFER_MATERIALS, scene["materials"])
        self.textures = [TextureArray(dev, scene[k]) if scene.get(k) is not None else None
                         for k in ("tex_diffuse", "tex_metallic_roughness", "tex_normal")]

    def all(self):
        return [self.nodes, self.tris, self.verts, self.lights, self.props, self.materials]

    def close(self):
        for b in self.all():
            b.close()
        for t in self.textures:
            if t is not None:
                t.close()


class Camera:
    """Host camera (gmupt_camera_*): Camera::update / setRotation / updateResolution of the reference."""

    def __init__(self, width, height):
        self.h = _P()
        _check(lib().gmupt_camera_create(width, height, C.byref(self.h)))

    def set_pose(self, x, y, z, pitch, yaw):
        lib().gmupt_camera_set_pose(self.h, x, y, z, pitch, yaw)

    def update(self, dt=0.0):
        lib().gmupt_camera_update(self.h, dt)

    def update_resolution(self, width, height):
        lib().gmupt_camera_update_resolution(self.h, width, height)

    def reset_accumulation(self):
        lib().gmupt_camera_reset_accumulation(self.h)

    def set_input(self, mouse_dx=0.0, mouse_dy=0.0, w=False, s=False, a=False, d=False):
        lib().gmupt_camera_set_input(self.h, mouse_dx, mouse_dy, (1 if w else 0) | (2 if s else 0) | (4 if a else 0) | (8 if d else 0))

    @property
    def buffer(self):
        return lib().gmupt_camera_get_buffer(self.h).contents

    def buffer_copy(self):
        out = CameraBuffer()
        C.memmove(C.byref(out), C.byref(self.buffer), C.sizeof(CameraBuffer))
        return out

    def close(self):
        if self.h:
            lib().gmupt_camera_destroy(self.h)
            self.h = _P()


class Renderer:
    def __init__(self, dev, width, height, pool_paths=0, live_paths=0, tile=None, path_budget=0, max_depth=0, collect_stats=False):
        d = RendererDesc(width, height, pool_paths, live_paths, 0, 0, 0, path_budget, max_depth, 1 if collect_stats else 0)
        if tile is not None:
            d.tile_enabled, d.tile_x0, d.tile_y0 = 1, tile[0], tile[1]
        self.desc = d
        self.dev = dev
        self.h = _P()
        _check(lib().gmupt_renderer_create(dev.h, C.byref(d), C.byref(self.h)))
        self.width, self.height = width, height
        self.pool = pool_paths or PATHCOUNT
        self._scene = None
        self._temporals = []   # history handles of this renderer: closed before it
        self._normals = []     # Normals handles of this renderer: closed before it
        self._poses = []       # Pose handles of this renderer: closed before it
        self._converges = []   # Converge handles of this renderer: closed before it

    def bind_scene(self, sb):
        self._scene = sb  # keep the buffers alive
        _check(lib().gmupt_renderer_bind_scene(self.h, *[b.h for b in sb.all()]))
        _check(lib().gmupt_renderer_bind_textures(self.h, *[(t.h if t is not None else None) for t in sb.textures]))

    def refit(self):
        """gmupt_renderer_refit after the vertex buffer was updated: the info fields as a dict."""
        info = RefitInfo()
        _check(lib().gmupt_renderer_refit(self.h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in RefitInfo._fields_}

    def tree_cost(self, nodes=None):
        """gmupt_renderer_tree_cost: the surface-area cost of a node buffer, computed where it lives (include/gmupt.h "Tree cost"), on the
        renderer's stream behind a preceding refit().  nodes=None: the node buffer the renderer is bound to; else any Buffer of kind
        BUFFER_BVH_NODES of this device, e.g. the one Lbvh.build just returned.  Returns the gmupt_tree_cost_info fields as a dict: sah,
        sum_inner, sum_leaf, root_half_area, num_inner, num_leaves, num_refs, max_leaf_refs and ms, the device time of the launches."""
        ti = TreeCostInfo()
        _check(lib().gmupt_renderer_tree_cost(self.h, nodes.h if nodes is not None else None, C.byref(ti)))
        return ti.as_dict()

    def set_camera(self, cam_buffer):
        _check(lib().gmupt_set_camera(self.h, C.byref(cam_buffer)))

    def iterate(self):
        _check(lib().gmupt_iterate(self.h))

    def run_stage(self, stage):
        _check(lib().gmupt_debug_run_stage(self.h, stage))

    def synchronize(self):
        _check(lib().gmupt_synchronize(self.h))

    def resize(self, w, h):
        _check(lib().gmupt_resize(self.h, w, h))
        self.width, self.height = w, h

    def framebuffer(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check(lib().gmupt_read_framebuffer(self.h, _ptr(out), out.nbytes))
        return out

    def copy_framebuffer_to_device(self, device_ptr, nbytes):
        _check(lib().gmupt_copy_framebuffer_to_device(self.h, C.c_void_p(device_ptr), nbytes))

    def counters(self):
        out = (C.c_uint32 * 8)()
        _check(lib().gmupt_get_counters(self.h, C.byref(out)))
        return np.array(list(out), dtype=np.uint32)

    def stats(self, check=True):
        """gmupt_get_stats.  A launch that flagged its results as invalid makes the call fail (GMUPT_ERR_CAST_FAULT) although the
        statistics are filled in: check=False returns them anyway (to look at the flags)."""
        s = Stats()
        rc = lib().gmupt_get_stats(self.h, C.byref(s))
        if rc != ERR_CAST_FAULT or check:
            _check(rc)
        return s

    def reset_stats(self):
        _check(lib().gmupt_reset_stats(self.h))

    def enable_timing(self, mode=1):
        _check(lib().gmupt_enable_timing(self.h, int(mode)))

    def render_budget(self, camera, max_iterations=1 << 20):
        it = C.c_uint32(0)
        _check(lib().gmupt_render_budget(self.h, camera.h, max_iterations, C.byref(it)))
        return it.value

    def converge(self):
        """A new convergence monitor of this renderer (Converge); closed with the renderer at the latest."""
        return Converge(self)

    def render_until(self, camera, converge, check_every=8, max_iterations=1 << 20, **params):
        """gmupt_render_until: the loop of render_budget with converge.update() after every check_every iterations; ends on `converged`
        or after max_iterations.  params: the converge_params fields (threshold, min_batches, allow_pixels).  Returns the last check's
        info dict (all zero when no check ran) with "iterations" added."""
        cp = converge_params(**params)
        it = C.c_uint32(0)
        ci = ConvergeInfo()
        _check(lib().gmupt_render_until(self.h, camera.h, converge.h, C.byref(cp), check_every, max_iterations, C.byref(it), C.byref(ci)))
        out = ci.as_dict()
        if out["pixels"]:                            # a check ran: the monitor holds the state of this frame
            converge._size = (self.height, self.width)
        out["iterations"] = it.value
        return out

    # ray queries (gmupt_trace_rays / gmupt_pick)
    def trace(self, closest=None, any=None, light_count=0, info=None):
        """Closest-hit and any-hit queries on caller rays in one launch (include/gmupt.h states the semantics).

        closest / any: (N, 8) float32 rays (origin xyz, tmax, direction xyz, pad) as torch tensors on this renderer's GPU, or numpy
        arrays (staged through a torch tensor on the GPU); None for an empty batch.  Returns (hits, occluded) of the kind given:
        hits (N, 8) float32 gmupt_hit records (hit_fields() splits them; words 3-7 are integers, compare them as bits), occluded (M,) int32 for torch / uint32 for numpy.  torch's
        current stream is synchronised first; the call itself synchronises the renderer's stream.  info: optional TraceInfo to fill."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        as_numpy = isinstance(closest, np.ndarray) or isinstance(any, np.ndarray)

        def stage(a):
            if a is None:
                return torch.empty((0, 8), dtype=torch.float32, device=dev)
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 8)).to(dev) if isinstance(a, np.ndarray) else a
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 8 or not t.is_cuda:
                raise GmuptError("trace: rays must be (N, 8) float32 on the GPU (or numpy)", ERR_INVALID_ARGUMENT)
            return t.contiguous()

        c, a = stage(closest), stage(any)
        hits = torch.empty((c.shape[0], 8), dtype=torch.float32, device=dev)
        occ = torch.empty((a.shape[0],), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        _check(lib().gmupt_trace_rays(self.h, ptr(c), c.shape[0], ptr(hits), ptr(a), a.shape[0], ptr(occ), int(light_count), C.byref(ti)))
        self.last_trace = ti
        if as_numpy:
            return hits.cpu().numpy(), occ.cpu().numpy().view(np.uint32)
        return hits, occ

    def pick(self, px, py, light_count=0):
        """gmupt_pick: (Ray, Hit) of the un-jittered primary ray through whole-frame pixel (px, py) of the current camera."""
        ray, hit = Ray(), Hit()
        _check(lib().gmupt_pick(self.h, float(px), float(py), int(light_count), C.byref(ray), C.byref(hit)))
        return ray, hit

    # AOV buffers (gmupt_render_aovs)
    def aovs(self, samples=1, info=None):
        """The per-pixel G-buffer of the current camera's rays over this renderer's framebuffer rectangle (the tile in tile mode):
        a (H, W, 16) float32 torch tensor on this renderer's GPU, one 64-byte gmupt_aov record per pixel (include/gmupt.h states the
        semantics; aov_fields() splits it -- words 12-15 are integers, compare them as bits).  samples: 1..8 (s*s stratified rays per pixel
        for the filtered albedo / normal planes when > 1).  torch's current stream is synchronised first; the call itself synchronises the
        renderer's stream.  info: optional TraceInfo to fill."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        out = torch.empty((self.height, self.width, 16), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(lib().gmupt_render_aovs(self.h, int(samples), C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(ti)))
        self.last_aovs = ti
        return out

    # motion plane (gmupt_render_aovs_motion)
    def aovs_motion(self, prev_verts, samples=1, info=None):
        """aovs() plus the motion plane against `prev_verts`: a float32 torch tensor on this renderer's GPU with the previous position of
        every vertex of the bound vertex buffer ((V, 3) or flat).  Returns (aov (H, W, 16), motion (H, W, 4)) float32 torch tensors; a
        motion record is gmupt_motion (motion_fields() splits it -- word 3 is an integer, compare it as bits)."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        if not hasattr(prev_verts, "is_cuda") or not prev_verts.is_cuda or prev_verts.dtype != torch.float32 or prev_verts.numel() % 3:
            raise GmuptError("aovs_motion: prev_verts must be a float32 tensor of 3 floats per vertex on the GPU", ERR_INVALID_ARGUMENT)
        if prev_verts.device.index != dev.index:
            raise GmuptError("aovs_motion: prev_verts lives on %s, the renderer on %s" % (prev_verts.device, dev), ERR_INVALID_ARGUMENT)
        pv = prev_verts.contiguous()
        out = torch.empty((self.height, self.width, 16), dtype=torch.float32, device=dev)
        mv = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(lib().gmupt_render_aovs_motion(self.h, int(samples), C.c_void_p(pv.data_ptr()), pv.numel() // 3, C.c_void_p(out.data_ptr()),
                                              out.numel() * 4, C.c_void_p(mv.data_ptr()), mv.numel() * 4, C.byref(ti)))
        self.last_aovs = ti
        return out, mv

    # denoiser (gmupt_render_denoised)
    def denoise(self, aov_samples=1, info=None, **params):
        """The a-trous denoiser on this renderer's frame (the tile in tile mode): gmupt_render_aovs(aov_samples) into internal scratch,
        a copy of the framebuffer, then the filter (include/gmupt.h states it).  Returns an (H, W, 4) float32 torch tensor on this
        renderer's GPU: rgb denoised, alpha the sample-count bits of the frame.  params: passes, sigma_color, sigma_normal, sigma_plane,
        sigma_albedo (the rest keep gmupt_denoise_default_params).  info: optional TraceInfo to fill (ms = AOVs + filter)."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        dp = denoise_params(**params)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(lib().gmupt_render_denoised(self.h, int(aov_samples), C.byref(dp), C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(ti)))
        self.last_denoise = ti
        return out

    # temporal reuse (gmupt_render_denoised_temporal)
    def denoise_temporal(self, handle, aov_samples=1, info=None, **params):
        """The denoiser with temporal reuse on this renderer's frame (the tile in tile mode): AOVs and a framebuffer copy as denoise(),
        then the frame integrated with the reprojected history of `handle` (a Temporal of this renderer) and filtered.  The first call
        after an iteration that cleared the frame, or after a resize, starts a new accumulation epoch (include/gmupt.h).  Returns an
        (H, W, 4) float32 torch tensor on this renderer's GPU: rgb denoised, alpha the effective sample-count bits.  params: the
        temporal_params fields.  info: optional TraceInfo to fill (ms = AOVs + integration + filter)."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        tp = temporal_params(**params)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(lib().gmupt_render_denoised_temporal(self.h, handle.h, int(aov_samples), C.byref(tp), C.c_void_p(out.data_ptr()), out.numel() * 4,
                                                    C.byref(ti)))
        self.last_denoise = ti
        return out

    def denoise_temporal_motion(self, handle, aov_samples=1, info=None, **params):
        """denoise_temporal() for geometry that moves (gmupt_render_denoised_temporal_motion): the handle keeps the vertex pose of its
        record sets, and after a refit() the history is looked up where each surface point was.  Without a refit since the history
        was written it is denoise_temporal() bit for bit."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        tp = temporal_params(**params)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(lib().gmupt_render_denoised_temporal_motion(self.h, handle.h, int(aov_samples), C.byref(tp), C.c_void_p(out.data_ptr()),
                                                           out.numel() * 4, C.byref(ti)))
        self.last_denoise = ti
        return out

    # preview chain (gmupt_render_preview)
    def preview(self, temporal=None, motion=False, aov_samples=1, infill=None, info=None, **params):
        """The preview of this renderer's frame in one call (gmupt_render_preview): AOVs -> integration with the history of `temporal`
        (a Temporal of this renderer, or None) -> guided infill -> the a-trous filter.  infill: None (off: the call is denoise(),
        denoise_temporal() or, with motion=True, denoise_temporal_motion() bit for bit), True (gmupt_infill_default_params) or a dict
        of infill_params fields.  params: the temporal_params fields (without a handle only the spatial ones are read).  Returns an
        (H, W, 4) float32 torch tensor on this renderer's GPU; a filled pixel has the alpha bits of sample count 1.  info: optional
        TraceInfo to fill, as for denoise() (ms = AOVs + integration + infill + filter)."""
        import torch
        dev = torch.device("cuda", getattr(self.dev, "index", 0))
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        tp = temporal_params(**params)
        ip = _infill_arg(infill)
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(lib().gmupt_render_preview(self.h, temporal.h if temporal is not None else None, PREVIEW_MOTION if motion else 0, int(aov_samples),
                                          C.byref(tp), C.byref(ip) if ip is not None else None, C.c_void_p(out.data_ptr()), out.numel() * 4,
                                          C.byref(ti)))
        self.last_denoise = ti
        return out

    # reference-layout debug access
    def read_path_state(self):
        out = np.empty(self.pool * STATE_BYTES, dtype=np.uint8)
        _check(lib().gmupt_debug_read_path_state(self.h, _ptr(out), out.nbytes))
        return out

    def write_path_state(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        _check(lib().gmupt_debug_write_path_state(self.h, _ptr(raw), raw.nbytes))

    def read_queues(self):
        out = np.empty(self.pool * 5, dtype=np.uint32)
        _check(lib().gmupt_debug_read_queues(self.h, _ptr(out), out.nbytes))
        return out.reshape(5, self.pool)

    def write_queues(self, q):
        q = np.ascontiguousarray(q, dtype=np.uint32)
        _check(lib().gmupt_debug_write_queues(self.h, _ptr(q), q.nbytes))

    def write_counters(self, qc):
        arr = (C.c_uint32 * 8)(*[int(v) for v in qc])
        _check(lib().gmupt_debug_write_counters(self.h, C.byref(arr)))

    def write_framebuffer(self, fb):
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        _check(lib().gmupt_debug_write_framebuffer(self.h, _ptr(fb), fb.nbytes))

    def read_travtables(self):
        """gmupt_debug_read_travtable for every kind: what this renderer holds of the traversal tables, its scalars and its refit maps, as
        {kind: uint8 array} with the keys of TRAVTABLE_KINDS, like travtables() (an absent table is empty)."""
        out = {}
        for which, kind in enumerate(TRAVTABLE_KINDS):
            n = C.c_size_t(0)
            _check(lib().gmupt_debug_read_travtable(self.h, which, None, 0, C.byref(n)))
            buf = np.zeros(n.value, np.uint8)
            if n.value:
                _check(lib().gmupt_debug_read_travtable(self.h, which, _ptr(buf), buf.nbytes, C.byref(n)))
            out[kind] = buf
        return out

    def close(self):
        if self.h:
            for t in self._temporals + self._normals + self._poses + list(self._converges):
                t.close()
            lib().gmupt_renderer_destroy(self.h)
            self.h = _P()


class Temporal:
    """gmupt_temporal: the history of one renderer's denoised frames (two record sets: the frozen history of earlier accumulations and
    the records of the latest call).  It uses the renderer's device and stream and is closed with it at the latest."""

    def __init__(self, renderer):
        self.renderer = renderer
        self.h = _P()
        _check(lib().gmupt_temporal_create(renderer.h, C.byref(self.h)))
        renderer._temporals.append(self)

    def reset(self):
        """Drops both record sets: the next output is the plain spatial denoise."""
        _check(lib().gmupt_temporal_reset(self.h))

    def close(self):
        if self.h:
            lib().gmupt_temporal_destroy(self.h)
            self.h = _P()


def converge_params(**params):
    """gmupt_converge_default_params with the given fields replaced (threshold, min_batches, allow_pixels)."""
    cp = ConvergeParams()
    lib().gmupt_converge_default_params(C.byref(cp))
    for k, v in params.items():
        if k not in ("threshold", "min_batches", "allow_pixels"):
            raise TypeError("unknown convergence parameter %r" % k)
        setattr(cp, k, v)
    return cp


class Converge:
    """gmupt_converge: the convergence monitor of one renderer (include/gmupt.h "Convergence"): a per-pixel batch-mean state from which
    every update estimates the standard error of the pixel's tone-mapped luminance mean.  It uses the renderer's device and stream and
    is closed with it at the latest."""

    def __init__(self, renderer):
        self.renderer = renderer
        self.h = _P()
        self._size = None   # (H, W) of the state, once an update has run
        _check(lib().gmupt_converge_create(renderer.h, C.byref(self.h)))
        renderer._converges.append(self)

    def _device(self):
        import torch
        return torch.device("cuda", getattr(self.renderer.dev, "index", 0))

    def update(self, error=False, **params):
        """gmupt_converge_update on the renderer's accumulation target, behind its pending iterations.  Returns the info dict; with
        error=True (info, error plane), the plane an (H, W) float32 torch tensor on the renderer's GPU (-1 = unknown)."""
        cp = converge_params(**params)
        ci = ConvergeInfo()
        H, W = self.renderer.height, self.renderer.width
        err = None
        if error:
            import torch
            err = torch.empty((H, W), dtype=torch.float32, device=self._device())
            torch.cuda.current_stream(err.device).synchronize()
        _check(lib().gmupt_converge_update(self.h, C.byref(cp), C.c_void_p(err.data_ptr()) if error else None, C.byref(ci)))
        self._size = (H, W)
        return (ci.as_dict(), err) if error else ci.as_dict()

    def update_image(self, tensor, error=False, **params):
        """gmupt_converge_update_image on an (H, W, 4) float32 torch tensor on the renderer's GPU (a = sample-count bits), e.g. a
        gathered frame.  torch's current stream is synchronised first.  Returns as update()."""
        import torch
        if not isinstance(tensor, torch.Tensor) or tensor.dim() != 3 or tensor.shape[2] != 4 or tensor.dtype != torch.float32 or tensor.device != self._device():
            raise GmuptError("update_image: an (H, W, 4) float32 tensor on %s" % self._device(), ERR_INVALID_ARGUMENT)
        tensor = tensor.contiguous()
        H, W = int(tensor.shape[0]), int(tensor.shape[1])
        cp = converge_params(**params)
        ci = ConvergeInfo()
        err = torch.empty((H, W), dtype=torch.float32, device=tensor.device) if error else None
        torch.cuda.current_stream(tensor.device).synchronize()
        _check(lib().gmupt_converge_update_image(self.h, C.c_void_p(tensor.data_ptr()), W, H, C.byref(cp),
                                                 C.c_void_p(err.data_ptr()) if error else None, C.byref(ci)))
        self._size = (H, W)
        return (ci.as_dict(), err) if error else ci.as_dict()

    def state(self):
        """gmupt_converge_read_state: the per-pixel state as an (H, W) array of converge_pixel_dtype (empty before the first update)."""
        if self._size is None:
            return np.zeros((0, 0), converge_pixel_dtype)
        out = np.zeros(self._size, converge_pixel_dtype)
        _check(lib().gmupt_converge_read_state(self.h, _ptr(out), out.nbytes))
        return out

    def reset(self):
        """Every pixel back to the initial state: the next update starts the estimate afresh."""
        _check(lib().gmupt_converge_reset(self.h))

    def close(self):
        if self.h:
            lib().gmupt_converge_destroy(self.h)
            self.h = _P()
            if self in self.renderer._converges:
                self.renderer._converges.remove(self)


def converge_host(state, rgba, error=False, **params):
    """gmupt_converge_host: the convergence rule on the CPU, bit for bit what Converge.update() computes.  state: an (H, W) array of
    converge_pixel_dtype, updated in place (np.zeros is the initial state); rgba: (H, W, 4) float32.  Returns the info dict; with
    error=True (info, (H, W) float32 error plane)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4 or state.dtype != converge_pixel_dtype or state.shape != rgba.shape[:2] or not state.flags.c_contiguous:
        raise GmuptError("converge_host: rgba must be (H, W, 4) float32 and state a contiguous (H, W) array of converge_pixel_dtype", ERR_INVALID_ARGUMENT)
    cp = converge_params(**params)
    ci = ConvergeInfo()
    err = np.empty(rgba.shape[:2], np.float32) if error else None
    _check(lib().gmupt_converge_host(_ptr(state), _ptr(rgba), rgba.shape[1], rgba.shape[0], C.byref(cp), _ptr(err) if error else None, C.byref(ci)))
    return (ci.as_dict(), err) if error else ci.as_dict()


class Normals:
    """gmupt_normals: smooth vertex normals of one index list, recomputed on the GPU from the vertex buffer the renderer is bound to and
    written into the `normal` field of its property records (include/gmupt.h "normals" states the rule).  indices: (n, 3) int32, a numpy
    array (uploaded) or a torch device tensor (used in place; the handle keeps its own copy).  It uses the renderer's device and stream
    and is closed with it at the latest."""

    def __init__(self, renderer, indices):
        import torch
        device = torch.device("cuda", getattr(renderer.dev, "index", 0))
        if isinstance(indices, torch.Tensor):
            if indices.device != device or indices.dtype != torch.int32:
                raise GmuptError("Normals: an index tensor must be int32 on %s" % device, ERR_INVALID_ARGUMENT)
            idx = indices.contiguous().reshape(-1)
        else:
            idx = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)).to(device)
        self.renderer = renderer
        self.h = _P()
        torch.cuda.current_stream(device).synchronize()
        _check(lib().gmupt_normals_create(renderer.h, C.c_void_p(idx.data_ptr()) if idx.numel() else None, idx.numel() // 3, C.byref(self.h)))
        renderer._normals.append(self)

    def update(self, info=False):
        """gmupt_normals_update on the renderer's stream.  info=False: no host synchronisation, returns None.  info=True: synchronises
        and returns the gmupt_normals_info fields as a dict (ms = device time of the two launches)."""
        if not info:
            _check(lib().gmupt_normals_update(self.h, None))
            return None
        ni = NormalsInfo()
        _check(lib().gmupt_normals_update(self.h, C.byref(ni)))
        return {"num_verts": int(ni.num_verts), "num_tris": int(ni.num_tris), "max_valence": int(ni.max_valence), "ms": float(ni.ms)}

    def close(self):
        if self.h:
            lib().gmupt_normals_destroy(self.h)
            self.h = _P()


def vertex_normals_host(verts, indices, threads=16):
    """gmupt_vertex_normals_host: the smooth-normal rule of include/gmupt.h on the CPU in binary32, bit for bit what Normals.update()
    writes.  verts (V, 3) float32, indices (n, 3) int32.  Returns (V, 3) float32."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    out = np.empty_like(verts)
    _check(lib().gmupt_vertex_normals_host(_ptr(verts), verts.shape[0], _ptr(indices), indices.shape[0], _ptr(out), int(threads)))
    return out


def _rig_arrays(rest, joints, weights, num_joints, deltas):
    """The arrays of a rig as contiguous numpy arrays of the C-ABI's types (None where the rule ignores them) and V, K, J, T."""
    rest = np.ascontiguousarray(rest, dtype=np.float32).reshape(-1, 3)
    V, J = rest.shape[0], int(num_joints)
    K = 0
    if J:
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(V, -1) if V else np.zeros((0, 1), np.float32)
        K = weights.shape[1]
        joints = np.ascontiguousarray(joints, dtype=np.uint16).reshape(V, K)
    else:
        joints = weights = None
    deltas = None if deltas is None else np.ascontiguousarray(deltas, dtype=np.float32).reshape(-1, V, 3)
    T = 0 if deltas is None else deltas.shape[0]
    return rest, joints, weights, (deltas if T else None), V, K, J, T


class Pose:
    """gmupt_pose: the rig of one mesh -- rest positions, skinning influences, dense morph targets -- kept on the GPU, and update(), which
    writes the posed vertices into the vertex buffer the renderer is bound to (include/gmupt.h "Pose" states the rule).  rest (V, 3)
    float32, joints (V, K) uint16, weights (V, K) float32, deltas (T, V, 3) float32 or None; each a numpy array (uploaded) or a torch
    device tensor of that dtype (used in place; the handle keeps its own copies).  num_joints = 0: morph only, joints and weights are
    ignored.  It uses the renderer's device and stream and is closed with it at the latest."""

    def __init__(self, renderer, rest, joints, weights, num_joints, deltas=None):
        import torch
        device = torch.device("cuda", getattr(renderer.dev, "index", 0))
        J = int(num_joints)

        def dev(a, np_dtype, t_dtype, what):
            if a is None:
                return None
            if isinstance(a, torch.Tensor):
                if a.device != device or a.dtype != t_dtype:
                    raise GmuptError("Pose: a %s tensor must be %s on %s" % (what, t_dtype, device), ERR_INVALID_ARGUMENT)
                return a.contiguous()
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(device)

        rest = dev(rest, np.float32, torch.float32, "rest")
        weights = dev(weights, np.float32, torch.float32, "weights") if J else None
        if J and isinstance(joints, torch.Tensor):
            if joints.device != device or joints.dtype not in (getattr(torch, "uint16", torch.int16), torch.int16):
                raise GmuptError("Pose: a joints tensor must be uint16 (or its bits as int16) on %s" % device, ERR_INVALID_ARGUMENT)
            joints = joints.contiguous()
        elif J:
            joints = torch.from_numpy(np.ascontiguousarray(joints, dtype=np.uint16).view(np.int16)).to(device)
        else:
            joints = None
        deltas = dev(deltas, np.float32, torch.float32, "deltas")
        V = rest.numel() // 3
        K = (weights.numel() // V if V else 0) if J else 0
        T = deltas.numel() // (3 * V) if (deltas is not None and V) else 0
        if J and (weights.numel() != V * K or joints.numel() != V * K):
            raise GmuptError("Pose: joints and weights must hold the same number of influences for each of the %d vertices" % V, ERR_INVALID_ARGUMENT)
        if deltas is not None and deltas.numel() != T * V * 3:
            raise GmuptError("Pose: deltas must hold 3 floats per vertex and target", ERR_INVALID_ARGUMENT)
        self.renderer = renderer
        self.num_verts, self.influences, self.num_joints, self.num_targets = V, K, J, T
        self._device = device
        self._pending = []     # device tensors of update() calls the stream may not have read yet
        self.h = _P()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        torch.cuda.current_stream(device).synchronize()
        _check(lib().gmupt_pose_create(renderer.h, p(rest), p(joints), p(weights), K, J, p(deltas) if T else None, T, C.byref(self.h)))
        renderer._poses.append(self)

    def update(self, joint_mats, target_weights=None, info=False):
        """gmupt_pose_update (numpy / host arrays) or gmupt_pose_update_device (joint_mats a torch device tensor; target_weights then a
        device tensor too, or a host array that is uploaded first) on the renderer's stream.  joint_mats: (J, 12) float32, None for a
        morph-only rig; target_weights: (T,) float32, None = all zero.  info=False: no host synchronisation, returns None.  info=True:
        synchronises and returns the gmupt_pose_info fields as a dict (ms = device time of the copies and the two launches).  Device
        tensors are kept referenced until a synchronising call has shown that the stream is past them."""
        J, T = self.num_joints, self.num_targets
        pi = PoseInfo() if info else None
        on_device = hasattr(joint_mats, "is_cuda") or hasattr(target_weights, "is_cuda")
        if on_device:
            import torch

            def dev(a, n, what):
                if n == 0:
                    return None
                if a is None:
                    return torch.zeros(n, dtype=torch.float32, device=self._device)
                if not isinstance(a, torch.Tensor):
                    a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
                if a.dtype != torch.float32 or a.numel() != n:
                    raise GmuptError("Pose.update: %s must hold %d float32" % (what, n), ERR_INVALID_ARGUMENT)
                if a.device != self._device:
                    if a.is_cuda:
                        raise GmuptError("Pose.update: %s is on %s, the renderer on %s" % (what, a.device, self._device), ERR_INVALID_ARGUMENT)
                    a = a.to(self._device)
                return a.contiguous()

            jm, tw = dev(joint_mats, 12 * J, "joint_mats"), dev(target_weights, T, "target_weights")
            torch.cuda.current_stream(self._device).synchronize()
            if len(self._pending) >= 64:
                self.renderer.synchronize(); self._pending.clear()
            self._pending.append((jm, tw))
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            _check(lib().gmupt_pose_update_device(self.h, p(jm), p(tw), C.byref(pi) if info else None))
        else:
            jm = None if J == 0 else np.ascontiguousarray(joint_mats, dtype=np.float32).reshape(-1)
            tw = None if T == 0 else (np.zeros(T, np.float32) if target_weights is None else np.ascontiguousarray(target_weights, dtype=np.float32).reshape(-1))
            if (J and jm.size != 12 * J) or (T and tw.size != T):
                raise GmuptError("Pose.update: %d joints need %d matrix floats, %d targets %d weights" % (J, 12 * J, T, T), ERR_INVALID_ARGUMENT)
            _check(lib().gmupt_pose_update(self.h, _ptr(jm) if J else None, _ptr(tw) if T else None, C.byref(pi) if info else None))
        if not info:
            return None
        self._pending.clear()                                    # the call has synchronised the stream
        return {"num_verts": int(pi.num_verts), "active_targets": int(pi.active_targets), "ms": float(pi.ms)}

    def close(self):
        if self.h:
            lib().gmupt_pose_destroy(self.h)                     # synchronises the stream
            self.h = _P()
            self._pending = []
            if self in self.renderer._poses:                     # (Renderer.close() walks a copy of the list)
                self.renderer._poses.remove(self)


def pose_host(rest, joints, weights, num_joints, joint_mats, deltas=None, target_weights=None, threads=16):
    """gmupt_pose_host: the pose rule of include/gmupt.h on the CPU in binary32, bit for bit what Pose.update() writes.  Arrays as for
    Pose and Pose.update (numpy).  Returns (V, 3) float32."""
    rest, joints, weights, deltas, V, K, J, T = _rig_arrays(rest, joints, weights, num_joints, deltas)
    jm = np.ascontiguousarray(joint_mats, dtype=np.float32).reshape(-1) if J else None
    if J and jm.size != 12 * J:
        raise GmuptError("pose_host: %d joints need %d matrix floats" % (J, 12 * J), ERR_INVALID_ARGUMENT)
    tw = None
    if T:
        tw = np.zeros(T, np.float32) if target_weights is None else np.ascontiguousarray(target_weights, dtype=np.float32).reshape(-1)
        if tw.size != T:
            raise GmuptError("pose_host: %d targets need %d weights" % (T, T), ERR_INVALID_ARGUMENT)
    out = np.empty_like(rest)
    p = lambda a: _ptr(a) if a is not None else None
    _check(lib().gmupt_pose_host(p(rest), V, p(joints), p(weights), K, p(jm), J, p(deltas), p(tw), T, _ptr(out), int(threads)))
    return out


def camera_pick_ray(cam_buffer, px, py):
    """gmupt_camera_pick_ray (host only): the un-jittered primary ray of newPath.hlsl:36-39 through whole-frame pixel (px, py)."""
    ray = Ray()
    _check(lib().gmupt_camera_pick_ray(C.byref(cam_buffer), float(px), float(py), C.byref(ray)))
    return ray


def hit_fields(hits):
    """Splits (N, 8) gmupt_hit records (numpy or torch) into a dict of numpy arrays: t, u, v (float32), triangle (int32), light,
    material (uint32)."""
    h = hits.cpu().numpy() if hasattr(hits, "cpu") else np.asarray(hits)
    rec = np.ascontiguousarray(h, dtype=np.float32).reshape(-1, 8).view(hit_dtype)[:, 0]
    return {k: rec[k].copy() for k in ("t", "u", "v", "triangle", "light", "material")}


def aov_ray(cam_buffer, x, y, samples, k):
    """gmupt_aov_ray (host only): ray k of whole-frame pixel (x, y) at `samples` -- k = 0 the centre ray, k = 1 + b*s + a the stratified ones."""
    ray = Ray()
    _check(lib().gmupt_aov_ray(C.byref(cam_buffer), int(x), int(y), int(samples), int(k), C.byref(ray)))
    return ray


def aov_rays(cam_buffer, xs, ys, samples):
    """All AOV rays of the pixels (xs[i], ys[i]) as an (N, R, 8) float32 array (gmupt_aov_ray per ray; R = 1 or samples^2 + 1)."""
    R = 1 if samples == 1 else samples * samples + 1
    out = np.empty((len(xs), R, 8), np.float32)
    for i, (x, y) in enumerate(zip(xs, ys)):
        for k in range(R):
            out[i, k] = np.frombuffer(bytes(aov_ray(cam_buffer, x, y, samples, k)), np.float32)
    return out


def aov_fields(aovs):
    """Splits (..., 16) gmupt_aov records (torch or numpy) into a dict of numpy arrays of shape (...): albedo, normal, position (..., 3),
    depth, roughness, metallic (float32), triangle (int32), material, light, coverage (uint32)."""
    a = aovs.cpu().numpy() if hasattr(aovs, "cpu") else np.asarray(aovs)
    a = np.ascontiguousarray(a, dtype=np.float32)
    rec = a.reshape(-1, 16).view(aov_dtype)[:, 0]
    shape = a.shape[:-1]
    return {k: rec[k].reshape(shape + rec[k].shape[1:]).copy() for k in aov_dtype.names}


def denoise_params(**params):
    """gmupt_denoise_default_params with the given fields replaced (passes, sigma_color, sigma_normal, sigma_plane, sigma_albedo)."""
    dp = DenoiseParams()
    lib().gmupt_denoise_default_params(C.byref(dp))
    for k, v in params.items():
        if k not in ("passes", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo"):
            raise TypeError("unknown denoiser parameter %r" % k)
        setattr(dp, k, v)
    return dp


def denoise_image(renderer, beauty, aov, ms=None, **params):
    """gmupt_denoise_image on torch tensors on the renderer's GPU: beauty (H, W, 4) float32 (a = sample-count bits), aov (H, W, 16)
    float32 gmupt_aov records.  Returns the (H, W, 4) float32 result.  Any image size; enqueued on the renderer's stream after torch's
    current stream is synchronised.  ms: optional list that receives the filter's device time."""
    import torch
    if beauty.dim() != 3 or beauty.shape[2] != 4 or aov.dim() != 3 or aov.shape[2] != 16 or tuple(aov.shape[:2]) != tuple(beauty.shape[:2]):
        raise GmuptError("denoise_image: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    if beauty.dtype != torch.float32 or aov.dtype != torch.float32 or not beauty.is_cuda or not aov.is_cuda:
        raise GmuptError("denoise_image: float32 tensors on the GPU", ERR_INVALID_ARGUMENT)
    beauty, aov = beauty.contiguous(), aov.contiguous()
    H, W = beauty.shape[0], beauty.shape[1]
    out = torch.empty_like(beauty)
    dp = denoise_params(**params)
    torch.cuda.current_stream(beauty.device).synchronize()
    t = C.c_float(0.0)
    _check(lib().gmupt_denoise_image(renderer.h, C.c_void_p(beauty.data_ptr()), C.c_void_p(aov.data_ptr()), W, H, C.byref(dp),
                                     C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(t)))
    if ms is not None:
        ms.append(t.value)
    return out


def denoise_host(beauty, aov, threads=16, **params):
    """gmupt_denoise_host: the same filter on the CPU, bit for bit the device result.  beauty (H, W, 4) float32, aov (H, W, 16) float32
    (or an (H, W) array of aov_dtype); numpy or torch.  Returns an (H, W, 4) float32 numpy array."""
    b = beauty.cpu().numpy() if hasattr(beauty, "cpu") else np.asarray(beauty)
    a = aov.cpu().numpy() if hasattr(aov, "cpu") else np.asarray(aov)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.dtype == aov_dtype:
        a = a.view(np.float32).reshape(a.shape + (16,))
    a = np.ascontiguousarray(a, dtype=np.float32)
    if b.ndim != 3 or b.shape[2] != 4 or a.shape != b.shape[:2] + (16,):
        raise GmuptError("denoise_host: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    out = np.empty_like(b)
    dp = denoise_params(**params)
    _check(lib().gmupt_denoise_host(_ptr(b), _ptr(a), b.shape[1], b.shape[0], C.byref(dp), _ptr(out), out.nbytes, int(threads)))
    return out


def infill_params(**params):
    """gmupt_infill_default_params with the given fields replaced (passes, sigma_normal, sigma_plane, sigma_albedo)."""
    ip = InfillParams()
    lib().gmupt_infill_default_params(C.byref(ip))
    for k, v in params.items():
        if k not in ("passes", "sigma_normal", "sigma_plane", "sigma_albedo"):
            raise TypeError("unknown infill parameter %r" % k)
        setattr(ip, k, v)
    return ip


def _infill_arg(infill):
    """The `infill` keyword of the preview calls: None / False -> None (off), True -> the defaults, a dict -> infill_params(**dict)."""
    if infill is None or infill is False:
        return None
    if isinstance(infill, InfillParams):
        return infill
    return infill_params(**({} if infill is True else dict(infill)))


def infill_image(renderer, beauty, aov, info=False, **params):
    """gmupt_infill_image on torch tensors on the renderer's GPU: beauty (H, W, 4) float32 (a = sample-count bits), aov (H, W, 16)
    float32 gmupt_aov records.  Returns the (H, W, 4) float32 result, enqueued on the renderer's stream after torch's current stream is
    synchronised; with info=True the call waits and returns (result, info dict), otherwise the renderer's stream is synchronised
    before the tensor is handed to torch.  params: the infill_params fields."""
    import torch
    if beauty.dim() != 3 or beauty.shape[2] != 4 or aov.dim() != 3 or aov.shape[2] != 16 or tuple(aov.shape[:2]) != tuple(beauty.shape[:2]):
        raise GmuptError("infill_image: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    if beauty.dtype != torch.float32 or aov.dtype != torch.float32 or not beauty.is_cuda or not aov.is_cuda:
        raise GmuptError("infill_image: float32 tensors on the GPU", ERR_INVALID_ARGUMENT)
    beauty, aov = beauty.contiguous(), aov.contiguous()
    H, W = beauty.shape[0], beauty.shape[1]
    out = torch.empty_like(beauty)
    ip = infill_params(**params)
    torch.cuda.current_stream(beauty.device).synchronize()
    ii = InfillInfo()
    _check(lib().gmupt_infill_image(renderer.h, C.c_void_p(beauty.data_ptr()), C.c_void_p(aov.data_ptr()), W, H, C.byref(ip),
                                    C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(ii) if info else None))
    if info:
        return out, ii.as_dict()
    renderer.synchronize()
    return out


def infill_host(beauty, aov, threads=16, **params):
    """gmupt_infill_host: the same rule on the CPU, bit for bit the device result.  beauty (H, W, 4) float32, aov (H, W, 16) float32
    (or an (H, W) array of aov_dtype); numpy or torch.  Returns ((H, W, 4) float32 numpy array, info dict)."""
    b = beauty.cpu().numpy() if hasattr(beauty, "cpu") else np.asarray(beauty)
    a = aov.cpu().numpy() if hasattr(aov, "cpu") else np.asarray(aov)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.dtype == aov_dtype:
        a = a.view(np.float32).reshape(a.shape + (16,))
    a = np.ascontiguousarray(a, dtype=np.float32)
    if b.ndim != 3 or b.shape[2] != 4 or a.shape != b.shape[:2] + (16,):
        raise GmuptError("infill_host: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    out = np.empty_like(b)
    ip = infill_params(**params)
    ii = InfillInfo()
    _check(lib().gmupt_infill_host(_ptr(b), _ptr(a), b.shape[1], b.shape[0], C.byref(ip), _ptr(out), out.nbytes, C.byref(ii), int(threads)))
    return out, ii.as_dict()


TEMPORAL_FIELDS = ("history_cap", "min_normal_cos", "plane_dist")


def temporal_params(**params):
    """gmupt_temporal_default_params with the given fields replaced: history_cap, min_normal_cos, plane_dist, and the spatial filter's
    passes, sigma_color, sigma_normal, sigma_plane, sigma_albedo."""
    tp = TemporalParams()
    lib().gmupt_temporal_default_params(C.byref(tp))
    for k, v in params.items():
        if k in TEMPORAL_FIELDS:
            setattr(tp, k, v)
        elif k in ("passes", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo"):
            setattr(tp.spatial, k, v)
        else:
            raise TypeError("unknown temporal denoiser parameter %r" % k)
    return tp


def temporal_denoise_image(handle, beauty, aov, cam_buffer, new_accumulation, origin=(0, 0), ms=None, motion=None, infill=None, **params):
    """gmupt_temporal_denoise_image on torch tensors on the handle's GPU: beauty (H, W, 4) float32 (a = sample-count bits), aov (H, W, 16)
    float32 records, rendered with cam_buffer (a CameraBuffer) at `origin` of its whole frame.  new_accumulation: move the latest
    call's records into the history first.  Returns the (H, W, 4) float32 result.  ms: optional list that receives the device time.
    motion: an (H, W, 4) float32 tensor of gmupt_motion records on the same GPU (gmupt_temporal_denoise_image_motion), or None.
    infill: None, or True / a dict of infill_params fields: the call goes through gmupt_temporal_preview_image, with the guided infill
    between the integration and the filter."""
    import torch
    if beauty.dim() != 3 or beauty.shape[2] != 4 or aov.dim() != 3 or aov.shape[2] != 16 or tuple(aov.shape[:2]) != tuple(beauty.shape[:2]):
        raise GmuptError("temporal_denoise_image: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    if beauty.dtype != torch.float32 or aov.dtype != torch.float32 or not beauty.is_cuda or not aov.is_cuda:
        raise GmuptError("temporal_denoise_image: float32 tensors on the GPU", ERR_INVALID_ARGUMENT)
    beauty, aov = beauty.contiguous(), aov.contiguous()
    H, W = beauty.shape[0], beauty.shape[1]
    out = torch.empty_like(beauty)
    tp = temporal_params(**params)
    if motion is not None:
        if motion.dtype != torch.float32 or not motion.is_cuda or tuple(motion.shape) != (H, W, 4) or motion.device != beauty.device:
            raise GmuptError("temporal_denoise_image: motion must be an (H, W, 4) float32 tensor on the GPU of beauty", ERR_INVALID_ARGUMENT)
        hdev = getattr(handle.renderer.dev, "index", 0)
        if beauty.device.index != hdev or aov.device != beauty.device:
            raise GmuptError("temporal_denoise_image: the tensors live on %s, the handle's renderer on cuda:%d" % (beauty.device, hdev), ERR_INVALID_ARGUMENT)
        motion = motion.contiguous()
    torch.cuda.current_stream(beauty.device).synchronize()
    t = C.c_float(0.0)
    ip = _infill_arg(infill)
    if ip is not None:
        _check(lib().gmupt_temporal_preview_image(handle.h, C.c_void_p(beauty.data_ptr()), C.c_void_p(aov.data_ptr()),
                                                  C.c_void_p(motion.data_ptr()) if motion is not None else None, C.byref(cam_buffer),
                                                  int(origin[0]), int(origin[1]), W, H, 1 if new_accumulation else 0, C.byref(tp),
                                                  C.byref(ip), C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(t)))
    elif motion is not None:
        _check(lib().gmupt_temporal_denoise_image_motion(handle.h, C.c_void_p(beauty.data_ptr()), C.c_void_p(aov.data_ptr()),
                                                         C.c_void_p(motion.data_ptr()), C.byref(cam_buffer), int(origin[0]), int(origin[1]), W, H,
                                                         1 if new_accumulation else 0, C.byref(tp), C.c_void_p(out.data_ptr()), out.numel() * 4,
                                                         C.byref(t)))
    else:
        _check(lib().gmupt_temporal_denoise_image(handle.h, C.c_void_p(beauty.data_ptr()), C.c_void_p(aov.data_ptr()), C.byref(cam_buffer),
                                                  int(origin[0]), int(origin[1]), W, H, 1 if new_accumulation else 0, C.byref(tp),
                                                  C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(t)))
    if ms is not None:
        ms.append(t.value)
    return out


def temporal_integrate_host(beauty, aov, prev=None, prev_cam=None, prev_origin=(0, 0), threads=16, **params):
    """gmupt_temporal_integrate_host: the integration step on the CPU, bit for bit the device's.  beauty (H, W, 4) float32, aov (H, W, 16)
    float32 (or aov_dtype); prev: an (h, w) history_dtype array (or (h, w, 12) float32) rendered with prev_cam at prev_origin, or None.
    Returns (integrated (H, W, 4) float32, history (H, W) history_dtype) as numpy arrays."""
    b = beauty.cpu().numpy() if hasattr(beauty, "cpu") else np.asarray(beauty)
    a = aov.cpu().numpy() if hasattr(aov, "cpu") else np.asarray(aov)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.dtype == aov_dtype:
        a = a.view(np.float32).reshape(a.shape + (16,))
    a = np.ascontiguousarray(a, dtype=np.float32)
    if b.ndim != 3 or b.shape[2] != 4 or a.shape != b.shape[:2] + (16,):
        raise GmuptError("temporal_integrate_host: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    H, W = b.shape[:2]
    ph = pw = 0
    pp = None
    if prev is not None:
        pv = np.asarray(prev)
        if pv.dtype != history_dtype:
            pv = np.ascontiguousarray(pv, dtype=np.float32).view(history_dtype)[..., 0]
        pv = np.ascontiguousarray(pv)
        if pv.ndim != 2:
            raise GmuptError("temporal_integrate_host: prev must be (h, w) records", ERR_INVALID_ARGUMENT)
        ph, pw = pv.shape
        pp = _ptr(pv)
    out = np.empty_like(b)
    hist = np.empty((H, W), history_dtype)
    tp = temporal_params(**params)
    _check(lib().gmupt_temporal_integrate_host(_ptr(b), _ptr(a), W, H, pp, C.byref(prev_cam) if prev_cam is not None else None,
                                               int(prev_origin[0]), int(prev_origin[1]), pw, ph, C.byref(tp), _ptr(out), _ptr(hist), int(threads)))
    return out, hist


def temporal_integrate_motion_host(beauty, aov, motion, prev=None, prev_cam=None, prev_origin=(0, 0), threads=16, **params):
    """gmupt_temporal_integrate_motion_host: temporal_integrate_host with a motion plane -- (H, W) motion_dtype records or (H, W, 4)
    float32, numpy or torch; None = temporal_integrate_host.  Returns (integrated, history) as that function."""
    b = beauty.cpu().numpy() if hasattr(beauty, "cpu") else np.asarray(beauty)
    a = aov.cpu().numpy() if hasattr(aov, "cpu") else np.asarray(aov)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.dtype == aov_dtype:
        a = a.view(np.float32).reshape(a.shape + (16,))
    a = np.ascontiguousarray(a, dtype=np.float32)
    if b.ndim != 3 or b.shape[2] != 4 or a.shape != b.shape[:2] + (16,):
        raise GmuptError("temporal_integrate_motion_host: beauty must be (H, W, 4) and aov (H, W, 16)", ERR_INVALID_ARGUMENT)
    H, W = b.shape[:2]
    mp = None
    if motion is not None:
        m = motion.cpu().numpy() if hasattr(motion, "cpu") else np.asarray(motion)
        if m.dtype == motion_dtype:
            m = m.view(np.float32).reshape(m.shape + (4,))
        m = np.ascontiguousarray(m, dtype=np.float32)
        if m.shape != (H, W, 4):
            raise GmuptError("temporal_integrate_motion_host: motion must be (H, W) records", ERR_INVALID_ARGUMENT)
        mp = _ptr(m)
    ph = pw = 0
    pp = None
    if prev is not None:
        pv = np.asarray(prev)
        if pv.dtype != history_dtype:
            pv = np.ascontiguousarray(pv, dtype=np.float32).view(history_dtype)[..., 0]
        pv = np.ascontiguousarray(pv)
        if pv.ndim != 2:
            raise GmuptError("temporal_integrate_motion_host: prev must be (h, w) records", ERR_INVALID_ARGUMENT)
        ph, pw = pv.shape
        pp = _ptr(pv)
    out = np.empty_like(b)
    hist = np.empty((H, W), history_dtype)
    tp = temporal_params(**params)
    _check(lib().gmupt_temporal_integrate_motion_host(_ptr(b), _ptr(a), mp, W, H, pp, C.byref(prev_cam) if prev_cam is not None else None,
                                                      int(prev_origin[0]), int(prev_origin[1]), pw, ph, C.byref(tp), _ptr(out), _ptr(hist),
                                                      int(threads)))
    return out, hist


def motion_host(hits, aov, tris, verts_now, verts_prev):
    """gmupt_motion_host: the motion plane's rule on the CPU, bit for bit the device's.  hits: (..., 8) float32 gmupt_hit records of the
    centre rays (or hit_dtype), aov: their (..., 16) float32 records (or aov_dtype), tris: triangle_dtype records, verts_now / verts_prev:
    (V, 3) float32.  Returns an array of motion_dtype with the leading shape of `aov`."""
    h = hits.cpu().numpy() if hasattr(hits, "cpu") else np.asarray(hits)
    a = aov.cpu().numpy() if hasattr(aov, "cpu") else np.asarray(aov)
    if h.dtype == hit_dtype:
        h = h.view(np.float32).reshape(h.shape + (8,))
    if a.dtype == aov_dtype:
        a = a.view(np.float32).reshape(a.shape + (16,))
    h = np.ascontiguousarray(h, dtype=np.float32)
    a = np.ascontiguousarray(a, dtype=np.float32)
    n = a.size // 16
    if h.size != n * 8:
        raise GmuptError("motion_host: one hit per AOV record", ERR_INVALID_ARGUMENT)
    tris = np.ascontiguousarray(tris, dtype=triangle_dtype)
    vn = np.ascontiguousarray(verts_now, dtype=np.float32).reshape(-1, 3)
    vp = np.ascontiguousarray(verts_prev, dtype=np.float32).reshape(-1, 3)
    if vn.shape != vp.shape:
        raise GmuptError("motion_host: %d vertices now, %d before" % (vn.shape[0], vp.shape[0]), ERR_INVALID_ARGUMENT)
    out = np.zeros(a.shape[:-1], motion_dtype)
    _check(lib().gmupt_motion_host(_ptr(h), _ptr(a), n, _ptr(tris), tris.shape[0], _ptr(vn), _ptr(vp), vn.shape[0], _ptr(out)))
    return out


def motion_fields(motion):
    """Splits (..., 4) gmupt_motion records (torch or numpy) into a dict of numpy arrays: prev_position (..., 3) float32, flags uint32."""
    m = motion.cpu().numpy() if hasattr(motion, "cpu") else np.asarray(motion)
    m = np.ascontiguousarray(m, dtype=np.float32)
    rec = m.reshape(-1, 4).view(motion_dtype)[:, 0]
    shape = m.shape[:-1]
    return {k: rec[k].reshape(shape + rec[k].shape[1:]).copy() for k in motion_dtype.names}


def bvh_refit_host(nodes, tris, verts, threads=16):
    """gmupt_bvh_refit_host on a copy: the nodes with the boxes of the given vertices, topology untouched."""
    out = np.array(nodes, dtype=bvh_node_dtype, copy=True)
    tris = np.ascontiguousarray(tris, dtype=triangle_dtype)
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    _check(lib().gmupt_bvh_refit_host(_ptr(out), out.shape[0], _ptr(tris), tris.shape[0], _ptr(verts), verts.shape[0], threads))
    return out


TRAVTABLE_KINDS = ("node64", "tri48", "tripair", "pair_ref", "wnode", "rec64", "scalars", "level_nodes", "level_off", "node_map", "wide_map", "opened")


def travtables(nodes, tris, verts, want_wide=True, top_order_bfs=False, node_pairing=True):
    """gmupt_debug_travtables_*: the traversal tables and refit maps a bind would build from these host arrays, no device involved.
    Returns {kind: uint8 array (a copy)} for TRAVTABLE_KINDS."""
    nodes = np.ascontiguousarray(nodes); tris = np.ascontiguousarray(tris)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    h = _P()
    _check(lib().gmupt_debug_travtables_build(_ptr(nodes), nodes.shape[0], _ptr(tris), tris.shape[0], _ptr(verts), verts.shape[0],
                                              int(want_wide), int(top_order_bfs), int(node_pairing), C.byref(h)))
    try:
        out = {}
        for which, kind in enumerate(TRAVTABLE_KINDS):
            n = C.c_size_t(0)
            p = lib().gmupt_debug_travtables_data(h, which, C.byref(n))
            out[kind] = np.frombuffer(C.string_at(p, n.value), np.uint8).copy() if p and n.value else np.zeros(0, np.uint8)
        return out
    finally:
        lib().gmupt_debug_travtables_destroy(h)


def wide_tables_addressable(wide_nodes, num_tris, num_pairs):
    """gmupt_debug_wide_tables_addressable: do tables of these sizes stay within the wide ray cast's 32-bit byte offsets?  No device involved."""
    return bool(lib().gmupt_debug_wide_tables_addressable(int(wide_nodes), int(num_tris), int(num_pairs)))


def sbvh_build(verts, indices, vertex_material=None, params=None):
    """Host SBVH build + flatten (gmupt_sbvh_*).  Returns dict(nodes, tris, ref_triangle, sah, depth)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    h = _P()
    pp = None
    if params is not None:
        pp = SbvhParams()
        lib().gmupt_sbvh_default_params(C.byref(pp))
        for k, v in params.items():
            setattr(pp, k, v)
        pp = C.byref(pp)
    _check(lib().gmupt_sbvh_build(_ptr(verts), verts.shape[0], _ptr(indices), indices.shape[0], pp, C.byref(h)))
    try:
        n = lib().gmupt_sbvh_num_nodes(h)
        nr = lib().gmupt_sbvh_num_references(h)
        nodes = np.zeros(n, dtype=bvh_node_dtype)
        tris = np.zeros(max(nr, 1), dtype=triangle_dtype)[:nr]
        ref = np.zeros(max(nr, 1), dtype=np.int32)[:nr]
        vm = None
        if vertex_material is not None:
            vm = np.ascontiguousarray(vertex_material, dtype=np.uint32)
        tris_buf = np.zeros(max(nr, 1), dtype=triangle_dtype)
        ref_buf = np.zeros(max(nr, 1), dtype=np.int32)
        _check(lib().gmupt_sbvh_flatten(h, _ptr(vm) if vm is not None else None, _ptr(nodes), _ptr(tris_buf), _ptr(ref_buf)))
        tris, ref = tris_buf[:nr], ref_buf[:nr]
        return {"nodes": nodes, "tris": tris, "ref_triangle": ref, "sah": float(lib().gmupt_sbvh_sah(h)), "depth": int(lib().gmupt_sbvh_depth(h))}
    finally:
        lib().gmupt_sbvh_destroy(h)


def lbvh_build_host(verts, indices, vertex_material=None, max_leaf_size=4):
    """gmupt_lbvh_build_host: the LBVH rule of include/gmupt.h on host arrays, the reference of Lbvh.build.  Returns the dict of sbvh_build
    (nodes, tris, ref_triangle, sah, depth) plus info (LbvhInfo.as_dict()); sah is the surface-area cost of the tree with the SBVH builder's
    default node / triangle costs of 1 (tree_sah)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    n = indices.shape[0]
    vm = np.ascontiguousarray(vertex_material, dtype=np.uint32) if vertex_material is not None else None
    if vm is not None and vm.shape[0] < verts.shape[0]:
        raise GmuptError("lbvh_build_host: %d vertex materials for %d vertices" % (vm.shape[0], verts.shape[0]), -1)
    nodes = np.zeros(max(2 * n - 1, 1), dtype=bvh_node_dtype)
    tris = np.zeros(max(n, 1), dtype=triangle_dtype)
    ref = np.zeros(max(n, 1), dtype=np.int32)
    pp, info = LbvhParams(int(max_leaf_size)), LbvhInfo()
    _check(lib().gmupt_lbvh_build_host(_ptr(verts), verts.shape[0], _ptr(indices), n, _ptr(vm) if vm is not None else None, C.byref(pp),
                                       _ptr(nodes), _ptr(tris), _ptr(ref), C.byref(info)))
    nodes = nodes[:info.num_nodes].copy()
    return {"nodes": nodes, "tris": tris[:n], "ref_triangle": ref[:n], "sah": tree_sah(nodes), "depth": int(info.depth), "info": info.as_dict()}


def tree_sah(nodes):
    """Surface-area cost of a reference-layout tree: A(node) / A(root) times 2 for an inner node (two box tests) and times the number of
    references for a leaf -- the measure gmupt_sbvh_sah reports at its default costs of 1, from the flattened boxes in float64 instead of
    the builder's running float products.  0 for a root without area."""
    nodes = np.asarray(nodes)
    e = np.maximum(nodes["max"].astype(np.float64) - nodes["min"].astype(np.float64), 0.0)
    area = 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    if not area[0] > 0:
        return 0.0
    leaf = nodes["isLeaf"] != 0
    count = np.where(leaf, nodes["right"] - nodes["left"], 2)
    return float((area * count).sum() / area[0])


def tree_cost_host(nodes, threads=16):
    """gmupt_tree_cost_host: the tree-cost rule of include/gmupt.h on the CPU, bit for bit what Renderer.tree_cost() returns for the same
    records (ms = 0).  nodes: an array of bvh_node_dtype; any records do, no link is followed.  The thread count changes no bit."""
    nodes = np.ascontiguousarray(nodes, dtype=bvh_node_dtype)
    ti = TreeCostInfo()
    _check(lib().gmupt_tree_cost_host(_ptr(nodes), nodes.shape[0], C.byref(ti), int(threads)))
    return ti.as_dict()


def tree_optimize_host(nodes, passes=3):
    """gmupt_tree_optimize_host: the treelet optimiser of include/gmupt.h ("Tree optimisation") on the CPU, bit for bit what
    TreeOptimizer.run returns for the same records.  Returns (nodes, info dict); ms = 0."""
    nodes = np.ascontiguousarray(nodes, dtype=bvh_node_dtype)
    out = np.zeros(max(nodes.shape[0], 1), dtype=bvh_node_dtype)[:nodes.shape[0]]
    pp, info = TreeoptParams(int(passes)), TreeoptInfo()
    _check(lib().gmupt_tree_optimize_host(_ptr(nodes), nodes.shape[0], C.byref(pp), _ptr(out), C.byref(info)))
    return out, info.as_dict()


class TreeOptimizer:
    """gmupt_treeopt: the GPU treelet optimiser of one device -- a stream and the scratch of the largest tree optimised so far."""

    def __init__(self, dev):
        self.dev = dev
        self.h = _P()
        _check(lib().gmupt_treeopt_create(dev.h, C.byref(self.h)))

    def run(self, nodes, passes=3):
        """gmupt_treeopt_run on `nodes`, a Buffer of kind BUFFER_BVH_NODES (left as it is).  Returns (a new nodes Buffer the caller closes,
        info dict)."""
        out, info = _P(), TreeoptInfo()
        pp = TreeoptParams(int(passes))
        _check(lib().gmupt_treeopt_run(self.h, nodes.h, C.byref(pp), C.byref(out), C.byref(info)))
        return Buffer.wrap(self.dev, out), info.as_dict()

    def close(self):
        if self.h:
            lib().gmupt_treeopt_destroy(self.h)
            self.h = _P()


class Lbvh:
    """gmupt_lbvh: the GPU LBVH builder of one device -- a stream and the scratch of the largest mesh built so far, kept between builds."""

    def __init__(self, dev):
        self.dev = dev
        self.h = _P()
        _check(lib().gmupt_lbvh_create(dev.h, C.byref(self.h)))
        self.optimizer = None     # the TreeOptimizer of build(optimize=...), created by the first such build

    def build(self, vertex_buffer, indices, vertex_material=None, max_leaf_size=4, ref_triangle=False, optimize=0):
        """gmupt_lbvh_build on the device-resident vertices of `vertex_buffer` (a Buffer of kind BUFFER_VERTICES).  indices / vertex_material:
        torch device tensors (int32 / a 4-byte integer type, used in place) or numpy arrays (uploaded).  Returns (nodes Buffer, tris Buffer,
        info dict); the caller closes the buffers.  ref_triangle=True adds info["ref_triangle"], the source triangle of every record.
        optimize=N > 0 runs N passes of the treelet optimiser (TreeOptimizer.run) on the new tree: the nodes Buffer is the optimised one,
        info["optimize"] its info dict and info["depth"] the new depth; an optimiser error (a tree that became too deep) is raised and no
        buffer is left behind."""
        import torch
        device = torch.device("cuda", self.dev.index)

        def on_device(x, dtype):
            if isinstance(x, torch.Tensor):
                if x.device != device or x.element_size() != 4 or x.is_floating_point():
                    raise GmuptError("Lbvh.build: a tensor must hold 4-byte integers on %s" % device, -1)
                return x.contiguous()
            arr = np.ascontiguousarray(x, dtype=dtype)
            return torch.from_numpy(arr.view(np.int32)).to(device)      # (the bits; torch has no arithmetic on uint32 and needs none here)

        idx = on_device(indices, np.int32).reshape(-1)
        n = idx.numel() // 3
        vm = on_device(vertex_material, np.uint32).reshape(-1) if vertex_material is not None else None
        nverts = int(lib().gmupt_buffer_size(vertex_buffer.h)) // 12
        if vm is not None and vm.numel() < nverts:
            raise GmuptError("Lbvh.build: %d vertex materials for %d vertices" % (vm.numel(), nverts), -1)
        ref = torch.empty(max(n, 1), dtype=torch.int32, device=device) if ref_triangle else None
        torch.cuda.synchronize(device)    # the builder has its own stream: uploads and the caller's writes are done before it starts
        nodes, tris, info = _P(), _P(), LbvhInfo()
        pp = LbvhParams(int(max_leaf_size))
        _check(lib().gmupt_lbvh_build(self.h, vertex_buffer.h, idx.data_ptr(), n, vm.data_ptr() if vm is not None else None, C.byref(pp),
                                      C.byref(nodes), C.byref(tris), ref.data_ptr() if ref is not None else None, C.byref(info)))
        out = info.as_dict()
        if ref is not None:
            out["ref_triangle"] = ref[:n].cpu().numpy()
        nodes, tris = Buffer.wrap(self.dev, nodes), Buffer.wrap(self.dev, tris)
        if optimize:
            if self.optimizer is None:
                self.optimizer = TreeOptimizer(self.dev)
            try:
                better, out["optimize"] = self.optimizer.run(nodes, passes=optimize)
            except GmuptError:
                tris.close()
                raise
            finally:
                nodes.close()
            nodes = better
            out["depth"] = out["optimize"]["depth_after"]
        return nodes, tris, out

    def close(self):
        if self.optimizer is not None:
            self.optimizer.close()
            self.optimizer = None
        if self.h:
            lib().gmupt_lbvh_destroy(self.h)
            self.h = _P()

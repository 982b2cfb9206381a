"""The host camera and the renderer."""
import ctypes as C

import numpy as np

from ._abi import (_P, ERR_CAST_FAULT, ERR_INVALID_ARGUMENT, PATHCOUNT, PREVIEW_MOTION, STATE_BYTES, TRAVTABLE_KINDS, CameraBuffer,
                   ConvergeInfo, GmuptError, Hit, Ray, RefitInfo, RendererDesc, Stats, TraceInfo, TreeCostInfo, _info_dict)
from ._lib import _check, _ptr, lib
from ._stage import Handle, device_tensor, torch_device
from .converge import Converge, converge_params
from .denoise import _infill_arg, denoise_params, temporal_params


class Camera(Handle):
    """Host camera (gmupt_camera_*): Camera::update / setRotation / updateResolution of the reference."""
    _destroy = "gmupt_camera_destroy"

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
        # the live handles of this renderer by class (Handle._siblings): closed before it
        self._temporals, self._normals, self._poses, self._converges, self._adaptives = [], [], [], [], []

    def bind_scene(self, sb):
        self._scene = sb  # keep the buffers alive
        _check(lib().gmupt_renderer_bind_scene(self.h, *[b.h for b in sb.all()]))
        _check(lib().gmupt_renderer_bind_textures(self.h, *[(t.h if t is not None else None) for t in sb.textures]))

    def refit(self):
        """gmupt_renderer_refit after the vertex buffer was updated: the info fields as a dict."""
        info = RefitInfo()
        _check(lib().gmupt_renderer_refit(self.h, C.byref(info)))
        return _info_dict(info)

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
        torch, dev = torch_device(self.dev)
        as_numpy = isinstance(closest, np.ndarray) or isinstance(any, np.ndarray)

        def stage(a):
            if a is None:
                return torch.empty((0, 8), dtype=torch.float32, device=dev)
            return device_tensor(a, dev, np.float32, (-1, 8), lambda t: t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 8 and t.is_cuda,
                                 "trace: rays must be (N, 8) float32 on the GPU (or numpy)")

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

    def _frame(self, info, channels, call):
        """What the frame calls below share: an (H, W, n) float32 tensor on this renderer's GPU for each n of `channels`, torch's current
        stream synchronised, then call(pointer and byte count of each tensor in turn, TraceInfo), the tail of every such C function's
        arguments.  Returns (the tensors, the TraceInfo) for the caller's last_* attribute."""
        torch, dev = torch_device(self.dev)
        outs = [torch.empty((self.height, self.width, n), dtype=torch.float32, device=dev) for n in channels]
        torch.cuda.current_stream(dev).synchronize()
        ti = info if info is not None else TraceInfo()
        _check(call(*[x for o in outs for x in (C.c_void_p(o.data_ptr()), o.numel() * 4)], C.byref(ti)))
        return outs, ti

    # AOV buffers (gmupt_render_aovs)
    def aovs(self, samples=1, info=None):
        """The per-pixel G-buffer of the current camera's rays over this renderer's framebuffer rectangle (the tile in tile mode):
        a (H, W, 16) float32 torch tensor on this renderer's GPU, one 64-byte gmupt_aov record per pixel (include/gmupt.h states the
        semantics; aov_fields() splits it -- words 12-15 are integers, compare them as bits).  samples: 1..8 (s*s stratified rays per pixel
        for the filtered albedo / normal planes when > 1).  torch's current stream is synchronised first; the call itself synchronises the
        renderer's stream.  info: optional TraceInfo to fill."""
        (out,), self.last_aovs = self._frame(info, (16,), lambda *tail: lib().gmupt_render_aovs(self.h, int(samples), *tail))
        return out

    # motion plane (gmupt_render_aovs_motion)
    def aovs_motion(self, prev_verts, samples=1, info=None):
        """aovs() plus the motion plane against `prev_verts`: a float32 torch tensor on this renderer's GPU with the previous position of
        every vertex of the bound vertex buffer ((V, 3) or flat).  Returns (aov (H, W, 16), motion (H, W, 4)) float32 torch tensors; a
        motion record is gmupt_motion (motion_fields() splits it -- word 3 is an integer, compare it as bits)."""
        torch, dev = torch_device(self.dev)
        if not hasattr(prev_verts, "is_cuda") or not prev_verts.is_cuda or prev_verts.dtype != torch.float32 or prev_verts.numel() % 3:
            raise GmuptError("aovs_motion: prev_verts must be a float32 tensor of 3 floats per vertex on the GPU", ERR_INVALID_ARGUMENT)
        if prev_verts.device.index != dev.index:
            raise GmuptError("aovs_motion: prev_verts lives on %s, the renderer on %s" % (prev_verts.device, dev), ERR_INVALID_ARGUMENT)
        pv = prev_verts.contiguous()
        (out, mv), self.last_aovs = self._frame(info, (16, 4), lambda *tail: lib().gmupt_render_aovs_motion(
            self.h, int(samples), C.c_void_p(pv.data_ptr()), pv.numel() // 3, *tail))
        return out, mv

    # denoiser (gmupt_render_denoised)
    def denoise(self, aov_samples=1, info=None, **params):
        """The a-trous denoiser on this renderer's frame (the tile in tile mode): gmupt_render_aovs(aov_samples) into internal scratch,
        a copy of the framebuffer, then the filter (include/gmupt.h states it).  Returns an (H, W, 4) float32 torch tensor on this
        renderer's GPU: rgb denoised, alpha the sample-count bits of the frame.  params: passes, sigma_color, sigma_normal, sigma_plane,
        sigma_albedo (the rest keep gmupt_denoise_default_params).  info: optional TraceInfo to fill (ms = AOVs + filter)."""
        dp = denoise_params(**params)
        (out,), self.last_denoise = self._frame(info, (4,), lambda *tail: lib().gmupt_render_denoised(self.h, int(aov_samples), C.byref(dp), *tail))
        return out

    # temporal reuse (gmupt_render_denoised_temporal)
    def denoise_temporal(self, handle, aov_samples=1, info=None, **params):
        """The denoiser with temporal reuse on this renderer's frame (the tile in tile mode): AOVs and a framebuffer copy as denoise(),
        then the frame integrated with the reprojected history of `handle` (a Temporal of this renderer) and filtered.  The first call
        after an iteration that cleared the frame, or after a resize, starts a new accumulation epoch (include/gmupt.h).  Returns an
        (H, W, 4) float32 torch tensor on this renderer's GPU: rgb denoised, alpha the effective sample-count bits.  params: the
        temporal_params fields.  info: optional TraceInfo to fill (ms = AOVs + integration + filter)."""
        tp = temporal_params(**params)
        (out,), self.last_denoise = self._frame(info, (4,), lambda *tail: lib().gmupt_render_denoised_temporal(
            self.h, handle.h, int(aov_samples), C.byref(tp), *tail))
        return out

    def denoise_temporal_motion(self, handle, aov_samples=1, info=None, **params):
        """denoise_temporal() for geometry that moves (gmupt_render_denoised_temporal_motion): the handle keeps the vertex pose of its
        record sets, and after a refit() the history is looked up where each surface point was.  Without a refit since the history
        was written it is denoise_temporal() bit for bit."""
        tp = temporal_params(**params)
        (out,), self.last_denoise = self._frame(info, (4,), lambda *tail: lib().gmupt_render_denoised_temporal_motion(
            self.h, handle.h, int(aov_samples), C.byref(tp), *tail))
        return out

    # preview chain (gmupt_render_preview)
    def preview(self, temporal=None, motion=False, aov_samples=1, infill=None, info=None, **params):
        """The preview of this renderer's frame in one call (gmupt_render_preview): AOVs -> integration with the history of `temporal`
        (a Temporal of this renderer, or None) -> guided infill -> the a-trous filter.  infill: None (off: the call is denoise(),
        denoise_temporal() or, with motion=True, denoise_temporal_motion() bit for bit), True (gmupt_infill_default_params) or a dict
        of infill_params fields.  params: the temporal_params fields (without a handle only the spatial ones are read).  Returns an
        (H, W, 4) float32 torch tensor on this renderer's GPU; a filled pixel has the alpha bits of sample count 1.  info: optional
        TraceInfo to fill, as for denoise() (ms = AOVs + integration + infill + filter)."""
        tp = temporal_params(**params)
        ip = _infill_arg(infill)
        (out,), self.last_denoise = self._frame(info, (4,), lambda *tail: lib().gmupt_render_preview(
            self.h, temporal.h if temporal is not None else None, PREVIEW_MOTION if motion else 0, int(aov_samples), C.byref(tp),
            C.byref(ip) if ip is not None else None, *tail))
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
            for t in self._temporals + self._normals + self._poses + self._converges + self._adaptives:
                t.close()
            lib().gmupt_renderer_destroy(self.h)
            self.h = _P()

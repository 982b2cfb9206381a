"""The denoiser, the guided infill and temporal reuse on caller images: their parameter builders, the *_image calls on device tensors,
the *_host restatements on the CPU, and the Temporal history handle."""
import ctypes as C

import numpy as np

from ._abi import (ERR_INVALID_ARGUMENT, DenoiseParams, GmuptError, InfillInfo, InfillParams, TemporalParams, history_dtype,
                   motion_dtype)
from ._lib import _check, _ptr, lib
from ._stage import Handle, device_images, host_images, host_words, make_params

_SPATIAL_FIELDS = ("passes", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo")
TEMPORAL_FIELDS = ("history_cap", "min_normal_cos", "plane_dist")


def denoise_params(**params):
    """gmupt_denoise_default_params with the given fields replaced (passes, sigma_color, sigma_normal, sigma_plane, sigma_albedo)."""
    return make_params(DenoiseParams, "gmupt_denoise_default_params", "denoiser", params, _SPATIAL_FIELDS)


def infill_params(**params):
    """gmupt_infill_default_params with the given fields replaced (passes, sigma_normal, sigma_plane, sigma_albedo)."""
    return make_params(InfillParams, "gmupt_infill_default_params", "infill", params, ("passes", "sigma_normal", "sigma_plane", "sigma_albedo"))


def temporal_params(**params):
    """gmupt_temporal_default_params with the given fields replaced: history_cap, min_normal_cos, plane_dist, and the spatial filter's
    passes, sigma_color, sigma_normal, sigma_plane, sigma_albedo."""
    return make_params(TemporalParams, "gmupt_temporal_default_params", "temporal denoiser", params, TEMPORAL_FIELDS, "spatial", _SPATIAL_FIELDS)


def _infill_arg(infill):
    """The `infill` keyword of the preview calls: None / False -> None (off), True -> the defaults, a dict -> infill_params(**dict)."""
    if infill is None or infill is False:
        return None
    if isinstance(infill, InfillParams):
        return infill
    return infill_params(**({} if infill is True else dict(infill)))


class Temporal(Handle):
    """gmupt_temporal: the history of one renderer's denoised frames (two record sets: the frozen history of earlier accumulations and
    the records of the latest call).  It uses the renderer's device and stream and is closed with it at the latest."""
    _destroy, _siblings = "gmupt_temporal_destroy", "_temporals"

    def __init__(self, renderer):
        self.renderer = renderer
        self._open(renderer, "gmupt_temporal_create")

    def reset(self):
        """Drops both record sets: the next output is the plain spatial denoise."""
        _check(lib().gmupt_temporal_reset(self.h))


def denoise_image(renderer, beauty, aov, ms=None, **params):
    """gmupt_denoise_image on torch tensors on the renderer's GPU: beauty (H, W, 4) float32 (a = sample-count bits), aov (H, W, 16)
    float32 gmupt_aov records.  Returns the (H, W, 4) float32 result.  Any image size; enqueued on the renderer's stream after torch's
    current stream is synchronised.  ms: optional list that receives the filter's device time."""
    import torch
    beauty, aov = device_images("denoise_image", beauty, aov)
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
    b, a = host_images("denoise_host", beauty, aov)
    out = np.empty_like(b)
    dp = denoise_params(**params)
    _check(lib().gmupt_denoise_host(_ptr(b), _ptr(a), b.shape[1], b.shape[0], C.byref(dp), _ptr(out), out.nbytes, int(threads)))
    return out


def infill_image(renderer, beauty, aov, info=False, **params):
    """gmupt_infill_image on torch tensors on the renderer's GPU: beauty (H, W, 4) float32 (a = sample-count bits), aov (H, W, 16)
    float32 gmupt_aov records.  Returns the (H, W, 4) float32 result, enqueued on the renderer's stream after torch's current stream is
    synchronised; with info=True the call waits and returns (result, info dict), otherwise the renderer's stream is synchronised
    before the tensor is handed to torch.  params: the infill_params fields."""
    import torch
    beauty, aov = device_images("infill_image", beauty, aov)
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
    b, a = host_images("infill_host", beauty, aov)
    out = np.empty_like(b)
    ip = infill_params(**params)
    ii = InfillInfo()
    _check(lib().gmupt_infill_host(_ptr(b), _ptr(a), b.shape[1], b.shape[0], C.byref(ip), _ptr(out), out.nbytes, C.byref(ii), int(threads)))
    return out, ii.as_dict()


def temporal_denoise_image(handle, beauty, aov, cam_buffer, new_accumulation, origin=(0, 0), ms=None, motion=None, infill=None, **params):
    """gmupt_temporal_denoise_image on torch tensors on the handle's GPU: beauty (H, W, 4) float32 (a = sample-count bits), aov (H, W, 16)
    float32 records, rendered with cam_buffer (a CameraBuffer) at `origin` of its whole frame.  new_accumulation: move the latest
    call's records into the history first.  Returns the (H, W, 4) float32 result.  ms: optional list that receives the device time.
    motion: an (H, W, 4) float32 tensor of gmupt_motion records on the same GPU (gmupt_temporal_denoise_image_motion), or None.
    infill: None, or True / a dict of infill_params fields: the call goes through gmupt_temporal_preview_image, with the guided infill
    between the integration and the filter."""
    import torch
    beauty, aov = device_images("temporal_denoise_image", beauty, aov)
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
    # (handle, beauty, aov[, motion], camera, origin, size, new accumulation, params[, infill params], out, bytes, ms) for all three
    images = [C.c_void_p(beauty.data_ptr()), C.c_void_p(aov.data_ptr())]
    frame = [C.byref(cam_buffer), int(origin[0]), int(origin[1]), W, H, 1 if new_accumulation else 0, C.byref(tp)]
    result = [C.c_void_p(out.data_ptr()), out.numel() * 4, C.byref(t)]
    if ip is not None:
        mp = C.c_void_p(motion.data_ptr()) if motion is not None else None
        _check(lib().gmupt_temporal_preview_image(handle.h, *images, mp, *frame, C.byref(ip), *result))
    elif motion is not None:
        _check(lib().gmupt_temporal_denoise_image_motion(handle.h, *images, C.c_void_p(motion.data_ptr()), *frame, *result))
    else:
        _check(lib().gmupt_temporal_denoise_image(handle.h, *images, *frame, *result))
    if ms is not None:
        ms.append(t.value)
    return out


def temporal_integrate_host(beauty, aov, prev=None, prev_cam=None, prev_origin=(0, 0), threads=16, **params):
    """gmupt_temporal_integrate_host: the integration step on the CPU, bit for bit the device's.  beauty (H, W, 4) float32, aov (H, W, 16)
    float32 (or aov_dtype); prev: an (h, w) history_dtype array (or (h, w, 12) float32) rendered with prev_cam at prev_origin, or None.
    Returns (integrated (H, W, 4) float32, history (H, W) history_dtype) as numpy arrays."""
    return _integrate_host("temporal_integrate_host", beauty, aov, None, prev, prev_cam, prev_origin, threads, params)


def temporal_integrate_motion_host(beauty, aov, motion, prev=None, prev_cam=None, prev_origin=(0, 0), threads=16, **params):
    """gmupt_temporal_integrate_motion_host: temporal_integrate_host with a motion plane -- (H, W) motion_dtype records or (H, W, 4)
    float32, numpy or torch; None = temporal_integrate_host.  Returns (integrated, history) as that function."""
    return _integrate_host("temporal_integrate_motion_host", beauty, aov, motion, prev, prev_cam, prev_origin, threads, params)


def _integrate_host(who, beauty, aov, motion, prev, prev_cam, prev_origin, threads, params):
    """Both integrate_host functions: gmupt_<who>, which takes the motion plane (a null pointer for none) only in the motion form."""
    b, a = host_images(who, beauty, aov)
    H, W = b.shape[:2]
    mp = None
    if motion is not None:
        m = host_words(motion, motion_dtype)
        if m.shape != (H, W, 4):
            raise GmuptError("%s: motion must be (H, W) records" % who, ERR_INVALID_ARGUMENT)
        mp = _ptr(m)
    ph = pw = 0
    pp = None
    if prev is not None:
        pv = np.asarray(prev)
        if pv.dtype != history_dtype:
            pv = np.ascontiguousarray(pv, dtype=np.float32).view(history_dtype)[..., 0]
        pv = np.ascontiguousarray(pv)
        if pv.ndim != 2:
            raise GmuptError("%s: prev must be (h, w) records" % who, ERR_INVALID_ARGUMENT)
        ph, pw = pv.shape
        pp = _ptr(pv)
    out = np.empty_like(b)
    hist = np.empty((H, W), history_dtype)
    tp = temporal_params(**params)
    rest = (W, H, pp, C.byref(prev_cam) if prev_cam is not None else None, int(prev_origin[0]), int(prev_origin[1]), pw, ph, C.byref(tp),
            _ptr(out), _ptr(hist), int(threads))
    if who == "temporal_integrate_motion_host":
        _check(lib().gmupt_temporal_integrate_motion_host(_ptr(b), _ptr(a), mp, *rest))
    else:
        _check(lib().gmupt_temporal_integrate_host(_ptr(b), _ptr(a), *rest))
    return out, hist

"""Adaptive sampling (include/gmupt_adaptive.h), reached as capi.adaptive.NAME: the structures and prototypes of its part
of the C-ABI, its parameter builder, the Adaptive handle of a renderer (a sampling plan), what attaches a plan to a renderer and
renders with it, and the two rules on the CPU.  The module keeps its ABI itself and adds nothing to capi's own names, to the Renderer
class or to capi.SYMBOLS: those are the recorded surface of the binding."""
import ctypes as C

import numpy as np

from ._abi import _EXTRA_SYMBOLS, _P, ERR_INVALID_ARGUMENT, ConvergeInfo, ConvergeParams, GmuptError, _AsDict
from ._lib import _check, _ptr, lib
from ._stage import Handle, make_params, torch_device
from .converge import converge_params


class AdaptiveParams(C.Structure):
    """gmupt_adaptive_params: 12 bytes (threshold finite and > 0; max_repeat 1..64; uniform_every 0 = off)."""
    _fields_ = [("threshold", C.c_float), ("max_repeat", C.c_uint32), ("uniform_every", C.c_uint32)]


class AdaptiveInfo(_AsDict, C.Structure):
    """gmupt_adaptive_info: 32 bytes."""
    _fields_ = [("pixels", C.c_uint32), ("active", C.c_uint32), ("entries", C.c_uint32), ("skipped_nonfinite", C.c_uint32), ("max_rep", C.c_uint32),
                ("pad", C.c_uint32), ("ms", C.c_double)]


assert C.sizeof(AdaptiveParams) == 12 and C.sizeof(AdaptiveInfo) == 32

# name -> (restype, argtypes), as capi.SYMBOLS; bound with it on every load (_abi._EXTRA_SYMBOLS)
SYMBOLS = {
    "gmupt_adaptive_default_params": (None, [C.POINTER(AdaptiveParams)]),
    "gmupt_adaptive_select_host": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(AdaptiveParams), _P, C.c_size_t, C.POINTER(AdaptiveInfo)]),
    "gmupt_adaptive_pixel_host": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gmupt_adaptive_create": (C.c_int, [_P, C.POINTER(_P)]),
    "gmupt_adaptive_destroy": (None, [_P]),
    "gmupt_adaptive_select": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveInfo)]),
    "gmupt_adaptive_set_list": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "gmupt_adaptive_read_list": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_uint32)]),
    "gmupt_renderer_set_adaptive": (C.c_int, [_P, _P]),
    "gmupt_render_adaptive": (C.c_int, [_P, _P, _P, _P, C.POINTER(ConvergeParams), C.POINTER(AdaptiveParams), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(ConvergeInfo), C.POINTER(AdaptiveInfo)]),
}
_EXTRA_SYMBOLS.update(SYMBOLS)


def adaptive_params(**params):
    """gmupt_adaptive_default_params with the given fields replaced (threshold, max_repeat, uniform_every)."""
    return make_params(AdaptiveParams, "gmupt_adaptive_default_params", "adaptive sampling", params, ("threshold", "max_repeat", "uniform_every"))


class Adaptive(Handle):
    """gmupt_adaptive: a sampling plan of one renderer: a list of pixels that the renderer, once the plan is attached (set_adaptive),
    aims its fresh camera paths at.  It uses the renderer's device and stream and is closed with it at the latest."""
    _destroy, _siblings = "gmupt_adaptive_destroy", "_adaptives"

    def __init__(self, renderer):
        self.renderer = renderer
        self._open(renderer, "gmupt_adaptive_create")

    def select(self, error, **params):
        """gmupt_adaptive_select: the plan from an (H, W) float32 error plane on the renderer's GPU (torch; what Converge.update(error=True)
        returns) under threshold, max_repeat and uniform_every.  torch's current stream is synchronised first.  Returns the info dict."""
        torch, device = torch_device(self.renderer.dev)
        if not isinstance(error, torch.Tensor) or error.dim() != 2 or error.dtype != torch.float32 or error.device != device:
            raise GmuptError("select: an (H, W) float32 tensor on %s" % device, ERR_INVALID_ARGUMENT)
        error = error.contiguous()
        ap = adaptive_params(**params)
        ai = AdaptiveInfo()
        torch.cuda.current_stream(device).synchronize()
        _check(lib().gmupt_adaptive_select(self.h, C.c_void_p(error.data_ptr()), int(error.shape[1]), int(error.shape[0]), C.byref(ap), C.byref(ai)))
        return ai.as_dict()

    def set_list(self, pixels, width, height, uniform_every=0):
        """gmupt_adaptive_set_list: a caller's own list of rectangle-local pixel indices y * width + x (repeats weigh a pixel) as the plan."""
        arr = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        _check(lib().gmupt_adaptive_set_list(self.h, _ptr(arr) if arr.size else None, arr.size, int(width), int(height), int(uniform_every)))

    def list(self):
        """gmupt_adaptive_read_list: the plan's list as a uint32 array."""
        n = C.c_uint32(0)
        _check(lib().gmupt_adaptive_read_list(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if n.value:
            _check(lib().gmupt_adaptive_read_list(self.h, _ptr(out), out.nbytes, C.byref(n)))
        return out


def set_adaptive(renderer, plan):
    """gmupt_renderer_set_adaptive: attaches `plan` (an Adaptive of this renderer) -- from the next iteration on the fresh camera paths
    go to the pixels of its list -- or, with None, detaches: the iterations are again what they always were."""
    _check(lib().gmupt_renderer_set_adaptive(renderer.h, plan.h if plan is not None else None))


def render_adaptive(renderer, camera, converge, plan, check_every=8, max_iterations=1 << 20, max_repeat=1, uniform_every=0, adaptive_threshold=0.0,
                    **params):
    """gmupt_render_adaptive: Renderer.render_until() with the plan in it -- after every check that does not end the loop the monitor's
    error plane becomes the plan of the next check_every iterations.  params: the converge_params fields; adaptive_threshold 0 = the
    monitor's threshold.  Returns the last check's info dict with "iterations" added and, under "plan", the last selection's info
    dict (all zero when none ran)."""
    cp = converge_params(**params)
    ap = adaptive_params(threshold=adaptive_threshold, max_repeat=max_repeat, uniform_every=uniform_every)
    it = C.c_uint32(0)
    ci, ai = ConvergeInfo(), AdaptiveInfo()
    _check(lib().gmupt_render_adaptive(renderer.h, camera.h, converge.h, plan.h, C.byref(cp), C.byref(ap), check_every, max_iterations, C.byref(it),
                                       C.byref(ci), C.byref(ai)))
    out = ci.as_dict()
    if out["pixels"]:
        converge._size = (renderer.height, renderer.width)
    out["iterations"] = it.value
    out["plan"] = ai.as_dict()
    return out


def adaptive_select_host(error, **params):
    """gmupt_adaptive_select_host: the selection rule on the CPU, bit for bit what Adaptive.select() computes.  error: (H, W) float32.
    Returns (list as a uint32 array, info dict)."""
    error = np.ascontiguousarray(error, dtype=np.float32)
    if error.ndim != 2:
        raise GmuptError("adaptive_select_host: error must be (H, W) float32", ERR_INVALID_ARGUMENT)
    ap = adaptive_params(**params)
    ai = AdaptiveInfo()
    H, W = error.shape
    _check(lib().gmupt_adaptive_select_host(_ptr(error), W, H, C.byref(ap), None, 0, C.byref(ai)))
    out = np.zeros(ai.entries, np.uint32)
    if ai.entries:
        _check(lib().gmupt_adaptive_select_host(_ptr(error), W, H, C.byref(ap), _ptr(out), out.size, C.byref(ai)))
    return out, ai.as_dict()


def adaptive_pixel_host(pixels, uniform_every, width, height, k):
    """gmupt_adaptive_pixel_host: the pixel of the width * height rectangle that the fresh camera path k goes to under the plan."""
    arr = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
    pix = C.c_uint32(0)
    _check(lib().gmupt_adaptive_pixel_host(_ptr(arr) if arr.size else None, arr.size, int(uniform_every), int(width), int(height), int(k) & 0xFFFFFFFF, C.byref(pix)))
    return pix.value

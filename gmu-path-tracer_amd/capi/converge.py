"""The convergence monitor: its parameter builder, the Converge handle of a renderer and the rule on the CPU."""
import ctypes as C

import numpy as np

from ._abi import ERR_INVALID_ARGUMENT, ConvergeInfo, ConvergeParams, GmuptError, converge_pixel_dtype
from ._lib import _check, _ptr, lib
from ._stage import Handle, make_params, torch_device


def converge_params(**params):
    """gmupt_converge_default_params with the given fields replaced (threshold, min_batches, allow_pixels)."""
    return make_params(ConvergeParams, "gmupt_converge_default_params", "convergence", params, ("threshold", "min_batches", "allow_pixels"))


class Converge(Handle):
    """gmupt_converge: the convergence monitor of one renderer (include/gmupt.h "Convergence"): a per-pixel batch-mean state from which
    every update estimates the standard error of the pixel's tone-mapped luminance mean.  It uses the renderer's device and stream and
    is closed with it at the latest."""
    _destroy, _siblings = "gmupt_converge_destroy", "_converges"

    def __init__(self, renderer):
        self.renderer = renderer
        self._size = None   # (H, W) of the state, once an update has run
        self._open(renderer, "gmupt_converge_create")

    def update(self, error=False, **params):
        """gmupt_converge_update on the renderer's accumulation target, behind its pending iterations.  Returns the info dict; with
        error=True (info, error plane), the plane an (H, W) float32 torch tensor on the renderer's GPU (-1 = unknown)."""
        cp = converge_params(**params)
        ci = ConvergeInfo()
        H, W = self.renderer.height, self.renderer.width
        err = None
        if error:
            torch, device = torch_device(self.renderer.dev)
            err = torch.empty((H, W), dtype=torch.float32, device=device)
            torch.cuda.current_stream(device).synchronize()
        _check(lib().gmupt_converge_update(self.h, C.byref(cp), C.c_void_p(err.data_ptr()) if error else None, C.byref(ci)))
        self._size = (H, W)
        return (ci.as_dict(), err) if error else ci.as_dict()

    def update_image(self, tensor, error=False, **params):
        """gmupt_converge_update_image on an (H, W, 4) float32 torch tensor on the renderer's GPU (a = sample-count bits), e.g. a
        gathered frame.  torch's current stream is synchronised first.  Returns as update()."""
        torch, device = torch_device(self.renderer.dev)
        if not isinstance(tensor, torch.Tensor) or tensor.dim() != 3 or tensor.shape[2] != 4 or tensor.dtype != torch.float32 or tensor.device != device:
            raise GmuptError("update_image: an (H, W, 4) float32 tensor on %s" % device, ERR_INVALID_ARGUMENT)
        tensor = tensor.contiguous()
        H, W = int(tensor.shape[0]), int(tensor.shape[1])
        cp = converge_params(**params)
        ci = ConvergeInfo()
        err = torch.empty((H, W), dtype=torch.float32, device=device) if error else None
        torch.cuda.current_stream(device).synchronize()
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

"""Lens-filtered AOV planes (include/gmupt_lens_aov.h), reached as capi.lens_aov.NAME: the guide records of a frame with depth of
field, the rays they are made of on the CPU, and the denoiser on them.  Like capi.lens the module keeps its prototypes itself and
adds nothing to capi's own names, to the Renderer class or to capi.SYMBOLS: those are the recorded surface of the binding."""
import ctypes as C

from . import _stage
from ._abi import _EXTRA_SYMBOLS, _P, CameraBuffer, DenoiseParams, Ray, TraceInfo
from ._lib import _check, lib
from .denoise import denoise_params
from .lens import Lens

# name -> (restype, argtypes), as capi.SYMBOLS; bound with it on every load (_abi._EXTRA_SYMBOLS)
SYMBOLS = {
    "gmupt_render_aovs_lens": (C.c_int, [_P, C.POINTER(Lens), C.c_uint32, _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_aov_lens_ray": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Ray)]),
    "gmupt_render_denoised_lens": (C.c_int, [_P, C.POINTER(Lens), C.c_uint32, C.POINTER(DenoiseParams), _P, C.c_size_t, C.POINTER(TraceInfo)]),
}
_EXTRA_SYMBOLS.update(SYMBOLS)


def aovs(renderer, samples=1, lens=None, info=None):
    """gmupt_render_aovs_lens: the G-buffer of the renderer's rectangle seen through `lens` (a capi.lens.Lens; None = the lens attached
    to the renderer, a pinhole when none is) -- samples * samples rays per pixel, each pixel-filter cell through its own lens stratum.
    Returns an (H, W, 16) float32 torch tensor on the renderer's GPU shaped like Renderer.aovs (capi.aov_fields splits it); the
    renderer's last_aovs is its TraceInfo.  The renderer's frame, state and attached lens are not touched."""
    (out,), renderer.last_aovs = renderer._frame(info, (16,), lambda *tail: lib().gmupt_render_aovs_lens(renderer.h, _stage.opt_ref(lens), int(samples), *tail))
    return out


def aov_lens_ray(cam_buffer, lens, x, y, samples, k):
    """gmupt_aov_lens_ray (host only): ray k = b*s + a of whole-frame pixel (x, y) at `samples` under `lens`."""
    ray = Ray()
    _check(lib().gmupt_aov_lens_ray(C.byref(cam_buffer), C.byref(lens), int(x), int(y), int(samples), int(k), C.byref(ray)))
    return ray


def aov_lens_rays(cam_buffer, lens, xs, ys, samples):
    """All lens AOV rays of the pixels (xs[i], ys[i]) as an (N, R, 8) float32 array of gmupt_ray records (R = samples^2)."""
    return _stage.aov_ray_table(lib().gmupt_aov_lens_ray, cam_buffer, lens, xs, ys, samples)


def guided_inputs(renderer, aov_samples=1, lens=None):
    """What an *_image stage takes for a frame with depth of field: (beauty, aov), the renderer's frame as an (H, W, 4) float32 tensor
    (gmupt_copy_framebuffer_to_device) and the lens records of aovs(renderer, aov_samples, lens), both on the renderer's GPU."""
    return _stage.guided_inputs(renderer, aovs(renderer, aov_samples, lens))


def denoise(renderer, aov_samples=1, lens=None, info=None, **params):
    """gmupt_render_denoised_lens: Renderer.denoise with the lens records of aovs(renderer, aov_samples, lens) as the guides.
    Returns an (H, W, 4) float32 torch tensor on the renderer's GPU; params: the denoise_params fields."""
    dp = denoise_params(**params)
    (out,), renderer.last_denoise = renderer._frame(info, (4,), lambda *tail: lib().gmupt_render_denoised_lens(
        renderer.h, _stage.opt_ref(lens), int(aov_samples), C.byref(dp), *tail))
    return out

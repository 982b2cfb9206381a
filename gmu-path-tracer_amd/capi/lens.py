"""The thin lens (include/gmupt_lens.h), reached as capi.lens.NAME: the structure and prototypes of its part of the C-ABI,
what attaches a lens to a renderer, the autofocus and the rule on the CPU.  Like capi.adaptive the module keeps its ABI itself and adds
nothing to capi's own names, to the Renderer class or to capi.SYMBOLS: those are the recorded surface of the binding."""
import ctypes as C

import numpy as np

from ._abi import _EXTRA_SYMBOLS, _P, CameraBuffer, Ray
from ._lib import _check, lib
from ._stage import make_params


class Lens(C.Structure):
    """gmupt_lens: 8 bytes, scene units (aperture_radius 0 = a pinhole; focus_distance along the camera's forward axis)."""
    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float)]


assert C.sizeof(Lens) == 8

# name -> (restype, argtypes), as capi.SYMBOLS; bound with it on every load (_abi._EXTRA_SYMBOLS)
SYMBOLS = {
    "gmupt_lens_default_params": (None, [C.POINTER(Lens)]),
    "gmupt_renderer_set_lens": (C.c_int, [_P, C.POINTER(Lens)]),
    "gmupt_renderer_get_lens": (C.c_int, [_P, C.POINTER(Lens)]),
    "gmupt_lens_ray_host": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Lens), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Ray)]),
    "gmupt_lens_focus_at": (C.c_int, [_P, C.c_float, C.c_float, C.c_uint32, C.POINTER(Lens)]),
}
_EXTRA_SYMBOLS.update(SYMBOLS)


def lens_params(**params):
    """gmupt_lens_default_params with the given fields replaced (aperture_radius, focus_distance)."""
    return make_params(Lens, "gmupt_lens_default_params", "lens", params, ("aperture_radius", "focus_distance"))


def set_lens(renderer, lens):
    """gmupt_renderer_set_lens: attaches `lens` (a Lens) -- from the next iteration on every fresh camera path starts on the lens disk
    and aims through its focal point -- or, with None or an aperture of 0, detaches: the iterations are again what they always were.
    The frame is not cleared."""
    _check(lib().gmupt_renderer_set_lens(renderer.h, C.byref(lens) if lens is not None else None))


def get_lens(renderer):
    """gmupt_renderer_get_lens: the attached Lens (aperture_radius 0 when none is)."""
    out = Lens()
    _check(lib().gmupt_renderer_get_lens(renderer.h, C.byref(out)))
    return out


def focus_at(renderer, px, py, light_count=0, aperture_radius=0.0):
    """gmupt_lens_focus_at: a Lens of `aperture_radius` focused on what whole-frame pixel (px, py) of the renderer's current camera
    sees (the depth of gmupt_pick's hit along the forward axis).  GmuptError when the pixel sees nothing.  Nothing is attached."""
    out = lens_params(aperture_radius=aperture_radius)
    _check(lib().gmupt_lens_focus_at(renderer.h, float(px), float(py), int(light_count), C.byref(out)))
    return out


def lens_ray_host(cam_buffer, lens, q, cx, cy):
    """gmupt_lens_ray_host: the rule on the CPU, bit for bit what the renderer's lens launch stores -- the Ray of the fresh camera path
    at entry q of the new-path queue whose screen coordinate is whole-frame pixel (cx, cy)."""
    ray = Ray()
    _check(lib().gmupt_lens_ray_host(C.byref(cam_buffer), C.byref(lens), int(q), int(cx), int(cy), C.byref(ray)))
    return ray


def lens_rays_host(cam_buffer, lens, qs, cxs, cys):
    """lens_ray_host for arrays of (q, cx, cy): an (N, 8) float32 array of gmupt_ray records (origin xyz, tmax, direction xyz, pad)."""
    out = np.empty((len(qs), 8), np.float32)
    ray = Ray()
    fn, pc, pl, pr = lib().gmupt_lens_ray_host, C.byref(cam_buffer), C.byref(lens), C.byref(ray)
    for i, (q, cx, cy) in enumerate(zip(qs, cxs, cys)):
        _check(fn(pc, pl, int(q), int(cx), int(cy), pr))
        out[i] = np.frombuffer(ray, np.float32)
    return out

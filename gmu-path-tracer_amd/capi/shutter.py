"""The shutter (include/gmupt_shutter.h), reached as capi.shutter.NAME: camera motion blur -- the structure and prototypes of its part
of the C-ABI, what attaches a close pose to a renderer, and the rule on the CPU.  Like capi.lens the module keeps its ABI itself and
adds nothing to capi's own names, to the Renderer class or to capi.SYMBOLS: those are the recorded surface of the binding."""
import ctypes as C

import numpy as np

from ._abi import _EXTRA_SYMBOLS, _P, CameraBuffer, Ray
from ._lib import _check, lib
from ._stage import opt_ref
from .lens import Lens
from .projection import Projection


class Shutter(C.Structure):
    """gmupt_shutter: 48 bytes, the camera pose at shutter close (t = 1); the renderer's camera is the pose at shutter open."""
    _fields_ = [("position", C.c_float * 3), ("upperLeftCorner", C.c_float * 3), ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3)]


assert C.sizeof(Shutter) == 48

# name -> (restype, argtypes), as capi.SYMBOLS; bound with it on every load (_abi._EXTRA_SYMBOLS)
SYMBOLS = {
    "gmupt_renderer_set_shutter": (C.c_int, [_P, C.POINTER(Shutter)]),
    "gmupt_renderer_get_shutter": (C.c_int, [_P, C.POINTER(Shutter), C.POINTER(C.c_int)]),
    "gmupt_shutter_from_camera": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Shutter)]),
    "gmupt_shutter_camera_host": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Shutter), C.c_float, C.POINTER(CameraBuffer)]),
    "gmupt_shutter_time_host": (C.c_int, [C.POINTER(CameraBuffer), C.c_uint32, C.POINTER(C.c_float)]),
    "gmupt_shutter_ray_host": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Shutter), C.POINTER(Lens), C.POINTER(Projection), C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(Ray)]),
}
_EXTRA_SYMBOLS.update(SYMBOLS)


def from_camera(close_buffer):
    """gmupt_shutter_from_camera: the Shutter whose close pose is that of `close_buffer` (a CameraBuffer)."""
    out = Shutter()
    _check(lib().gmupt_shutter_from_camera(C.byref(close_buffer), C.byref(out)))
    return out


def set_shutter(renderer, shutter):
    """gmupt_renderer_set_shutter: attaches `shutter` (a Shutter) -- from the next iteration on every fresh camera path draws a time
    and its ray is made from the camera interpolated between the renderer's camera and the close pose -- or, with None, detaches: the
    iterations are again what they always were.  The frame is not cleared."""
    _check(lib().gmupt_renderer_set_shutter(renderer.h, opt_ref(shutter)))


def get_shutter(renderer):
    """gmupt_renderer_get_shutter: the attached Shutter, None when none is."""
    out, attached = Shutter(), C.c_int()
    _check(lib().gmupt_renderer_get_shutter(renderer.h, C.byref(out), C.byref(attached)))
    return out if attached.value else None


def camera_host(cam_buffer, shutter, t):
    """gmupt_shutter_camera_host: step 2 of the rule, the CameraBuffer at time t."""
    out = CameraBuffer()
    _check(lib().gmupt_shutter_camera_host(C.byref(cam_buffer), C.byref(shutter), float(t), C.byref(out)))
    return out


def time_host(cam_buffer, q):
    """gmupt_shutter_time_host: step 1 of the rule, the time of the fresh camera path at entry q of the new-path queue."""
    t = C.c_float()
    _check(lib().gmupt_shutter_time_host(C.byref(cam_buffer), int(q), C.byref(t)))
    return t.value


def times_host(cam_buffer, qs):
    """time_host for an array of q: a float32 array."""
    out = np.empty(len(qs), np.float32)
    t = C.c_float()
    fn, pc, pt = lib().gmupt_shutter_time_host, C.byref(cam_buffer), C.byref(t)
    for i, q in enumerate(qs):
        _check(fn(pc, int(q), pt))
        out[i] = t.value
    return out


def ray_host(cam_buffer, shutter, q, cx, cy, lens=None, projection=None):
    """gmupt_shutter_ray_host: the rule on the CPU, bit for bit what the renderer's shutter launch stores -- the Ray of the fresh
    camera path at entry q of the new-path queue whose screen coordinate is whole-frame pixel (cx, cy), under `lens` (a capi.lens.Lens),
    `projection` (a capi.projection.Projection) or neither, the pinhole."""
    ray = Ray()
    _check(lib().gmupt_shutter_ray_host(C.byref(cam_buffer), C.byref(shutter), opt_ref(lens), opt_ref(projection), int(q), int(cx), int(cy), C.byref(ray)))
    return ray


def rays_host(cam_buffer, shutter, qs, cxs, cys, lens=None, projection=None):
    """ray_host for arrays of (q, cx, cy): an (N, 8) float32 array of gmupt_ray records (origin xyz, tmax, direction xyz, pad)."""
    out = np.empty((len(qs), 8), np.float32)
    ray = Ray()
    fn, pc, ps, pl, pp, pr = lib().gmupt_shutter_ray_host, C.byref(cam_buffer), C.byref(shutter), opt_ref(lens), opt_ref(projection), C.byref(ray)
    for i, (q, cx, cy) in enumerate(zip(qs, cxs, cys)):
        _check(fn(pc, ps, pl, pp, int(q), int(cx), int(cy), pr))
        out[i] = np.frombuffer(ray, np.float32)
    return out

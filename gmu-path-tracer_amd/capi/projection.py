"""Camera projections (include/gmupt_projection.h), reached as capi.projection.NAME: orthographic, equidistant fisheye and 360-degree
equirectangular panorama -- the structure and prototypes of their part of the C-ABI, what attaches a projection to a renderer, the
rule and its inverse on the CPU, picking, and the AOV records and the denoiser under a projection.  Like capi.lens the module keeps
its ABI itself and adds nothing to capi's own names, to the Renderer class or to capi.SYMBOLS: those are the recorded surface of the
binding."""
import ctypes as C
import math

import numpy as np

from ._abi import _EXTRA_SYMBOLS, _P, CameraBuffer, DenoiseParams, Hit, Ray, TraceInfo
from ._lib import _check, lib
from . import _stage
from .denoise import denoise_params

PINHOLE, ORTHOGRAPHIC, FISHEYE, EQUIRECT = 0, 1, 2, 3
KINDS = {"pinhole": PINHOLE, "orthographic": ORTHOGRAPHIC, "ortho": ORTHOGRAPHIC, "fisheye": FISHEYE, "equirect": EQUIRECT}


class Projection(C.Structure):
    """gmupt_projection: 16 bytes (kind: one of PINHOLE / ORTHOGRAPHIC / FISHEYE / EQUIRECT; fov: the fisheye's angle across its image
    circle in radians, (0, 2 pi]; extent: the world-space height of the orthographic view)."""
    _fields_ = [("kind", C.c_uint32), ("fov", C.c_float), ("extent", C.c_float), ("pad", C.c_uint32)]


assert C.sizeof(Projection) == 16

# name -> (restype, argtypes), as capi.SYMBOLS; bound with it on every load (_abi._EXTRA_SYMBOLS)
SYMBOLS = {
    "gmupt_projection_default_params": (None, [C.POINTER(Projection)]),
    "gmupt_renderer_set_projection": (C.c_int, [_P, C.POINTER(Projection)]),
    "gmupt_renderer_get_projection": (C.c_int, [_P, C.POINTER(Projection)]),
    "gmupt_projection_ray_host": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Projection), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Ray)]),
    "gmupt_projection_pick_ray": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Projection), C.c_float, C.c_float, C.POINTER(Ray)]),
    "gmupt_projection_project_host": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Projection), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                                C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "gmupt_pick_projected": (C.c_int, [_P, C.c_float, C.c_float, C.c_uint32, C.POINTER(Ray), C.POINTER(Hit)]),
    "gmupt_aov_projected_ray": (C.c_int, [C.POINTER(CameraBuffer), C.POINTER(Projection), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Ray)]),
    "gmupt_render_aovs_projected": (C.c_int, [_P, C.POINTER(Projection), C.c_uint32, _P, C.c_size_t, C.POINTER(TraceInfo)]),
    "gmupt_debug_read_aov_rays": (C.c_int, [_P, _P, C.c_uint32]),
    "gmupt_render_denoised_projected": (C.c_int, [_P, C.POINTER(Projection), C.c_uint32, C.POINTER(DenoiseParams), _P, C.c_size_t, C.POINTER(TraceInfo)]),
}
_EXTRA_SYMBOLS.update(SYMBOLS)


def projection_params(kind=PINHOLE, **params):
    """gmupt_projection_default_params with the given fields replaced (kind: a number or a name of KINDS; fov, extent)."""
    return _stage.make_params(Projection, "gmupt_projection_default_params", "projection", dict(params, kind=KINDS.get(kind, kind)), ("kind", "fov", "extent"))


def fisheye(fov_degrees=180.0):
    return projection_params(FISHEYE, fov=math.radians(fov_degrees))


def orthographic(extent):
    return projection_params(ORTHOGRAPHIC, extent=extent)


def equirect():
    return projection_params(EQUIRECT)


def set_projection(renderer, proj):
    """gmupt_renderer_set_projection: attaches `proj` (a Projection) -- from the next iteration on every fresh camera path gets that
    projection's ray -- or, with None or the pinhole kind, detaches: the iterations are again what they always were.  The frame is
    not cleared.  GmuptError (ERR_UNSUPPORTED) while a lens with an aperture is attached."""
    _check(lib().gmupt_renderer_set_projection(renderer.h, _stage.opt_ref(proj)))


def get_projection(renderer):
    """gmupt_renderer_get_projection: the attached Projection (kind PINHOLE when none is)."""
    out = Projection()
    _check(lib().gmupt_renderer_get_projection(renderer.h, C.byref(out)))
    return out


def projection_ray_host(cam_buffer, proj, q, cx, cy):
    """gmupt_projection_ray_host: the rule on the CPU, bit for bit what the renderer's projection launch stores -- the Ray of the fresh
    camera path at entry q of the new-path queue whose screen coordinate is whole-frame pixel (cx, cy)."""
    ray = Ray()
    _check(lib().gmupt_projection_ray_host(C.byref(cam_buffer), C.byref(proj), int(q), int(cx), int(cy), C.byref(ray)))
    return ray


def projection_rays_host(cam_buffer, proj, qs, cxs, cys):
    """projection_ray_host for arrays of (q, cx, cy): an (N, 8) float32 array of gmupt_ray records (origin xyz, tmax, direction xyz, pad)."""
    out = np.empty((len(qs), 8), np.float32)
    ray = Ray()
    fn, pc, pp, pr = lib().gmupt_projection_ray_host, C.byref(cam_buffer), C.byref(proj), C.byref(ray)
    for i, (q, cx, cy) in enumerate(zip(qs, cxs, cys)):
        _check(fn(pc, pp, int(q), int(cx), int(cy), pr))
        out[i] = np.frombuffer(ray, np.float32)
    return out


def pick_ray(cam_buffer, proj, px, py):
    """gmupt_projection_pick_ray: the un-jittered Ray through whole-frame pixel coordinates (px, py)."""
    ray = Ray()
    _check(lib().gmupt_projection_pick_ray(C.byref(cam_buffer), C.byref(proj), float(px), float(py), C.byref(ray)))
    return ray


def pick_rays(cam_buffer, proj, pxs, pys):
    """pick_ray for arrays of coordinates: an (N, 8) float32 array of gmupt_ray records."""
    out = np.empty((len(pxs), 8), np.float32)
    ray = Ray()
    fn, pc, pp, pr = lib().gmupt_projection_pick_ray, C.byref(cam_buffer), C.byref(proj), C.byref(ray)
    for i, (px, py) in enumerate(zip(pxs, pys)):
        _check(fn(pc, pp, float(px), float(py), pr))
        out[i] = np.frombuffer(ray, np.float32)
    return out


def project_host(cam_buffer, proj, world):
    """gmupt_projection_project_host: the whole-frame pixel coordinates (px, py) at which `world` (three floats) appears, as Python
    floats (binary64), or None when the point is not on the image.  The inverse of pick_ray; no bit-for-bit promise."""
    w = (C.c_float * 3)(*[float(x) for x in world])
    px, py, on = C.c_double(), C.c_double(), C.c_int()
    _check(lib().gmupt_projection_project_host(C.byref(cam_buffer), C.byref(proj), w, C.byref(px), C.byref(py), C.byref(on)))
    return (px.value, py.value) if on.value else None


def pick(renderer, px, py, light_count=0):
    """gmupt_pick_projected: (Ray, Hit) of the closest hit of the attached projection's ray through whole-frame pixel (px, py)."""
    ray, hit = Ray(), Hit()
    _check(lib().gmupt_pick_projected(renderer.h, float(px), float(py), int(light_count), C.byref(ray), C.byref(hit)))
    return ray, hit


def aov_projected_ray(cam_buffer, proj, x, y, samples, k):
    """gmupt_aov_projected_ray (host only): ray k = b*s + a of whole-frame pixel (x, y) at `samples` under `proj`."""
    ray = Ray()
    _check(lib().gmupt_aov_projected_ray(C.byref(cam_buffer), C.byref(proj), int(x), int(y), int(samples), int(k), C.byref(ray)))
    return ray


def aov_projected_rays(cam_buffer, proj, xs, ys, samples):
    """All projected AOV rays of the pixels (xs[i], ys[i]) as an (N, R, 8) float32 array of gmupt_ray records (R = samples^2)."""
    return _stage.aov_ray_table(lib().gmupt_aov_projected_ray, cam_buffer, proj, xs, ys, samples)


def aovs(renderer, samples=1, proj=None, info=None):
    """gmupt_render_aovs_projected: the G-buffer of the renderer's rectangle under `proj` (None = the projection attached to the
    renderer, the pinhole when none is) -- samples * samples stratified rays per pixel.  Returns an (H, W, 16) float32 torch tensor on
    the renderer's GPU shaped like Renderer.aovs (capi.aov_fields splits it); the renderer's last_aovs is its TraceInfo."""
    (out,), renderer.last_aovs = renderer._frame(info, (16,), lambda *tail: lib().gmupt_render_aovs_projected(renderer.h, _stage.opt_ref(proj), int(samples), *tail))
    return out


def read_aov_rays(renderer, count):
    """gmupt_debug_read_aov_rays: the first `count` rays of the renderer's AOV chunk scratch as a (count, 8) float32 array -- after an
    aovs() call whose frame fits one chunk, the rays its ray generation wrote, pixel-major."""
    out = np.empty((int(count), 8), np.float32)
    _check(lib().gmupt_debug_read_aov_rays(renderer.h, out.ctypes.data_as(C.c_void_p), int(count)))
    return out


def guided_inputs(renderer, aov_samples=1, proj=None):
    """What an *_image stage takes for a frame under a projection: (beauty, aov), the renderer's frame as an (H, W, 4) float32 tensor
    and the records of aovs(renderer, aov_samples, proj), both on the renderer's GPU."""
    return _stage.guided_inputs(renderer, aovs(renderer, aov_samples, proj))


def denoise(renderer, aov_samples=1, proj=None, info=None, **params):
    """gmupt_render_denoised_projected: Renderer.denoise with the records of aovs(renderer, aov_samples, proj) as the guides.
    Returns an (H, W, 4) float32 torch tensor on the renderer's GPU; params: the denoise_params fields."""
    dp = denoise_params(**params)
    (out,), renderer.last_denoise = renderer._frame(info, (4,), lambda *tail: lib().gmupt_render_denoised_projected(
        renderer.h, _stage.opt_ref(proj), int(aov_samples), C.byref(dp), *tail))
    return out

"""Host side of the ray queries and AOVs: pick and AOV rays of a camera block, the field views of hit, AOV and motion records, and the
motion plane's rule on the CPU."""
import ctypes as C

import numpy as np

from ._abi import ERR_INVALID_ARGUMENT, GmuptError, Ray, aov_dtype, hit_dtype, motion_dtype, triangle_dtype
from ._lib import _check, _ptr, lib
from ._stage import host_words


def camera_pick_ray(cam_buffer, px, py):
    """gmupt_camera_pick_ray (host only): the un-jittered primary ray of newPath.hlsl:36-39 through whole-frame pixel (px, py)."""
    ray = Ray()
    _check(lib().gmupt_camera_pick_ray(C.byref(cam_buffer), float(px), float(py), C.byref(ray)))
    return ray


def hit_fields(hits):
    """Splits (N, 8) gmupt_hit records (numpy or torch) into a dict of numpy arrays: t, u, v (float32), triangle (int32), light,
    material (uint32)."""
    rec = host_words(hits).reshape(-1, 8).view(hit_dtype)[:, 0]
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


def _fields(records, dtype):
    """(..., words) float32 records (torch or numpy) as a dict of numpy arrays of shape (...), one per field of `dtype`."""
    a = host_words(records)
    rec = a.reshape(-1, dtype.itemsize // 4).view(dtype)[:, 0]
    shape = a.shape[:-1]
    return {k: rec[k].reshape(shape + rec[k].shape[1:]).copy() for k in dtype.names}


def aov_fields(aovs):
    """Splits (..., 16) gmupt_aov records (torch or numpy) into a dict of numpy arrays of shape (...): albedo, normal, position (..., 3),
    depth, roughness, metallic (float32), triangle (int32), material, light, coverage (uint32)."""
    return _fields(aovs, aov_dtype)


def motion_fields(motion):
    """Splits (..., 4) gmupt_motion records (torch or numpy) into a dict of numpy arrays: prev_position (..., 3) float32, flags uint32."""
    return _fields(motion, motion_dtype)


def motion_host(hits, aov, tris, verts_now, verts_prev):
    """gmupt_motion_host: the motion plane's rule on the CPU, bit for bit the device's.  hits: (..., 8) float32 gmupt_hit records of the
    centre rays (or hit_dtype), aov: their (..., 16) float32 records (or aov_dtype), tris: triangle_dtype records, verts_now / verts_prev:
    (V, 3) float32.  Returns an array of motion_dtype with the leading shape of `aov`."""
    h, a = host_words(hits, hit_dtype), host_words(aov, aov_dtype)
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

"""What the projection tests share: a numpy restatement of the rule of include/gmupt_projection.h, written from the header in float32
arrays with the oracle's sin / cos (oracle_lib.detmath), independent of csrc/pt_projection.hpp; the float64 inverse; the projections
under test."""
import math

import numpy as np

import lens_aov_util as LA
import lens_util as LU

F = np.float32
PINHOLE, ORTHO, FISHEYE, EQUIRECT = 0, 1, 2, 3
PI32, HALF_PI32 = F(3.14159274), F(1.57079637)
RESOLUTIONS = [(64, 36), (48, 64)]           # one that is not 2:1, one portrait


def f(x):
    return np.asarray(x).astype(F)


def projections(capi):
    """name -> Projection: every kind, the fisheye at two fields of view."""
    P = capi.projection
    return {"ortho": P.orthographic(6.0), "fisheye180": P.fisheye(180.0), "fisheye360": P.projection_params(P.FISHEYE, fov=2 * math.pi),
            "fisheye120": P.fisheye(120.0), "equirect": P.equirect(), "pinhole": P.projection_params(P.PINHOLE)}


def frame(cb):
    pos, ulc, hor, ver = LU.cam_vectors(cb)
    right, up = LU.normalize3(hor), LU.normalize3(ver)
    fn = LU.normalize3(f(f(ulc + f(hor * F(0.5))) - f(ver * F(0.5))))
    return pos, ulc, hor, ver, right, up, fn


def rule_uv(O, cb, proj, u, v):
    """The rule on arrays of screen coordinates (u, v), float32 of any one shape.  Returns (origin, direction) with a last axis of 3."""
    pos, ulc, hor, ver, right, up, fn = frame(cb)
    u, v = f(u), f(v)
    shape = u.shape + (3,)
    kind = int(proj.kind)
    if kind == PINHOLE:
        return np.broadcast_to(pos, shape).copy(), LU.normalize3(f(f(ulc + f(hor * u[..., None])) - f(ver * v[..., None])))
    sx = f(f(F(2.0) * u) - F(1.0))
    sy = f(F(1.0) - f(F(2.0) * v))
    Wf, Hf = f(F(1.0) / F(cb.pixelSize[0])), f(F(1.0) / F(cb.pixelSize[1]))
    if kind == ORTHO:
        halfH = f(F(proj.extent) * F(0.5))
        halfW = f(halfH * f(Wf / Hf))
        origin = f(f(pos + f(right * f(sx * halfW)[..., None])) + f(up * f(sy * halfH)[..., None]))
        return origin, np.broadcast_to(fn, shape).copy()
    origin = np.broadcast_to(pos, shape).copy()
    if kind == FISHEYE:
        m = Wf if Wf < Hf else Hf
        ax, ay = f(sx * f(Wf / m)), f(sy * f(Hf / m))
        r = f(np.sqrt(f(f(ax * ax) + f(ay * ay))))
        theta = f(r * f(F(proj.fov) * F(0.5)))
        c, s = O.detmath(1, theta).reshape(theta.shape), O.detmath(0, theta).reshape(theta.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            side = f(f(right * f(ax / r)[..., None]) + f(up * f(ay / r)[..., None]))
            d = LU.normalize3(f(f(fn * c[..., None]) + f(side * s[..., None])))
        d = np.where((r == 0)[..., None], fn, d)
        d = np.where((r > 1)[..., None], F(0.0), d)
        return origin, f(d)
    lon, lat = f(sx * PI32), f(sy * HALF_PI32)
    cl = O.detmath(1, lat).reshape(lat.shape)
    a = f(cl * O.detmath(1, lon).reshape(lon.shape))
    b = f(cl * O.detmath(0, lon).reshape(lon.shape))
    sl = O.detmath(0, lat).reshape(lat.shape)
    return origin, LU.normalize3(f(f(f(fn * a[..., None]) + f(right * b[..., None])) + f(up * sl[..., None])))


def jittered_uv(O, cb, q, cx, cy):
    """(u, v, jx, jy) of the fresh path at entry q and whole-frame pixel (cx, cy): newPath.hlsl:27,36-37."""
    g = LU.Rng(O, q, cb.randomSeed[0], cb.randomSeed[1])
    jx = f(f(g.next() * F(2.0)) - F(1.0))
    jy = f(f(g.next() * F(2.0)) - F(1.0))
    u = f(f(np.asarray(cx, np.uint32).astype(F) + jx) * F(cb.pixelSize[0]))
    v = f(f(np.asarray(cy, np.uint32).astype(F) + jy) * F(cb.pixelSize[1]))
    return u, v, jx, jy


def rule_fresh(O, cb, proj, q, cx, cy):
    u, v, _, _ = jittered_uv(O, cb, q, cx, cy)
    return rule_uv(O, cb, proj, u, v)


def rule_pixel(O, cb, proj, px, py):
    return rule_uv(O, cb, proj, f(f(px) * F(cb.pixelSize[0])), f(f(py) * F(cb.pixelSize[1])))


def rule_aov(O, cb, proj, x, y, s):
    """(origin, direction) over (N, R, 3): the s*s stratified rays of the pixels (x[i], y[i])."""
    px, py = LA.pixel_coords(x, y, s)
    return rule_pixel(O, cb, proj, px, py)


def words(origin, direction):
    """gmupt_ray words (..., 8) of rays: origin, FLT_MAX, direction, 0."""
    out = np.zeros(origin.shape[:-1] + (8,), F)
    out[..., 0:3] = origin; out[..., 3] = np.finfo(F).max; out[..., 4:7] = direction
    return out


def frame64(cb):
    pos, ulc, hor, ver = (x.astype(np.float64) for x in LU.cam_vectors(cb))
    fwd = ulc + hor / 2 - ver / 2
    return pos, hor / np.linalg.norm(hor), ver / np.linalg.norm(ver), fwd / np.linalg.norm(fwd)


def forward64(cb, proj, px, py):
    """The rule in float64 with numpy's functions: (origin, direction) of whole-frame pixel coordinates; NaN direction outside the circle."""
    pos, right, up, fn = frame64(cb)
    Wf, Hf = 1.0 / np.float64(F(cb.pixelSize[0])), 1.0 / np.float64(F(cb.pixelSize[1]))
    sx = 2.0 * np.asarray(px, np.float64) / Wf - 1.0
    sy = 1.0 - 2.0 * np.asarray(py, np.float64) / Hf
    kind = int(proj.kind)
    o = np.broadcast_to(pos, sx.shape + (3,)).copy()
    if kind == PINHOLE:
        _, ulc, hor, ver = (x.astype(np.float64) for x in LU.cam_vectors(cb))
        return o, ulc + hor * ((sx + 1) / 2)[..., None] - ver * ((1 - sy) / 2)[..., None]
    if kind == ORTHO:
        hh = float(proj.extent) / 2
        return o + right * (sx * hh * Wf / Hf)[..., None] + up * (sy * hh)[..., None], np.broadcast_to(fn, o.shape).copy()
    if kind == FISHEYE:
        m = min(Wf, Hf)
        ax, ay = sx * Wf / m, sy * Hf / m
        r = np.hypot(ax, ay)
        th = r * float(proj.fov) / 2
        rr = np.where(r > 0, r, 1.0)
        d = fn * np.cos(th)[..., None] + (right * (ax / rr)[..., None] + up * (ay / rr)[..., None]) * np.sin(th)[..., None]
        return o, np.where((r > 1)[..., None], np.nan, d)
    lon, lat = sx * np.float64(PI32), sy * np.float64(HALF_PI32)
    return o, fn * (np.cos(lat) * np.cos(lon))[..., None] + right * (np.cos(lat) * np.sin(lon))[..., None] + up * np.sin(lat)[..., None]

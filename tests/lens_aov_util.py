"""What the lens-AOV tests share: a numpy restatement of the rays and of the record rule of include/gmupt_lens_aov.h, written from the
header in float32 arrays with the oracle's sin / cos (oracle_lib.detmath), independent of csrc/pt_lens_aov.hpp."""
import numpy as np

import lens_util as LU

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def cells(s):
    """(a, b) pixel-filter cell and (a2, b2) lens stratum of ray k = b*s + a, k = 0 .. s*s - 1, as uint32 arrays."""
    k = np.arange(s * s, dtype=np.uint32)
    a, b = k % np.uint32(s), k // np.uint32(s)
    return a, b, b.copy(), (np.uint32(s - 1) - a).astype(np.uint32)


def pixel_coords(x, y, s):
    """(px, py) of every ray of the pixels (x[i], y[i]): (N, R) float32, step 1 of the header."""
    a, b, _, _ = cells(s)
    fx, fy = np.asarray(x, np.uint32).astype(F)[:, None], np.asarray(y, np.uint32).astype(F)[:, None]
    if s == 1:
        return fx + np.zeros((1, 1), F), fy + np.zeros((1, 1), F)
    ox = (((np.uint32(2) * a + np.uint32(1)).astype(F) / F(s)).astype(F) - F(1.0)).astype(F)
    oy = (((np.uint32(2) * b + np.uint32(1)).astype(F) / F(s)).astype(F) - F(1.0)).astype(F)
    return (fx + ox[None, :]).astype(F), (fy + oy[None, :]).astype(F)


def pinhole_direction(cb, px, py):
    """gmupt_camera_pick_ray's direction through (px, py): newPath.hlsl:36-39 with the jitter folded in."""
    pos, ulc, hor, ver = LU.cam_vectors(cb)
    u = (px * F(cb.pixelSize[0])).astype(F)
    v = (py * F(cb.pixelSize[1])).astype(F)
    return LU.normalize3(((ulc + (hor * u[..., None]).astype(F)).astype(F) - (ver * v[..., None]).astype(F)).astype(F))


def rule(O, cb, aperture, focus, x, y, s):
    """The rays of the pixels (x[i], y[i]) at s samples per axis.  Returns a dict of float32 arrays over (N, R): px, py, d, lx, ly, Pf,
    origin, direction (the vectors with a last axis of 3), and fn."""
    pos, ulc, hor, ver = LU.cam_vectors(cb)
    _, _, a2, b2 = cells(s)
    px, py = pixel_coords(x, y, s)
    d = pinhole_direction(cb, px, py)
    r1 = ((a2.astype(F) + F(0.5)).astype(F) / F(s)).astype(F)
    r2 = ((b2.astype(F) + F(0.5)).astype(F) / F(s)).astype(F)
    rad = (F(aperture) * np.sqrt(r1).astype(F)).astype(F)
    phi = (r2 * LU.TWO_PI).astype(F)
    lx = np.broadcast_to((rad * O.detmath(1, phi)).astype(F)[None, :], px.shape)
    ly = np.broadcast_to((rad * O.detmath(0, phi)).astype(F)[None, :], px.shape)
    right, up = LU.normalize3(hor), LU.normalize3(ver)
    fn = LU.normalize3(((ulc + (hor * F(0.5)).astype(F)).astype(F) - (ver * F(0.5)).astype(F)).astype(F))
    t = (F(focus) / LU.dot3(d, fn)).astype(F)
    Pf = (pos + (d * t[..., None]).astype(F)).astype(F)
    origin = ((pos + (right * lx[..., None]).astype(F)).astype(F) + (up * ly[..., None]).astype(F)).astype(F)
    direction = LU.normalize3((Pf - origin).astype(F))
    return dict(px=px, py=py, d=d, lx=lx, ly=ly, Pf=Pf, origin=origin, direction=direction, fn=fn)


def rays_of(r):
    """The (N, R, 8) gmupt_ray words of rule()'s result: origin, FLT_MAX, direction, 0."""
    N, R = r["px"].shape
    out = np.zeros((N, R, 8), F)
    out[..., 0:3] = r["origin"]; out[..., 3] = FLT_MAX; out[..., 4:7] = r["direction"]
    return out


def reduce_records(v, rays):
    """The record rule of the header on per-ray values.  v: dict over the N*R rays (pixel-major) with t, light, rec (the triangle record
    of the hit), hit_tri, surface, albedo, normal, metallic, roughness, material -- tests/test_aov_gpu.per_ray gives it; rays: (N, R, 8).
    Returns ((N, 16) uint32 records with word 12 left 0, the expected triangle records (N, 4), which pixels name a triangle (N,))."""
    N, R = rays.shape[:2]
    g = lambda k: v[k].reshape((N, R) + v[k].shape[1:])
    surf = g("surface")
    sa = np.zeros((N, 3), F); sn = np.zeros((N, 3), F); sp = np.zeros((N, 3), F)
    st = np.zeros(N, F); sr = np.zeros(N, F); sm = np.zeros(N, F)
    cov = np.zeros(N, np.uint32)
    first = np.zeros(N, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(R):                                              # every sum from 0.0f, in k order
            sa = (sa + g("albedo")[:, k]).astype(F)
            sn = (sn + g("normal")[:, k]).astype(F)                     # per_ray leaves the normal of a non-surface sample 0
            m = surf[:, k]
            first = np.where(m & (cov == 0), k, first)
            cov = cov + m.astype(np.uint32)
            tk = g("t")[:, k]
            point = (rays[:, k, 0:3] + (rays[:, k, 4:7] * tk[:, None]).astype(F)).astype(F)
            st = np.where(m, (st + tk).astype(F), st)
            sp = np.where(m[:, None], (sp + point).astype(F), sp)
            sr = np.where(m, (sr + g("roughness")[:, k]).astype(F), sr)
            sm = np.where(m, (sm + g("metallic")[:, k]).astype(F), sm)
        c = np.maximum(cov, 1).astype(F)
        exp = np.zeros((N, 16), F)
        exp[:, 0:3] = sa / F(R); exp[:, 4:7] = sn / F(R)
        some = cov > 0
        # coverage == 0: ray 0 as gmupt_render_aovs treats its centre ray
        t0, l0, hit0 = g("t")[:, 0], g("light")[:, 0], g("hit_tri")[:, 0]
        found0 = hit0 | (l0 > 0)
        p0 = np.where(found0[:, None], (rays[:, 0, 0:3] + (rays[:, 0, 4:7] * t0[:, None]).astype(F)).astype(F), F(0.0))
        exp[:, 3] = np.where(some, st / c, t0)
        exp[:, 7] = np.where(some, sr / c, F(0.0))
        exp[:, 8:11] = np.where(some[:, None], sp / c[:, None], p0)
        exp[:, 11] = np.where(some, sm / c, F(0.0))
    e = exp.view(np.uint32)
    idx = np.arange(N)
    e[:, 13] = np.where(some, g("material")[idx, first], g("material")[:, 0])
    e[:, 14] = np.where(some, 0, l0)
    e[:, 15] = cov
    rec = np.where(some[:, None], g("rec")[idx, first], g("rec")[:, 0])
    names = np.where(some, True, hit0)
    return e, rec, names

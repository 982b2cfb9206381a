"""CPU tests of temporal reuse (include/gmupt.h, "temporal reuse"): the layouts, exports, argument checks that need no device, the
projection into a previous camera, and the host integration gmupt_temporal_integrate_host against an independent float64 restatement
plus its exact cases.  The device path is compared with the host chain bit for bit in tests/test_temporal_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_denoise_cpu import beauty_of, random_inputs, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gmupt.h"
#define OFF(T, f) printf(" %zu", offsetof(T, f))
int main(void) {
    printf("%zu", sizeof(gmupt_history));
    OFF(gmupt_history, color); OFF(gmupt_history, count); OFF(gmupt_history, normal); OFF(gmupt_history, material);
    OFF(gmupt_history, position); OFF(gmupt_history, valid);
    printf("\n%zu", sizeof(gmupt_temporal_params));
    OFF(gmupt_temporal_params, spatial); OFF(gmupt_temporal_params, history_cap); OFF(gmupt_temporal_params, min_normal_cos);
    OFF(gmupt_temporal_params, plane_dist);
    printf("\n%g\n", (double)GMUPT_TEMPORAL_MAX_CAP);
    return 0;
}
"""

SYMBOLS = ("gmupt_temporal_default_params", "gmupt_temporal_create", "gmupt_temporal_destroy", "gmupt_temporal_reset",
           "gmupt_temporal_denoise_image", "gmupt_render_denoised_temporal", "gmupt_temporal_integrate_host")


def test_layout_of_header_and_binding(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    hist, params = [list(map(int, l.split())) for l in lines[:2]]
    capi = pkg.capi
    dt = capi.history_dtype
    assert hist == [48, 0, 12, 16, 28, 32, 44]
    assert hist == [dt.itemsize] + [dt.fields[n][1] for n in ("color", "count", "normal", "material", "position", "valid")]
    assert params == [32, 0, 20, 24, 28]
    assert params == [C.sizeof(capi.TemporalParams)] + [getattr(capi.TemporalParams, n).offset for n in ("spatial",) + capi.TEMPORAL_FIELDS]
    assert float(lines[2]) == capi.TEMPORAL_MAX_CAP == 65536.0


def test_library_exports_temporal_reuse(pkg):
    lib = pkg.capi.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS
    t = pkg.capi.temporal_params()
    d = pkg.capi.denoise_params()
    assert bytes(t.spatial) == bytes(d), "the spatial defaults are the denoiser's"
    assert t.history_cap == 32.0 and t.min_normal_cos == f32(0.9) and t.plane_dist == f32(0.02)
    t = pkg.capi.temporal_params(passes=2, history_cap=4.0)
    assert t.spatial.passes == 2 and t.history_cap == 4.0
    with pytest.raises(TypeError):
        pkg.capi.temporal_params(history=1.0)


# ---------------------------------------------------------------------------------------------------- a synthetic scene
def camera(pkg, W, H, pose):
    cam = pkg.capi.Camera(W, H)
    cam.set_pose(*pose)
    cam.update(0.0)
    buf = cam.buffer_copy()
    cam.close()
    return buf


def cam_vectors(buf):
    v = lambda a: np.array(a[:3], np.float64)
    return v(buf.position), v(buf.upperLeftCorner), v(buf.horizontal), v(buf.vertical), np.array(buf.pixelSize[:], np.float64)


# a box room seen from inside: floor, ceiling, three walls (normal, offset, material): dot(n, x) = offset
PLANES = [((0, 1, 0), 0.0, 1), ((0, -1, 0), -6.0, 2), ((-1, 0, 0), -6.0, 3), ((0, 0, 1), -4.0, 4), ((0, 0, -1), -4.0, 5)]


def trace_room(buf, W, H, x0=0, y0=0):
    """Per pixel of the W x H rectangle at (x0, y0) of buf's frame: the centre ray's nearest room plane -> position, normal, depth,
    material (float32, positions from float32 o + d * t)."""
    P, U, Hv, V, ps = cam_vectors(buf)
    ys, xs = np.mgrid[y0:y0 + H, x0:x0 + W].astype(np.float64)
    d = U + Hv * (xs * ps[0])[..., None] - V * (ys * ps[1])[..., None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best = np.full((H, W), np.inf)
    mat = np.zeros((H, W), np.uint32)
    nrm = np.zeros((H, W, 3))
    for n, off, m in PLANES:
        n = np.array(n, np.float64)
        den = d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (off - P @ n) / den
        hit = (den < 0) & (t > 0) & (t < best)
        best[hit] = t[hit]; mat[hit] = m; nrm[hit] = n
    pos = (P + d * best[..., None]).astype(f32)
    return pos, nrm.astype(f32), best.astype(f32), mat


def room_aov(buf, W, H, x0=0, y0=0, seed=0, specials=True):
    """gmupt_aov records of the room (with misses, light spheres and zero normals sprinkled in when specials)."""
    rng = np.random.default_rng(seed)
    pos, nrm, depth, mat = trace_room(buf, W, H, x0, y0)
    n = nrm * rng.uniform(0.5, 2.0, (H, W, 1)).astype(f32)            # not normalised
    tri = np.arange(H * W, dtype=np.int32).reshape(H, W)
    light = np.zeros((H, W), np.uint32)
    if specials:
        kind = rng.random((H, W))
        tri[kind < 0.03] = -1
        light[(kind >= 0.03) & (kind < 0.05)] = 1
        n[(kind >= 0.05) & (kind < 0.07)] = 0.0
    aov = records(np.full((H, W, 3), 0.5, f32), depth, n, pos, tri, light)
    aov.view(np.uint32)[..., 13] = mat
    return aov


def room_history(buf, W, H, x0=0, y0=0, seed=1, defects=True):
    """A history record set of the room from camera buf: colour and count smooth in world space, with defects (invalid records, zero
    counts, material mismatches, flipped normals, records off their plane) sprinkled in when asked."""
    rng = np.random.default_rng(seed)
    pos, nrm, depth, mat = trace_room(buf, W, H, x0, y0)
    h = np.zeros((H, W), np.dtype([("color", "<f4", 3), ("count", "<f4"), ("normal", "<f4", 3), ("material", "<u4"),
                                    ("position", "<f4", 3), ("valid", "<u4")]))
    p64 = pos.astype(np.float64)
    h["color"] = np.stack([0.3 + 0.02 * p64[..., 0], 0.5 + 0.015 * p64[..., 1], 0.4 + 0.01 * p64[..., 2]], -1) + 0.05 * mat[..., None]
    h["count"] = 3.0 + 0.1 * np.abs(p64[..., 0]) + 0.05 * np.abs(p64[..., 2])
    h["normal"] = nrm; h["material"] = mat; h["position"] = pos; h["valid"] = 1
    if defects:
        k = rng.random((H, W))
        h["valid"][k < 0.05] = 0
        h["count"][(k >= 0.05) & (k < 0.08)] = 0.0
        h["material"][(k >= 0.08) & (k < 0.11)] += 7
        h["normal"][(k >= 0.11) & (k < 0.14)] *= -1
        h["position"][(k >= 0.14) & (k < 0.17)] += nrm[(k >= 0.14) & (k < 0.17)] * f32(0.5)
    return h


def noisy_beauty(W, H, seed, zero_frac=0.3):
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 5, (H, W)).astype(np.uint32)
    count[rng.random((H, W)) < zero_frac] = 0
    rgb = rng.uniform(0, 1, (H, W, 3)).astype(f32)
    rgb[count == 0] = 0.0
    return beauty_of(rgb, count)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def project64(buf, X):
    """(u, v, in_front) of world points X (..., 3) in camera buf, in float64."""
    P, U, Hv, V, ps = cam_vectors(buf)
    F = (U + 0.5 * Hv) - 0.5 * V
    d = X.astype(np.float64) - P
    lam = (d @ F) / (F @ F)
    front = lam > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = d / lam[..., None]
    e = r - U
    return ((e @ Hv) / (Hv @ Hv)) / ps[0], (-(e @ V) / (V @ V)) / ps[1], front


def reference(beauty, aov, prev, prev_cam, prev_origin, history_cap=32.0, min_normal_cos=0.9, plane_dist=0.02, margin=1e-3):
    """The integration of include/gmupt.h in float64: (rgb, alpha bits, count, surface, ambiguous, spread).  ambiguous marks the pixels
    where a decision sits within `margin` of its threshold (a tap cell boundary, a tap test): float32 and float64 may decide them
    differently.  spread (H, W, 4): max - min of the counted taps' colour and count -- the binary32 projection is a few ulps of (u, v) off
    the exact one, which moves the bilinear mean by that much times the spread."""
    H, W = beauty.shape[:2]
    u32 = aov.view(np.uint32)
    n_raw = aov[..., 4:7].astype(np.float64)
    surface = (u32[..., 12].view(np.int32) != -1) & (u32[..., 14] == 0) & (np.linalg.norm(n_raw, axis=-1) > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_p = n_raw / np.linalg.norm(n_raw, axis=-1, keepdims=True)
    x_p = aov[..., 8:11].astype(np.float64)
    z_p = aov[..., 3].astype(np.float64)
    mat = u32[..., 13]
    nh = np.zeros((H, W)); hc = np.zeros((H, W, 3))
    amb = np.zeros((H, W), bool)
    lo, hi = np.full((H, W, 4), np.inf), np.full((H, W, 4), -np.inf)
    if prev is not None:
        ph, pw = prev.shape
        u, v, front = project64(prev_cam, x_p)
        with np.errstate(invalid="ignore"):
            ul, vl = u - prev_origin[0], v - prev_origin[1]
            fu, fv = np.floor(ul), np.floor(vl)
        fx, fy = ul - fu, vl - fv
        amb |= surface & front & ((np.minimum(fx, 1 - fx) < margin) | (np.minimum(fy, 1 - fy) < margin))
        sw = np.zeros((H, W)); sc = np.zeros((H, W, 3)); sn = np.zeros((H, W))
        for k, (dx, dy, w) in enumerate([(0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)]):
            with np.errstate(invalid="ignore"):
                qx, qy = fu + dx, fv + dy
                inside = surface & front & (qx >= 0) & (qx < pw) & (qy >= 0) & (qy < ph)
            q = prev[np.where(inside, qy, 0).astype(np.int64), np.where(inside, qx, 0).astype(np.int64)]
            cosq = (n_p * q["normal"]).sum(-1)
            dist = np.abs((n_p * (q["position"].astype(np.float64) - x_p)).sum(-1))
            lim = plane_dist * z_p
            ok = inside & (q["valid"] == 1) & (q["count"] > 0) & (q["material"] == mat)
            amb |= ok & ((np.abs(cosq - min_normal_cos) < 1e-5) | (np.abs(dist - lim) < 1e-5 * np.maximum(lim, 1e-3)))
            ok &= (cosq >= min_normal_cos) & (dist <= lim)
            sw += np.where(ok, w, 0); sc += np.where(ok[..., None], w[..., None] * q["color"], 0); sn += np.where(ok, w * q["count"], 0)
            val = np.concatenate([q["color"], q["count"][..., None]], -1).astype(np.float64)
            lo = np.where(ok[..., None], np.minimum(lo, val), lo); hi = np.where(ok[..., None], np.maximum(hi, val), hi)
        has = sw > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            hc = np.where(has[..., None], sc / sw[..., None], 0.0)
            nh = np.where(has, np.fmin(history_cap, sn / sw), 0.0)          # the rule's min drops a NaN
    n = beauty[..., 3].view(np.uint32).astype(np.int64)
    nf = n.astype(np.float64)
    B = beauty[..., :3].astype(np.float64)
    use = surface & (nh > 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rgb = np.where(use[..., None], (nh[..., None] * hc + nf[..., None] * B) / (nh + nf)[..., None], B)
    ceil = np.ceil(nh).astype(np.int64)
    amb |= use & (np.abs(nh - np.round(nh)) < 1e-4)
    alpha = np.where(use, n + ceil, n).astype(np.uint32)
    count = np.where(surface, nh + nf, 0.0)
    spread = np.where(hi >= lo, hi - lo, 0.0)
    return rgb, alpha, count, surface, amb, spread


def check_against_reference(pkg, beauty, aov, prev, prev_cam, origin, **params):
    capi = pkg.capi
    got, hist = capi.temporal_integrate_host(beauty, aov, prev, prev_cam, origin, **params)
    rgb, alpha, count, surface, amb, spread = reference(beauty, aov, prev, prev_cam, origin, **params)
    assert amb.mean() < 0.02, amb.mean()
    ok = ~amb
    ulps = lambda x: np.spacing(np.abs(x).astype(f32)).astype(np.float64)
    # a few ulps of the result, plus what 1e-4 px of projection error can move the bilinear means of the taps (the colour, and the
    # count that weighs it against the beauty)
    err = np.abs(got[..., :3] - rgb)
    assert np.all((err <= 8 * ulps(rgb) + 1e-4 * (spread[..., :3] + spread[..., 3:]))[ok]), float(err[ok].max())
    assert np.array_equal(got[..., 3].view(np.uint32)[ok], alpha[ok])
    assert np.all((np.abs(hist["count"] - count) <= 8 * ulps(count) + 1e-4 * spread[..., 3])[ok])
    assert np.array_equal(hist["color"][surface], got[..., :3][surface])
    assert np.array_equal(hist["valid"], (surface & (hist["count"] > 0)).astype(np.uint32))
    assert np.array_equal(hist["material"][surface], aov.view(np.uint32)[..., 13][surface])
    assert np.array_equal(hist["position"][surface], aov[..., 8:11][surface])
    assert not hist.view(np.uint32).reshape(hist.shape + (12,))[~surface].any(), "records of other pixels are all zero"
    assert np.array_equal(got.view(np.uint32)[~surface], beauty.view(np.uint32)[~surface]), "other pixels: the beauty texel"
    return got, hist, rgb, surface


BASE = (0.5, 1.5, 1.0, -5.0, 200.0)   # inside the room, looking at the far walls


@pytest.mark.parametrize("case", ["translated", "rotated", "both", "other_rect", "tile"])
def test_integration_matches_the_float64_restatement(pkg, case):
    W, H = 96, 54
    prev_pose, x0, y0, pW, pH, px0, py0, cw, ch = BASE, 0, 0, W, H, 0, 0, W, H
    if case == "translated":
        prev_pose = (0.7, 1.4, 1.1, -5.0, 200.0)
    elif case == "rotated":
        prev_pose = (0.5, 1.5, 1.0, -3.0, 196.0)
    elif case == "both":
        prev_pose = (0.3, 1.6, 0.8, -7.0, 203.0)
    elif case == "other_rect":                        # a previous frame of another size, seen through a shifted origin
        prev_pose, pW, pH, px0, py0, cw, ch = (0.6, 1.5, 1.0, -5.0, 198.0), 70, 40, 13, 9, W, H
    elif case == "tile":                              # the current image is a tile of the frame, the previous one another tile
        prev_pose, x0, y0, W, H, px0, py0, pW, pH = (0.5, 1.5, 1.0, -4.0, 199.0), 20, 12, 50, 30, 10, 4, 70, 40
    cur = camera(pkg, cw, ch, BASE)
    prev_cam = camera(pkg, cw, ch, prev_pose)
    aov = room_aov(cur, W, H, x0, y0, seed=3)
    prev = room_history(prev_cam, pW, pH, px0, py0, seed=4)
    beauty = noisy_beauty(W, H, 5)
    got, hist, rgb, surface = check_against_reference(pkg, beauty, aov, prev, prev_cam, (px0, py0))
    took = surface & (got[..., 3].view(np.uint32) != beauty[..., 3].view(np.uint32))
    assert took.mean() > 0.3, "a good share of the pixels uses history"
    zero = surface & (beauty[..., 3].view(np.uint32) == 0)
    assert (took & zero).sum() > 0.5 * zero.sum(), "pixels without samples take the history"
    # every rejection kind happened: some surface pixels with taps inside got no history although their neighbours did
    assert (surface & ~took).sum() > 0


def test_rejections_each_drop_history(pkg):
    """One defect at a time on an otherwise perfect history from the same camera: each kind removes history where it sits."""
    W, H = 64, 36
    cam = camera(pkg, W, H, BASE)
    aov = room_aov(cam, W, H, seed=7, specials=False)
    beauty = noisy_beauty(W, H, 8, zero_frac=1.0)               # no samples: the output is the history or nothing
    clean = room_history(cam, W, H, seed=9, defects=False)
    base, _ = pkg.capi.temporal_integrate_host(beauty, aov, clean, cam)
    assert np.all(base[..., 3].view(np.uint32) > 0), "a perfect history reaches every pixel"
    for name, spoil in [("valid", lambda h: h["valid"].fill(0)), ("count", lambda h: h["count"].fill(0.0)),
                        ("material", lambda h: h["material"].__iadd__(1)), ("normal", lambda h: h["normal"].__imul__(-1)),
                        ("plane", lambda h: h["position"].__iadd__(h["normal"] * f32(1e5)))]:
        h = clean.copy()
        spoil(h)
        got, _ = pkg.capi.temporal_integrate_host(beauty, aov, h, cam)
        assert np.array_equal(got.view(np.uint32), beauty.view(np.uint32)), name
    # taps off the previous rectangle: a previous rectangle far to the side gives nothing
    got, _ = pkg.capi.temporal_integrate_host(beauty, aov, clean, cam, (500, 0))
    assert np.array_equal(got.view(np.uint32), beauty.view(np.uint32))


def test_projection_round_trip(pkg):
    """A point on gmupt_camera_pick_ray(cam, x, y) projects back onto (x, y): in the float64 restatement, and in the library (history
    colours that hold their own whole-frame pixel coordinates come back as the bilinear mean at the projection, i.e. (u, v))."""
    capi = pkg.capi
    for (W, H, pose, x0, y0, tw, th) in [(64, 36, BASE, 0, 0, 64, 36), (1920, 1080, (1.0, 3.0, 8.0, 0.0, 270.0), 800, 400, 48, 32),
                                         (333, 177, (-2.0, 0.5, 4.0, 31.0, 117.0), 100, 50, 40, 30), (40, 90, (0.0, 0.0, 0.0, -80.0, 10.0), 0, 0, 40, 90)]:
        cam = camera(pkg, W, H, pose)
        rng = np.random.default_rng(W)
        xs = np.arange(x0 + 1, x0 + tw - 1, 3, dtype=np.float64)
        ys = np.arange(y0 + 1, y0 + th - 1, 3, dtype=np.float64)
        gy, gx = np.meshgrid(ys, xs, indexing="ij")
        pts = np.zeros(gx.shape + (3,), f32)
        for i in range(gx.shape[0]):
            for j in range(gx.shape[1]):
                ray = capi.camera_pick_ray(cam, float(gx[i, j]), float(gy[i, j]))
                t = rng.uniform(0.5, 50.0)
                pts[i, j] = np.array(ray.origin[:3], np.float64) + np.array(ray.direction[:3], np.float64) * t
        u, v, front = project64(cam, pts)
        assert front.all()
        assert np.abs(u - gx).max() < 1e-3 and np.abs(v - gy).max() < 1e-3
        # behind the camera: the mirror point is rejected
        P = np.array(cam.position[:3], np.float64)
        assert not project64(cam, (2 * P - pts.astype(np.float64)).astype(f32))[2].any()
        # the library: one current pixel per point (n = 0), a history rectangle (tw x th at (x0, y0)) holding its own coordinates
        h, w = gx.shape
        aov = records(np.full((h, w, 3), 0.5, f32), np.full((h, w), 1.0, f32), np.tile(f32([0, 0, 1]), (h, w, 1)), pts,
                      np.zeros((h, w), np.int32), np.zeros((h, w), np.uint32))
        hist = np.zeros((th, tw), capi.history_dtype)
        hy, hx = np.mgrid[y0:y0 + th, x0:x0 + tw]
        hist["color"] = np.stack([hx, hy, np.zeros_like(hx)], -1)
        hist["count"] = 1.0; hist["normal"] = (0, 0, 1); hist["material"] = 1; hist["valid"] = 1
        hist["position"] = pts.reshape(-1, 3).mean(0)
        beauty = beauty_of(np.zeros((h, w, 3), f32), np.zeros((h, w), np.uint32))
        got, _ = capi.temporal_integrate_host(beauty, aov, hist, cam, (x0, y0), min_normal_cos=-1.0, plane_dist=1e30)
        assert np.all(got[..., 3].view(np.uint32) == 1)
        assert np.abs(got[..., 0] - gx).max() < 1e-3 and np.abs(got[..., 1] - gy).max() < 1e-3
        behind = (2 * P - pts.astype(np.float64)).astype(f32)
        aov[..., 8:11] = behind
        got, _ = capi.temporal_integrate_host(beauty, aov, hist, cam, (x0, y0), min_normal_cos=-1.0, plane_dist=1e30)
        assert np.array_equal(got.view(np.uint32), beauty.view(np.uint32)), "behind the camera: no history"


def test_exact_cases(pkg):
    capi = pkg.capi
    W, H = 80, 45
    cam = camera(pkg, W, H, BASE)
    prev_cam = camera(pkg, W, H, (0.6, 1.5, 1.0, -5.0, 198.0))
    aov = room_aov(cam, W, H, seed=11)
    beauty = noisy_beauty(W, H, 12)
    prev = room_history(prev_cam, W, H, seed=13)
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    # no history, or history_cap = 0: the beauty, bit for bit; the records still describe the surface pixels
    for got, hist in [capi.temporal_integrate_host(beauty, aov), capi.temporal_integrate_host(beauty, aov, prev, prev_cam, history_cap=0.0)]:
        assert same(got, beauty)
        nb = beauty[..., 3].view(np.uint32)
        surface = hist["material"] > 0
        assert np.array_equal(hist["count"][surface], nb[surface].astype(f32))
        assert np.array_equal(hist["valid"], (surface & (nb > 0)).astype(np.uint32))
    # the thread count changes no bit
    runs = [capi.temporal_integrate_host(beauty, aov, prev, prev_cam, threads=t) for t in (1, 3, 16)]
    for got, hist in runs[1:]:
        assert same(got, runs[0][0]) and same(hist, runs[0][1])
    # invalid pixels (misses, light spheres, zero normals) come through unchanged
    u = aov.view(np.uint32)
    inval = (u[..., 12].view(np.int32) == -1) | (u[..., 14] != 0) | ~aov[..., 4:7].any(-1)
    assert inval.sum() > 0 and same(runs[0][0][inval], beauty[inval])
    # n = 0 with history: rgb == H exactly.  Colours that are powers of two make H exact whatever the weights: sum(w * c) = c * sum(w)
    flat = prev.copy()
    flat["color"] = (0.5, 0.25, 0.125)
    got, hist = capi.temporal_integrate_host(beauty, aov, flat, prev_cam)
    zero = beauty[..., 3].view(np.uint32) == 0
    took = got[..., 3].view(np.uint32) > 0
    sel = zero & took
    assert sel.sum() > 50
    assert np.all(got[sel][:, :3] == f32([0.5, 0.25, 0.125]))
    assert np.array_equal(got[sel][:, 3].view(np.uint32).astype(np.float64), np.ceil(hist["count"][sel].astype(np.float64)))
    # the cap bounds the history's weight
    got, hist = capi.temporal_integrate_host(beauty, aov, prev, prev_cam, history_cap=1.5)
    assert hist["count"].max() <= 1.5 + beauty[..., 3].view(np.uint32).max()
    surface_with = (hist["count"] > 0) & zero
    assert np.all(hist["count"][surface_with] <= 1.5)


def test_arguments_are_refused_without_a_gpu(pkg):
    capi = pkg.capi
    lib = capi.lib()
    P = C.c_void_p
    W, H = 16, 8
    cam = camera(pkg, W, H, BASE)
    beauty, aov = random_inputs(W, H, 1)
    prev = np.zeros((H, W), capi.history_dtype)
    out = np.zeros_like(beauty)
    hist = np.zeros((H, W), capi.history_dtype)
    tp = capi.temporal_params()

    def host(b=beauty, a=aov, pv=prev, pc=cam, o=out, oh=hist, p=tp, w=W, h=H, pw=W, ph=H):
        g = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
        return lib.gmupt_temporal_integrate_host(P(g(b)), P(g(a)), w, h, P(g(pv)), C.byref(pc) if pc is not None else None, 0, 0, pw, ph,
                                                 C.byref(p) if p is not None else None, P(g(o)), P(g(oh)), 4)
    assert host() == 0 and host(p=None) == 0
    assert host(pv=None, pc=None) == 0
    bad = [{"b": None}, {"a": None}, {"o": None}, {"oh": None}, {"pc": None}, {"w": 0}, {"pw": 0}, {"o": beauty}, {"oh": out}, {"oh": prev},
           {"o": aov}]
    for kw, field, value in [(None, "history_cap", -1.0), (None, "history_cap", float("nan")), (None, "history_cap", 70000.0),
                             (None, "min_normal_cos", 1.5), (None, "min_normal_cos", float("inf")), (None, "plane_dist", -0.1),
                             (None, "plane_dist", float("nan")), ("spatial", "passes", 0), ("spatial", "sigma_color", 0.0)]:
        p = capi.temporal_params()
        setattr(p.spatial if kw else p, field, value)
        bad.append({"p": p})
    for kw in bad:
        assert host(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    # the device entries check their arguments before they touch the handle or a device
    dp = capi.temporal_params()
    n = out.nbytes

    def dev(t=None, b=16, a=4096, c=cam, o=8192, nbytes=n, p=dp, w=W, h=H):
        return lib.gmupt_temporal_denoise_image(t, P(b), P(a), C.byref(c) if c is not None else None, 0, 0, w, h, 1,
                                                C.byref(p) if p is not None else None, P(o), nbytes, None)
    for kw in ({"b": 0}, {"a": 0}, {"o": 0}, {"b": 24}, {"a": 4100}, {"o": 8200}, {"o": 16 + 64}, {"nbytes": n - 16}, {"w": 0},
               {"p": capi.temporal_params(history_cap=-1.0)}, {"p": capi.temporal_params(passes=6)}, {"c": None}, {}):
        assert dev(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    assert b"null handle" in lib.gmupt_last_error()
    assert lib.gmupt_render_denoised_temporal(None, None, 1, C.byref(dp), P(16), n, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_temporal_create(None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_temporal_reset(None) == capi.ERR_INVALID_ARGUMENT
    lib.gmupt_temporal_destroy(None)
    with pytest.raises(capi.GmuptError):
        capi.temporal_integrate_host(beauty, aov[:, :3])


def test_session_resets_history_on_light_edits(pkg):
    """ProgressiveSession: set_lights drops the history (the old light made it), resize keeps it."""
    events = []

    class Fake:
        def __getattr__(self, name):
            return lambda *a, **k: events.append(name)

    class Buf:
        lightCount = 0

    cam = Fake()
    cam.buffer = Buf()
    sess = pkg.progressive.ProgressiveSession(Fake(), cam, 8, 4, preview_every=0)
    sess.temporal = Fake()
    sess.resize(16, 8)
    assert "reset" not in events
    sess.set_lights(Fake(), None, 1)
    assert events.count("reset") == 1 and "reset_accumulation" in events

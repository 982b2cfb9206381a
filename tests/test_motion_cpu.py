"""CPU tests of motion-aware temporal reuse (include/gmupt.h, "motion"): the gmupt_motion layout, gmupt_motion_host against a float64
restatement, the exact cases of unmoved geometry, the translation identity, gmupt_temporal_integrate_motion_host against the float64
restatement of tests/test_temporal_cpu.py, and the argument checks that need no device.  The device path is compared with this host
chain bit for bit in tests/test_motion_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_denoise_cpu import beauty_of, records
from test_temporal_cpu import BASE, camera, noisy_beauty, room_aov, room_history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gmupt.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(gmupt_motion), offsetof(gmupt_motion, prev_position), offsetof(gmupt_motion, flags));
    return 0;
}
"""

SYMBOLS = ("gmupt_render_aovs_motion", "gmupt_motion_host", "gmupt_temporal_integrate_motion_host", "gmupt_temporal_denoise_image_motion",
           "gmupt_render_denoised_temporal_motion")


def test_layout_and_exports(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    dt = pkg.capi.motion_dtype
    assert got == [16, 0, 12] == [dt.itemsize, dt.fields["prev_position"][1], dt.fields["flags"][1]]
    lib = pkg.capi.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in pkg.capi.SYMBOLS, name


# ---------------------------------------------------------------------------------------------------- hits by brute force
def pixel_rays(pkg, cam, W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return pkg.capi.aov_rays(cam, xs.ravel(), ys.ravel(), 1)[:, 0, :]


def brute_hits(rays, tris, verts):
    """The nearest triangle of every ray by Moeller-Trumbore over all records, in float64: gmupt_hit records (the lowest index wins a tie)."""
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    v = verts.astype(np.float64)
    p0, p1, p2 = (v[tris["v"][:, k]] for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    hits = np.zeros(len(rays), np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("triangle", "<i4"), ("light", "<u4"), ("material", "<u4"),
                                         ("pad", "<u4", 2)]))
    hits["t"] = np.finfo(f32).max; hits["triangle"] = -1
    for i in range(len(rays)):
        pv = np.cross(d[i], e2)
        det = (e1 * pv).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o[i] - p0
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1)
            w = (qv * d[i]).sum(-1) * inv
            t = (e2 * qv).sum(-1) * inv
            ok = (np.abs(det) > 1e-12) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 1e-6)
        if ok.any():
            k = int(np.flatnonzero(ok)[np.argmin(t[ok])])
            hits[i] = (t[k], u[k], w[k], k, 0, tris["materialID"][k], (0, 0))
    return hits


def aov_of_hits(rays, hits, tris, verts, H, W):
    """gmupt_aov records of the centre-ray hits: position = o + d * t in binary32, the geometric normal towards the ray, depth, ids."""
    o, d = rays[:, 0:3], rays[:, 4:7]
    hit = (hits["triangle"] >= 0) & (hits["light"] == 0)
    pos = np.where(hit[:, None], o + d * hits["t"][:, None], 0).astype(f32)
    tv = tris["v"][np.maximum(hits["triangle"], 0)]
    v = verts.astype(np.float64)
    n = np.cross(v[tv[:, 1]] - v[tv[:, 0]], v[tv[:, 2]] - v[tv[:, 0]])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    n = np.where(((n * d).sum(-1) > 0)[:, None], -n, n)
    n = np.where(hit[:, None], n, 0).astype(f32)
    aov = records(np.full((H, W, 3), 0.5, f32), hits["t"].reshape(H, W), n.reshape(H, W, 3), pos.reshape(H, W, 3),
                  hits["triangle"].reshape(H, W).astype(np.int32), hits["light"].reshape(H, W))
    aov.view(np.uint32)[..., 13] = hits["material"].reshape(H, W)
    return aov


@pytest.fixture(scope="module")
def scenes3(pkg, cornell_scene, soup_scene):
    return {"cornell": cornell_scene, "soup": soup_scene, "textured": pkg.scenes.build_scene(pkg.scenes.textured_mesh())}


def scene_frame(pkg, scene, W, H, verts, pose=None, specials=True):
    """(camera buffer, rays, hits, aov) of `scene` with the given vertices; some hits are turned into light-sphere hits when asked."""
    cam = camera(pkg, W, H, pose or scene["camera"])
    rays = pixel_rays(pkg, cam, W, H)
    hits = brute_hits(rays, scene["tris"], verts)
    if specials:
        hits["light"][::17] = 1
    return cam, rays, hits, aov_of_hits(rays, hits, scene["tris"], verts, H, W)


# ---------------------------------------------------------------------------------------------------- 1: the rule
@pytest.mark.parametrize("name", ["cornell", "textured", "soup"])
def test_motion_host_matches_the_float64_restatement(pkg, scenes3, name):
    """Tolerance, from the number format: each barycentric sum is three products and two additions (at most 2.5 ulps of the largest
    magnitude involved), their difference and the addition to the position at most half an ulp each, and w = (1 - u) - v carries one
    rounding that both sums share: below 8 ulps of the largest of |p_i|, |q_i|, |position| per component."""
    capi, scene = pkg.capi, scenes3[name]
    W, H = 40, 24
    tris = scene["tris"]
    for phase_prev, phase_now in [(0.0, 0.3), (0.3, 0.7), (0.7, 0.0)]:
        prev, now = pkg.scenes.wobble(scene, phase_prev, 0.05), pkg.scenes.wobble(scene, phase_now, 0.05)
        cam, rays, hits, aov = scene_frame(pkg, scene, W, H, now)
        mv = capi.motion_host(hits, aov, tris, now, prev)
        assert mv.shape == (H, W) and mv.dtype == capi.motion_dtype
        hit = ((hits["triangle"] >= 0) & (hits["light"] == 0)).reshape(H, W)
        assert hit.sum() > W * H // 4 and (~hit).sum() > 0
        assert not mv.view(np.uint32).reshape(H, W, 4)[~hit].any(), "misses and light spheres: all zero"
        assert np.all(mv["flags"][hit] == 1)
        h = hits.reshape(H, W)[hit]
        tv = tris["v"][h["triangle"]]
        u, v = h["u"].astype(np.float64)[:, None], h["v"].astype(np.float64)[:, None]
        w = 1.0 - u - v
        p, q = now.astype(np.float64), prev.astype(np.float64)
        b_now = w * p[tv[:, 0]] + u * p[tv[:, 1]] + v * p[tv[:, 2]]
        b_prev = w * q[tv[:, 0]] + u * q[tv[:, 1]] + v * q[tv[:, 2]]
        pos = aov[..., 8:11][hit].astype(np.float64)
        want = pos + (b_prev - b_now)
        mag = np.maximum(np.abs(pos), np.maximum(np.abs(p[tv]).max(1), np.abs(q[tv]).max(1)))
        err = np.abs(mv["prev_position"][hit] - want)
        in_ulps = err / np.spacing(mag.astype(f32))
        assert np.all(in_ulps <= 8), float(in_ulps.max())
        # the bound is the worst case; roundings mostly cancel, so the typical error sits far below it (a wrong vertex or swapped
        # barycentrics on a small displacement could hide under 8 ulps of a large coordinate, but not under this)
        assert np.median(in_ulps) <= 1.0 and np.mean(in_ulps <= 2.0) > 0.9, (float(np.median(in_ulps)), float(np.mean(in_ulps <= 2.0)))
        assert np.abs(b_prev - b_now).max() > 1e-3, "the wobble moves the visible surface"


# ---------------------------------------------------------------------------------------------------- 2: nothing moved
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_unmoved_vertices_take_the_existing_path_bit_for_bit(pkg, scenes3, name):
    capi, scene = pkg.capi, scenes3[name]
    W, H = 40, 24
    now = pkg.scenes.wobble(scene, 0.3, 0.05)
    cam, rays, hits, aov = scene_frame(pkg, scene, W, H, now)
    aov[3, 5, 8] = -0.0                                        # a -0.0f component stays -0.0f
    mv = capi.motion_host(hits, aov, scene["tris"], now, now.copy())
    hit = mv["flags"] == 1
    assert hit.sum() > 100 and same(mv["prev_position"][hit], aov[..., 8:11][hit])
    prev_cam = camera(pkg, W, H, tuple(np.add(scene["camera"], (0.05, 0.02, 0.0, 0.5, -1.0))))
    _, _, phits, paov = scene_frame(pkg, scene, W, H, now, pose=tuple(np.add(scene["camera"], (0.05, 0.02, 0.0, 0.5, -1.0))), specials=False)
    _, prev = capi.temporal_integrate_host(noisy_beauty(W, H, 2, zero_frac=0.0), paov)
    beauty = noisy_beauty(W, H, 3)
    base = capi.temporal_integrate_host(beauty, aov, prev, prev_cam)
    assert (base[0][..., 3].view(np.uint32) != beauty[..., 3].view(np.uint32)).mean() > 0.1, "the history is used (a sanity check of the inputs: the soup is mostly empty space)"
    for motion in (mv, None):
        got = capi.temporal_integrate_motion_host(beauty, aov, motion, prev, prev_cam)
        assert same(got[0], base[0]) and same(got[1], base[1])
    # flags == 0 everywhere: prev_position is ignored
    junk = mv.copy(); junk["flags"] = 0; junk["prev_position"] = 1e9
    got = capi.temporal_integrate_motion_host(beauty, aov, junk, prev, prev_cam)
    assert same(got[0], base[0]) and same(got[1], base[1])


# ---------------------------------------------------------------------------------------------------- 3: the translation identity
def neighbourhood_spread(hist):
    """max - min of colour and count over every pixel's 3x3 neighbourhood: what a sub-pixel shift of the taps can move, per pixel of shift."""
    val = np.concatenate([hist["color"], hist["count"][..., None]], -1).astype(np.float64)
    pad = np.pad(val, ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = hist.shape
    stack = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return stack.max(0) - stack.min(0)


def test_translating_scene_and_camera_together_changes_nothing(pkg, cornell_scene):
    """Vertices and camera both moved by d: prev_position = x_p - d, which projects into the previous camera at the pixel's own
    coordinate (1e-3 px, the bound of test_projection_round_trip), and the integrated image is the static one's to the tolerance of
    tests/test_temporal_cpu.py (8 ulps plus what 1e-4 px moves the bilinear mean)."""
    from test_temporal_cpu import project64
    capi, scene = pkg.capi, cornell_scene
    W, H = 48, 27
    d = f32([0.5, -0.25, 0.375])
    prev_v = scene["verts"]
    now_v = (prev_v + d).astype(f32)
    pose = scene["camera"]
    pose_now = (pose[0] + float(d[0]), pose[1] + float(d[1]), pose[2] + float(d[2])) + tuple(pose[3:])
    prev_cam, _, phits, paov = scene_frame(pkg, scene, W, H, prev_v, specials=False)
    cam, rays, hits, aov = scene_frame(pkg, scene, W, H, now_v, pose=pose_now, specials=False)
    assert np.array_equal(hits["triangle"], phits["triangle"]), "the same triangles are seen"
    mv = capi.motion_host(hits, aov, scene["tris"], now_v, prev_v)
    hit = mv["flags"] == 1
    assert hit.mean() > 0.5
    x_p = aov[..., 8:11].astype(np.float64)
    scale = np.abs(x_p).max()
    assert np.abs(mv["prev_position"][hit] - (x_p[hit] - d)).max() <= 16 * np.spacing(f32(scale))
    u, v, front = project64(prev_cam, mv["prev_position"])
    ys, xs = np.mgrid[0:H, 0:W]
    assert front[hit].all() and np.abs(u - xs)[hit].max() < 1e-3 and np.abs(v - ys)[hit].max() < 1e-3
    # a smooth history written from the previous camera on the previous pose
    hist = np.zeros((H, W), capi.history_dtype)
    pp = paov[..., 8:11].astype(np.float64)
    hist["color"] = np.stack([0.3 + 0.02 * pp[..., 0], 0.5 + 0.015 * pp[..., 1], 0.4 + 0.01 * pp[..., 2]], -1)
    hist["count"] = 3.0 + 0.1 * np.abs(pp[..., 0])
    n = paov[..., 4:7]
    hist["normal"] = n; hist["material"] = paov.view(np.uint32)[..., 13]; hist["position"] = paov[..., 8:11]
    hist["valid"] = (phits["triangle"] >= 0).reshape(H, W)
    beauty = noisy_beauty(W, H, 4)
    static, _ = capi.temporal_integrate_host(beauty, paov, hist, prev_cam)
    moved, rec = capi.temporal_integrate_motion_host(beauty, aov, mv, hist, prev_cam)
    assert same(rec["position"][hit], aov[..., 8:11][hit]), "the new record holds the current pose"
    took = moved[..., 3].view(np.uint32) != beauty[..., 3].view(np.uint32)
    assert np.array_equal(took, hit), "every surface pixel finds its history"
    assert np.array_equal(moved[..., 3].view(np.uint32), static[..., 3].view(np.uint32))
    spread = neighbourhood_spread(hist)
    ulps = np.spacing(np.abs(static[..., :3]).astype(f32)).astype(np.float64)
    err = np.abs(moved[..., :3].astype(np.float64) - static[..., :3])
    assert np.all(err <= 8 * ulps + 1e-4 * (spread[..., :3] + spread[..., 3:])), float(err.max())
    # without the motion plane the same history is looked up d away: it is another image
    plain, _ = capi.temporal_integrate_host(beauty, aov, hist, prev_cam)
    assert np.abs(plain[..., :3] - static[..., :3]).max() > 100 * err.max()


# ---------------------------------------------------------------------------------------------------- 4: moved poses against float64
def reference_motion(beauty, aov, mv, prev, prev_cam, prev_origin, history_cap=32.0, min_normal_cos=0.9, plane_dist=0.02, margin=1e-3):
    """The integration with a motion plane in float64, written out from include/gmupt.h: (rgb, alpha bits, count, surface, ambiguous,
    spread, Sw, magnitude).  x_h = prev_position where flags == 1, else x_p, is what is projected and what the taps' plane distance is measured
    from.  ambiguous: a decision within `margin` of its threshold.  spread: max - min of the counted taps' colour and count;
    magnitude: the largest |colour| that enters the pixel's blend (the room's synthetic history has negative colours far out, so a blend
    can cancel)."""
    from test_temporal_cpu import project64
    H, W = beauty.shape[:2]
    u32 = aov.view(np.uint32)
    n_raw = aov[..., 4:7].astype(np.float64)
    surface = (u32[..., 12].view(np.int32) != -1) & (u32[..., 14] == 0) & (np.linalg.norm(n_raw, axis=-1) > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_p = n_raw / np.linalg.norm(n_raw, axis=-1, keepdims=True)
    x_h = np.where((mv["flags"] == 1)[..., None], mv["prev_position"], aov[..., 8:11]).astype(np.float64)
    lim = plane_dist * aov[..., 3].astype(np.float64)
    mat = u32[..., 13]
    ph, pw = prev.shape
    u, v, front = project64(prev_cam, x_h)
    with np.errstate(invalid="ignore"):
        ul, vl = u - prev_origin[0], v - prev_origin[1]
        fu, fv = np.floor(ul), np.floor(vl)
    fx, fy = ul - fu, vl - fv
    amb = surface & front & ((np.minimum(fx, 1 - fx) < margin) | (np.minimum(fy, 1 - fy) < margin))
    sw = np.zeros((H, W)); sc = np.zeros((H, W, 3)); sn = np.zeros((H, W))
    lo, hi = np.full((H, W, 4), np.inf), np.full((H, W, 4), -np.inf)
    for dx, dy, w in [(0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)]:
        with np.errstate(invalid="ignore"):
            qx, qy = fu + dx, fv + dy
            inside = surface & front & (qx >= 0) & (qx < pw) & (qy >= 0) & (qy < ph)
        q = prev[np.where(inside, qy, 0).astype(np.int64), np.where(inside, qx, 0).astype(np.int64)]
        cosq = (n_p * q["normal"]).sum(-1)
        dist = np.abs((n_p * (q["position"].astype(np.float64) - x_h)).sum(-1))
        ok = inside & (q["valid"] == 1) & (q["count"] > 0) & (q["material"] == mat)
        amb |= ok & ((np.abs(cosq - min_normal_cos) < 1e-5) | (np.abs(dist - lim) < 1e-5 * np.maximum(lim, 1e-3)))
        ok &= (cosq >= min_normal_cos) & (dist <= lim)
        sw += np.where(ok, w, 0); sc += np.where(ok[..., None], w[..., None] * q["color"], 0); sn += np.where(ok, w * q["count"], 0)
        val = np.concatenate([q["color"], q["count"][..., None]], -1).astype(np.float64)
        lo = np.where(ok[..., None], np.minimum(lo, val), lo); hi = np.where(ok[..., None], np.maximum(hi, val), hi)
    has = sw > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        hc = np.where(has[..., None], sc / sw[..., None], 0.0)
        nh = np.where(has, np.minimum(history_cap, sn / sw), 0.0)
    n = beauty[..., 3].view(np.uint32).astype(np.int64)
    nf = n.astype(np.float64)
    B = beauty[..., :3].astype(np.float64)
    use = surface & (nh > 0)
    rgb = np.where(use[..., None], (nh[..., None] * hc + nf[..., None] * B) / np.maximum(nh + nf, 1e-30)[..., None], B)
    amb |= use & (np.abs(nh - np.round(nh)) < 1e-4)
    alpha = np.where(use, n + np.ceil(nh).astype(np.int64), n).astype(np.uint32)
    mag = np.maximum(np.abs(B), np.where(hi >= lo, np.maximum(np.abs(lo), np.abs(hi)), 0.0)[..., :3])
    return rgb, alpha, np.where(surface, nh + nf, 0.0), surface, amb, np.where(hi >= lo, hi - lo, 0.0), sw, mag


def check_motion_against_reference(pkg, beauty, aov, mv, prev, prev_cam, origin, **params):
    """Tolerance: 8 ulps of the largest colour in the pixel's blend (the 8 ulps of tests/test_temporal_cpu.py, which takes them of the
    result: the same unless the blend cancels) plus what 1e-4 px of projection error moves the
    normalised bilinear mean of the counted taps: a shift of the weights by 1e-4 changes sum(w * c) / sum(w) by at most 1e-4 * spread /
    Sw (that file leaves the 1 / Sw out, which holds only while no tap of a pixel is refused; here many are)."""
    capi = pkg.capi
    got, hist = capi.temporal_integrate_motion_host(beauty, aov, mv, prev, prev_cam, origin, **params)
    rgb, alpha, count, surface, amb, spread, sw, mag = reference_motion(beauty, aov, mv, prev, prev_cam, origin, **params)
    # a pixel whose accepted taps weigh next to nothing gets a tolerance of many times the spread and checks nothing: such pixels
    # count as ambiguous, under the same 2 % cap
    amb = amb | ((sw > 0) & (sw < 0.05))
    assert amb.mean() < 0.02, amb.mean()
    ok = ~amb
    ulps = lambda x: np.spacing(np.abs(x).astype(f32)).astype(np.float64)
    moved = 1e-4 * spread / np.maximum(sw, 1e-6)[..., None]
    err = np.abs(got[..., :3] - rgb)
    assert np.all((err <= 8 * ulps(np.maximum(mag, np.abs(rgb))) + (moved[..., :3] + moved[..., 3:]))[ok]), float(err[ok].max())
    assert np.array_equal(got[..., 3].view(np.uint32)[ok], alpha[ok])
    assert np.all((np.abs(hist["count"] - count) <= 8 * ulps(count) + moved[..., 3])[ok])
    assert same(hist["position"][surface], aov[..., 8:11][surface]), "the record keeps the current pose"
    assert same(hist["color"][surface], got[..., :3][surface])
    assert np.array_equal(hist["valid"], (surface & (hist["count"] > 0)).astype(np.uint32))
    assert not hist.view(np.uint32).reshape(hist.shape + (12,))[~surface].any()
    assert same(got[~surface], beauty[~surface])
    return got, hist, surface


@pytest.mark.parametrize("case", ["wobble", "wobble_camera", "other_rect", "tile"])
def test_motion_integration_matches_the_float64_restatement(pkg, case):
    """The box room of tests/test_temporal_cpu.py; its walls move by a smooth displacement field (every pixel's prev_position is its
    position minus the field there), some pixels carry flags == 0, and where the field is large the history holds another surface."""
    W, H = 96, 54
    prev_pose, x0, y0, pW, pH, px0, py0, cw, ch = BASE, 0, 0, W, H, 0, 0, W, H
    if case == "wobble":                              # (nearly the same camera: not exactly, or the flags == 0 pixels would all sit on tap cell boundaries)
        prev_pose = (0.52, 1.5, 1.0, -5.1, 200.3)
    elif case == "wobble_camera":
        prev_pose = (0.6, 1.45, 1.05, -4.0, 198.0)
    elif case == "other_rect":
        prev_pose, pW, pH, px0, py0 = (0.6, 1.5, 1.0, -5.0, 198.0), 70, 40, 13, 9
    elif case == "tile":
        prev_pose, x0, y0, W, H, px0, py0, pW, pH = (0.5, 1.5, 1.0, -4.0, 199.0), 20, 12, 50, 30, 10, 4, 70, 40
    cur = camera(pkg, cw, ch, BASE)
    prev_cam = camera(pkg, cw, ch, prev_pose)
    aov = room_aov(cur, W, H, x0, y0, seed=3)
    prev = room_history(prev_cam, pW, pH, px0, py0, seed=4)
    beauty = noisy_beauty(W, H, 5)
    x = aov[..., 8:11].astype(np.float64)
    n = aov[..., 4:7].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.nan_to_num(n / np.linalg.norm(n, axis=-1, keepdims=True))
    # the surface slid along itself (tangential), except in one region where it also moved off its plane by far more than plane_dist
    field = 0.15 * np.stack([np.sin(0.9 * x[..., 1] + 0.3), np.sin(1.1 * x[..., 2]), np.sin(0.7 * x[..., 0] + 1.0)], -1)
    field -= n * (field * n).sum(-1, keepdims=True)
    off_plane = (x[..., 0] > 4.0)
    field[off_plane] += n[off_plane] * 0.8
    mv = np.zeros((H, W), pkg.capi.motion_dtype)
    u32 = aov.view(np.uint32)
    hit = (u32[..., 12].view(np.int32) != -1) & (u32[..., 14] == 0)
    mv["prev_position"][hit] = (x - field)[hit]
    mv["flags"][hit] = 1
    rng = np.random.default_rng(6)
    drop = hit & (rng.random((H, W)) < 0.1)
    mv["flags"][drop] = 0; mv["prev_position"][drop] = 0
    got, hist, surface = check_motion_against_reference(pkg, beauty, aov, mv, prev, prev_cam, (px0, py0))
    took = surface & (got[..., 3].view(np.uint32) != beauty[..., 3].view(np.uint32))
    assert took.mean() > 0.3, "a good share of the pixels uses history"
    sel = surface & off_plane & (mv["flags"] == 1)
    if sel.sum() > 20:
        assert took[sel].mean() < 0.2, "where another surface lies at the previous position the plane test refuses the taps"
    plain, _ = pkg.capi.temporal_integrate_host(beauty, aov, prev, prev_cam, (px0, py0))
    assert not same(plain, got), "the motion plane changes the lookup"
    # the thread count changes no bit
    for t in (1, 3):
        g2, h2 = pkg.capi.temporal_integrate_motion_host(beauty, aov, mv, prev, prev_cam, (px0, py0), threads=t)
        assert same(g2, got) and same(h2, hist)


def test_arguments_are_refused_without_a_gpu(pkg, cornell_scene):
    capi = pkg.capi
    lib = capi.lib()
    P = C.c_void_p
    scene = cornell_scene
    W, H = 16, 8
    cam, rays, hits, aov = scene_frame(pkg, scene, W, H, scene["verts"])
    tris, verts = scene["tris"], scene["verts"]
    out = np.zeros((H, W), capi.motion_dtype)
    g = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x

    def host(h=hits, a=aov, n=W * H, t=tris, nt=len(tris), vn=verts, vp=verts, nv=len(verts), o=out):
        return lib.gmupt_motion_host(P(g(h)), P(g(a)), n, P(g(t)), nt, P(g(vn)), P(g(vp)), nv, P(g(o)))
    assert host() == 0 and host(n=0, h=None) == 0
    hit_tri = int(hits["triangle"].max())
    assert hit_tri >= 0
    for kw in ({"h": None}, {"a": None}, {"t": None}, {"vn": None}, {"vp": None}, {"o": None}, {"nt": hit_tri}, {"nv": 1}):
        assert host(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(capi.GmuptError):
        capi.motion_host(hits, aov, tris, verts, verts[:-1])               # vertex count mismatch
    # the integration: the motion plane is one more input that no output may overlap; NULL is allowed
    beauty = noisy_beauty(W, H, 1)
    res, hist = np.zeros_like(beauty), np.zeros((H, W), capi.history_dtype)
    tp = capi.temporal_params()

    def integ(m=out, o=res, oh=hist, b=beauty):
        return lib.gmupt_temporal_integrate_motion_host(P(g(b)), P(g(aov)), P(g(m)), W, H, None, None, 0, 0, 0, 0, C.byref(tp), P(g(o)), P(g(oh)), 2)
    assert integ() == 0 and integ(m=None) == 0
    big = np.zeros((H, W, 12), f32)
    for kw in ({"o": out.view(f32).reshape(H, W, 4)}, {"m": big, "oh": big}, {"b": None}, {"o": None}):
        assert integ(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    # the device entries check what needs no device first
    n = res.nbytes
    assert lib.gmupt_temporal_denoise_image_motion(None, P(16), P(4096), P(8), C.byref(cam), 0, 0, W, H, 1, C.byref(tp), P(8192), n, None) == capi.ERR_INVALID_ARGUMENT
    assert b"misaligned motion" in lib.gmupt_last_error()
    assert lib.gmupt_temporal_denoise_image_motion(None, P(16), P(4096), P(32768), C.byref(cam), 0, 0, W, H, 1, C.byref(tp), P(8192), n, None) == capi.ERR_INVALID_ARGUMENT
    assert b"null handle" in lib.gmupt_last_error()
    assert lib.gmupt_render_denoised_temporal_motion(None, None, 1, C.byref(tp), P(16), n, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_aovs_motion(None, 1, P(16), 4, P(16), 64, P(16), 16, None) == capi.ERR_INVALID_ARGUMENT


def test_session_keeps_the_history_only_when_asked(pkg):
    """ProgressiveSession.set_vertices: the default drops the history; keep_history=True keeps the handle and routes the preview through
    the motion entry point."""
    events = []

    class Fake:
        def __getattr__(self, name):
            return lambda *a, **k: (events.append(name), Result())[1]

    class Result:
        def cpu(self):
            return self

        def numpy(self):
            return "image"

    cam = Fake()
    sess = pkg.progressive.ProgressiveSession(Fake(), cam, 8, 4, preview_every=0)
    sess.temporal = Fake()
    sb = Fake(); sb.verts = Fake()
    sess.set_vertices(sb, np.zeros((3, 3), f32))
    assert events.count("reset") == 1 and not sess.motion
    sess.denoised_temporal()
    assert "denoise_temporal" in events and "denoise_temporal_motion" not in events
    del events[:]
    # the first keep_history=True meets record sets of the plain entry point (no pose): dropped once, then kept
    sess.set_vertices(sb, np.zeros((3, 3), f32), keep_history=True)
    assert events.count("reset") == 1 and "refit" in events and "reset_accumulation" in events and sess.motion
    assert sess.denoised_temporal() == "image"
    assert "denoise_temporal_motion" in events and "denoise_temporal" not in events
    del events[:]
    sess.set_vertices(sb, np.zeros((3, 3), f32), keep_history=True)
    assert "reset" not in events and "refit" in events
    sess.set_vertices(sb, np.zeros((3, 3), f32))
    assert events.count("reset") == 1, "the default still drops it"
    # a session made for moving geometry uses the motion entry point from the start and drops nothing
    del events[:]
    sess = pkg.progressive.ProgressiveSession(Fake(), cam, 8, 4, preview_every=0, motion=True)
    sess.temporal = Fake()
    sess.denoised_temporal()
    sess.set_vertices(sb, np.zeros((3, 3), f32), keep_history=True)
    assert "reset" not in events and "denoise_temporal_motion" in events and "denoise_temporal" not in events

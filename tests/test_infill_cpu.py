"""CPU tests of the guided infill (include/gmupt.h, "Infill"): struct layouts and exports, the host rule gmupt_infill_host against an
independent float64 restatement written from the header text, the exact consequences the header states (frames without holes or without
sources, the reach, material and facing, 1x1 images, NaN guides, alpha bits, pass-through, thread count) and the argument checks.  The
device stage is compared with the host rule bit for bit in tests/test_infill_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_SYMBOLS = ("gmupt_infill_default_params", "gmupt_infill_image", "gmupt_infill_host", "gmupt_temporal_preview_image", "gmupt_render_preview")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gmupt.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(gmupt_infill_params), offsetof(gmupt_infill_params, passes), offsetof(gmupt_infill_params, sigma_normal),
           offsetof(gmupt_infill_params, sigma_plane), offsetof(gmupt_infill_params, sigma_albedo));
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(gmupt_infill_info), offsetof(gmupt_infill_info, sources), offsetof(gmupt_infill_info, holes),
           offsetof(gmupt_infill_info, filled), offsetof(gmupt_infill_info, open_left), offsetof(gmupt_infill_info, ms));
    printf("%d %u\n", GMUPT_INFILL_MAX_PASSES, GMUPT_PREVIEW_MOTION);
    return 0;
}
"""


def test_layouts_of_header_and_binding(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    prm, info, consts = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    capi = pkg.capi
    assert prm == [16, 0, 4, 8, 12]
    assert prm == [C.sizeof(capi.InfillParams)] + [getattr(capi.InfillParams, n).offset for n in ("passes", "sigma_normal", "sigma_plane", "sigma_albedo")]
    assert info == [24, 0, 4, 8, 12, 16]
    assert info == [C.sizeof(capi.InfillInfo)] + [getattr(capi.InfillInfo, n).offset for n in ("sources", "holes", "filled", "open_left", "ms")]
    assert consts == [capi.INFILL_MAX_PASSES, capi.PREVIEW_MOTION] == [8, 1]


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in pkg.capi.SYMBOLS, name
        assert getattr(lib, name, None) is not None, name
    assert "---- Infill" in header
    d = pkg.capi.infill_params()
    assert d.passes == 6 and d.sigma_plane == f32(0.02) and d.sigma_albedo == f32(0.1) and 0 < d.sigma_normal <= 128
    with pytest.raises(TypeError):
        pkg.capi.infill_params(sigma_color=1.0)   # there is no luminance term


# ---------------------------------------------------------------------------------------------------- inputs
def records(albedo, depth, normal, position, triangle, light, material):
    """(H, W, 16) float32 gmupt_aov records from per-pixel planes."""
    H, W = depth.shape
    a = np.zeros((H, W, 16), f32)
    a[..., 0:3] = albedo; a[..., 3] = depth; a[..., 4:7] = normal; a[..., 7] = 0.5
    a[..., 8:11] = position; a[..., 11] = 0.0
    u = a.view(np.uint32)
    u[..., 12] = np.asarray(triangle, np.int32).view(np.uint32); u[..., 13] = material; u[..., 14] = light; u[..., 15] = 1
    return a


def beauty_of(rgb, count):
    b = np.zeros(rgb.shape[:2] + (4,), f32)
    b[..., :3] = rgb
    b[..., 3] = np.asarray(count, np.uint32).view(f32)
    return b


# six planar regions: normal, in-plane axes and material.  Regions 0 / 1 are parallel planes of one material (a depth step), 0 / 2 a
# crease of one material whose normals face apart (cosine < 0: weight exactly 0 in any precision), 3 / 5 another such crease, 4 alone.
REGION_N = np.array([[0, 0, 1], [0, 0, 1], [0, 0.6, -0.8], [1, 0, 0], [0, -0.8, 0.6], [-0.6, 0, 0.8]], np.float64)
REGION_MAT = np.array([1, 1, 1, 2, 7, 2], np.uint32)


def random_inputs(W, H, seed, density=0.3):
    """A scene-like random frame: planar regions (several materials, a crease, a depth step), sparse samples, and every kind of pixel
    that is no surface.  Within a region the guides are smooth, so every weight that is not exactly 0 is far above binary32 underflow
    (the exponent stays below ~40): which holes are filled is the same in binary32 and in float64."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    region = (xs * 3 // max(W, 1) + 3 * (ys * 2 // max(H, 1))).astype(int)
    nrm = REGION_N[region]
    e1 = np.cross(nrm, np.where(np.abs(nrm[..., :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])); e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)
    e2 = np.cross(nrm, e1)
    pos = e1 * (xs * 0.05)[..., None] + e2 * (ys * 0.05)[..., None] + nrm * (region * 0.3 + rng.normal(0, 0.002, (H, W)))[..., None]
    n = (nrm + rng.normal(0, 0.01, (H, W, 3))) * rng.uniform(0.5, 3.0, (H, W, 1))       # bumpy, not normalised
    depth = rng.uniform(1.0, 8.0, (H, W))
    albedos = rng.uniform(0.05, 0.95, (6, 3))
    alb = albedos[region] + rng.normal(0, 0.01, (H, W, 3))
    rgb = np.clip(alb * 0.6 + rng.normal(0, 0.15, (H, W, 3)), 0, 1)
    count = np.where(rng.random((H, W)) < density, rng.integers(1, 6, (H, W)), 0).astype(np.uint32)
    tri = rng.integers(0, 1000, (H, W)).astype(np.int32)
    light = np.zeros((H, W), np.uint32)
    kind = rng.random((H, W))
    tri[kind < 0.05] = -1                                                   # misses
    light[(kind >= 0.05) & (kind < 0.08)] = 1 + rng.integers(0, 3)          # light spheres
    n[(kind >= 0.08) & (kind < 0.10)] = 0.0                                 # zero normal
    rgb[tri == -1] = rng.uniform(0, 1, 3)
    return beauty_of(rgb, count), records(alb, depth, n, pos, tri, light, REGION_MAT[region])


def plane(W, H, seed=0, material=1, normal=(0.0, 0.0, 1.0)):
    """One flat surface of one material facing `normal`, every pixel sampled once, random colours."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    pos = np.stack([xs * 0.05, ys * 0.05, np.zeros((H, W))], -1)
    aov = records(np.full((H, W, 3), 0.5), np.full((H, W), 2.0), np.broadcast_to(np.asarray(normal, np.float64), (H, W, 3)), pos,
                  np.arange(H * W, dtype=np.int32).reshape(H, W), np.zeros((H, W), np.uint32), np.full((H, W), material, np.uint32))
    return beauty_of(rng.uniform(0.1, 0.9, (H, W, 3)), np.ones((H, W), np.uint32)), aov


def uncount(beauty, mask):
    """The frame with the pixels of `mask` turned into pixels without a sample (colour 0, count 0)."""
    b = beauty.copy()
    b[mask] = 0.0
    return b


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def shifted(a, dy, dx):
    """(out, inside): out[y, x] = a[y + dy, x + dx] where that lies inside the image."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((H, W), bool)
    if abs(dy) >= H or abs(dx) >= W:
        return out, inside
    dst = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
    src = (slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx)))
    out[dst] = a[src]
    inside[dst] = True
    return out, inside


def reference(beauty, aov, passes, sigma_normal, sigma_plane, sigma_albedo):
    """The rule of include/gmupt.h ("Infill") in float64 numpy (exp / pow of numpy, sums in any order): (rgb, filled mask, classes)."""
    u = aov.view(np.uint32)
    count = beauty[..., 3].view(np.uint32)
    nraw = aov[..., 4:7].astype(np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt((nraw ** 2).sum(-1))
        surface = (u[..., 12].view(np.int32) != -1) & (u[..., 14] == 0) & (length > 0)
        n = nraw / np.where(length > 0, length, 1)[..., None]
        known = surface & (count > 0)
        opened = surface & (count == 0)
        sources, holes = known.copy(), opened.copy()
        c = beauty[..., :3].astype(np.float64)
        z = aov[..., 3].astype(np.float64); x = aov[..., 8:11].astype(np.float64); a = aov[..., 0:3].astype(np.float64)
        mat = u[..., 13]
        h5 = {-2: 1 / 16, -1: 0.25, 0: 0.375, 1: 0.25, 2: 1 / 16}
        for k in range(passes):
            s = 1 << k
            sw = np.zeros(z.shape); sc = np.zeros(c.shape)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    kq, ins = shifted(known, s * j, s * i)
                    m = ins & kq & opened & (shifted(mat, s * j, s * i)[0] == mat)
                    nq = shifted(n, s * j, s * i)[0]; xq = shifted(x, s * j, s * i)[0]
                    aq = shifted(a, s * j, s * i)[0]; cq = shifted(c, s * j, s * i)[0]
                    cos = (n * nq).sum(-1)
                    wn = np.where(cos > 0, cos, 0) ** sigma_normal
                    dxp = np.abs((n * (xq - x)).sum(-1)) / (sigma_plane * z)
                    da = np.abs(aq - a).sum(-1) / sigma_albedo
                    w = np.where(m, h5[i] * h5[j] * wn * np.exp(-(dxp + da)), 0.0)
                    sw += w; sc += w[..., None] * np.where(m[..., None], cq, 0)
            fill = opened & (sw > 0)
            c = np.where(fill[..., None], sc / np.where(sw > 0, sw, 1)[..., None], c)
            known = known | fill; opened = opened & ~fill
    return c, holes & ~opened, (surface, sources, holes)


# |host - float64| on a filled colour, in ulps of 1.0 (2^-23), the top of the colour range.  A filled colour is a normalised mean of
# source colours in [0, 1]: the rounding of a weight moves it by a share of the spread of those colours, not of its own size, so a dark
# result is no more exact than a bright one (in ulps of the value the same errors read 295 and 30).  The weights carry the error: dpow =
# dexp2(sigma_normal * dlog2(cos)) multiplies the few ulps of dlog2 by sigma_normal, so the bound is per parameter set.  Measured on the
# frames below: 18.1 ulps (2.16e-6) at sigma_normal = 128 and 2.4 ulps (2.9e-7) at sigma_normal = 16; asserted at twice that.
ULP1 = 2.0 ** -23
TOL_ULPS = [36.0, 5.0]
PSETS = [{"sigma_normal": 128.0, "sigma_plane": 0.02, "sigma_albedo": 0.1}, {"sigma_normal": 16.0, "sigma_plane": 0.5, "sigma_albedo": 0.8}]


@pytest.mark.parametrize("W,H,seed,density", [(37, 23, 1, 0.3), (64, 48, 2, 0.02), (1, 1, 3, 0.5), (5, 40, 4, 0.1), (48, 33, 5, 0.005)])
def test_host_rule_matches_the_float64_restatement(pkg, W, H, seed, density):
    beauty, aov = random_inputs(W, H, seed, density)
    worst = 0.0
    for params, tol in zip(PSETS, TOL_ULPS):
        for passes in range(1, 9):
            got, info = pkg.capi.infill_host(beauty, aov, threads=4, passes=passes, **params)
            ref, filled, (surface, sources, holes) = reference(beauty, aov, passes, **params)
            assert got.shape == (H, W, 4) and got.dtype == np.float32
            got_filled = holes & (bits(got)[..., 3] == 1)
            assert np.array_equal(got_filled, filled), (W, H, passes, params, int((got_filled ^ filled).sum()))   # the same set of pixels
            assert (info["sources"], info["holes"], info["filled"], info["open_left"]) == (sources.sum(), holes.sum(), filled.sum(), (holes & ~filled).sum())
            err = np.abs(got[..., :3].astype(np.float64) - ref)[filled]
            if err.size:
                worst = max(worst, float(err.max()))
                assert err.max() <= tol * ULP1, (W, H, passes, params, float(err.max() / ULP1))
            keep = ~filled
            assert np.array_equal(bits(got)[keep], bits(beauty)[keep])
    print("largest |host - float64| on a filled colour: %.3g = %.1f ulps of 1.0" % (worst, worst / ULP1))


def test_thread_count_does_not_change_a_bit(pkg):
    beauty, aov = random_inputs(97, 61, 5, 0.05)
    one, info1 = pkg.capi.infill_host(beauty, aov, threads=1)
    assert info1["filled"] > 1000
    for t in (0, 2, 3, 7, 16, 64):
        out, info = pkg.capi.infill_host(beauty, aov, threads=t)
        assert np.array_equal(bits(out), bits(one)) and info == info1, t


def test_frames_without_holes_or_without_sources_come_through(pkg):
    beauty, aov = random_inputs(40, 30, 6, 1.0)                    # every surface pixel sampled
    out, info = pkg.capi.infill_host(beauty, aov)
    assert np.array_equal(bits(out), bits(beauty)) and info["holes"] == 0 and info["filled"] == 0 and info["sources"] > 900
    beauty, aov = random_inputs(40, 30, 6, 0.0)                    # no sample anywhere
    beauty[..., :3] = np.random.default_rng(1).uniform(0, 1, beauty[..., :3].shape)   # whatever the colours hold
    out, info = pkg.capi.infill_host(beauty, aov, passes=8)
    assert np.array_equal(bits(out), bits(beauty)) and info["sources"] == 0 and info["filled"] == 0 and info["open_left"] == info["holes"] > 900


def test_reach_is_twice_two_to_the_passes_minus_one(pkg):
    b, aov = plane(40, 1)
    holes = np.ones((1, 40), bool); holes[0, 0] = False            # one source at x = 0
    for passes in (1, 2, 3, 4):
        out, info = pkg.capi.infill_host(uncount(b, holes), aov, passes=passes)
        reach = 2 * (2 ** passes - 1)
        alpha = bits(out)[0, :, 3]
        assert np.array_equal(alpha[1:], (np.arange(1, 40) <= reach).astype(np.uint32)), passes   # filled: alpha is the bits of count 1
        assert info["filled"] == min(reach, 39) and info["open_left"] == 39 - min(reach, 39)
        assert np.array_equal(bits(out)[0, reach + 1:], bits(uncount(b, holes))[0, reach + 1:])   # open holes keep their input bits
        # one source: its colour, but for the rounding of (w * c) / w, at most one ulp (2^-23 relative) per pass of the chain
        assert np.allclose(out[0, 1:reach + 1, :3], b[0, 0, :3], rtol=passes * 2.0 ** -23, atol=0)
    # the same along y, and 126 at passes = 6
    b, aov = plane(1, 140)
    holes = np.ones((140, 1), bool); holes[139, 0] = False
    out, info = pkg.capi.infill_host(uncount(b, holes), aov, passes=6)
    assert info["filled"] == 126 and np.array_equal(bits(out)[:139, 0, 3], (np.arange(139) >= 139 - 126).astype(np.uint32))


def test_other_material_or_other_facing_leaves_the_hole_open(pkg):
    b, aov = plane(9, 9)
    hole = np.zeros((9, 9), bool); hole[4, 4] = True
    base = uncount(b, hole)
    out, info = pkg.capi.infill_host(base, aov)
    assert info == dict(info, sources=80, holes=1, filled=1, open_left=0) and bits(out)[4, 4, 3] == 1
    other = aov.copy(); other.view(np.uint32)[..., 13] = 2; other.view(np.uint32)[4, 4, 13] = 1         # every source has another material
    out, info = pkg.capi.infill_host(base, other, passes=8)
    assert info["filled"] == 0 and info["open_left"] == 1 and np.array_equal(bits(out), bits(base))
    back = aov.copy(); back[..., 4:7] = (0, 0, -1); back[4, 4, 4:7] = (0, 0, 1)                          # every source faces the other way
    out, info = pkg.capi.infill_host(base, back, passes=8)
    assert info["filled"] == 0 and info["open_left"] == 1 and np.array_equal(bits(out), bits(base))
    side = aov.copy(); side[..., 4:7] = (1, 0, 0); side[4, 4, 4:7] = (0, 0, 1)                           # perpendicular: cosine 0, weight 0
    out, info = pkg.capi.infill_host(base, side, passes=8)
    assert info["filled"] == 0 and np.array_equal(bits(out), bits(base))


def test_one_pixel_images(pkg):
    b, aov = plane(1, 1)
    out, info = pkg.capi.infill_host(b, aov, passes=8)
    assert np.array_equal(bits(out), bits(b)) and (info["sources"], info["holes"], info["filled"], info["open_left"]) == (1, 0, 0, 0)
    hole = uncount(b, np.ones((1, 1), bool))
    out, info = pkg.capi.infill_host(hole, aov, passes=8)
    assert np.array_equal(bits(out), bits(hole)) and (info["sources"], info["holes"], info["filled"], info["open_left"]) == (0, 1, 0, 1)


def test_nan_guides_leave_the_hole_open_and_nan_colours_propagate(pkg):
    b, aov = plane(9, 9)
    hole = np.zeros((9, 9), bool); hole[4, 4] = True
    base = uncount(b, hole)
    bad = aov.copy(); bad[4, 4, 8] = np.nan                        # the hole's position: every weight is NaN, W > 0 is false
    out, info = pkg.capi.infill_host(base, bad, passes=4)
    assert info["open_left"] == 1 and np.array_equal(bits(out), bits(base))
    bad = aov.copy(); bad[4, 5, 10] = np.inf                       # one source's position along the normal: d_x = inf, its weight is 0, the others fill
    out, info = pkg.capi.infill_host(base, bad, passes=1)
    assert info["filled"] == 1 and np.all(np.isfinite(out[4, 4, :3]))
    bad = aov.copy(); bad[4, 5, 9] = np.inf                        # across the normal: 0 * inf is NaN in the plane distance, W is NaN, the hole stays open
    out, info = pkg.capi.infill_host(base, bad, passes=1)
    assert info["filled"] == 0 and np.array_equal(bits(out), bits(base))
    nanc = base.copy(); nanc[4, 5, 0] = np.nan                     # one source's red: the filled red is NaN, green and blue are not
    out, info = pkg.capi.infill_host(nanc, aov, passes=1)
    assert info["filled"] == 1 and np.isnan(out[4, 4, 0]) and np.all(np.isfinite(out[4, 4, 1:3])) and bits(out)[4, 4, 3] == 1
    keep = ~hole
    assert np.array_equal(bits(out)[keep], bits(nanc)[keep])


def test_everything_but_filled_holes_comes_through_bit_for_bit(pkg):
    beauty, aov = random_inputs(64, 48, 8, 0.1)
    _, _, (surface, sources, holes) = reference(beauty, aov, 1, **PSETS[0])
    bv = bits(beauty).copy()
    junk = np.random.default_rng(7).integers(0, 2 ** 32, (int((~surface).sum()), 4), dtype=np.uint64).astype(np.uint32)
    junk[0] = [0x7FC00001, 0x7F800000, 0xFF800000, 0x7FC12345]     # what is no surface holds arbitrary bits, alpha included
    bv[~surface] = junk
    b2 = bv.view(np.float32)
    out, info = pkg.capi.infill_host(b2, aov)
    ov = bits(out)
    assert np.array_equal(ov[~surface], bv[~surface]) and np.array_equal(ov[sources], bv[sources])
    filled = holes & (ov[..., 3] == 1)
    assert info["filled"] == filled.sum() > 1000
    assert np.array_equal(ov[holes & ~filled], bv[holes & ~filled])
    clean, _ = pkg.capi.infill_host(beauty, aov)
    assert np.array_equal(bits(clean)[surface], ov[surface])        # and they are never read as taps
    # a filled colour is a convex combination of source colours
    assert out[filled][:, :3].min() >= beauty[sources][:, :3].min() - 1e-6 and out[filled][:, :3].max() <= beauty[sources][:, :3].max() + 1e-6


def test_argument_checks(pkg):
    capi, lib = pkg.capi, pkg.capi.lib()
    beauty, aov = random_inputs(8, 6, 9, 0.3)
    W, H = 8, 6
    out = np.full_like(beauty, 7.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ip = capi.infill_params()
    info = capi.InfillInfo(); info.sources = 77

    def call(b=ptr(beauty), a=ptr(aov), w=W, h=H, p=ip, o=ptr(out), nbytes=out.nbytes):
        return lib.gmupt_infill_host(b, a, w, h, C.byref(p) if p is not None else None, o, nbytes, C.byref(info), 2)

    assert call() == 0 and info.sources + info.holes > 0
    ok = out.copy()
    assert call(p=None) == 0 and np.array_equal(bits(out), bits(ok))                      # NULL params: the defaults
    out[:] = 7.0; info.sources = 77
    bad = capi.ERR_INVALID_ARGUMENT
    assert call(b=None) == bad and call(a=None) == bad and call(o=None) == bad
    assert call(w=0) == bad and call(h=0) == bad
    assert call(nbytes=out.nbytes - 1) == bad
    assert call(o=ptr(beauty)) == bad                                                      # overlapping output
    for passes in (0, 9, 2 ** 31):
        assert call(p=capi.infill_params(passes=passes)) == bad, passes
    for field in ("sigma_normal", "sigma_plane", "sigma_albedo"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert call(p=capi.infill_params(**{field: v})) == bad, (field, v)
    assert b"infill" in lib.gmupt_last_error()
    assert np.all(out == 7.0) and info.sources == 77                                       # nothing is written on an error
    for passes in (1, 8):
        assert call(p=capi.infill_params(passes=passes)) == 0
    # the entry points that need a device refuse before they touch one
    ms = C.c_float(0)
    assert lib.gmupt_infill_image(None, ptr(beauty), ptr(aov), W, H, None, ptr(out), out.nbytes, None) == bad
    assert lib.gmupt_temporal_preview_image(None, ptr(beauty), ptr(aov), None, None, 0, 0, W, H, 0, None, C.byref(ip), ptr(out), out.nbytes, C.byref(ms)) == bad
    assert lib.gmupt_render_preview(None, None, 0, 1, None, C.byref(ip), ptr(out), out.nbytes, None) == bad
    assert lib.gmupt_render_preview(None, None, 2, 1, None, None, ptr(out), out.nbytes, None) == bad          # unknown flag
    assert lib.gmupt_render_preview(None, None, capi.PREVIEW_MOTION, 1, None, None, ptr(out), out.nbytes, None) == bad   # motion without a handle
    with pytest.raises(capi.GmuptError):
        capi.infill_host(beauty[:, :4], aov)

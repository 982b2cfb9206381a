"""CPU tests of the a-trous denoiser (include/gmupt.h): the parameter layout, exports, argument checks that need no device, the host
filter gmupt_denoise_host against an independent float64 restatement of the filter, its invariants (thread count, invalid pixels, alpha
bits, the normal crease, albedo edges, noise reduction) and the C++ driver's --denoise option.  The device filter is compared with the
host filter bit for bit in tests/test_denoise_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gmu-path-tracer_amd", "host")
f32 = np.float32
FIELDS = ("passes", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gmupt.h"
#define OFF(f) printf(" %zu", offsetof(gmupt_denoise_params, f))
int main(void) {
    printf("%zu", sizeof(gmupt_denoise_params));
    OFF(passes); OFF(sigma_color); OFF(sigma_normal); OFF(sigma_plane); OFF(sigma_albedo);
    printf("\n%d\n", GMUPT_DENOISE_MAX_PASSES);
    return 0;
}
"""


def test_params_layout_of_header_and_binding(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rec, consts = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    capi = pkg.capi
    assert rec == [20, 0, 4, 8, 12, 16]
    assert rec == [C.sizeof(capi.DenoiseParams)] + [getattr(capi.DenoiseParams, n).offset for n in FIELDS]
    assert consts == [capi.DENOISE_MAX_PASSES] == [5]


def test_library_exports_the_denoiser(pkg):
    lib = pkg.capi.lib()
    for name in ("gmupt_denoise_image", "gmupt_render_denoised", "gmupt_denoise_host", "gmupt_denoise_default_params"):
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS
    d = pkg.capi.denoise_params()
    assert (d.passes, d.sigma_color, d.sigma_normal) == (5, 4.0, 128.0)
    assert d.sigma_plane == f32(0.02) and d.sigma_albedo == f32(0.1)
    with pytest.raises(TypeError):
        pkg.capi.denoise_params(sigma_spatial=1.0)


# ---------------------------------------------------------------------------------------------------- inputs
def records(albedo, depth, normal, position, triangle, light):
    """(H, W, 16) float32 gmupt_aov records from per-pixel planes."""
    H, W = depth.shape
    a = np.zeros((H, W, 16), f32)
    a[..., 0:3] = albedo; a[..., 3] = depth; a[..., 4:7] = normal; a[..., 7] = 0.5
    a[..., 8:11] = position; a[..., 11] = 0.0
    u = a.view(np.uint32)
    u[..., 12] = np.asarray(triangle, np.int32).view(np.uint32); u[..., 13] = 1; u[..., 14] = light; u[..., 15] = 1
    return a


def beauty_of(rgb, count):
    b = np.zeros(rgb.shape[:2] + (4,), f32)
    b[..., :3] = rgb
    b[..., 3] = np.asarray(count, np.uint32).view(f32)
    return b


def random_inputs(W, H, seed):
    """A scene-like random frame: a few planes with their own normals and albedos, noisy colours, and every kind of invalid pixel."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    region = (xs * 3 // W + 3 * (ys * 2 // H)).astype(int)                 # 6 regions
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8], [0, -0.8, 0.6], [0.3, 0.3, 0.9]], np.float64)
    albedos = rng.uniform(0.05, 0.95, (6, 3))
    n = normals[region] + rng.normal(0, 0.05, (H, W, 3))                    # bumpy, not normalised
    n[rng.random((H, W)) < 0.05] *= 3.0
    pos = np.stack([xs * 0.05, ys * 0.05, rng.normal(0, 0.01, (H, W)) + region * 0.3], -1)
    depth = rng.uniform(1.0, 8.0, (H, W))
    alb = albedos[region] + rng.normal(0, 0.02, (H, W, 3)) * (rng.random((H, W, 1)) < 0.3)
    rgb = np.clip(alb * 0.6 + rng.normal(0, 0.15, (H, W, 3)), 0, 1)
    count = rng.integers(1, 6, (H, W)).astype(np.uint32)
    tri = rng.integers(0, 1000, (H, W)).astype(np.int32)
    light = np.zeros((H, W), np.uint32)
    kind = rng.random((H, W))
    tri[kind < 0.06] = -1                                                   # misses
    light[(kind >= 0.06) & (kind < 0.1)] = 1 + rng.integers(0, 3)          # light spheres
    count[(kind >= 0.1) & (kind < 0.13)] = 0                                # no samples yet
    n[(kind >= 0.13) & (kind < 0.15)] = 0.0                                 # zero normal
    rgb[tri == -1] = rng.uniform(0, 1, 3)
    aov = records(alb, depth, n, pos, tri, light)
    return beauty_of(rgb, count), aov


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


def reference(beauty, aov, passes=5, sigma_color=4.0, sigma_normal=128.0, sigma_plane=0.02, sigma_albedo=0.1):
    """The filter of include/gmupt.h in float64 numpy (exp / pow / sqrt of numpy, sums in any order), with the rule's IEEE behaviour on
    non-finite values: max(0, .) drops a NaN (np.fmax), dexp2 is 0 at or below 2^-150 and inf above 2^128, and no denominator of a
    valid pixel is masked."""
    with np.errstate(all="ignore"):
        return _reference(beauty, aov, passes, sigma_color, sigma_normal, sigma_plane, sigma_albedo)


def _exp(d):
    """exp(-d) as the rule's dexp2(-d * log2(e)): 0 for an exponent at or below -150, inf above 128, NaN kept."""
    y = -d * 1.4426950408889634
    return np.where(y > 128.0, np.inf, np.where(y > -150.0, np.exp2(np.clip(y, -150.0, 128.0)), np.where(np.isnan(y), np.nan, 0.0)))


def _reference(beauty, aov, passes, sigma_color, sigma_normal, sigma_plane, sigma_albedo):
    u = aov.view(np.uint32)
    count = beauty[..., 3].view(np.uint32)
    nraw = aov[..., 4:7].astype(np.float64)
    length = np.sqrt((nraw ** 2).sum(-1))
    valid = (count > 0) & (u[..., 12].view(np.int32) != -1) & (u[..., 14] == 0) & (length > 0)
    n = nraw / np.where(length > 0, length, 1)[..., None]
    c = beauty[..., :3].astype(np.float64)
    l = (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]
    z = aov[..., 3].astype(np.float64)
    x = aov[..., 8:11].astype(np.float64)
    a = aov[..., 0:3].astype(np.float64)
    s1 = np.zeros(l.shape); s2 = np.zeros(l.shape); cnt = np.zeros(l.shape)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            lq, ins = shifted(l, dy, dx); vq, _ = shifted(valid, dy, dx)
            m = ins & vq
            s1 += np.where(m, lq, 0); s2 += np.where(m, lq * lq, 0); cnt += m
    cnt = np.maximum(cnt, 1)
    v = np.fmax(0.0, s2 / cnt - (s1 / cnt) ** 2)
    h3 = {-1: 0.25, 0: 0.5, 1: 0.25}
    h5 = {-2: 1 / 16, -1: 0.25, 0: 0.375, 1: 0.25, 2: 1 / 16}
    for k in range(passes):
        s = 1 << k
        gw = np.zeros(l.shape); gv = np.zeros(l.shape)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ins = shifted(v, dy, dx); ok, _ = shifted(valid, dy, dx)
                m = ins & ok
                gw += np.where(m, h3[dx] * h3[dy], 0); gv += np.where(m, h3[dx] * h3[dy] * vq, 0)
        g = gv / np.where(gw > 0, gw, 1)
        den_l = sigma_color * np.sqrt(g) + 1e-6
        den_x = sigma_plane * np.where(valid, z, 1)
        sw = np.zeros(l.shape); sc = np.zeros(c.shape); sv = np.zeros(l.shape)
        for j in range(-2, 3):
            for i in range(-2, 3):
                ok, ins = shifted(valid, s * j, s * i)
                m = ins & ok & valid
                nq = shifted(n, s * j, s * i)[0]; lq = shifted(l, s * j, s * i)[0]; xq = shifted(x, s * j, s * i)[0]
                aq = shifted(a, s * j, s * i)[0]; cq = shifted(c, s * j, s * i)[0]; vq = shifted(v, s * j, s * i)[0]
                cos = np.fmax(0.0, (n * nq).sum(-1))
                wn = np.where(cos > 0, cos, 0) ** sigma_normal
                dl = np.abs(l - lq) / den_l
                dxp = np.abs((n * (xq - x)).sum(-1)) / den_x
                da = np.abs(aq - a).sum(-1) / sigma_albedo
                w = np.where(m, h5[i] * h5[j] * wn * _exp(dl + dxp + da), 0.0)
                sw += w; sc += w[..., None] * np.where(m[..., None], cq, 0); sv += w * w * np.where(m, vq, 0)
        ok = valid & (sw > 0)
        c = np.where(ok[..., None], sc / np.where(sw > 0, sw, 1)[..., None], c)
        v = np.where(ok, sv / np.where(sw > 0, sw * sw, 1), v)
    out = beauty.astype(np.float64).copy()
    out[..., :3] = np.where(valid[..., None], c, beauty[..., :3])
    return out, valid


TOL = 2e-5   # |host - float64| on colours in [0, 1], measured at most 2.8e-6: the deterministic exp2 / log2 are within a few ulp


@pytest.mark.parametrize("W,H,seed", [(37, 23, 1), (64, 48, 2), (1, 1, 3), (5, 40, 4)])
def test_host_filter_matches_the_float64_restatement(pkg, W, H, seed):
    beauty, aov = random_inputs(W, H, seed)
    psets = [{}, {"sigma_color": 1.5, "sigma_normal": 16.0, "sigma_plane": 0.5, "sigma_albedo": 0.8}]
    for params in psets:
        for passes in range(1, 6):
            got = pkg.capi.denoise_host(beauty, aov, threads=4, passes=passes, **params)
            ref, valid = reference(beauty, aov, passes=passes, **params)
            assert got.shape == (H, W, 4) and got.dtype == np.float32
            err = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
            assert err.max() <= TOL, (W, H, passes, params, float(err.max()))
            if valid.sum() > 20:
                moved = np.abs(got[..., :3] - beauty[..., :3])[valid].max()
                assert moved > 1e-3, "the filter did something"


def test_thread_count_does_not_change_a_bit(pkg):
    beauty, aov = random_inputs(97, 61, 5)
    one = pkg.capi.denoise_host(beauty, aov, threads=1)
    for t in (2, 3, 7, 16, 64):
        assert np.array_equal(pkg.capi.denoise_host(beauty, aov, threads=t).view(np.uint32), one.view(np.uint32)), t


def test_invalid_pixels_and_alpha_come_through(pkg):
    beauty, aov = random_inputs(64, 48, 6)
    u = aov.view(np.uint32)
    # the colours of invalid pixels are arbitrary bits, NaN and inf included: they are never read as neighbours
    _, valid = reference(beauty, aov, passes=1)
    inv = ~valid
    junk = np.random.default_rng(7).integers(0, 2 ** 32, (int(inv.sum()), 3), dtype=np.uint64).astype(np.uint32)
    junk[0] = [0x7FC00001, 0x7F800000, 0xFF800000]
    bv = beauty.view(np.uint32).copy()
    bv[inv, :3] = junk
    b2 = bv.view(np.float32)
    out = pkg.capi.denoise_host(b2, aov, passes=3)
    ov = out.view(np.uint32)
    assert np.array_equal(ov[inv], bv[inv]), "invalid pixels are copied bit for bit"
    assert np.array_equal(ov[..., 3], bv[..., 3]), "alpha bits preserved"
    assert np.isfinite(out[valid]).all()
    clean = pkg.capi.denoise_host(beauty, aov, passes=3)
    assert np.array_equal(clean.view(np.uint32)[valid], ov[valid]), "invalid colours never reach a valid pixel"
    kinds = {"miss": (u[..., 12].view(np.int32) == -1).sum(), "light": (u[..., 14] > 0).sum(),
             "empty": (beauty[..., 3].view(np.uint32) == 0).sum(), "flat": (np.abs(aov[..., 4:7]).sum(-1) == 0).sum()}
    assert all(v > 0 for v in kinds.values()), kinds


def luminance32(rgb):
    return (f32(0.2126) * rgb[..., 0] + f32(0.7152) * rgb[..., 1]) + f32(0.0722) * rgb[..., 2]


def same_luminance(rgb):
    """Other colours with bit-identical binary32 luminance: red up, green down, blue searched ulp by ulp."""
    target = luminance32(rgb)
    new = rgb.copy()
    new[..., 0] = rgb[..., 0] + f32(0.1)
    new[..., 1] = rgb[..., 1] - f32(0.03)
    b0 = ((target.astype(np.float64) - f32(0.2126) * new[..., 0].astype(np.float64) - f32(0.7152) * new[..., 1].astype(np.float64)) / 0.0722).astype(f32)
    best = np.full(b0.shape, np.nan, f32)
    for k in range(0, 400):
        for sgn in (1, -1):
            cand = (b0.view(np.int32) + sgn * k).view(f32)
            trial = new.copy(); trial[..., 2] = cand
            hit = (luminance32(trial).view(np.uint32) == target.view(np.uint32)) & np.isnan(best)
            best[hit] = cand[hit]
    found = ~np.isnan(best)
    new[..., 2] = np.where(found, best, rgb[..., 2])
    new[~found] = rgb[~found]
    assert np.array_equal(luminance32(new).view(np.uint32), target.view(np.uint32))
    return new, found


def test_colour_does_not_cross_a_right_angle_crease(pkg):
    W, H = 48, 32
    rng = np.random.default_rng(11)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    right = xs >= W // 2
    n = np.where(right[..., None], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0])       # a 90-degree crease between the halves
    pos = np.where(right[..., None], np.stack([np.full_like(xs, 1.2), ys * 0.05, 3.0 - (xs - W // 2) * 0.05], -1),
                   np.stack([xs * 0.05, ys * 0.05, np.full_like(xs, 3.0)], -1))
    alb = np.full((H, W, 3), 0.5)
    rgb = rng.uniform(0.2, 0.8, (H, W, 3)).astype(f32)
    aov = records(alb, np.full((H, W), 4.0), n, pos, np.zeros((H, W), np.int32), np.zeros((H, W), np.uint32))
    beauty = beauty_of(rgb, np.full((H, W), 2, np.uint32))
    other, found = same_luminance(rgb)
    assert found[right].mean() > 0.95
    b2 = beauty.copy()
    b2[right, :3] = other[right]
    assert (b2[right, :3] != beauty[right, :3]).any(-1).mean() > 0.95
    a = pkg.capi.denoise_host(beauty, aov)
    b = pkg.capi.denoise_host(b2, aov)
    assert np.array_equal(a[~right].view(np.uint32), b[~right].view(np.uint32)), "the other half's colours leaked across the crease"
    assert not np.array_equal(a[right].view(np.uint32), b[right].view(np.uint32))
    # the test can see a leak: with one plane (same normals everywhere) the same change does move the left half
    flat = records(alb, np.full((H, W), 4.0), np.tile([0.0, 0.0, 1.0], (H, W, 1)), np.stack([xs * 0.05, ys * 0.05, np.full_like(xs, 3.0)], -1),
                   np.zeros((H, W), np.int32), np.zeros((H, W), np.uint32))
    assert not np.array_equal(pkg.capi.denoise_host(beauty, flat)[~right], pkg.capi.denoise_host(b2, flat)[~right])


NOISE_GAIN = 30.0   # MSE(noisy) / MSE(denoised) on the two-albedo plane below: measured 69.7


def test_noise_drops_and_albedo_edges_stay(pkg):
    W, H = 64, 48
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    right = xs >= W // 2
    alb = np.where(right[..., None], [0.2, 0.5, 0.8], [0.8, 0.3, 0.2])
    clean = (alb * 0.7).astype(f32)
    noisy = (clean + np.random.default_rng(3).normal(0, 0.1, clean.shape)).astype(f32)
    aov = records(alb, np.full((H, W), 3.0), np.tile([0.0, 0.0, 1.0], (H, W, 1)), np.stack([xs * 0.02, ys * 0.02, np.full_like(xs, 3.0)], -1),
                  np.zeros((H, W), np.int32), np.zeros((H, W), np.uint32))
    out = pkg.capi.denoise_host(beauty_of(noisy, np.full((H, W), 4, np.uint32)), aov)[..., :3]
    mse_noisy = float(((noisy - clean) ** 2).mean())
    mse_out = float(((out - clean) ** 2).mean())
    assert mse_noisy / mse_out >= NOISE_GAIN, (mse_noisy, mse_out, mse_noisy / mse_out)
    other = np.where(right[..., None], [0.8, 0.3, 0.2], [0.2, 0.5, 0.8]) * 0.7
    edge = (xs == W // 2 - 1) | (xs == W // 2)
    own = np.abs(out - clean).sum(-1); far = np.abs(out - other).sum(-1)
    assert (own[edge] < far[edge]).all(), "pixels next to the albedo edge stay on their side"
    assert own[edge].max() < 0.25


def test_arguments_are_refused_without_a_gpu(pkg):
    capi = pkg.capi
    lib = capi.lib()
    P = C.c_void_p
    W, H = 8, 4
    beauty = np.zeros((H, W, 4), f32); aov = np.zeros((H, W, 16), f32); out = np.zeros((H, W, 4), f32)
    b, a, o = (P(x.ctypes.data) for x in (beauty, aov, out))
    dp = capi.denoise_params()
    ok = lambda **kw: lib.gmupt_denoise_host(kw.get("b", b), kw.get("a", a), kw.get("w", W), kw.get("h", H), C.byref(kw.get("p", dp)),
                                            kw.get("o", o), kw.get("n", out.nbytes), 4)
    assert ok() == 0
    assert lib.gmupt_denoise_host(b, a, W, H, None, o, out.nbytes, 1) == 0          # NULL params: the defaults
    big = np.zeros((2 * H, W, 4), f32)                                               # overlapping ranges inside one buffer
    inside = lambda off: P(big.ctypes.data + off)
    assert ok(b=inside(0), o=inside(H * W * 16)) == 0                               # adjacent, not overlapping
    for bad in ({"b": None}, {"a": None}, {"o": None}, {"o": b}, {"b": inside(0), "o": inside(16)}, {"b": inside(16 * W), "o": inside(0)},
                {"n": out.nbytes - 1}, {"w": 0}, {"h": 0}, {"w": 70000}):
        assert ok(**bad) == capi.ERR_INVALID_ARGUMENT, bad
    for passes in (0, 6, 100):
        assert ok(p=capi.denoise_params(passes=passes)) == capi.ERR_INVALID_ARGUMENT
    assert b"passes" in lib.gmupt_last_error()
    for name in FIELDS[1:]:
        for v in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert ok(p=capi.denoise_params(**{name: v})) == capi.ERR_INVALID_ARGUMENT, (name, v)
            assert name.encode() in lib.gmupt_last_error()
    with pytest.raises(capi.GmuptError) as e:
        capi.denoise_host(beauty, aov, sigma_normal=-2.0)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.GmuptError):
        capi.denoise_host(beauty, aov[:, :4])
    # the device entries refuse a missing renderer before touching anything
    ms = C.c_float(5.0)
    assert lib.gmupt_denoise_image(None, b, a, W, H, C.byref(dp), o, out.nbytes, C.byref(ms)) == capi.ERR_INVALID_ARGUMENT
    assert ms.value == 0.0
    info = capi.TraceInfo(); info.redo_rays = 9
    assert lib.gmupt_render_denoised(None, 1, C.byref(dp), o, out.nbytes, C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert info.redo_rays == 0


def test_structured_aov_input(pkg):
    beauty, aov = random_inputs(20, 10, 8)
    rec = aov.reshape(-1, 16).view(pkg.capi.aov_dtype)[:, 0].reshape(10, 20)
    assert np.array_equal(pkg.capi.denoise_host(beauty, rec).view(np.uint32), pkg.capi.denoise_host(beauty, aov).view(np.uint32))


def test_cpp_driver_lists_denoise_and_refuses_ranks(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    exe = os.path.join(HOST, "gmupt_render")
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--denoise PREFIX" in out and "--aov-samples S" in out
    r = subprocess.run([exe, "--denoise", "/nonexistent/x", "--ranks", "2", "--rank", "0", "--no-gather"], capture_output=True, text=True)
    assert r.returncode != 0 and "--denoise" in r.stderr and "--ranks" in r.stderr

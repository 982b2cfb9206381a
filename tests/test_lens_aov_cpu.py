"""CPU tests of the lens-filtered AOV planes (include/gmupt_lens_aov.h): the host rule gmupt_aov_lens_ray against the numpy restatement
of lens_aov_util.py bit for bit, the two permutations of a pixel's rays, the focal-plane geometry in float64, and the surface -- header,
exports, bindings, build list, argument errors, and ProgressiveSession's lens_guides switch on stand-ins.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lens_aov_util as LA
import lens_util as LU

F = LU.F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOCUS = 13.0
APERTURES = (0.0, 0.3)
NEW_SYMBOLS = ["gmupt_render_aovs_lens", "gmupt_aov_lens_ray", "gmupt_render_denoised_lens"]


def pixels_of(W, H, seed):
    """The corners, a tile origin and a few dozen random pixels of a W x H frame."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([[0, W - 1, 0, W - 1, W // 3], rng.integers(0, W, 40)]).astype(np.uint32)
    y = np.concatenate([[0, 0, H - 1, H - 1, H // 3], rng.integers(0, H, 40)]).astype(np.uint32)
    return x, y


@pytest.fixture(scope="module")
def max_s(pkg):
    return int(pkg.capi.AOV_MAX_SAMPLES) if hasattr(pkg.capi, "AOV_MAX_SAMPLES") else 8


@pytest.fixture(scope="module")
def cases(pkg, oracle, max_s):
    """Per (pose, resolution, s, aperture): the camera buffer, the pixels, the host rays and the restatement, computed once."""
    out = []
    for pi, pose in enumerate(LU.POSES):
        for (W, H) in LU.RESOLUTIONS:
            cam = LU.camera(pkg.capi, W, H, pose, updates=1 + pi)
            cb = cam.buffer_copy()
            cam.close()
            x, y = pixels_of(W, H, 31 * pi + W)
            for s in (1, 2, 3, max_s):
                for aperture in APERTURES:
                    lens = LU.lens_struct(pkg.capi, aperture, FOCUS)
                    rays = pkg.capi.lens_aov.aov_lens_rays(cb, lens, x.tolist(), y.tolist(), s)
                    out.append(dict(pose=pose, size=(W, H), s=s, aperture=aperture, cb=cb, x=x, y=y, rays=rays,
                                    want=LA.rule(oracle, cb, aperture, FOCUS, x, y, s)))
    return out


def test_host_rule_equals_the_restatement(cases, max_s):
    assert max_s == 8 and len(cases) == 3 * 2 * 4 * 2
    for c in cases:
        rays, want = c["rays"], LA.rays_of(c["want"])
        tag = (c["pose"], c["size"], c["s"], c["aperture"])
        assert rays.shape == (c["x"].size, c["s"] ** 2, 8), tag
        assert np.array_equal(LU.bits(rays), LU.bits(want)), tag
        assert np.isfinite(rays[..., :3]).all() and np.isfinite(rays[..., 4:7]).all() and np.all(rays[..., 3] == np.finfo(F).max)
        if c["aperture"] == 0.0:
            assert np.array_equal(rays[..., 0:3], np.broadcast_to(np.array(list(c["cb"].position)[:3], F), rays[..., 0:3].shape)), tag
        elif c["s"] > 1:
            assert (np.abs(c["want"]["lx"]) + np.abs(c["want"]["ly"]) > 0).all(), "no stratum centre is the lens centre"


def test_pixel_cells_are_the_aov_rays_cells(pkg, cases):
    """Step 1 against the shipped host function: the pixel coordinates of ray k are those of gmupt_aov_ray's ray k + 1 (s > 1) or of its
    only ray (s = 1), so the pinhole direction d of the restatement is that ray's direction bit for bit."""
    for c in cases:
        if c["aperture"] != APERTURES[0]:
            continue
        s = c["s"]
        ref = pkg.capi.aov_rays(c["cb"], c["x"][:9].tolist(), c["y"][:9].tolist(), s)
        ref = ref[:, 1:] if s > 1 else ref
        assert np.array_equal(LU.bits(ref[..., 4:7]), LU.bits(c["want"]["d"][:9])), (c["pose"], c["size"], s)


def test_cells_and_strata_are_permutations(max_s):
    """For every s the pixel cells (a, b) and the lens strata (a2, b2) of a pixel's R rays are each a permutation of the s*s cells, and
    the map between them is the one the header states."""
    for s in range(1, max_s + 1):
        a, b, a2, b2 = LA.cells(s)
        every = set((i, j) for i in range(s) for j in range(s))
        assert set(zip(a.tolist(), b.tolist())) == every and set(zip(a2.tolist(), b2.tolist())) == every, s
        assert len(a) == s * s and np.array_equal(a2, b) and np.array_equal(b2, s - 1 - a)


def test_strata_of_the_host_rays(pkg, cases):
    """The same from the host function's rays alone: the lens offsets of a pixel's rays, recovered from the origins, are the s*s stratum
    centres (radius a * sqrt((i + 1/2) / s), angle 2 pi (j + 1/2) / s), each exactly once and the same set in every pixel."""
    for c in cases:
        s, a = c["s"], c["aperture"]
        if a == 0.0:
            continue
        pos, _, hor, ver = (v.astype(np.float64) for v in LU.cam_vectors(c["cb"]))
        right, up = hor / np.linalg.norm(hor), ver / np.linalg.norm(ver)
        off = c["rays"][..., 0:3].astype(np.float64) - pos
        lx, ly = off @ right, off @ up
        want = sorted((round(a * np.sqrt((i + 0.5) / s) * np.cos(2 * np.pi * (j + 0.5) / s), 4), round(a * np.sqrt((i + 0.5) / s) * np.sin(2 * np.pi * (j + 0.5) / s), 4))
                      for i in range(s) for j in range(s))
        for p in range(0, lx.shape[0], 11):
            got = sorted((round(float(u), 4), round(float(v), 4)) for u, v in zip(lx[p], ly[p]))
            assert np.abs(np.array(got) - np.array(want)).max() <= 2e-4, (c["pose"], c["size"], s, p)


def test_every_ray_meets_its_pinhole_ray_on_the_focal_plane(cases):
    """In float64, from the stored float32 rays alone: the point of ray (origin, direction) on the plane dot(X - pos, fn) = focus must be
    Pf = pos + d * focus / dot(d, fn), the point of the pinhole ray through the ray's pixel coordinate on that plane.

    The bound is test_lens_cpu.py's, for the same cameras, focus and statements (steps 3-5 are the lens rule's): the pixel coordinate
    of a stratified ray lies within one pixel of the pixel's own, as the jitter there, so dot(d, fn) >= 0.6, |Pf - pos| < 22 and the
    obliquity 1 / dot(direction, fn) <= 1.7 hold again; with S = 32: Pf32 within 12 eps S, the origin 4 eps S, the direction
    (13 + 5) eps S across the ray and 1.7 times that along the plane, the origin's share twice: < 39 eps S = 19.5 * 2^-23 * S.  The
    bound asserted is 20 * 2^-23 * S."""
    S = 32.0
    bound = 20 * 2.0 ** -23 * S
    worst = 0.0
    for c in cases:
        cb, want = c["cb"], c["want"]
        pos = np.array(list(cb.position)[:3], np.float64)
        assert np.abs(pos).max() <= 8.0
        fn = want["fn"].astype(np.float64)
        d = want["d"].astype(np.float64)
        Pf = pos + d * (FOCUS / (d @ fn))[..., None]
        assert (d @ fn).min() >= 0.6 and np.linalg.norm(Pf - pos, axis=-1).max() < 22.0
        o = c["rays"][..., 0:3].astype(np.float64)
        w = c["rays"][..., 4:7].astype(np.float64)
        assert ((w @ fn) >= 1 / 1.7).all()
        t = (FOCUS - (o - pos) @ fn) / (w @ fn)
        X = o + w * t[..., None]
        err = np.abs(X - Pf).max()
        worst = max(worst, err)
        assert err <= bound, (c["pose"], c["size"], c["s"], c["aperture"], err, bound)
        assert np.abs((o - pos) @ fn).max() <= 8 * 2.0 ** -23 * S, "the origins lie in the lens plane through pos"
    print("focal plane: worst |X - Pf| = %.3g, bound %.3g" % (worst, bound))


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt_lens_aov.h")).read()
    lens_header = open(os.path.join(ROOT, "include", "gmupt_lens.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    assert "gmupt_lens_aov.h" in lens_header and "follow-up" not in lens_header
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.lens_aov.SYMBOLS and name not in pkg.capi.SYMBOLS and getattr(lib, name, None) is not None, name
    assert not hasattr(pkg.capi.Renderer, "aovs_lens")
    for words in ("(a2, b2) = (b, s - 1 - a)", "6.2831853f", "NOT promised", "surface pixel exactly when", "What stays a pinhole", "coverage == 0"):
        assert words in header, words
    sources = open(os.path.join(ROOT, "gmu-path-tracer_amd", "build.py")).read()
    for f in ("csrc/pt_lens_aov.hip", "csrc/pt_lens_aov.cpp", "csrc/gmupt_capi_lens_aov.hip", "csrc/pt_lens_aov.hpp", "../include/gmupt_lens_aov.h"):
        assert '"%s"' % f in sources, f
    run_sh = open(os.path.join(ROOT, "tools", "sanitize", "run.sh")).read()
    assert "pt_lens_aov.cpp" in run_sh


def test_argument_errors_leave_the_outputs_untouched(pkg):
    capi = pkg.capi
    lib = capi.lib()
    cam = LU.camera(capi, 32, 18, LU.POSES[0])
    cb = cam.buffer_copy()
    cam.close()
    ray = capi.Ray()
    C.memset(C.byref(ray), 0xAB, C.sizeof(ray))
    was = bytes(ray)
    nan, inf = float("nan"), float("inf")
    fn = lib.gmupt_aov_lens_ray
    for a, f in [(nan, 1.0), (inf, 1.0), (-inf, 1.0), (-1e-30, 1.0), (0.1, nan), (0.1, inf), (0.1, 0.0), (0.1, -2.0)]:
        l = LU.lens_struct(capi, a, f)
        assert fn(C.byref(cb), C.byref(l), 0, 0, 1, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, (a, f)
        assert b"gmupt_aov_lens_ray" in lib.gmupt_last_error() and bytes(ray) == was
    ok = LU.lens_struct(capi, 0.1, 2.0)
    for args in [(None, C.byref(ok), 0, 0, 1, 0, C.byref(ray)), (C.byref(cb), None, 0, 0, 1, 0, C.byref(ray)), (C.byref(cb), C.byref(ok), 0, 0, 1, 0, None)]:
        assert fn(*args) == capi.ERR_INVALID_ARGUMENT
    for s, k in [(0, 0), (9, 0), (1, 1), (2, 4), (8, 64)]:                       # samples outside 1..8, k >= s*s (no centre ray: s = 2 has 4 rays)
        assert fn(C.byref(cb), C.byref(ok), 0, 0, s, k, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, (s, k)
    assert bytes(ray) == was
    assert fn(C.byref(cb), C.byref(ok), 0, 0, 2, 3, C.byref(ray)) == 0 and fn(C.byref(cb), C.byref(ok), 31, 17, 8, 63, C.byref(ray)) == 0
    # aperture 0 is accepted whatever the focus says
    assert fn(C.byref(cb), C.byref(LU.lens_struct(capi, 0.0, 2.0)), 3, 1, 1, 0, C.byref(ray)) == 0 and list(ray.origin) == list(cb.position)[:3]
    # the renderer's entry points refuse a missing handle before any device is touched, and write nothing
    out = np.full(16, 7.0, np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert lib.gmupt_render_aovs_lens(None, C.byref(ok), 1, ptr, out.nbytes, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_denoised_lens(None, C.byref(ok), 1, None, ptr, out.nbytes, None) == capi.ERR_INVALID_ARGUMENT
    assert b"gmupt_render_denoised_lens" in lib.gmupt_last_error() and (out == 7.0).all()


class _Camera:
    class _Buffer:
        lightCount = 2
        iterationCounter = 5

    def __init__(self):
        self.buffer = self._Buffer()


class _Image:
    def __init__(self, tag):
        self.tag = tag

    def cpu(self):
        return self

    def numpy(self):
        return self.tag


class _Renderer:
    def __init__(self):
        self.calls = []

    def denoise(self, aov_samples=1, **params):
        self.calls.append(("pinhole", aov_samples, params))
        return _Image("pinhole")

    def denoise_temporal(self, handle, aov_samples=1, **params):
        self.calls.append(("pinhole temporal", aov_samples, params))
        return _Image("pinhole temporal")


def test_session_lens_guides_take_the_lens_path_only_with_a_lens(pkg, monkeypatch):
    """On stand-ins: denoised(lens_guides=True) and denoised_temporal(lens_guides=True) go through capi.lens_aov only while the renderer
    has a lens attached; without one, and by default, they are today's calls."""
    capi = pkg.capi
    attached = [capi.lens.lens_params()]                                          # aperture 0: none attached
    calls = []
    monkeypatch.setattr(capi.lens, "get_lens", lambda r: attached[0])
    monkeypatch.setattr(capi.lens_aov, "denoise", lambda r, aov_samples=1, lens=None, **params: calls.append(("lens", aov_samples, params)) or _Image("lens"))
    monkeypatch.setattr(capi.lens_aov, "guided_inputs", lambda r, aov_samples=1, lens=None: calls.append(("inputs", aov_samples)) or ("beauty", "records"))
    monkeypatch.setattr(capi, "temporal_denoise_image", lambda handle, beauty, aov, cb, new, origin=(0, 0), infill=None, **params:
                        calls.append(("temporal", beauty, aov, bool(new), origin, infill, params)) or _Image("lens temporal"))
    r, cam = _Renderer(), _Camera()
    s = pkg.progressive.ProgressiveSession(r, cam, 8, 8, preview_every=0)
    s.temporal = object()
    assert s.denoised(2, passes=3) == "pinhole" and s.denoised(2, lens_guides=True, passes=3) == "pinhole"
    assert s.denoised_temporal(2, lens_guides=True) == "pinhole temporal"
    assert calls == [] and [c[0] for c in r.calls] == ["pinhole", "pinhole", "pinhole temporal"]
    attached[0] = capi.lens.lens_params(aperture_radius=0.25, focus_distance=4.0)
    assert s.denoised(2, passes=3) == "pinhole" and calls == []                  # the default stays as it was
    assert s.denoised(2, lens_guides=True, passes=3) == "lens" and calls == [("lens", 2, {"passes": 3})]
    del calls[:]
    assert s.denoised_temporal(3, lens_guides=True, history_cap=8) == "lens temporal"
    assert s.denoised_temporal(3, lens_guides=True) == "lens temporal"
    assert calls == [("inputs", 3), ("temporal", "beauty", "records", True, (0, 0), None, {"history_cap": 8}),
                     ("inputs", 3), ("temporal", "beauty", "records", False, (0, 0), None, {})], "the history folds on the first call only"
    assert len(r.calls) == 4

"""CPU tests of the camera projections (include/gmupt_projection.h): the host rules against the numpy restatement of
projection_util.py bit for bit, the geometry in float64, the round trip through the inverse, the jitter against the pinhole's, the
argument checks, the layout and the session on stand-ins.  No device (the lens x projection refusal needs a renderer:
tests/test_projection_gpu.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lens_util as LU
import projection_util as PU

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_projection_default_params", "gmupt_renderer_set_projection", "gmupt_renderer_get_projection", "gmupt_projection_ray_host",
               "gmupt_projection_pick_ray", "gmupt_projection_project_host", "gmupt_pick_projected", "gmupt_aov_projected_ray",
               "gmupt_render_aovs_projected", "gmupt_render_denoised_projected", "gmupt_debug_read_aov_rays"]


def samples(W, H, seed):
    """A few hundred (q, cx, cy): random ones, the corners of the frame, tile-origin pixels paired with q = 0, the largest q of a 2^21 pool."""
    rng = np.random.default_rng(seed)
    n = 300
    q = rng.integers(0, 1 << 21, n).astype(np.uint32)
    cx = rng.integers(0, W, n).astype(np.uint32)
    cy = rng.integers(0, H, n).astype(np.uint32)
    e = np.array([(0, 0, 0), (0, W - 1, 0), (0, 0, H - 1), (1, W - 1, H - 1), ((1 << 21) - 1, W - 1, H - 1), ((1 << 21) - 1, 0, 0),
                  (0, W // 3, H // 3), (255, W // 2, H // 2), (256, W // 3 + 1, H // 3), (257, W // 2, H - 1)], np.uint32)
    return np.concatenate([q, e[:, 0]]), np.concatenate([cx, e[:, 1]]), np.concatenate([cy, e[:, 2]])


@pytest.fixture(scope="module")
def cameras(pkg):
    """(pose, (W, H), camera buffer) for three poses at two resolutions, another randomSeed per pose."""
    out = []
    for pi, pose in enumerate(LU.POSES):
        for (W, H) in PU.RESOLUTIONS:
            cam = LU.camera(pkg.capi, W, H, pose, updates=1 + pi)
            out.append((pose, (W, H), cam.buffer_copy()))
            cam.close()
    return out


def test_host_rules_equal_the_restatement(pkg, oracle, cameras):
    P = pkg.capi.projection
    projs = PU.projections(pkg.capi)
    outside = 0
    for pose, (W, H), cb in cameras:
        q, cx, cy = samples(W, H, 17 * W + H)
        assert int(q.max()) == (1 << 21) - 1
        px = np.concatenate([cx.astype(F) + F(0.25), F([0, W, W / 2, 0.5])])
        py = np.concatenate([cy.astype(F) - F(0.5), F([0, H, H / 2, H - 0.5])])
        xs, ys = cx[::5], cy[::5]
        for name, proj in projs.items():
            got = P.projection_rays_host(cb, proj, q, cx, cy)
            want = PU.words(*PU.rule_fresh(oracle, cb, proj, q, cx, cy))
            assert np.array_equal(LU.bits(got), LU.bits(want)), (pose, W, H, name, "fresh")
            got = P.pick_rays(cb, proj, px, py)
            want = PU.words(*PU.rule_pixel(oracle, cb, proj, px, py))
            assert np.array_equal(LU.bits(got), LU.bits(want)), (pose, W, H, name, "pick")
            for s in (1, 2, 3):
                got = P.aov_projected_rays(cb, proj, xs, ys, s)
                want = PU.words(*PU.rule_aov(oracle, cb, proj, xs, ys, s))
                assert got.shape == (len(xs), s * s, 8) and np.array_equal(LU.bits(got), LU.bits(want)), (pose, W, H, name, "aov", s)
            if name.startswith("fisheye"):
                outside += int((np.abs(want[..., 4:7]).max(axis=-1) == 0).sum())
        # the pinhole kind is gmupt_camera_pick_ray
        for i in range(0, px.size, 9):
            a, b = P.pick_ray(cb, projs["pinhole"], px[i], py[i]), pkg.capi.camera_pick_ray(cb, float(px[i]), float(py[i]))
            assert bytes(a) == bytes(b)
    assert outside > 0, "some fisheye rays lie outside the image circle"


def test_geometry_in_float64(pkg, cameras):
    P = pkg.capi.projection
    projs = PU.projections(pkg.capi)
    tol = 4e-6      # a unit vector built from ~10 binary32 operations on terms <= 1, and pi as binary32 (error 8.7e-8 rad): < 32 * 2^-23
    for pose, (W, H), cb in cameras:
        pos, right, up, fn = PU.frame64(cb)
        d = lambda proj, px, py: np.array(P.pick_ray(cb, proj, px, py).direction[:], np.float64)
        o = lambda proj, px, py: np.array(P.pick_ray(cb, proj, px, py).origin[:], np.float64)
        eq = projs["equirect"]
        assert np.abs(d(eq, W / 2, H / 2) - fn).max() < tol, "the centre looks along fn"
        for py in (0.5, H / 2, H - 1):
            row = np.cos((1 - 2 * py / H) * math.pi / 2)     # the edge columns look along -fn in the row's latitude
            for px in (0.0, float(W)):
                got = d(eq, px, py)
                assert abs(got @ fn + row) < tol and abs(got @ right) < tol, (px, py)
        for px in (0.0, W / 3, W - 1.0):
            assert np.abs(d(eq, px, 0.0) - up).max() < tol, "the top row looks along up"
        # fisheye: r = 1 on the shorter side's edge
        m = min(W, H)
        rim = [(W / 2 + m / 2, H / 2), (W / 2 - m / 2, H / 2), (W / 2, H / 2 + m / 2), (W / 2, H / 2 - m / 2)]
        for px, py in rim:
            v = d(projs["fisheye180"], px, py)
            assert abs(v @ fn) < tol and abs(np.linalg.norm(v) - 1) < tol, "fov pi: r = 1 is perpendicular to fn"
            assert np.abs(d(projs["fisheye360"], px, py) + fn).max() < tol, "fov 2 pi: r = 1 is -fn"
        assert np.abs(d(projs["fisheye180"], W / 2, H / 2) - fn).max() < tol
        corners = [(0.0, 0.0), (float(W), 0.0), (0.0, float(H)), (float(W), float(H)), (W / 2 + m / 2 + 1, H / 2)]
        for px, py in corners:     # r > 1: exactly zero
            assert bytes(np.array(P.pick_ray(cb, projs["fisheye180"], px, py).direction[:], F)) == bytes(np.zeros(3, F))
        # orthographic
        orth = projs["ortho"]
        E = 6.0
        for px, py in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W / 2, H / 2)]:
            assert np.abs(d(orth, px, py) - fn).max() < 2e-7
        c00, c10, c01 = o(orth, 0, 0), o(orth, W, 0), o(orth, 0, H)
        assert abs((c10 - c00) @ right - E * W / H) < 1e-5 and abs((c00 - c01) @ up - E) < 1e-5, "the frame spans extent * W/H by extent"
        p00, p11 = o(orth, 0, 0), o(orth, W - 1, H - 1)      # the corner pixels' own rays: one pixel less (a pixel's ray is its upper left)
        assert abs((p11 - p00) @ right - E * W / H * (W - 1) / W) < 1e-5 and abs((p00 - p11) @ up - E * (H - 1) / H) < 1e-5
        assert np.abs(o(orth, W / 2, H / 2) - pos).max() < 1e-5


def test_round_trip_through_the_inverse(pkg, oracle, cameras):
    """project_host(origin + direction * t) is the pixel the ray came from, within 1e-3 px (the bound the temporal projection's round
    trip holds the library to).  Left out: points within 1 degree of an equirect pole and fisheye points with r < 1e-3 -- none of the
    samples is one (pixel centres of every row and column at 64x36 and 48x64, asserted), so the excluded share is 0.  The same round trip
    of the float64 restatement of the forward rule is printed next to it."""
    P = pkg.capi.projection
    projs = PU.projections(pkg.capi)
    worst = {}
    for pose, (W, H), cb in cameras:
        ys, xs = np.mgrid[0:H, 0:W]
        px, py = xs.ravel().astype(np.float64) + 0.5, ys.ravel().astype(np.float64) + 0.5
        lat = np.abs(1 - 2 * py / H) * 90.0
        m = min(W, H)
        r = np.hypot((2 * px / W - 1) * W / m, (1 - 2 * py / H) * H / m)
        assert (lat > 89.0).sum() == 0 and (r < 1e-3).sum() == 0, "the excluded share is 0"
        for name in ("ortho", "fisheye180", "fisheye360", "fisheye120", "equirect", "pinhole"):
            proj = projs[name]
            rays = P.pick_rays(cb, proj, px, py)
            inside = np.abs(rays[:, 4:7]).max(axis=1) > 0
            if name.startswith("fisheye"):
                assert np.array_equal(inside[np.abs(r - 1) > 1e-5], (r <= 1)[np.abs(r - 1) > 1e-5]) and (~inside).any()
            else:
                assert inside.all()
            o64, d64 = PU.forward64(cb, proj, px, py)
            err = err64 = 0.0
            for i in np.flatnonzero(inside):
                for t in (0.5, 7.0):
                    back = P.project_host(cb, proj, rays[i, 0:3].astype(np.float64) + rays[i, 4:7].astype(np.float64) * t)
                    assert back is not None, (name, i)
                    err = max(err, abs(back[0] - px[i]), abs(back[1] - py[i]))
                    w = (o64[i] + d64[i] / np.linalg.norm(d64[i]) * t).astype(F)     # the inverse takes binary32 points
                    back = P.project_host(cb, proj, w)
                    assert back is not None or abs(r[i] - 1) < 1e-6, (name, i)      # on the rim the rounding of w decides
                    if back is not None:
                        err64 = max(err64, abs(back[0] - px[i]), abs(back[1] - py[i]))
            worst[name] = max(worst.get(name, (0, 0))[0], err), max(worst.get(name, (0, 0))[1], err64)
    for name, (e32, e64) in worst.items():
        print("round trip %-10s: binary32 rule %.3g px, float64 restatement %.3g px" % (name, e32, e64))
    for name, (e32, e64) in worst.items():
        assert e32 <= 1e-3, (name, e32, e64)
    # not on the image
    _, _, cb = cameras[0]
    pos, right, up, fn = PU.frame64(cb)
    behind = pos - fn * 3 + right * 0.1
    assert P.project_host(cb, projs["ortho"], behind) is None and P.project_host(cb, projs["fisheye180"], behind) is None
    assert P.project_host(cb, projs["pinhole"], behind) is None and P.project_host(cb, projs["fisheye120"], pos + right) is None
    assert P.project_host(cb, projs["fisheye360"], behind) is not None and P.project_host(cb, projs["equirect"], behind) is not None
    assert P.project_host(cb, projs["equirect"], pos) is None


def test_jitter_is_the_pinholes(pkg, oracle):
    """Over 2^16 consecutive q in one pixel the jittered (u, v) are the pinhole's two draws: the orthographic origin, which is affine in
    (u, v), recovers them, and they must be those of the restated stage_new_path -- whose ray through the same draws is
    gmupt_camera_pick_ray's, bit for bit -- with its mean and range."""
    P = pkg.capi.projection
    N, W, H, cx, cy = 1 << 16, 64, 36, 21, 13
    cam = LU.camera(pkg.capi, W, H, LU.POSES[1], updates=3)
    cb = cam.buffer_copy()
    cam.close()
    q = np.arange(N, dtype=np.uint32)
    cxs, cys = np.full(N, cx, np.uint32), np.full(N, cy, np.uint32)
    u, v, jx, jy = PU.jittered_uv(oracle, cb, q, cxs, cys)
    pin = P.projection_rays_host(cb, P.projection_params(P.PINHOLE), q, cxs, cys)
    for i in range(0, N, 997):
        want = pkg.capi.camera_pick_ray(cb, float(F(F(cx) + jx[i])), float(F(F(cy) + jy[i])))
        assert bytes(np.frombuffer(want, F)) == bytes(pin[i])
    E = 6.0
    rays = P.projection_rays_host(cb, P.orthographic(E), q, cxs, cys)
    pos, right, up, fn = PU.frame64(cb)
    off = rays[:, 0:3].astype(np.float64) - pos
    u_got = ((off @ right) / (E / 2 * W / H) + 1) / 2
    v_got = (1 - (off @ up) / (E / 2)) / 2
    assert np.abs(u_got - u).max() < 1e-5 and np.abs(v_got - v).max() < 1e-5
    assert jx.min() >= -1 and jx.max() < 1 and jy.min() >= -1 and jy.max() < 1
    s = 2 / math.sqrt(12 * N)     # the mean of N uniform draws of [-1, 1): sigma
    print("jitter: mean %.4g %.4g (5 sigma %.4g), range [%.4f, %.4f] [%.4f, %.4f]" % (jx.mean(), jy.mean(), 5 * s, jx.min(), jx.max(), jy.min(), jy.max()))
    assert abs(jx.mean()) < 5 * s and abs(jy.mean()) < 5 * s and jx.max() - jx.min() > 1.99 and jy.max() - jy.min() > 1.99


def test_layout_symbols_and_argument_checks(pkg, cameras):
    capi = pkg.capi
    P = capi.projection
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "gmupt_projection.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in P.SYMBOLS and name not in capi.SYMBOLS and getattr(lib, name, None) is not None, name
    sources = open(os.path.join(ROOT, "gmu-path-tracer_amd", "build.py")).read()
    for src in ("csrc/pt_projection.hip", "csrc/pt_projection.cpp", "csrc/gmupt_capi_projection.hip", "csrc/pt_projection.hpp", "../include/gmupt_projection.h"):
        assert '"%s"' % src in sources, src
    for shipped in ("pt_kernels.hip", "pt_shading.hpp", "pt_device.hpp", "pt_kernel_util.hpp", "pt_traverse_wide.hip", "pt_lens.hip", "pt_lens_aov.hip"):
        assert "pt_projection" not in open(os.path.join(ROOT, "gmu-path-tracer_amd", "csrc", shipped)).read(), shipped
    for words in ("do not combine", "GMUPT_ERR_UNSUPPORTED"):
        assert words in header and words in open(os.path.join(ROOT, "include", "gmupt_lens.h")).read()
    S = P.Projection
    assert C.sizeof(S) == 16 and (S.kind.offset, S.fov.offset, S.extent.offset, S.pad.offset) == (0, 4, 8, 12)
    d = P.projection_params()
    assert (d.kind, d.fov, d.extent, d.pad) == (P.PINHOLE, F(3.14159274), 1.0, 0)
    assert (P.PINHOLE, P.ORTHOGRAPHIC, P.FISHEYE, P.EQUIRECT) == (0, 1, 2, 3)
    with pytest.raises(TypeError):
        P.projection_params(squeeze=2.0)
    _, (W, H), cb = cameras[0]
    ray = capi.Ray()
    C.memset(C.byref(ray), 0xAB, C.sizeof(ray))
    was = bytes(ray)
    px, py, on = C.c_double(-7.0), C.c_double(-7.0), C.c_int(5)
    world = (C.c_float * 3)(0, 0, 0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(kind=4), dict(kind=0xFFFFFFFF)]
    bad += [dict(kind=P.FISHEYE, fov=x) for x in (nan, inf, -inf, 0.0, -1.0, 6.2831860)]
    bad += [dict(kind=P.ORTHOGRAPHIC, extent=x) for x in (nan, inf, 0.0, -0.0, -2.0)]
    for kw in bad:
        p = P.projection_params(**kw)
        assert lib.gmupt_projection_ray_host(C.byref(cb), C.byref(p), 0, 0, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, kw
        assert b"gmupt_projection_ray_host" in lib.gmupt_last_error()
        assert lib.gmupt_projection_pick_ray(C.byref(cb), C.byref(p), 1.0, 1.0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, kw
        assert lib.gmupt_aov_projected_ray(C.byref(cb), C.byref(p), 0, 0, 1, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, kw
        assert lib.gmupt_projection_project_host(C.byref(cb), C.byref(p), world, C.byref(px), C.byref(py), C.byref(on)) == capi.ERR_INVALID_ARGUMENT, kw
    # each check applies only to the kind that uses the field
    for kw in (dict(kind=P.FISHEYE, fov=1.0, extent=nan), dict(kind=P.ORTHOGRAPHIC, extent=2.0, fov=nan), dict(kind=P.EQUIRECT, fov=-1.0, extent=-1.0),
               dict(kind=P.PINHOLE, fov=nan, extent=nan), dict(kind=P.FISHEYE, fov=float(F(6.28318548)))):
        p = P.projection_params(**kw)
        assert lib.gmupt_projection_ray_host(C.byref(cb), C.byref(p), 0, 0, 0, C.byref(capi.Ray())) == 0, kw
    ok = P.fisheye(180.0)
    for args in [(None, C.byref(ok), 0, 0, 0, C.byref(ray)), (C.byref(cb), None, 0, 0, 0, C.byref(ray)), (C.byref(cb), C.byref(ok), 0, 0, 0, None)]:
        assert lib.gmupt_projection_ray_host(*args) == capi.ERR_INVALID_ARGUMENT
    for args in [(None, C.byref(ok), 0.0, 0.0, C.byref(ray)), (C.byref(cb), None, 0.0, 0.0, C.byref(ray)), (C.byref(cb), C.byref(ok), 0.0, 0.0, None)]:
        assert lib.gmupt_projection_pick_ray(*args) == capi.ERR_INVALID_ARGUMENT
    for s, k in [(0, 0), (capi.AOV_MAX_SAMPLES + 1, 0), (2, 4), (1, 1)]:
        assert lib.gmupt_aov_projected_ray(C.byref(cb), C.byref(ok), 0, 0, s, k, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, (s, k)
    assert lib.gmupt_aov_projected_ray(None, C.byref(ok), 0, 0, 1, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_projection_project_host(C.byref(cb), C.byref(ok), None, C.byref(px), C.byref(py), C.byref(on)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_projection_project_host(C.byref(cb), C.byref(ok), world, None, C.byref(py), C.byref(on)) == capi.ERR_INVALID_ARGUMENT
    assert bytes(ray) == was and (px.value, py.value, on.value) == (-7.0, -7.0, 5), "no error path writes an output"
    # the renderer's entry points refuse a missing handle before any device is touched
    assert lib.gmupt_renderer_set_projection(None, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_renderer_get_projection(None, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_pick_projected(None, 0.0, 0.0, 0, C.byref(ray), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_aovs_projected(None, C.byref(ok), 1, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_denoised_projected(None, C.byref(ok), 1, None, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    lib.gmupt_projection_default_params(None)


class _Camera:
    class _Buffer:
        lightCount = 2
        iterationCounter = 5

    def __init__(self):
        self.buffer, self.resets = self._Buffer(), 0

    def reset_accumulation(self):
        self.resets += 1


class _Resettable:
    resets = 0

    def reset(self):
        self.resets += 1

    def close(self):
        pass


def test_session_set_projection_on_stand_ins(pkg, monkeypatch):
    """The projection reaches the renderer through capi.projection, the accumulation, the monitor and the history restart, and what
    inverts a pinhole refuses while it is attached; set_lens with nothing attached is what it was."""
    P, L = pkg.capi.projection, pkg.capi.lens
    calls = []
    monkeypatch.setattr(P, "set_projection", lambda r, proj: calls.append(("proj", proj.kind, proj.fov, proj.extent)))
    monkeypatch.setattr(L, "set_lens", lambda r, lens: calls.append(("lens", lens.aperture_radius, lens.focus_distance)))
    monkeypatch.setattr(P, "pick", lambda r, px, py, lights: calls.append(("pick", px, py, lights)) or (pkg.capi.Ray(), pkg.capi.Hit()))
    renderer, cam = object(), _Camera()
    s = pkg.progressive.ProgressiveSession(renderer, cam, 8, 8, preview_every=0)
    s.converge, s.temporal = _Resettable(), _Resettable()
    s.set_lens(0.25, focus=4.0)
    assert calls == [("lens", 0.25, 4.0)] and cam.resets == 1
    s.set_lens(0.0)
    proj = s.set_projection("fisheye", fov=2.0)
    assert (proj.kind, proj.fov) == (P.FISHEYE, 2.0) and calls[-1] == ("proj", P.FISHEYE, 2.0, 1.0)
    assert cam.resets == 3 and s.converge.resets == 3 and s.temporal.resets == 1
    s.pick(3, 4)
    assert calls[-1] == ("pick", 3, 4, 2)
    n = len(calls)
    for refused in (lambda: s.denoised_temporal(), lambda: s.set_lens(0.25, focus=4.0), lambda: s.set_vertices(None, None, keep_history=True),
                    lambda: s.set_pose(None, None, None, keep_history=True)):
        with pytest.raises(ValueError, match="projection"):
            refused()
    assert len(calls) == n and cam.resets == 3
    s.set_lens(0.0)                      # no aperture: allowed
    assert calls[-1] == ("lens", 0.0, 1.0)
    assert s.set_projection("ortho", extent=3.0).extent == 3.0 and s.set_projection("equirect").kind == P.EQUIRECT
    assert s.set_projection(None) is None and calls[-1][:2] == ("proj", P.PINHOLE) and s.projection is None
    s.set_lens(0.25, focus=4.0)
    assert calls[-1] == ("lens", 0.25, 4.0)

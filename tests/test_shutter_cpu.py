"""CPU tests of the shutter (include/gmupt_shutter.h): the host rules gmupt_shutter_ray_host, _camera_host and _time_host against the
numpy restatement of shutter_util.py bit for bit, their composition with the lens's and the projection's host rules, the identity, the
statistics of the time draw, and the surface (sizes, errors, the binding's round trips).  No device."""
import ctypes as C

import numpy as np
import pytest

import lens_util as LU
import projection_util as PU
import shutter_util as SU

F = LU.F
APERTURE, FOCUS = 0.3, 13.0


def rules(capi):
    """name -> (lens, projection): the pinhole, a lens, every projection kind."""
    P = capi.projection
    out = {"pinhole": (None, None), "lens": (LU.lens_struct(capi, APERTURE, FOCUS), None)}
    out.update({name: (None, p) for name, p in (("ortho", P.orthographic(6.0)), ("fisheye", P.fisheye(180.0)), ("equirect", P.equirect()))})
    return out


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    """Per (pose pair, resolution, rule): the camera, the shutter, the samples, the host rays and times, and the restatement; once."""
    capi = pkg.capi
    out = []
    for pi, name in enumerate(sorted(SU.POSE_PAIRS)):
        for (W, H) in SU.RESOLUTIONS:
            cb, sh = SU.pair(capi, W, H, name, updates=1 + pi)
            q, cx, cy = SU.samples(W, H)
            times = capi.shutter.times_host(cb, q)
            for rname, (lens, proj) in rules(capi).items():
                rays = capi.shutter.rays_host(cb, sh, q, cx, cy, lens=lens, projection=proj)
                want, ts = SU.rule(oracle, cb, sh, q, cx, cy, lens=lens, proj=proj)
                out.append(dict(pair=name, size=(W, H), rule=rname, lens=lens, proj=proj, cb=cb, sh=sh, q=q, cx=cx, cy=cy, rays=rays, times=times, want=want, ts=ts))
    return out


def test_host_rule_equals_the_restatement(pkg, cases):
    assert len(cases) == 3 * 2 * 5
    moved = 0
    for c in cases:
        tag = (c["pair"], c["size"], c["rule"])
        assert sorted(set(int(x) for x in c["q"])) == SU.QS
        assert np.array_equal(LU.bits(c["times"]), LU.bits(c["ts"])), tag
        assert np.all(c["times"] >= 0) and np.all(c["times"] < 1)
        assert np.array_equal(LU.bits(c["rays"]), LU.bits(c["want"])), tag
        assert np.all(c["rays"][:, 3] == np.finfo(F).max) and not LU.bits(c["rays"][:, 7]).any()
        # and the camera at the path's time, word for word (everything but the twelve components is the open camera's)
        for i in range(0, c["q"].size, 5):
            got = pkg.capi.shutter.camera_host(c["cb"], c["sh"], float(c["times"][i]))
            assert bytes(got) == bytes(SU.camera_at(c["cb"], c["sh"], c["times"][i])), tag
        if c["rule"] == "pinhole":
            moved += int((np.abs(c["rays"][:, 0:3] - np.array(list(c["cb"].position)[:3], F)).max(axis=1) > 0).sum()) if c["pair"] != "yaw3" else 0
    assert moved > 0, "a translating shutter moves the origins"


def test_composition_with_the_lens_and_projection_rules(pkg, cases):
    """ray_host(cam, sh, rule, q, ..) is the rule's own host function on camera_host(cam, sh, time_host(cam, q)), bit for bit; the
    pinhole is gmupt_camera_pick_ray's arithmetic on the jittered coordinates of that camera."""
    capi = pkg.capi
    for c in cases:
        tag = (c["pair"], c["size"], c["rule"])
        for i in range(c["q"].size):
            q, cx, cy = int(c["q"][i]), int(c["cx"][i]), int(c["cy"][i])
            cam_t = capi.shutter.camera_host(c["cb"], c["sh"], capi.shutter.time_host(c["cb"], q))
            if c["lens"] is not None:
                want = LU.ray_words(capi.lens.lens_ray_host(cam_t, c["lens"], q, cx, cy))
            elif c["proj"] is not None:
                want = LU.ray_words(capi.projection.projection_ray_host(cam_t, c["proj"], q, cx, cy))
            else:
                jx, jy = (float(v[0]) for v in _jitter(pkg, c, i))
                ray = capi.camera_pick_ray(cam_t, float(F(F(cx) + F(jx))), float(F(F(cy) + F(jy))))
                want = LU.ray_words(ray)
                assert list(want[0:3]) == list(cam_t.position)[:3]
            assert np.array_equal(LU.bits(want[[0, 1, 2, 4, 5, 6]]), LU.bits(c["rays"][i][[0, 1, 2, 4, 5, 6]])), (tag, q, cx, cy)


def _jitter(pkg, c, i):
    import oracle_lib
    _, _, jx, jy = PU.jittered_uv(oracle_lib, c["cb"], c["q"][i:i + 1], c["cx"][i:i + 1], c["cy"][i:i + 1])
    return jx, jy


def test_both_a_lens_and_a_projection_is_refused(pkg, cases):
    capi, c = pkg.capi, cases[0]
    ray = capi.Ray()
    C.memset(C.byref(ray), 0xAB, C.sizeof(ray))
    was = bytes(ray)
    lens, proj = LU.lens_struct(capi, APERTURE, FOCUS), capi.projection.equirect()
    rc = capi.lib().gmupt_shutter_ray_host(C.byref(c["cb"]), C.byref(c["sh"]), C.byref(lens), C.byref(proj), 0, 0, 0, C.byref(ray))
    assert rc == capi.ERR_INVALID_ARGUMENT and b"gmupt_shutter_ray_host" in capi.lib().gmupt_last_error() and bytes(ray) == was


def test_identity_gives_the_shading_stages_ray(pkg, oracle):
    """A close pose bit-equal to the camera's (no -0.0 component): without a lens the origin is the camera position and the direction
    step 1 of the lens rule -- the words the shading stage writes (newPath.hlsl:27,36-39; tests/test_lens_cpu.py holds step 1 against
    gmupt_camera_pick_ray, the GPU tests hold the stage against the oracle).  With a lens: gmupt_lens_ray_host's ray."""
    capi = pkg.capi
    for pi, pose in enumerate(LU.POSES):
        for (W, H) in SU.RESOLUTIONS:
            cam = LU.camera(capi, W, H, pose, updates=1 + pi)
            cb = cam.buffer_copy()
            cam.close()
            assert not SU.has_negative_zero(cb)
            sh = capi.shutter.from_camera(cb)
            q, cx, cy = SU.samples(W, H)
            rays = capi.shutter.rays_host(cb, sh, q, cx, cy)
            step1 = LU.rule(oracle, cb, 0.0, 1.0, q, cx, cy)["d"]
            assert np.array_equal(LU.bits(rays[:, 4:7]), LU.bits(step1)), (pose, W, H)
            assert np.array_equal(LU.bits(rays[:, 0:3]), LU.bits(np.tile(np.array(list(cb.position)[:3], F), (q.size, 1))))
            lens = LU.lens_struct(capi, APERTURE, FOCUS)
            assert np.array_equal(LU.bits(capi.shutter.rays_host(cb, sh, q, cx, cy, lens=lens)), LU.bits(capi.lens.lens_rays_host(cb, lens, q, cx, cy)))
            for t in (0.0, 0.37, 1.0):
                assert bytes(capi.shutter.camera_host(cb, sh, t)) == bytes(cb)
    # the stated exception: a component that is -0.0 comes out as +0.0
    cb.position[0] = -0.0
    sh = capi.shutter.from_camera(cb)
    got = capi.shutter.camera_host(cb, sh, 0.5)
    assert np.signbit(F(cb.position[0])) and not np.signbit(F(got.position[0])) and got.position[0] == 0.0


def correlations(d):
    """|corr(t, draw k)| for the four earlier draws of a (5, N) array of draws."""
    t = d[4].astype(np.float64)
    return [abs(float(np.corrcoef(t, d[k].astype(np.float64))[0, 1])) for k in range(4)]


def test_the_time_draw_is_uniform_and_independent_of_the_earlier_draws(pkg, oracle):
    """Over q = 0 .. 2^16 - 1 the time (gmupt_shutter_time_host) has |mean - 1/2| <= 0.0056 and |E[t^2] - 1/3| <= 0.0058, five standard
    errors of a uniform variate at N = 65 536 (sigma 1/sqrt(12) and 2/(3 sqrt 5), over sqrt N), and its correlation with each of the four
    earlier draws of the same generator (the jitter, the lens point) is at most 5 / sqrt N = 0.0195.  The seed pair is that of the lens
    statistics test (tests/test_lens_cpu.py).  Measured with the real generator: DESIGN.md "Shutter" has both ranges; q >= 2^20, where
    frac(q / pi) has few fraction bits left in binary32, is printed here and not asserted."""
    N = 1 << 16
    capi = pkg.capi
    cam = LU.camera(capi, 32, 18, LU.POSES[1], updates=3)
    cb = cam.buffer_copy()
    cam.close()
    q = np.arange(N, dtype=np.uint32)
    t = capi.shutter.times_host(cb, q)
    d = SU.draws(oracle, cb, q)
    assert np.array_equal(LU.bits(t), LU.bits(d[4])), "the host function is the fifth draw"
    t64 = t.astype(np.float64)
    mean, m2, corr = float(t64.mean()), float((t64 * t64).mean()), correlations(d)
    print("time draw, seeds (%.6f, %.6f), q < 2^16: mean %.5f, E[t^2] %.5f, |corr| with draws 1-4 %s" %
          (cb.randomSeed[0], cb.randomSeed[1], mean, m2, ", ".join("%.4f" % c for c in corr)))
    hi = np.arange(1 << 20, (1 << 20) + N, dtype=np.uint32)
    dh = SU.draws(oracle, cb, hi)
    th = dh[4].astype(np.float64)
    print("time draw, q in [2^20, 2^20 + 2^16): mean %.5f, E[t^2] %.5f, |corr| with draws 1-4 %s (not asserted)" %
          (th.mean(), (th * th).mean(), ", ".join("%.4f" % c for c in correlations(dh))))
    assert t.min() >= 0 and t.max() < 1
    assert abs(mean - 0.5) <= 0.0056 and abs(m2 - 1.0 / 3.0) <= 0.0058
    assert max(corr) <= 0.0195, corr


def test_surface_sizes_errors_and_round_trips(pkg):
    capi = pkg.capi
    S, lib = capi.shutter, capi.lib()
    assert C.sizeof(S.Shutter) == 48 and S.Shutter.upperLeftCorner.offset == 12 and S.Shutter.horizontal.offset == 24 and S.Shutter.vertical.offset == 36
    assert set(S.SYMBOLS) == {"gmupt_renderer_set_shutter", "gmupt_renderer_get_shutter", "gmupt_shutter_from_camera", "gmupt_shutter_camera_host",
                              "gmupt_shutter_time_host", "gmupt_shutter_ray_host"}
    assert not set(S.SYMBOLS) & set(capi.SYMBOLS) and not hasattr(capi.Renderer, "set_shutter")
    cb, sh = SU.pair(capi, 32, 18, "both")
    close = LU.camera(capi, 32, 18, SU.POSE_PAIRS["both"][1])
    for name in SU.VECTORS:
        assert list(getattr(sh, name)) == list(getattr(close.buffer, name))[:3]
    close.close()
    # t = 0 is the open camera; t = 1 is the close pose up to the rounding of a + (b - a)
    assert bytes(S.camera_host(cb, sh, 0.0))[:64] == bytes(SU.camera_at(cb, sh, 0.0))[:64]
    one = S.camera_host(cb, sh, 1.0)
    for name in SU.VECTORS:
        assert np.allclose(np.array(getattr(one, name)[:3]), np.array(getattr(sh, name)[:]), rtol=0, atol=4e-7 * 16)
        assert getattr(one, name)[3] == getattr(cb, name)[3]
    assert bytes(one)[64:] == bytes(cb)[64:], "pixelSize, randomSeed, envColor and the counts are the open camera's"
    # errors: each leaves its outputs untouched
    ray, out_cam, out_sh, t = capi.Ray(), capi.CameraBuffer(), S.Shutter(), C.c_float(-7.0)
    for o in (ray, out_cam, out_sh):
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
    was = (bytes(ray), bytes(out_cam), bytes(out_sh))
    E = capi.ERR_INVALID_ARGUMENT
    cam_p, sh_p = C.byref(cb), C.byref(sh)
    assert lib.gmupt_shutter_ray_host(None, sh_p, None, None, 0, 0, 0, C.byref(ray)) == E
    assert lib.gmupt_shutter_ray_host(cam_p, None, None, None, 0, 0, 0, C.byref(ray)) == E
    assert lib.gmupt_shutter_ray_host(cam_p, sh_p, None, None, 0, 0, 0, None) == E
    assert lib.gmupt_shutter_camera_host(None, sh_p, 0.5, C.byref(out_cam)) == E and lib.gmupt_shutter_camera_host(cam_p, None, 0.5, C.byref(out_cam)) == E
    assert lib.gmupt_shutter_camera_host(cam_p, sh_p, 0.5, None) == E and lib.gmupt_shutter_camera_host(cam_p, sh_p, float("nan"), C.byref(out_cam)) == E
    assert lib.gmupt_shutter_time_host(None, 0, C.byref(t)) == E and lib.gmupt_shutter_time_host(cam_p, 0, None) == E
    assert lib.gmupt_shutter_from_camera(None, C.byref(out_sh)) == E and lib.gmupt_shutter_from_camera(cam_p, None) == E
    assert lib.gmupt_renderer_set_shutter(None, sh_p) == E and lib.gmupt_renderer_get_shutter(None, C.byref(out_sh), C.byref(C.c_int())) == E
    for name in SU.VECTORS:
        for k in range(3):
            for bad in (float("nan"), float("inf"), -float("inf")):
                b = S.Shutter.from_buffer_copy(bytes(sh))
                getattr(b, name)[k] = bad
                assert lib.gmupt_shutter_ray_host(cam_p, C.byref(b), None, None, 0, 0, 0, C.byref(ray)) == E, (name, k, bad)
                assert b"gmupt_shutter_ray_host" in lib.gmupt_last_error()
                assert lib.gmupt_shutter_camera_host(cam_p, C.byref(b), 0.5, C.byref(out_cam)) == E
                nb = SU.copy_buffer(cb)
                getattr(nb, name)[k] = bad
                assert lib.gmupt_shutter_from_camera(C.byref(nb), C.byref(out_sh)) == E
    bad_lens, bad_proj = LU.lens_struct(capi, -1.0, 1.0), capi.projection.projection_params(capi.projection.FISHEYE, fov=-1.0)
    assert lib.gmupt_shutter_ray_host(cam_p, sh_p, C.byref(bad_lens), None, 0, 0, 0, C.byref(ray)) == E
    assert lib.gmupt_shutter_ray_host(cam_p, sh_p, None, C.byref(bad_proj), 0, 0, 0, C.byref(ray)) == E
    assert (bytes(ray), bytes(out_cam), bytes(out_sh)) == was and t.value == -7.0
    with pytest.raises(capi.GmuptError):
        S.ray_host(cb, sh, 0, 0, 0, lens=LU.lens_struct(capi, APERTURE, FOCUS), projection=capi.projection.equirect())
    # a lens of aperture 0 is allowed in the host function and runs the lens rule
    z = S.ray_host(cb, sh, 5, 3, 2, lens=LU.lens_struct(capi, 0.0, FOCUS))
    cam_t = S.camera_host(cb, sh, S.time_host(cb, 5))
    assert bytes(z) == bytes(capi.lens.lens_ray_host(cam_t, LU.lens_struct(capi, 0.0, FOCUS), 5, 3, 2))

"""CPU tests of the thin lens (include/gmupt_lens.h): the host rule gmupt_lens_ray_host against the numpy restatement of lens_util.py
bit for bit, the pinhole prefix against gmupt_camera_pick_ray, the focal-plane geometry in float64 and the statistics of the lens disk.
No device."""
import numpy as np
import pytest

import lens_util as LU

F = LU.F
APERTURE, FOCUS = 0.3, 13.0          # Cornell: a few per cent of the 10-unit room, the back wall seen from the default camera


def samples(W, H, seed):
    """A few hundred (q, cx, cy): random ones, the corners of the frame, tile-origin pixels paired with q = 0, and the largest q of a
    2^21 pool."""
    rng = np.random.default_rng(seed)
    n = 300
    q = rng.integers(0, 1 << 21, n).astype(np.uint32)
    cx = rng.integers(0, W, n).astype(np.uint32)
    cy = rng.integers(0, H, n).astype(np.uint32)
    edge = [(0, 0, 0), (0, W - 1, 0), (0, 0, H - 1), (1, W - 1, H - 1), ((1 << 21) - 1, W - 1, H - 1), ((1 << 21) - 1, 0, 0),
            (0, W // 3, H // 3), (255, W // 3, H // 3), (256, W // 3 + 1, H // 3), (257, W // 2, H - 1)]     # (W/3, H/3): a tile origin
    e = np.array(edge, np.uint32)
    return np.concatenate([q, e[:, 0]]), np.concatenate([cx, e[:, 1]]), np.concatenate([cy, e[:, 2]])


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    """Per (pose, resolution): the camera buffer, the samples, the host rays and the restatement, computed once."""
    out = []
    for pi, pose in enumerate(LU.POSES):
        for (W, H) in LU.RESOLUTIONS:
            cam = LU.camera(pkg.capi, W, H, pose, updates=1 + pi)      # another randomSeed per pose
            cb = cam.buffer_copy()
            cam.close()
            q, cx, cy = samples(W, H, 17 * pi + W)
            lens = LU.lens_struct(pkg.capi, APERTURE, FOCUS)
            rays = pkg.capi.lens.lens_rays_host(cb, lens, q, cx, cy)
            out.append(dict(pose=pose, size=(W, H), cb=cb, q=q, cx=cx, cy=cy, rays=rays, want=LU.rule(oracle, cb, APERTURE, FOCUS, q, cx, cy)))
    return out


def test_host_rule_equals_the_restatement(cases):
    assert len(cases) == 6 and all(c["q"].size >= 300 for c in cases)
    for c in cases:
        rays, want = c["rays"], c["want"]
        assert int(c["q"].max()) == (1 << 21) - 1
        assert np.array_equal(LU.bits(rays[:, 0:3]), LU.bits(want["origin"])), (c["pose"], c["size"], "origin")
        assert np.array_equal(LU.bits(rays[:, 4:7]), LU.bits(want["direction"])), (c["pose"], c["size"], "direction")
        assert np.all(rays[:, 3] == np.finfo(F).max) and not LU.bits(rays[:, 7]).any()
        assert np.isfinite(rays[:, :7]).all()
        assert (np.abs(want["lx"]) + np.abs(want["ly"]) > 0).mean() > 0.95, "the lens did move the origins (r1 = 0 is a legal draw)"


def test_pinhole_prefix_is_the_renderers_ray(pkg, cases):
    """Step 1 is the jittered primary ray of the shading stage: gmupt_camera_pick_ray through ((float)cx + jx, (float)cy + jy) runs
    newPath.hlsl:37-39 on those coordinates (it is what gmupt_aov_ray calls), so its direction must equal d bit for bit, and its
    origin is the centre of the lens disk."""
    for c in cases:
        want = c["want"]
        px = (c["cx"].astype(F) + want["jx"]).astype(F)
        py = (c["cy"].astype(F) + want["jy"]).astype(F)
        for i in range(0, c["q"].size, 7):
            ray = pkg.capi.camera_pick_ray(c["cb"], float(px[i]), float(py[i]))
            assert np.array_equal(LU.bits(np.array(ray.direction[:], F)), LU.bits(want["d"][i])), (c["pose"], c["size"], i)
            assert list(ray.origin) == list(c["cb"].position)[:3]
        assert np.all(want["jx"] >= -1) and np.all(want["jx"] < 1) and np.all(want["jy"] >= -1) and np.all(want["jy"] < 1)


def test_every_ray_meets_its_pinhole_ray_on_the_focal_plane(cases):
    """In float64, from the stored float32 rays alone: the point of ray (origin, direction) on the plane dot(X - pos, fn) = focus must be
    Pf = pos + d * focus / dot(d, fn), the pinhole ray's point on that plane.

    The bound, from binary32 rounding (eps = 2^-24 relative per operation).  Geometry of these cameras, not of the code under test: the
    corner of the frame lies at cos 0.6475 from the forward axis and the jitter reaches one pixel further, so dot(d, fn) >= 0.6,
    |Pf - pos| <= 13 / 0.6 < 22 and the obliquity 1 / dot(direction, fn) <= 1.7; |pos| components <= 8.  S = 32, the scene scale,
    covers every length that occurs.  The test recomputes Pf in float64 from the float32 d and fn, so their own rounding does not count.
      * Pf32, the rule's focal point: dot3 is 5 roundings on terms <= 1 against a value >= 0.6 (<= 8.3 eps relative), the division 1,
        d*t 1, pos + 1 on a result <= S: |Pf32 - Pf| <= 12 eps S.
      * origin = (pos + right*lx) + up*ly: 4 roundings per component, each <= eps S.
      * direction = normalize3(Pf32 - origin): the subtraction adds 1 eps S to the 12 above, the normalisation (dot3, sqrt, reciprocal,
        product) <= 5 eps relative.  Carried over the distance |Pf - origin| <= S that is (13 + 5) eps S = 18 eps S across the ray,
        and 1.7 times that along the oblique plane: 30.6 eps S.  The origin's 4 eps S move the crossing by at most twice that: 8 eps S.
      Sum: < 39 eps S = 19.5 * 2^-23 * S.  The bound asserted is 20 * 2^-23 * S."""
    S = 32.0
    bound = 20 * 2.0 ** -23 * S
    worst = 0.0
    for c in cases:
        cb, want = c["cb"], c["want"]
        pos = np.array(list(cb.position)[:3], np.float64)
        assert np.abs(pos).max() <= 8.0
        fn = want["fn"].astype(np.float64)
        d = want["d"].astype(np.float64)
        Pf = pos + d * (FOCUS / (d @ fn))[:, None]
        assert (d @ fn).min() >= 0.6 and np.linalg.norm(Pf - pos, axis=1).max() < 22.0
        o = c["rays"][:, 0:3].astype(np.float64)
        w = c["rays"][:, 4:7].astype(np.float64)
        assert ((w @ fn) >= 1 / 1.7).all()
        s = (FOCUS - (o - pos) @ fn) / (w @ fn)
        X = o + w * s[:, None]
        err = np.abs(X - Pf).max()
        worst = max(worst, err)
        assert err <= bound, (c["pose"], c["size"], err, bound)
        # the origins lie in the lens plane through pos: no component along fn beyond rounding
        assert np.abs((o - pos) @ fn).max() <= 8 * 2.0 ** -23 * S
    print("focal plane: worst |X - Pf| = %.3g, bound %.3g" % (worst, bound))


def test_the_lens_offsets_fill_the_disk_uniformly(pkg, oracle):
    """Over N = 2^16 consecutive q the offsets (lx, ly) -- recovered from the host function's origins as ((origin - pos) . right,
    (origin - pos) . up) -- lie in the disk of the aperture, have mean zero and E[lx^2 + ly^2] = a^2 / 2.
    Margins: 5 sigma of the sample means of N independent uniform points of a disk of radius a.  Var(lx) = a^2 / 4, so the mean of lx has
    sigma a / (2 sqrt N); r^2 = lx^2 + ly^2 is a^2 U with U uniform, Var(r^2) = a^4 / 12, so its mean has sigma a^2 / sqrt(12 N)."""
    N = 1 << 16
    a = APERTURE
    cam = LU.camera(pkg.capi, 32, 18, LU.POSES[1], updates=3)
    cb = cam.buffer_copy()
    cam.close()
    q = np.arange(N, dtype=np.uint32)
    cx, cy = (q % 32).astype(np.uint32), ((q // 32) % 18).astype(np.uint32)
    rays = pkg.capi.lens.lens_rays_host(cb, LU.lens_struct(pkg.capi, a, FOCUS), q, cx, cy)
    pos, _, hor, ver = (v.astype(np.float64) for v in LU.cam_vectors(cb))
    right, up = hor / np.linalg.norm(hor), ver / np.linalg.norm(ver)
    off = rays[:, 0:3].astype(np.float64) - pos
    lx, ly = off @ right, off @ up
    r2 = lx * lx + ly * ly
    assert r2.max() <= (a * (1 + 1e-5)) ** 2, "inside the disk (sqrt(r1) < 1, |cos|, |sin| <= 1 up to rounding)"
    # and they are the restatement's own offsets, to the rounding of the recovery
    want = LU.rule(oracle, cb, a, FOCUS, q, cx, cy)
    assert np.abs(lx - want["lx"]).max() < 1e-5 and np.abs(ly - want["ly"]).max() < 1e-5
    s_mean, s_r2 = a / (2 * np.sqrt(N)), a * a / np.sqrt(12 * N)
    print("disk: mean lx %.3g ly %.3g (5 sigma %.3g), E[r^2] %.6g want %.6g (5 sigma %.3g)" % (lx.mean(), ly.mean(), 5 * s_mean, r2.mean(), a * a / 2, 5 * s_r2))
    assert abs(lx.mean()) <= 5 * s_mean and abs(ly.mean()) <= 5 * s_mean
    assert abs(r2.mean() - a * a / 2) <= 5 * s_r2
    # aperture 0 through the host function: the origin is the camera position
    zero = pkg.capi.lens.lens_rays_host(cb, LU.lens_struct(pkg.capi, 0.0, FOCUS), q[:64], cx[:64], cy[:64])
    assert np.array_equal(zero[:, 0:3], np.tile(np.array(list(cb.position)[:3], F), (64, 1)))

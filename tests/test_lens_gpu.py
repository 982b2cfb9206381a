"""GPU tests of the thin lens (gmupt_renderer_set_lens, csrc/pt_lens.hip): the stage against its host rule bit for bit at the sizes at
which it can go wrong, whole iterations against a renderer whose fresh slots are patched on the host between the shipped stages, the
lens under a sampling plan, the detached cases, the life cycle, the errors, the autofocus, an image-level ordering and the session.
Cornell at 32 x 18 with a pool of 4096, as the adaptive tests."""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import adaptive_util as AU
import lens_util as LU

pytestmark = pytest.mark.gpu

W, H, POOL = 32, 18, 4096
RECT = (7, 5, 11, 6)
APERTURE, FOCUS = 0.3, 13.0      # a few per cent of the 10-unit room; the back wall from the default camera


@pytest.fixture(params=["wide", "cast0"])
def shipped_kernel(request, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", request.param)
    return request.param


def make(pkg, device, scene, tile=None, budget=0, pool=POOL, live=0, size=(W, H)):
    """tile: (x0, y0, w, h) of a tile renderer of the frame."""
    sb = pkg.capi.SceneBuffers(device, scene)
    if tile is None:
        r = pkg.capi.Renderer(device, size[0], size[1], pool_paths=pool, live_paths=live, path_budget=budget)
    else:
        r = pkg.capi.Renderer(device, tile[2], tile[3], pool_paths=pool, live_paths=live, tile=(tile[0], tile[1]), path_budget=budget)
    r.bind_scene(sb)
    cam = pkg.capi.Camera(*size); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return r, sb, cam


def close(*things):
    for t in things:
        t.close()


def step(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()


def lens_of(pkg, aperture=APERTURE, focus=FOCUS):
    return LU.lens_struct(pkg.capi, aperture, focus)


def snapshot(r):
    r.synchronize()
    return r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters()


def same(a, b):
    return np.array_equal(LU.bits(a[0]), LU.bits(b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def host_rays(pkg, cb, lens, raw, pool, q, slots):
    """gmupt_lens_ray_host of the fresh slots: their queue indices and the screen coordinates the state holds."""
    xy = LU.state_screen(raw, pool)[slots]
    return pkg.capi.lens.lens_rays_host(cb, lens, q, xy[:, 0], xy[:, 1])


# name: (make() arguments, iterations before the stage, render the budget out first, what the fresh count must look like)
STAGE_CASES = {
    "first_stage_16_blocks": (dict(), 0, False, lambda n: n == POOL),
    "live_3000_of_4096": (dict(live=3000), 0, False, lambda n: n == 3000 and n % 256),
    "fourth_iteration_ragged": (dict(), 3, False, lambda n: 0 < n < POOL and n % 256),
    "budget_retires_part": (dict(budget=2500), 0, False, lambda n: n == POOL),
    "nothing_ended": (dict(budget=1000), 0, True, lambda n: n == 0),
    "tile_origin_7_5": (dict(tile=RECT, pool=1024), 0, False, lambda n: n == 1024),
}


@pytest.mark.parametrize("case", sorted(STAGE_CASES))
def test_stage_equals_the_host_rule(pkg, device, shipped_kernel, cornell_scene, case):
    kw, before, render_out, count_ok = STAGE_CASES[case]
    pool, live, budget = kw.get("pool", POOL), kw.get("live", 0) or kw.get("pool", POOL), kw.get("budget", 0)
    runs = []
    for with_lens in (False, True):
        r, sb, cam = make(pkg, device, cornell_scene, **kw)
        if render_out:
            r.render_budget(cam)
        step(r, cam, before)
        if with_lens:
            pkg.capi.lens.set_lens(r, lens_of(pkg))
        cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(pkg.capi.STAGE_SHADE)
        runs.append(snapshot(r) + (cam.buffer_copy(),))
        close(r, sb, cam)
    plain, lensed = runs
    qc = lensed[3]
    n_new = min(int(qc[0]), live)
    q, slots = LU.fresh(qc, lensed[2], live, budget)
    print("%s: new-path count %d, fresh after the guards %d, lastPathCnt %d" % (case, n_new, q.size, int(qc[1])))
    assert count_ok(n_new), n_new
    if case == "budget_retires_part":
        assert q.size == 2500 and slots.size < n_new
    if case == "tile_origin_7_5":
        xy = LU.state_screen(lensed[1], pool)[slots]
        assert xy[:, 0].min() == 7 and xy[:, 1].min() == 5 and xy[:, 0].max() == 17 and xy[:, 1].max() == 10
    assert np.array_equal(LU.bits(plain[0]), LU.bits(lensed[0])) and np.array_equal(plain[2], lensed[2]) and np.array_equal(plain[3], lensed[3])
    want = LU.patch_rays(plain[1], pool, slots, host_rays(pkg, lensed[4], lens_of(pkg), plain[1], pool, q, slots)) if q.size else plain[1]
    assert np.array_equal(want, lensed[1]), "fresh slots hold the host rule's ray; every other word is the run without a lens"
    if q.size:
        o, _ = LU.state_rays(lensed[1], pool)
        assert (np.abs(o[slots] - np.array(list(lensed[4].position)[:3], LU.F)).max(axis=1) > 0).mean() > 0.95, "the origins did move"


@pytest.mark.parametrize("tile", [None, (4, 3, 20, 12)], ids=["frame", "tile"])
def test_whole_iterations_equal_the_patched_stages(pkg, device, shipped_kernel, cornell_scene, tile):
    """A: a lens attached, gmupt_iterate.  B: no lens; per iteration the shipped shading stage, the host rule patched into the fresh
    slots through the debug access, the shipped ray casts.  Equal after 1, 2 and 24 iterations in every word."""
    capi = pkg.capi
    pool = POOL if tile is None else 1024
    lens = lens_of(pkg)
    a, sba, cama = make(pkg, device, cornell_scene, tile=tile, pool=pool)
    b, sbb, camb = make(pkg, device, cornell_scene, tile=tile, pool=pool)
    capi.lens.set_lens(a, lens)
    moved = 0
    for it in range(1, 25):
        step(a, cama, 1)
        camb.update(0.0); b.set_camera(camb.buffer); b.run_stage(capi.STAGE_SHADE)
        raw, queues, qc = b.read_path_state(), b.read_queues(), b.counters()
        q, slots = LU.fresh(qc, queues, pool)
        if q.size:
            b.write_path_state(LU.patch_rays(raw, pool, slots, host_rays(pkg, camb.buffer_copy(), lens, raw, pool, q, slots)))
            moved += q.size
        b.run_stage(capi.STAGE_RAYCASTS)
        if it in (1, 2, 24):
            assert same(snapshot(a), snapshot(b)), "iteration %d" % it
    assert moved > pool and int(a.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    close(a, sba, cama, b, sbb, camb)


def test_lens_follows_an_attached_sampling_plan(pkg, device, cornell_scene):
    """The rectangle plan of the adaptive tests: k_ad_retarget first, then the lens on the pixels it stored."""
    capi = pkg.capi
    runs = []
    for with_lens in (False, True):
        r, sb, cam = make(pkg, device, cornell_scene)
        plan = capi.adaptive.Adaptive(r)
        plan.set_list(AU.rect_list(W, *RECT), W, H)
        capi.adaptive.set_adaptive(r, plan)
        if with_lens:
            capi.lens.set_lens(r, lens_of(pkg))
        step(r, cam, 2)
        cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(capi.STAGE_SHADE)
        runs.append(snapshot(r) + (cam.buffer_copy(),))
        close(r, sb, cam)
    plain, lensed = runs
    q, slots = LU.fresh(lensed[3], lensed[2], POOL)
    xy = LU.state_screen(lensed[1], POOL)[slots]
    x0, y0, w, h = RECT
    assert q.size > 0 and ((xy[:, 0] >= x0) & (xy[:, 0] < x0 + w) & (xy[:, 1] >= y0) & (xy[:, 1] < y0 + h)).all(), "the plan's pixels"
    got_o, got_d = LU.state_rays(lensed[1], POOL)
    rays = host_rays(pkg, lensed[4], lens_of(pkg), lensed[1], POOL, q, slots)
    assert np.array_equal(LU.bits(got_o[slots]), LU.bits(rays[:, 0:3])) and np.array_equal(LU.bits(got_d[slots]), LU.bits(rays[:, 4:7]))
    # the screen coordinates are the plan's, lens or not (the states of the two runs differ from the first iteration on)
    qp, sp = LU.fresh(plain[3], plain[2], POOL)
    pxy = LU.state_screen(plain[1], POOL)[sp]
    assert ((pxy[:, 0] >= x0) & (pxy[:, 0] < x0 + w) & (pxy[:, 1] >= y0) & (pxy[:, 1] < y0 + h)).all()


def test_nothing_attached_aperture_zero_and_detach_are_the_plain_renderer(pkg, device, shipped_kernel, cornell_scene):
    capi = pkg.capi

    def run(prepare):
        r, sb, cam = make(pkg, device, cornell_scene)
        prepare(r)
        step(r, cam, 12)
        out = snapshot(r)
        close(r, sb, cam)
        return out

    def attach_and_detach(r):
        capi.lens.set_lens(r, lens_of(pkg))
        capi.lens.set_lens(r, None)

    def reopen_and_zero(r):
        capi.lens.set_lens(r, lens_of(pkg))
        capi.lens.set_lens(r, lens_of(pkg, 0.0, -1.0))     # aperture 0 detaches whatever the focus says

    plain = run(lambda r: None)
    assert int(plain[0][..., 3].view(np.uint32).sum()) > 0
    for prepare in (lambda r: capi.lens.set_lens(r, None), lambda r: capi.lens.set_lens(r, lens_of(pkg, 0.0, FOCUS)), attach_and_detach, reopen_and_zero):
        assert same(plain, run(prepare))
    assert not same(plain, run(lambda r: capi.lens.set_lens(r, lens_of(pkg)))), "an open lens does change the frame"
    # detached in the middle: from there on it continues like a renderer brought to that state that never had a lens
    r, sb, cam = make(pkg, device, cornell_scene)
    capi.lens.set_lens(r, lens_of(pkg))
    step(r, cam, 6)
    snap = snapshot(r)
    capi.lens.set_lens(r, None)
    cams = []
    for _ in range(6):
        cam.update(0.0); cams.append(cam.buffer_copy()); r.set_camera(cams[-1]); r.iterate()
    after = snapshot(r)
    r2, sb2, cam2 = make(pkg, device, cornell_scene)
    r2.write_framebuffer(snap[0]); r2.write_path_state(snap[1]); r2.write_queues(snap[2]); r2.write_counters(snap[3])
    for cb in cams:
        r2.set_camera(cb); r2.iterate()
    assert same(after, snapshot(r2))
    close(r, sb, cam, r2, sb2, cam2)


def test_life_cycle_and_errors(pkg, device, cornell_scene):
    capi = pkg.capi
    lib = capi.lib()
    L = capi.lens
    r, sb, cam = make(pkg, device, cornell_scene)
    d = L.get_lens(r)
    assert (d.aperture_radius, d.focus_distance) == (0.0, 1.0)
    L.set_lens(r, lens_of(pkg, 0.25, 7.5))
    got = L.get_lens(r)
    assert (got.aperture_radius, got.focus_distance) == (0.25, 7.5)
    step(r, cam, 2)
    r.resize(24, 12); cam.update_resolution(24, 12)
    got = L.get_lens(r)
    assert (got.aperture_radius, got.focus_distance) == (0.25, 7.5), "the lens survives gmupt_resize"
    step(r, cam, 2)                                    # and gmupt_set_camera
    got = L.get_lens(r)
    assert (got.aperture_radius, got.focus_distance) == (0.25, 7.5)
    # and it is still launched: the fresh slots of the next shading stage hold the rule's rays at the new size
    cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(capi.STAGE_SHADE)
    _, raw, queues, qc = snapshot(r)
    q, slots = LU.fresh(qc, queues, POOL)
    rays = host_rays(pkg, cam.buffer_copy(), lens_of(pkg, 0.25, 7.5), raw, POOL, q, slots)
    o, d = LU.state_rays(raw, POOL)
    assert q.size > 0 and np.array_equal(LU.bits(o[slots]), LU.bits(rays[:, 0:3])) and np.array_equal(LU.bits(d[slots]), LU.bits(rays[:, 4:7]))
    assert int(LU.state_screen(raw, POOL)[slots][:, 0].max()) == 23
    # every stated error, and the attached lens is left as it was
    nan, inf = float("nan"), float("inf")
    bad = [(nan, 1.0), (inf, 1.0), (-0.1, 1.0), (0.1, nan), (0.1, inf), (0.1, 0.0), (0.1, -2.0)]
    ray = capi.Ray()
    C.memset(C.byref(ray), 0xAB, C.sizeof(ray))
    was = bytes(ray)
    cb = cam.buffer_copy()
    for a, f in bad:
        l = lens_of(pkg, a, f)
        assert lib.gmupt_renderer_set_lens(r.h, C.byref(l)) == capi.ERR_INVALID_ARGUMENT, (a, f)
        assert b"gmupt_renderer_set_lens" in lib.gmupt_last_error()
        assert lib.gmupt_lens_ray_host(C.byref(cb), C.byref(l), 0, 0, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, (a, f)
    ok = lens_of(pkg)
    assert lib.gmupt_renderer_set_lens(None, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_renderer_get_lens(None, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT and lib.gmupt_renderer_get_lens(r.h, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_lens_ray_host(None, C.byref(ok), 0, 0, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_lens_ray_host(C.byref(cb), None, 0, 0, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_lens_ray_host(C.byref(cb), C.byref(ok), 0, 0, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_lens_focus_at(None, 1.0, 1.0, 0, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_lens_focus_at(r.h, 1.0, 1.0, 0, None) == capi.ERR_INVALID_ARGUMENT
    got = L.get_lens(r)
    assert bytes(ray) == was and (got.aperture_radius, got.focus_distance) == (0.25, 7.5)
    assert (ok.aperture_radius, ok.focus_distance) == (LU.F(APERTURE), LU.F(FOCUS))
    close(r, sb, cam)


WALL_PIXEL = (18, 4)      # of the 32 x 18 frame: up and to the right of both boxes, on the back wall (z = -5, the camera at z = 8)


def test_focus_at(pkg, device, oracle, cornell_scene):
    capi = pkg.capi
    r, sb, cam = make(pkg, device, cornell_scene)
    cam.update(0.0); r.set_camera(cam.buffer)
    cb = cam.buffer_copy()
    ray, hit = r.pick(WALL_PIXEL[0], WALL_PIXEL[1], 0)
    assert hit.triangle >= 0
    lens = capi.lens.focus_at(r, WALL_PIXEL[0], WALL_PIXEL[1], 0, aperture_radius=0.2)
    fn = LU.rule(oracle, cb, 0.2, 1.0, [0], [0], [0])["fn"]
    want = LU.F(LU.F(hit.t) * LU.dot3(np.array(ray.direction[:], LU.F), fn))
    print("focus_at %r: t %.6f, depth along fn %.6f" % (WALL_PIXEL, hit.t, lens.focus_distance))
    assert lens.aperture_radius == LU.F(0.2) and LU.bits(LU.F(lens.focus_distance)) == LU.bits(want)
    assert abs(lens.focus_distance - 13.0) < 1e-3, "the back wall of the room from the default camera"
    assert capi.lens.get_lens(r).aperture_radius == 0.0, "focus_at attaches nothing"
    # a miss: the camera turned away from the room (every pixel of the default camera sees a wall)
    x, y, z, pitch, yaw = cornell_scene["camera"]
    cam.set_pose(x, y, z, pitch, yaw - 180.0); cam.update(0.0); r.set_camera(cam.buffer)
    ray, hit = r.pick(WALL_PIXEL[0], WALL_PIXEL[1], 0)
    assert hit.triangle < 0 and hit.light == 0
    keep = capi.lens.lens_params(aperture_radius=0.2, focus_distance=5.0)
    assert capi.lib().gmupt_lens_focus_at(r.h, float(WALL_PIXEL[0]), float(WALL_PIXEL[1]), 0, C.byref(keep)) == capi.ERR_INVALID_ARGUMENT
    assert b"nothing to focus on" in capi.lib().gmupt_last_error() and (keep.aperture_radius, keep.focus_distance) == (LU.F(0.2), 5.0)
    with pytest.raises(capi.GmuptError):
        capi.lens.focus_at(r, WALL_PIXEL[0], WALL_PIXEL[1], 0, aperture_radius=0.2)
    close(r, sb, cam)


DOF_POSE = (-3.5, 8.0, 7.0, 0.0, 270.0)      # outside the room's opening (z = 5), high and to the left, looking at the back wall


def test_depth_of_field_blurs_the_near_field_not_the_focal_plane(pkg, device, cornell_scene):
    """Cornell 64 x 36 at 256 spp (the statistical test of test_parity_gpu.py), the lens focused on the back wall through focus_at on the
    centre pixel, aperture 0.5 (5 % of the room).  Against the pinhole render of the same spp: the mean absolute difference over the
    pixels whose depth along the forward axis lies within 5 % of the focus distance, and over the pixels nearer than half of it.  The
    noise: the same two measures between two pinhole renders with different seeds (another pool size); a mean absolute difference
    between two renders contains that much without any lens, so what the lens did to a region is its figure less the region's noise
    figure.  Asserted: only the ordering of those two, near > in focus.  Margin: a noise figure is a mean over M pixels of per-pixel
    values of about its own size, so it varies by about n / sqrt(M) from run to run; three of those for the larger n and the smaller M.

    The view.  A lens changes an image only where the image has contrast inside the circle of confusion.  From the scenes' default
    camera every pixel sees the inside of the room; what lies nearer than half the focus distance is the inner faces of the walls
    around the opening and the front of the short box, each one flat material under smooth light, and their blurred image is the same
    image: at 256 spp the measure cannot tell a lens from none there (what the lens did came out as 0.0010 near / 0.0023 in focus in
    one run and 0.0020 / 0.0013 with other seeds, against a margin of 0.0030: noise).  So the camera stands outside the opening, high
    and to the left, where the rim of the red wall (x = -5, at depth 2 of a focus of 12) stands inside the frame against the dark
    environment, and the boxes lie low in the frame.  That the view is of this kind is asserted from the pinhole AOVs alone, before
    any lens figure is looked at: near-field pixels border pixels that see no surface.
    Measured on the MI355X: 482 pixels in focus, 888 near; mean |lens - pinhole| in focus 0.01596, near 0.02487; pinhole against other
    seeds 0.01649 and 0.01644; what the lens did: near 0.00843, in focus -0.00052, margin 0.0023."""
    capi = pkg.capi
    Wd, Hd, spp, aperture = 64, 36, 256, 0.5
    sb = capi.SceneBuffers(device, cornell_scene)

    def render(pool, with_lens):
        r = capi.Renderer(device, Wd, Hd, pool_paths=pool, path_budget=Wd * Hd * spp)
        r.bind_scene(sb)
        cam = capi.Camera(Wd, Hd); cam.set_pose(*DOF_POSE); cam.buffer.lightCount = cornell_scene["light_count"]
        lens = None
        if with_lens:
            cam.update(0.0); r.set_camera(cam.buffer)
            lens = capi.lens.focus_at(r, Wd / 2, Hd / 2, 0, aperture_radius=aperture)
            cam.reset_accumulation()
            capi.lens.set_lens(r, lens)
        r.render_budget(cam, 100000)
        fb = r.framebuffer()
        assert np.all(fb[..., 3].view(np.uint32) == spp)
        cam.update(0.0); r.set_camera(cam.buffer)
        aov = capi.aov_fields(r.aovs(1))
        cb = cam.buffer_copy()
        close(r, cam)
        return np.minimum(fb[..., :3].astype(np.float64), 4.0), aov, cb, lens

    pin, aov, cb, _ = render(4096, False)
    other, _, _, _ = render(3072, False)
    dof, _, _, lens = render(4096, True)
    sb.close()
    assert abs(float(aov["position"][Hd // 2, Wd // 2][2]) + 5.0) < 1e-3 and abs(lens.focus_distance - 12.0) < 1e-3, "focused on the back wall (z = -5)"
    pos, ulc, hor, ver = (v.astype(np.float64) for v in LU.cam_vectors(cb))
    fn = ulc + hor / 2 - ver / 2
    fn /= np.linalg.norm(fn)
    z = (aov["position"].astype(np.float64) - pos) @ fn
    surface = aov["triangle"] >= 0
    focus = surface & (np.abs(z - lens.focus_distance) <= 0.05 * lens.focus_distance)
    near = surface & (z < 0.5 * lens.focus_distance)
    # the view has what the check needs, from the pinhole AOVs alone: near-field pixels next to pixels that see nothing
    void = np.pad(~surface, 1)
    beside_void = void[1:-1, :-2] | void[1:-1, 2:] | void[:-2, 1:-1] | void[2:, 1:-1]
    rim = int((near & beside_void).sum())
    assert focus.sum() > 50 and near.sum() > 50 and rim >= 16, (int(focus.sum()), int(near.sum()), rim)
    mad = lambda a, b, m: float(np.abs(a - b)[m].mean())
    d_focus, d_near = mad(dof, pin, focus), mad(dof, pin, near)
    n_focus, n_near = mad(other, pin, focus), mad(other, pin, near)
    print("depth of field, Cornell %dx%d at %d spp, aperture %.2f, focus %.3f: %d pixels in focus, %d near (%d on the rim); mean |lens - pinhole| "
          "in focus %.5f, near %.5f; pinhole against other seeds in focus %.5f, near %.5f" % (Wd, Hd, spp, aperture, lens.focus_distance, int(focus.sum()),
                                                                                             int(near.sum()), rim, d_focus, d_near, n_focus, n_near))
    margin = 3.0 * max(n_focus, n_near) / np.sqrt(min(int(focus.sum()), int(near.sum())))
    print("what the lens did: near %.5f, in focus %.5f, margin %.5f" % (d_near - n_near, d_focus - n_focus, margin))
    assert d_near - n_near > (d_focus - n_focus) + margin, (d_near, d_focus, n_focus, n_near, margin)


def test_session_set_lens_restarts_and_previews(pkg, device, cornell_scene):
    capi = pkg.capi
    r, sb, cam = make(pkg, device, cornell_scene)
    s = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    s.run(6)
    before = int(r.framebuffer()[..., 3].view(np.uint32).max())
    lens = s.set_lens(0.3, focus_at=WALL_PIXEL)
    assert abs(lens.focus_distance - 13.0) < 1e-3 and capi.lens.get_lens(r).aperture_radius == LU.F(0.3)
    s.run(1)
    r.synchronize()
    assert cam.buffer.iterationCounter == 0, "the frame after set_lens clears the target"
    s.run(3)
    after = int(r.framebuffer()[..., 3].view(np.uint32).max())
    assert before > 1 and 0 < after <= before
    img = s.denoised_temporal()
    assert img.shape == (H, W, 4) and np.isfinite(img[..., :3]).all() and float(img[..., :3].max()) > 0
    with pytest.raises(ValueError):
        s.set_lens(0.3)
    with pytest.raises(ValueError):
        s.set_lens(0.3, focus=2.0, focus_at=(1, 1))
    s.set_lens(0.0)
    assert capi.lens.get_lens(r).aperture_radius == 0.0
    s.run(2)
    s.close()
    close(r, sb, cam)

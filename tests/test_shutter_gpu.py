"""GPU tests of the shutter (gmupt_renderer_set_shutter, csrc/pt_shutter.hip): the stage against its host rule bit for bit at the sizes
at which it can go wrong, under every rule and under a sampling plan; whole iterations against a renderer whose fresh slots are patched
on the host between the shipped stages; the detached cases; the life cycle and the errors; an image-level check against fixed-time
renders; the session.  Cornell at 32 x 18 with a pool of 4096, as the lens tests."""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import adaptive_util as AU
import lens_util as LU
import shutter_util as SU

pytestmark = pytest.mark.gpu

W, H, POOL = 32, 18, 4096
RECT = (7, 5, 11, 6)
APERTURE, FOCUS = 0.3, 13.0      # the lens of the lens tests


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


CLOSE_POSE = lambda scene: (scene["camera"][0] + 0.5, scene["camera"][1] + 0.1, scene["camera"][2] - 0.2, scene["camera"][3] + 1.0, scene["camera"][4] + 3.0)


def shutter_of(pkg, scene, size=(W, H), pose=None):
    """The Shutter of a camera at `pose` (default: CLOSE_POSE, a translation and a turn of 3 degrees away from the scene's camera)."""
    c = pkg.capi.Camera(*size); c.set_pose(*(pose or CLOSE_POSE(scene))); c.update(0.0)
    sh = pkg.capi.shutter.from_camera(c.buffer_copy())
    c.close()
    return sh


def rule_args(pkg, rule):
    """(lens, projection) of a rule name; the renderer gets the same attached."""
    P = pkg.capi.projection
    return {"pinhole": (None, None), "lens": (lens_of(pkg), None), "ortho": (None, P.orthographic(6.0)), "fisheye": (None, P.fisheye(180.0)),
            "equirect": (None, P.equirect())}[rule]


def attach_rule(pkg, r, lens, proj):
    if lens is not None:
        pkg.capi.lens.set_lens(r, lens)
    if proj is not None:
        pkg.capi.projection.set_projection(r, proj)


# name: (make() arguments, iterations before the stage, render the budget out first, what the fresh count must look like)
STAGE_CASES = {
    "first_stage_16_blocks": (dict(), 0, False, lambda n: n == POOL),
    "live_3000_of_4096": (dict(live=3000), 0, False, lambda n: n == 3000 and n % 256),
    "fourth_iteration_ragged": (dict(), 3, False, lambda n: 0 < n < POOL and n % 256),
    "budget_retires_part": (dict(budget=2500), 0, False, lambda n: n == POOL),
    "nothing_ended": (dict(budget=1000), 0, True, lambda n: n == 0),
    "tile_origin_7_5": (dict(tile=RECT, pool=1024), 0, False, lambda n: n == 1024),
}
STAGE_RUNS = [(case, rule) for case in sorted(STAGE_CASES) for rule in ("pinhole", "lens")] + \
             [(case, rule) for case in ("first_stage_16_blocks", "fourth_iteration_ragged") for rule in ("ortho", "fisheye", "equirect")]


def stage_pair(pkg, device, scene, kw, before, render_out, lens, proj, plan_list=None):
    """Two renderers brought to the same state with the rule attached from the start (so that their states agree), the second with the
    shutter attached for the one shading stage that is compared.  Returns (without, with, shutter)."""
    capi = pkg.capi
    sh = shutter_of(pkg, scene)
    runs = []
    for with_shutter in (False, True):
        r, sb, cam = make(pkg, device, scene, **kw)
        plan = None
        if plan_list is not None:
            plan = capi.adaptive.Adaptive(r)
            plan.set_list(plan_list, W, H)
            capi.adaptive.set_adaptive(r, plan)
        attach_rule(pkg, r, lens, proj)
        if render_out:
            r.render_budget(cam)
        step(r, cam, before)
        if with_shutter:
            capi.shutter.set_shutter(r, sh)
        cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(capi.STAGE_SHADE)
        runs.append(snapshot(r) + (cam.buffer_copy(),))
        close(r, sb, cam)
    return runs[0], runs[1], sh


def check_stage(pkg, plain, blurred, sh, pool, live, budget, lens, proj):
    """The six ray words of every live fresh path are the host rule's; every other word of state, queues, counters and frame is the
    run's without a shutter.  Returns (queue indices, slots)."""
    q, slots = LU.fresh(blurred[3], blurred[2], live, budget)
    assert np.array_equal(LU.bits(plain[0]), LU.bits(blurred[0])) and np.array_equal(plain[2], blurred[2]) and np.array_equal(plain[3], blurred[3])
    want = LU.patch_rays(plain[1], pool, slots, SU.host_rays(pkg.capi, blurred[4], sh, plain[1], pool, q, slots, lens, proj)) if q.size else plain[1]
    assert np.array_equal(want, blurred[1]), "fresh slots hold the host rule's ray; every other word is the run without a shutter"
    return q, slots


@pytest.mark.parametrize("case, rule", STAGE_RUNS, ids=["%s-%s" % cr for cr in STAGE_RUNS])
def test_stage_equals_the_host_rule(pkg, device, cornell_scene, case, rule):
    kw, before, render_out, count_ok = STAGE_CASES[case]
    pool, live, budget = kw.get("pool", POOL), kw.get("live", 0) or kw.get("pool", POOL), kw.get("budget", 0)
    lens, proj = rule_args(pkg, rule)
    plain, blurred, sh = stage_pair(pkg, device, cornell_scene, kw, before, render_out, lens, proj)
    n_new = min(int(blurred[3][0]), live)
    q, slots = check_stage(pkg, plain, blurred, sh, pool, live, budget, lens, proj)
    print("%s / %s: new-path count %d, fresh after the guards %d, lastPathCnt %d" % (case, rule, n_new, q.size, int(blurred[3][1])))
    assert count_ok(n_new), n_new
    if case == "budget_retires_part":
        assert q.size == 2500 and slots.size < n_new
    if case == "tile_origin_7_5":
        xy = LU.state_screen(blurred[1], pool)[slots]
        assert xy[:, 0].min() == 7 and xy[:, 1].min() == 5 and xy[:, 0].max() == 17 and xy[:, 1].max() == 10
    if q.size and rule in ("pinhole", "lens"):
        o, _ = LU.state_rays(blurred[1], pool)
        o0, _ = LU.state_rays(plain[1], pool)
        assert (np.abs(o[slots] - o0[slots]).max(axis=1) > 0).mean() > 0.95, "the origins did move"


@pytest.mark.parametrize("plan", ["identity", "rectangle"])
@pytest.mark.parametrize("rule", ["pinhole", "lens"])
def test_stage_follows_an_attached_sampling_plan(pkg, device, cornell_scene, plan, rule):
    """k_ad_retarget first, then the shutter on the pixels it stored: an identity plan (every pixel once, row-major) and the rectangle
    plan of the adaptive tests, which moves the paths."""
    lens, proj = rule_args(pkg, rule)
    lst = AU.rect_list(W, 0, 0, W, H) if plan == "identity" else AU.rect_list(W, *RECT)
    plain, blurred, sh = stage_pair(pkg, device, cornell_scene, dict(), 2, False, lens, proj, plan_list=lst)
    q, slots = check_stage(pkg, plain, blurred, sh, POOL, POOL, 0, lens, proj)
    xy = LU.state_screen(blurred[1], POOL)[slots]
    x0, y0, w, h = (0, 0, W, H) if plan == "identity" else RECT
    assert q.size > 0 and ((xy[:, 0] >= x0) & (xy[:, 0] < x0 + w) & (xy[:, 1] >= y0) & (xy[:, 1] < y0 + h)).all(), "the plan's pixels"


@pytest.mark.parametrize("rule", ["pinhole", "lens"])
@pytest.mark.parametrize("tile", [None, (4, 3, 20, 12)], ids=["frame", "tile"])
def test_whole_iterations_equal_the_patched_stages(pkg, device, shipped_kernel, cornell_scene, tile, rule):
    """A: a shutter attached, gmupt_iterate.  B: no shutter; per iteration the shipped shading stage (with the rule's own launch), the
    host rule patched into the fresh slots through the debug access, the shipped ray casts.  Equal after 1, 2 and 24 iterations in
    every word."""
    capi = pkg.capi
    pool = POOL if tile is None else 1024
    lens, proj = rule_args(pkg, rule)
    sh = shutter_of(pkg, cornell_scene)
    a, sba, cama = make(pkg, device, cornell_scene, tile=tile, pool=pool)
    b, sbb, camb = make(pkg, device, cornell_scene, tile=tile, pool=pool)
    attach_rule(pkg, a, lens, proj); attach_rule(pkg, b, lens, proj)
    capi.shutter.set_shutter(a, sh)
    moved = 0
    for it in range(1, 25):
        step(a, cama, 1)
        camb.update(0.0); b.set_camera(camb.buffer); b.run_stage(capi.STAGE_SHADE)
        raw, queues, qc = b.read_path_state(), b.read_queues(), b.counters()
        q, slots = LU.fresh(qc, queues, pool)
        if q.size:
            b.write_path_state(LU.patch_rays(raw, pool, slots, SU.host_rays(capi, camb.buffer_copy(), sh, raw, pool, q, slots, lens, proj)))
            moved += q.size
        b.run_stage(capi.STAGE_RAYCASTS)
        if it in (1, 2, 24):
            assert same(snapshot(a), snapshot(b)), "iteration %d" % it
    assert moved > pool and int(a.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    close(a, sba, cama, b, sbb, camb)


def test_detached_resized_and_identity_are_the_plain_renderer(pkg, device, shipped_kernel, cornell_scene):
    capi = pkg.capi
    S = capi.shutter
    sh = shutter_of(pkg, cornell_scene)

    def run(prepare, resize=False):
        r, sb, cam = make(pkg, device, cornell_scene)
        prepare(r, cam)
        if resize:
            r.resize(24, 12); cam.update_resolution(24, 12)
        step(r, cam, 12)
        out = snapshot(r), S.get_shutter(r)
        close(r, sb, cam)
        return out

    def attach_and_detach(r, cam):
        S.set_shutter(r, sh)
        S.set_shutter(r, None)

    def identity(r, cam):
        c = capi.Camera(W, H); c.set_pose(*cornell_scene["camera"]); c.update(0.0)
        assert not SU.has_negative_zero(c.buffer)
        S.set_shutter(r, S.from_camera(c.buffer_copy()))
        c.close()

    plain, none = run(lambda r, cam: None)
    assert none is None and int(plain[0][..., 3].view(np.uint32).sum()) > 0
    got, attached = run(attach_and_detach)
    assert same(plain, got) and attached is None
    got, attached = run(identity)
    assert same(plain, got) and attached is not None, "a close pose equal to the camera's stays attached and changes nothing"
    got, attached = run(lambda r, cam: S.set_shutter(r, sh))
    assert not same(plain, got) and bytes(attached) == bytes(sh), "a shutter does change the frame, and survives gmupt_set_camera"
    resized, _ = run(lambda r, cam: None, resize=True)
    got, attached = run(lambda r, cam: S.set_shutter(r, sh), resize=True)
    assert same(resized, got) and attached is None, "gmupt_resize detaches"


def test_life_cycle_and_errors(pkg, device, cornell_scene):
    capi = pkg.capi
    S, lib = capi.shutter, capi.lib()
    r, sb, cam = make(pkg, device, cornell_scene)
    sh = shutter_of(pkg, cornell_scene)
    assert S.get_shutter(r) is None
    step(r, cam, 3)
    before = r.framebuffer()
    S.set_shutter(r, sh)
    r.synchronize()
    assert np.array_equal(LU.bits(before), LU.bits(r.framebuffer())), "setting a shutter does not clear the frame"
    assert bytes(S.get_shutter(r)) == bytes(sh)
    # lens and projection refuse each other exactly as without a shutter, and either may come and go while it is attached
    capi.lens.set_lens(r, lens_of(pkg))
    assert lib.gmupt_renderer_set_projection(r.h, C.byref(capi.projection.equirect())) == capi.ERR_UNSUPPORTED
    capi.lens.set_lens(r, None)
    capi.projection.set_projection(r, capi.projection.equirect())
    assert lib.gmupt_renderer_set_lens(r.h, C.byref(lens_of(pkg))) == capi.ERR_UNSUPPORTED
    capi.projection.set_projection(r, None)
    # every stated error leaves the attached shutter as it was
    for name in SU.VECTORS:
        for bad in (float("nan"), float("inf")):
            b = S.Shutter.from_buffer_copy(bytes(sh))
            getattr(b, name)[1] = bad
            assert lib.gmupt_renderer_set_shutter(r.h, C.byref(b)) == capi.ERR_INVALID_ARGUMENT and b"gmupt_renderer_set_shutter" in lib.gmupt_last_error()
    out, flag = S.Shutter(), C.c_int(-3)
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    assert lib.gmupt_renderer_get_shutter(r.h, None, C.byref(flag)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_renderer_get_shutter(r.h, C.byref(out), None) == capi.ERR_INVALID_ARGUMENT
    assert bytes(out) == b"\xab" * 48 and flag.value == -3 and bytes(S.get_shutter(r)) == bytes(sh)
    step(r, cam, 2)
    assert bytes(S.get_shutter(r)) == bytes(sh), "survives gmupt_set_camera"
    r.resize(24, 12); cam.update_resolution(24, 12)
    assert S.get_shutter(r) is None, "gmupt_resize detaches"
    step(r, cam, 2)
    close(r, sb, cam)


BLUR_POSE = (0.0, 5.0, 2.0, -20.0, 270.0)      # inside the room at half its height, two fifths of the way in, looking 20 degrees down at the boxes
BLUR_SHIFT = 0.2                               # sideways (x) across the shutter: a median of 7 changed pixels in the rows that change


def blur_figures(pkg, device, scene, pose, shift, spp, K=16, Wd=64, Hd=36, pools=(4096, 3072)):
    """The renders and figures of the image-level check for a camera at `pose` that moves `shift` in x across the shutter.  pools: the
    pool sizes of A, B and C, and of C' (another pool size is another assignment of seeds to pixels)."""
    capi = pkg.capi
    S = capi.shutter
    sb = capi.SceneBuffers(device, scene)
    sh = shutter_of(pkg, scene, (Wd, Hd), (pose[0] + shift,) + tuple(pose[1:]))

    def setup(pool, n):
        r = capi.Renderer(device, Wd, Hd, pool_paths=pool, path_budget=Wd * Hd * n)
        r.bind_scene(sb)
        cam = capi.Camera(Wd, Hd); cam.set_pose(*pose); cam.buffer.lightCount = scene["light_count"]
        return r, cam

    def frame_of(r, n):
        fb = r.framebuffer()
        assert np.all(fb[..., 3].view(np.uint32) == n)
        return np.minimum(fb[..., :3].astype(np.float64), 4.0)

    def render(pool, shutter):
        r, cam = setup(pool, spp)
        if shutter is not None:
            S.set_shutter(r, shutter)
        r.render_budget(cam, 100000)
        out = frame_of(r, spp)
        close(r, cam)
        return out

    def camera_at(cam, t):
        cam.update(0.0)
        return S.camera_host(cam.buffer_copy(), sh, t)

    def triangles_at(t):
        r, cam = setup(pools[0], 1)
        r.set_camera(camera_at(cam, t))
        tri = capi.aov_fields(r.aovs(1))["triangle"].copy()
        close(r, cam)
        return tri

    def render_at(t):
        r, cam = setup(pools[0], spp // K)
        for it in range(100000):
            r.set_camera(camera_at(cam, t)); r.iterate()
            if it % 16 == 15 and np.all(r.framebuffer()[..., 3].view(np.uint32) == spp // K):
                break
        out = frame_of(r, spp // K)
        close(r, cam)
        return out

    # the moving-edge pixels, from the pinhole AOVs at the two ends alone
    edge = triangles_at(0.0) != triangles_at(1.0)
    per_row = edge.sum(axis=1)
    A = render(pools[0], sh)
    Bm = np.mean([render_at((k + 0.5) / K) for k in range(K)], axis=0)
    Cs = render(pools[0], None)
    Co = render(pools[1], None)
    sb.close()
    mad = lambda a, b: float(np.abs(a - b)[edge].mean())
    n = mad(Cs, Co)
    return dict(pixels=int(edge.sum()), per_row=float(np.median(per_row[per_row > 0])) if edge.any() else 0.0, ab=mad(A, Bm), ac=mad(A, Cs), n=n,
                margin=3.0 * n / np.sqrt(max(int(edge.sum()), 1)))


def test_motion_blur_is_the_mean_of_the_fixed_time_renders(pkg, device, cornell_scene):
    """Cornell 64 x 36, the camera translating sideways across the shutter.  A: the shutter render at M = 256 spp.  B: the mean of 16
    renders at fixed times t = (k + 0.5) / 16 through gmupt_shutter_camera_host, 16 spp each.  C: the static render at t = 0, 256 spp;
    C': the same with other seeds (another pool size), the noise n = mean |C - C'|.  Every frame is the mean of its per-sample
    tone-mapped values (clamped at 4, as the depth-of-field test), so A and B estimate the same image: a pure translation is
    interpolated exactly.  Over the moving-edge pixels -- those whose t = 0 and t = 1 pinhole AOVs see another triangle (or none) --
    mean |A - B| <= n + margin and mean |A - C| > n + margin, margin = 3 n / sqrt(pixels) as in
    test_depth_of_field_blurs_the_near_field_not_the_focal_plane.  That the view has moving edges is asserted from the AOVs alone,
    before a beauty figure is looked at: in the rows that change at all, the median number of changed pixels is at least 3.
    Measured on the MI355X, this view: 270 moving-edge pixels, a median of 7 per changed row; mean |A - B| 0.01103 and mean |A - C|
    0.13968 against n 0.01492 + margin 0.00272 = 0.01764.  C' takes its other seeds from another pool size (3072 against 4096), which
    assigns the generator's draws to other pixels; the camera's seed pairs are the same sequence.
    The view.  The second bound compares the noise of a blurred pixel with that of a static one, and it does not hold in every view:
    a pixel that an edge sweeps across takes each sample from one of two surfaces, a variance that a static pixel away from an edge
    does not have, so |A - B| (noise, not a bias: four times the samples halve it together with n) grows against n with the contrast
    across the edge and with the length of the blur.  The first view tried, the depth-of-field test's (-3.5, 8, 7) with a shift of 0.4,
    where the rim of the red wall crosses the dark environment, missed it (0.01453 against 0.00875 + 0.00127), as did two inside
    views.  A grid of 72 poses inside and in front of the room at shifts 0.3 and 0.6 then gave ratios of mean |A - B| to n + margin
    from 0.84 to 1.42, most above 1 and lower at the shorter shift; five poses were measured again at shifts 0.1 to 0.3 with three
    seed assignments each (other pool sizes).  This pose held the bound in all twelve of those runs (0.49 to 0.84) while mean |A - C|
    stayed 6.6 to 7.9 times the limit; the four other poses were above 1 in 39 of their 48 runs.  It is not the lowest single
    figure of the grid but the one that did not depend on the seeds.  DESIGN.md "Shutter" has the table.
    What the check can see (a limit).  With mean |A - B| at 0.63 of its limit here, the second bound has about 40 % of slack: it
    catches a shutter whose times miss a large part of [0, 1) or pile up at one end, not a subtle skew of the draw.  The statistics of
    the draw are tests/test_shutter_cpu.py's, the rays the bit-for-bit tests' above."""
    f = blur_figures(pkg, device, cornell_scene, BLUR_POSE, BLUR_SHIFT, 256)
    print("motion blur, Cornell 64x36 at 256 spp, pose %r shifted %.2f in x: %d moving-edge pixels (median %.1f per changed row); mean |A - B| %.5f, "
          "mean |A - C| %.5f, noise mean |C - C'| %.5f, margin %.5f" % (BLUR_POSE, BLUR_SHIFT, f["pixels"], f["per_row"], f["ab"], f["ac"], f["n"], f["margin"]))
    assert f["pixels"] > 50 and f["per_row"] >= 3, f
    assert f["ab"] <= f["n"] + f["margin"], f
    assert f["ac"] > f["n"] + f["margin"], f


def test_session_set_shutter_restarts_and_keeps_the_history(pkg, device, cornell_scene):
    capi = pkg.capi
    S = capi.shutter
    r, sb, cam = make(pkg, device, cornell_scene)
    s = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    s.run(6)
    s.denoised_temporal()
    history = s.temporal
    dropped = []
    history_reset, history.reset = history.reset, lambda: dropped.append(1)
    before = int(r.framebuffer()[..., 3].view(np.uint32).max())
    c = capi.Camera(W, H); c.set_pose(*CLOSE_POSE(cornell_scene)); c.update(0.0)
    sh = s.set_shutter(c)
    assert bytes(S.get_shutter(r)) == bytes(S.from_camera(c.buffer_copy())) == bytes(sh)
    c.close()
    s.run(1)
    r.synchronize()
    assert cam.buffer.iterationCounter == 0, "the frame after set_shutter clears the target"
    s.run(3)
    after = int(r.framebuffer()[..., 3].view(np.uint32).max())
    assert before > 1 and 0 < after <= before
    assert s.temporal is history and not dropped, "the temporal history is kept"
    history.reset = history_reset
    img = s.denoised_temporal()
    assert img.shape == (H, W, 4) and np.isfinite(img[..., :3]).all() and float(img[..., :3].max()) > 0
    with pytest.raises(ValueError):
        s.set_shutter(c, fraction=0.5)
    with pytest.raises(ValueError):
        s.set_shutter(fraction=0.0)
    assert s.set_shutter() is None and S.get_shutter(r) is None
    # fraction: on a camera event the close pose trails the camera by f of the way back to the previous pose, and is then held
    s.set_shutter(fraction=0.5)
    s.run(2)
    first = cam.buffer_copy()
    assert S.get_shutter(r) is None, "no camera event yet: nothing attached, the frames of a session without a shutter"
    s.move_camera(d=True)
    s.frame(0.1)
    now = cam.buffer_copy()
    want = S.from_camera(now)
    f = LU.F(0.5)
    for name in SU.VECTORS:
        a, b = np.array(getattr(now, name)[:3], LU.F), np.array(getattr(first, name)[:3], LU.F)
        getattr(want, name)[:] = [float(x) for x in (a + ((b - a).astype(LU.F) * f).astype(LU.F)).astype(LU.F)]
    assert list(now.position)[:3] != list(first.position)[:3] and bytes(S.get_shutter(r)) == bytes(want)
    s.move_camera()
    s.run(3)
    assert list(cam.buffer.position)[:3] == list(now.position)[:3] and bytes(S.get_shutter(r)) == bytes(want), "held until the next camera event"
    s.resize(24, 12)
    assert S.get_shutter(r) is None
    s.run(2)
    assert S.get_shutter(r) is None, "after a resize there is no previous pose of that aspect until the camera moves again"
    s.close()
    close(r, sb, cam)

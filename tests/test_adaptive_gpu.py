"""GPU tests of adaptive sampling (gmupt_adaptive_*, csrc/pt_adaptive.hip): the device selection against its host rule bit for bit on the
crafted planes of the CPU test; the re-aim kernel held to the renderer itself -- an identity plan leaves a render as it was, a
rectangle plan on the full frame equals the tile renderer of that rectangle (which other tests hold against the oracle), an arbitrary
plan puts exactly the counted number of samples on every pixel --; starvation, the life cycle of an attached plan, and the loops that
plan as they go.  Cornell at 32 x 18 with a pool of 4096, or synthetic planes."""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import adaptive_util as AU

pytestmark = pytest.mark.gpu

W, H, POOL = 32, 18, 4096
RECT = (7, 5, 11, 6)
RECT_EDGE = (21, 12, 11, 6)      # touches the last row and the last column


@pytest.fixture(params=["wide", "cast0"])
def shipped_kernel(request, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", request.param)
    return request.param


def make(pkg, device, scene, tile=None, budget=0, pool=POOL):
    """tile: (x0, y0, w, h) of a tile renderer of the W x H frame."""
    sb = pkg.capi.SceneBuffers(device, scene)
    if tile is None:
        r = pkg.capi.Renderer(device, W, H, pool_paths=pool, path_budget=budget)
    else:
        r = pkg.capi.Renderer(device, tile[2], tile[3], pool_paths=pool, tile=(tile[0], tile[1]), path_budget=budget)
    r.bind_scene(sb)
    cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return r, sb, cam


def step(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()


def counts(fb):
    return fb[..., 3].view(np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def screen_coords(r):
    """(pool, 2) uint32: F_SCR_X, F_SCR_Y of every slot (structs.h: screenCoord at byte 236 of a path, fields stored one after the other)."""
    raw = r.read_path_state()
    return raw[236 * r.pool:244 * r.pool].view(np.uint32).reshape(r.pool, 2)


@pytest.fixture(scope="module")
def host_plans(pkg):
    """The host rule on every crafted plane, computed once."""
    out = {}
    for size in AU.SIZES:
        for mr in AU.MAX_REPEATS:
            planes = [AU.plane(size, mr, seed) for seed in range(2)] + list(AU.uniform_planes(size))
            out[(size, mr)] = [(e, pkg.capi.adaptive.adaptive_select_host(e, threshold=AU.T, max_repeat=mr)) for e in planes]
    return out


@pytest.mark.parametrize("max_repeat", AU.MAX_REPEATS)
@pytest.mark.parametrize("size", AU.SIZES, ids=lambda s: "%dx%d" % s)
def test_device_selection_equals_host(pkg, device, host_plans, size, max_repeat):
    r = pkg.capi.Renderer(device, 8, 8, pool_paths=1024)
    a = pkg.capi.adaptive.Adaptive(r)
    assert a.list().size == 0
    for e, (want_list, want_info) in host_plans[(size, max_repeat)]:
        info = a.select(torch.from_numpy(e).cuda(), threshold=AU.T, max_repeat=max_repeat, uniform_every=3)
        got = a.list()
        bad = AU.same(got, info, want_list, want_info)
        print("%dx%d max_repeat %d: entries %d active %d nonfinite %d max_rep %d ms %.4f" % (size + (max_repeat, info["entries"], info["active"],
                                                                                              info["skipped_nonfinite"], info["max_rep"], info["ms"])))
        assert not bad, (bad, info, want_info)
        assert info["ms"] > 0.0
    r.close()


def test_identity_plan_changes_nothing(pkg, device, shipped_kernel, cornell_scene):
    runs = []
    for planned in (False, True):
        r, sb, cam = make(pkg, device, cornell_scene)
        if planned:
            a = pkg.capi.adaptive.Adaptive(r)
            a.set_list(np.arange(W * H, dtype=np.uint32), W, H)
            pkg.capi.adaptive.set_adaptive(r, a)
        step(r, cam, 12)
        r.synchronize()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters()))
        r.close(); sb.close(); cam.close()
    (fa, sa, qa, ca), (fb, sb_, qb, cb) = runs
    assert int(counts(fa).sum()) > 0
    assert np.array_equal(bits(fa), bits(fb)) and np.array_equal(sa, sb_) and np.array_equal(qa, qb) and np.array_equal(ca, cb)


def _tile_frame(pkg, device, scene, rect, iterations):
    r, sb, cam = make(pkg, device, scene, tile=rect)
    step(r, cam, iterations)
    fb = r.framebuffer()
    r.close(); sb.close(); cam.close()
    return fb


@pytest.mark.parametrize("rect", [RECT, RECT_EDGE], ids=["inner", "edge"])
def test_rectangle_plan_equals_the_tile_renderer(pkg, device, cornell_scene, rect):
    x0, y0, w, h = rect
    want = _tile_frame(pkg, device, cornell_scene, rect, 12)
    assert int(counts(want).min()) > 0
    r, sb, cam = make(pkg, device, cornell_scene)
    a = pkg.capi.adaptive.Adaptive(r)
    a.set_list(AU.rect_list(W, x0, y0, w, h), W, H)
    pkg.capi.adaptive.set_adaptive(r, a)
    step(r, cam, 12)
    fb = r.framebuffer()
    inside = fb[y0:y0 + h, x0:x0 + w]
    assert np.array_equal(bits(inside), bits(want)), "the frame inside the rectangle is the tile renderer's"
    outside = counts(fb).copy(); outside[y0:y0 + h, x0:x0 + w] = 0
    assert not outside.any(), "no sample outside the rectangle"
    r.close(); sb.close(); cam.close()


def test_rectangle_plan_on_a_tile_renderer(pkg, device, cornell_scene):
    """A tile renderer of (4, 3) 20 x 12 whose plan is the sub-rectangle that is RECT in frame coordinates: tileX0 / tileY0."""
    x0, y0, w, h = RECT
    tile = (4, 3, 20, 12)
    want = _tile_frame(pkg, device, cornell_scene, RECT, 12)
    r, sb, cam = make(pkg, device, cornell_scene, tile=tile)
    a = pkg.capi.adaptive.Adaptive(r)
    lx, ly = x0 - tile[0], y0 - tile[1]
    a.set_list(AU.rect_list(tile[2], lx, ly, w, h), tile[2], tile[3])
    pkg.capi.adaptive.set_adaptive(r, a)
    step(r, cam, 12)
    fb = r.framebuffer()
    assert fb.shape == (12, 20, 4)
    assert np.array_equal(bits(fb[ly:ly + h, lx:lx + w]), bits(want))
    outside = counts(fb).copy(); outside[ly:ly + h, lx:lx + w] = 0
    assert not outside.any()
    r.close(); sb.close(); cam.close()


def test_arbitrary_plan_counts_are_exact(pkg, device, cornell_scene):
    """A list with repeats and uniform_every = 5 under a path budget: every path k < budget ends as one sample on the pixel the
    mapping gives it."""
    rng = np.random.default_rng(11)
    lst = np.concatenate([rng.integers(0, W * H, 90), np.full(7, 40), np.full(3, W * H - 1), [0]]).astype(np.uint32)
    budget = 3 * POOL + 17
    r, sb, cam = make(pkg, device, cornell_scene, budget=budget)
    a = pkg.capi.adaptive.Adaptive(r)
    a.set_list(lst, W, H, uniform_every=5)
    assert np.array_equal(a.list(), lst)
    pkg.capi.adaptive.set_adaptive(r, a)
    # one shading stage: the new-path queue holds every slot, and each was aimed by the mapping
    cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(pkg.capi.STAGE_SHADE)
    qc = r.counters()
    n_new = min(int(qc[0]), r.pool)
    assert n_new == POOL and int(qc[1]) == 0
    slots = r.read_queues()[0][:n_new]
    pix = AU.pixel_of(lst, 5, W, H, np.arange(n_new))
    got = screen_coords(r)[slots]
    assert np.array_equal(got[:, 0], pix % W) and np.array_equal(got[:, 1], pix // W)
    r.close(); sb.close(); cam.close()
    # the whole budget
    r, sb, cam = make(pkg, device, cornell_scene, budget=budget)
    a = pkg.capi.adaptive.Adaptive(r)
    a.set_list(lst, W, H, uniform_every=5)
    pkg.capi.adaptive.set_adaptive(r, a)
    r.render_budget(cam)
    got = counts(r.framebuffer()).reshape(-1)
    want = np.bincount(AU.pixel_of(lst, 5, W, H, np.arange(budget)), minlength=W * H)
    print("budget %d: %d samples on %d pixels, most %d" % (budget, int(got.sum()), int((got > 0).sum()), int(got.max())))
    assert int(want.sum()) == budget and np.array_equal(got, want)
    r.close(); sb.close(); cam.close()


def test_life_cycle_of_an_attached_plan(pkg, device, cornell_scene):
    capi = pkg.capi
    r, sb, cam = make(pkg, device, cornell_scene)
    a = capi.adaptive.Adaptive(r)
    a.set_list(AU.rect_list(W, *RECT), W, H)
    pkg.capi.adaptive.set_adaptive(r, a)
    step(r, cam, 6)
    r.synchronize()
    snap = (r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters())
    pkg.capi.adaptive.set_adaptive(r, None)
    cams = []
    for _ in range(6):
        cam.update(0.0); cams.append(cam.buffer_copy()); r.set_camera(cams[-1]); r.iterate()
    after = (r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters())
    outside = counts(after[0]).copy(); outside[RECT[1]:RECT[1] + RECT[3], RECT[0]:RECT[0] + RECT[2]] = 0
    assert outside.any(), "detached: the paths go everywhere again"
    # a second renderer brought to the state at the detach continues the same way without ever having had a plan
    r2, sb2, _cam2 = make(pkg, device, cornell_scene)
    r2.write_framebuffer(snap[0]); r2.write_path_state(snap[1]); r2.write_queues(snap[2]); r2.write_counters(snap[3])
    for cb in cams:
        r2.set_camera(cb); r2.iterate()
    plain = (r2.framebuffer(), r2.read_path_state(), r2.read_queues(), r2.counters())
    assert np.array_equal(bits(after[0]), bits(plain[0])) and all(np.array_equal(x, y) for x, y in zip(after[1:], plain[1:]))
    r2.close(); sb2.close(); _cam2.close()
    # a plan for another rectangle is refused before anything is launched
    a.set_list([0, 1, 2], 8, 8)
    pkg.capi.adaptive.set_adaptive(r, a)
    before = (r.counters(), r.read_path_state())
    with pytest.raises(capi.GmuptError) as e:
        step(r, cam, 1)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "sampling plan" in str(e.value)
    assert np.array_equal(r.counters(), before[0]) and np.array_equal(r.read_path_state(), before[1])
    # gmupt_resize detaches: the plan for 8 x 8 would be refused again otherwise
    r.resize(24, 12); cam.update_resolution(24, 12)
    step(r, cam, 2)
    # destroying an attached plan detaches it first
    a.set_list(np.arange(24 * 12, dtype=np.uint32), 24, 12)
    pkg.capi.adaptive.set_adaptive(r, a)
    step(r, cam, 1)
    a.close()
    step(r, cam, 2)
    r.synchronize()
    assert int(counts(r.framebuffer()).sum()) > 0
    # refusals of the handle's own entry points leave the plan as it was
    b = capi.adaptive.Adaptive(r)
    b.set_list([5, 6], 24, 12)
    lib = capi.lib()
    bad = np.array([1, 24 * 12], np.uint32)
    assert lib.gmupt_adaptive_set_list(b.h, bad.ctypes.data_as(C.c_void_p), 2, 24, 12, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_set_list(b.h, None, 2, 24, 12, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_set_list(b.h, bad.ctypes.data_as(C.c_void_p), 1, 0, 12, 0) == capi.ERR_INVALID_ARGUMENT
    info = capi.adaptive.AdaptiveInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    was = bytes(info)
    e = torch.zeros(24 * 12 + 1, dtype=torch.float32, device="cuda")
    ok, none = capi.adaptive.adaptive_params(threshold=0.01), capi.adaptive.adaptive_params()
    assert lib.gmupt_adaptive_select(b.h, C.c_void_p(e.data_ptr() + 2), 24, 12, C.byref(ok), C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_select(b.h, C.c_void_p(e.data_ptr()), 24, 12, C.byref(none), C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_select(b.h, C.c_void_p(e.data_ptr()), 24, 12, C.byref(ok), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_select(b.h, None, 24, 12, C.byref(ok), C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    small = np.zeros(1, np.uint32)
    assert lib.gmupt_adaptive_read_list(b.h, small.ctypes.data_as(C.c_void_p), 4, None) == capi.ERR_INVALID_ARGUMENT
    other = capi.Renderer(device, 8, 8, pool_paths=1024)
    assert lib.gmupt_renderer_set_adaptive(other.h, b.h) == capi.ERR_INVALID_ARGUMENT
    other.close()
    assert bytes(info) == was and small[0] == 0 and b.list().tolist() == [5, 6]
    r.close(); sb.close(); cam.close()


def _threshold(pkg, device, scene):
    """What a uniform render reaches after 64 iterations: (max_error, pixels that never become known)."""
    r, sb, cam = make(pkg, device, scene)
    c = pkg.capi.Converge(r)
    for _ in range(8):
        step(r, cam, 8); info = c.update()
    r.close(); sb.close(); cam.close()
    return info["max_error"], info["pixels"] - info["known"]


def test_render_adaptive_end_to_end(pkg, device, shipped_kernel, cornell_scene):
    """render_until and render_adaptive both stop converged on the threshold a uniform run reaches in 64 iterations; the same loop
    spelled out check by check shows that a pixel with rep = 0 gets no new path until the next check (uniform_every = 0), and ends on
    the frame render_adaptive ends on.
    Starvation in integers.  Between two iterations every slot of the pool holds one path whose sample is not accumulated yet, aimed
    at the pixel in its screen coordinate.  So for every pixel, count(next check) - count(check) = in flight at the check + paths
    aimed at it in between - in flight at the next check, and for a pixel with rep = 0 the middle term is 0: an exact identity, held
    here.  "The same count bits at the next check" holds as it stands only for the rep = 0 pixels with nothing in flight at the check;
    it is asserted for those.  For the others it cannot hold in a renderer that keeps a pool of paths alive (DESIGN.md
    "Adaptive sampling", paths in flight, has the figures of this run; the test prints those of every check)."""
    capi = pkg.capi
    threshold, unknown = _threshold(pkg, device, cornell_scene)
    assert threshold > 0
    prm = dict(threshold=threshold, allow_pixels=unknown)
    r, sb, cam = make(pkg, device, cornell_scene)
    c = capi.Converge(r)
    uni = r.render_until(cam, c, check_every=8, max_iterations=4096, **prm)
    uni_paths = r.stats().paths_generated
    r.close(); sb.close(); cam.close()
    r, sb, cam = make(pkg, device, cornell_scene)
    c, a = capi.Converge(r), capi.adaptive.Adaptive(r)
    ada = capi.adaptive.render_adaptive(r, cam, c, a, check_every=8, max_iterations=4096, max_repeat=8, **prm)
    ada_paths = r.stats().paths_generated
    ada_frame = r.framebuffer()
    # attached plans are gone when the loop returns
    before = counts(ada_frame).copy()
    r.close(); sb.close(); cam.close()
    print("uniform: %d iterations, %d paths; adaptive: %d iterations, %d paths, ratio %.4f; last plan %r" % (
        uni["iterations"], uni_paths, ada["iterations"], ada_paths, ada_paths / uni_paths, ada["plan"]))
    assert uni["converged"] and ada["converged"] and ada["iterations"] % 8 == 0 and ada["iterations"] < 4096
    assert ada["plan"]["pixels"] == W * H and 0 < ada["plan"]["active"] < W * H and ada["plan"]["entries"] >= ada["plan"]["active"]
    # the loop check by check
    r, sb, cam = make(pkg, device, cornell_scene)
    c, a = capi.Converge(r), capi.adaptive.Adaptive(r)
    starved_checks = 0
    last, rep, flying = None, None, None
    exact_idle = 0
    for check in range(ada["iterations"] // 8):
        step(r, cam, 8)
        info, err = c.update(error=True, **prm)
        r.synchronize()
        now = counts(r.framebuffer()).reshape(-1).copy()
        xy = screen_coords(r).astype(np.int64)
        flying_now = np.bincount(xy[:, 1] * W + xy[:, 0], minlength=W * H)
        assert int(flying_now.sum()) == POOL
        if rep is not None:
            idle = rep == 0
            gained = now.astype(np.int64) - last
            if idle.any():
                print("check %d: %d pixels with rep = 0 had %d .. %d samples and gained %d .. %d from paths in flight" % (
                    check, int(idle.sum()), int(last[idle].min()), int(last[idle].max()), int(gained[idle].min()), int(gained[idle].max())))
            assert np.array_equal(gained[idle], (flying - flying_now)[idle]), "check %d: a new path went to a pixel with rep = 0" % check
            assert (gained[~idle] > (flying - flying_now)[~idle]).any(), "the others did get new paths"
            still = idle & (flying == 0)
            assert np.array_equal(now[still], last[still]), "check %d: a pixel with rep = 0 and nothing in flight was sampled" % check
            exact_idle += int(still.sum())
            starved_checks += int(idle.any())
        if info["converged"]:
            break
        plan = a.select(err, threshold=threshold, max_repeat=8)
        want_list, want_info = capi.adaptive.adaptive_select_host(err.cpu().numpy(), threshold=threshold, max_repeat=8)
        assert not AU.same(a.list(), plan, want_list, want_info)
        pkg.capi.adaptive.set_adaptive(r, a)
        rep, last, flying = (AU.reps(err.cpu().numpy(), threshold, 8) if plan["entries"] else None), now, flying_now
    print("checks with starved pixels: %d; rep = 0 pixels with nothing in flight, summed over the checks: %d" % (starved_checks, exact_idle))
    assert info["converged"] and check == ada["iterations"] // 8 - 1 and starved_checks > 0
    assert np.array_equal(bits(r.framebuffer()), bits(ada_frame)), "render_adaptive is this loop"
    assert np.array_equal(counts(r.framebuffer()), before)
    r.close(); sb.close(); cam.close()


def test_session_run_until_adaptive(pkg, device, cornell_scene):
    threshold, unknown = _threshold(pkg, device, cornell_scene)
    r, sb, cam = make(pkg, device, cornell_scene)
    s = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    out = s.run_until(threshold, check_every=8, max_frames=4096, allow_pixels=unknown, adaptive=True, max_repeat=8, uniform_every=16)
    print("run_until(adaptive): %d frames, plan %r" % (out["frames"], out.get("plan")))
    assert out["converged"] and 16 <= out["frames"] < 4096 and out["plan"]["entries"] > 0
    s.resize(24, 12)
    s.run(2)            # a plan left attached would be refused at the new size
    s.close()
    r.close(); sb.close(); cam.close()

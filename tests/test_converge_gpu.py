"""GPU tests of the convergence monitor (gmupt_converge_*, csrc/pt_converge.hip): the device against its host reference
gmupt_converge_host bit for bit -- on the crafted frame sequences of the CPU test, written into the accumulation target and given as
torch tensors, on the wide-range sequences that show the order of the sum and the seams of the reduction (one run, 256 partials, a
second level of one entry, four levels), and on real renders with both shipped ray casts --, restart detection, the renderer left untouched, and the loops that
stop on the estimate (gmupt_render_until, ProgressiveSession.run_until).  A word that is NaN on the host may be any NaN on the device,
fenced per field to the same words (the shade_util.compare convention)."""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (update_image takes torch tensors)

import converge_util as CU

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["wide", "cast0"])
def shipped_kernel(request, monkeypatch):
    """The tests that render run with both shipped fused ray casts: "wide" (the default) and "cast0"."""
    monkeypatch.setenv("GMUPT_TRAVERSAL", request.param)
    return request.param


@pytest.fixture(scope="module")
def chains(pkg):
    """The crafted sequences and the host reference of every update, computed once."""
    out = {}
    for W, H in CU.SIZES:
        frames = CU.crafted_frames(W, H, seed=W * 1000 + H)
        out[(W, H)] = (frames, CU.host_chain(pkg.capi, frames))
    return out


def make(pkg, device, scene, W, H, rows=None, y0=0, pool=4096):
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, rows if rows is not None else H, pool_paths=pool, tile=(0, y0) if rows is not None else None)
    r.bind_scene(sb)
    cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return r, sb, cam


def step(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()


def check(got_state, got_err, got_info, want, what):
    state, err, info = want
    bad = CU.differing(got_state, got_err, got_info, state, err, info, fence=True)
    print("%s: known %d below %d nonfinite %d max %.6g sum %.17g ms %.4f" % (what, got_info["known"], got_info["below"], got_info["nonfinite"],
                                                                        got_info["max_error"], got_info["sum_error"], got_info["ms"]))
    assert not bad, (what, bad, got_info, info)
    assert got_info["ms"] > 0.0


@pytest.mark.parametrize("size", CU.SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_on_crafted_frames(pkg, device, chains, size):
    """The same sequence twice: through the accumulation target (gmupt_debug_write_framebuffer + update) and as torch tensors
    (update_image); the error plane is asked for on every other update, so that both shapes of the launch are compared."""
    W, H = size
    frames, want = chains[size]
    r = pkg.capi.Renderer(device, W, H, pool_paths=1024)
    a, b = pkg.capi.Converge(r), pkg.capi.Converge(r)
    assert a.state().size == 0
    for u, f in enumerate(frames):
        prm = CU.PARAMS[u % len(CU.PARAMS)]
        r.write_framebuffer(f)
        info, err = a.update(error=True, **prm)
        check(a.state(), err.cpu().numpy(), info, want[u], "target %dx%d update %d" % (W, H, u))
        t = torch.from_numpy(f).cuda()
        if u % 2:
            info, err = b.update_image(t, error=True, **prm)
            err = err.cpu().numpy()
        else:
            info, err = b.update_image(t, **prm), want[u][1]
        check(b.state(), err, info, want[u], "tensor %dx%d update %d" % (W, H, u))
    # reset: the next update sees every pixel for the first time
    a.reset()
    assert not a.state().view(np.uint8).any()
    info = a.update()
    assert info["known"] == 0 and (a.state()["k"] <= 1).all()
    r.close()


@pytest.mark.parametrize("variant", CU.VARIANTS)
@pytest.mark.parametrize("size", CU.SEAM_SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_at_the_seams(pkg, device, size, variant):
    """The wide-range sequences (converge_util.py): the errors span 40 binades, so a sum in another order than the rule's -- atomics,
    wave first, neighbours first -- has other bits; the special pixels sit on both sides of every stride of the block reduction in
    the first, a middle and the last run and around the seam of the second level; in the "carrier" variant max_error is held by one
    pixel at such a place, another one at every update.  test_converge_cpu.py checks on the numpy restatement that the frames do show
    all this, and the host reference against the restatement on the same frames."""
    W, H = size
    frames = CU.wide_sequence(size, variant)
    want = CU.host_chain(pkg.capi, frames)
    r = pkg.capi.Renderer(device, 8, 8, pool_paths=1024)
    c = pkg.capi.Converge(r)
    for u, f in enumerate(frames):
        prm = CU.PARAMS[u % len(CU.PARAMS)]
        t = torch.from_numpy(f).cuda()
        if u % 2:
            info, err = c.update_image(t, error=True, **prm)
            err = err.cpu().numpy()
        else:
            info, err = c.update_image(t, **prm), want[u][1]
        check(c.state(), err, info, want[u], "%s %dx%d update %d" % (variant, W, H, u))
    assert info["pixels"] == W * H and (W * H == 1 or info["known"] > info["nonfinite"] > 0)
    r.close()


def test_four_levels_equal_host(pkg, device):
    """4097 x 4096 = 16 781 312 pixels = 256^3 + 4 096: 65 552 partials, then 257, then 2, then 1 -- the smallest frames with a fourth
    level are just above 256^3 pixels, and an 8K frame (33 M) has one.  Two successive read-outs of the 257 x 257 wide-range sequence,
    tiled and cropped; the special pixels of a run of that sequence are copied to the last run (65 551: entry 15 of the last run of the
    second level, entry 0 of the last run of the third) and to runs 65 535 and 65 536 (the two sides of the seam of the second AND of
    the third level); the pixel before the last one holds the largest error.  Device against gmupt_converge_host; the numpy restatement
    is not run at this size."""
    import time
    t0 = time.time()
    W, H = 4097, 4096
    N = W * H
    tile = CU.wide_sequence((257, 257), "specials")[1:3]     # update 1 -> 2: the NaN and inf colours, 0xFFFFFFFE and the drop to 0 arrive
    source = CU.run_places(257 * 257, 0)
    frames = []
    for v, f in enumerate(tile):
        big = np.ascontiguousarray(np.tile(f, (16, 16, 1))[:H, :W])
        flat = big.reshape(-1, 4)
        for shift, run in ((0, 65535), (3, 65536), (6, 65551)):
            assert (run + 1) * 256 <= N
            for q, p in enumerate(CU.run_places(N, run)):
                flat[p] = f.reshape(-1, 4)[source[(q + shift) % len(source)]]
        flat[N - 2, :3] = np.array((0.25, 0.5, 0.75) if v else (0.75, 0.5, 0.25), np.float32) * np.float32(2.0 ** 44)
        flat[N - 2, 3:] = np.array([3 * (v + 1)], np.uint32).view(np.float32)
        frames.append(big)
    state = np.zeros((H, W), pkg.capi.converge_pixel_dtype)
    r = pkg.capi.Renderer(device, 8, 8, pool_paths=1024)
    c = pkg.capi.Converge(r)
    t1 = time.time()
    for v, f in enumerate(frames):
        prm = CU.PARAMS[1 + v]
        want_info, want_err = pkg.capi.converge_host(state, f, error=True, **prm)
        t = torch.from_numpy(f).cuda()
        if v:
            info, err = c.update_image(t, error=True, **prm)
            err = err.cpu().numpy()
        else:
            info, err = c.update_image(t, **prm), want_err
        del t
        bad = CU.differing(c.state() if v else state, err, info, state, want_err, want_info, fence=True)   # the state once, after both updates
        print("four levels, update %d: known %d nonfinite %d max %.6g sum %.17g ms %.4f" % (v, info["known"], info["nonfinite"], info["max_error"],
                                                                                      info["sum_error"], info["ms"]))
        assert not bad, (v, bad, info, want_info)
    e = want_err.reshape(-1)
    finite = np.isfinite(e) & (e != -1.0)
    assert info["pixels"] == 16781312 and info["known"] > 0
    assert int(np.argmax(np.where(finite, e, -1.0))) == N - 2 and int((e == e[N - 2]).sum()) == 1 and info["max_error"] == e[N - 2]
    assert not np.isfinite(e[[65535 * 256 + 255, 65536 * 256, N - 1]]).any() and info["nonfinite"] > 8
    print("four levels: %.2f s building the frames, %.2f s host rule, device and comparison" % (t1 - t0, time.time() - t1))
    r.close()


def test_a_count_that_drops_to_zero_through_the_target(pkg, device):
    """Counts 5, 9, 0, 0, 4, 8 through gmupt_debug_write_framebuffer + gmupt_converge_update: at the drop the pixel restarts and has no
    new samples (bsz == 0), and its zeroed state must still be stored although nothing was folded in."""
    pixels = [0, 20, 63]
    frames = CU.wide_range_frames(8, 8, 3, kinds={p: "zero" for p in pixels})
    want = CU.host_chain(pkg.capi, frames)
    r = pkg.capi.Renderer(device, 8, 8, pool_paths=1024)
    c = pkg.capi.Converge(r)
    for u, f in enumerate(frames):
        r.write_framebuffer(f)
        info, err = c.update(error=True, **CU.PARAMS[u % len(CU.PARAMS)])
        state = c.state()
        check(state, err.cpu().numpy(), info, want[u], "zero count, update %d" % u)
        rec = state.reshape(-1)[pixels]
        if u == 1:
            assert (rec["n"] == 9).all() and (rec["k"] == 2).all() and (rec["m2"] > 0).all()
        if u in (2, 3):
            assert not rec.view(np.uint8).any() and (err.cpu().numpy().reshape(-1)[pixels] == -1.0).all()
            assert info["unsampled"] == int((np.arange(64) % 11 == 0).sum()) + 2       # pixel 0 never has a sample in the plain frames either
        if u == 5:
            assert (rec["n"] == 8).all() and (rec["k"] == 2).all() and (rec["w"] == 8).all()
    r.close()


def test_one_monitor_follows_a_change_of_image_size(pkg, device, chains):
    r = pkg.capi.Renderer(device, 8, 8, pool_paths=1024)
    c = pkg.capi.Converge(r)
    for size in (CU.SIZES[1], CU.SIZES[0], CU.SIZES[1]):
        frames, want = chains[size]
        for u in range(3):
            info, err = c.update_image(torch.from_numpy(frames[u]).cuda(), error=True, **CU.PARAMS[u])
            check(c.state(), err.cpu().numpy(), info, want[u], "size %r update %d" % (size, u))
    r.close()


@pytest.mark.parametrize("tile", [False, True], ids=["frame", "tile14"])
def test_real_render_equals_host(pkg, device, shipped_kernel, cornell_scene, tile):
    W, H = 32, 18
    r, sb, cam = make(pkg, device, cornell_scene, W, H, rows=14 if tile else None, y0=4)
    c = pkg.capi.Converge(r)
    state = np.zeros((r.height, W), pkg.capi.converge_pixel_dtype)
    for u in range(5):
        step(r, cam, 8)
        prm = CU.PARAMS[u % len(CU.PARAMS)]
        info, err = c.update(error=True, **prm)
        fb = r.framebuffer()
        want_info, want_err = pkg.capi.converge_host(state, fb, error=True, **prm)
        check(c.state(), err.cpu().numpy(), info, (state, want_err, want_info), "render update %d" % u)
    assert info["pixels"] == W * r.height and info["known"] > 0 and 0 < info["max_error"] < 1 and info["nonfinite"] == 0
    r.close(); sb.close(); cam.close()


def test_restarts_are_detected_in_a_render(pkg, device, shipped_kernel, cornell_scene):
    """A camera reset re-accumulates from zero; 24 iterations later most counts have passed the 8 iterations' worth the monitor last
    saw, so the counts alone would not show it.  gmupt_resize replaces the target."""
    W, H = 32, 18
    r, sb, cam = make(pkg, device, cornell_scene, W, H)
    c = pkg.capi.Converge(r)
    for _ in range(2):
        step(r, cam, 4); c.update()
    assert c.update()["known"] > 0
    cam.reset_accumulation()
    step(r, cam, 24)
    info = c.update()
    st = c.state()
    assert info["known"] == 0 and (st["k"] <= 1).all() and (st["n"] == st["w"]).all()
    assert np.array_equal(st["n"], r.framebuffer()[..., 3].view(np.uint32)), "one batch that holds everything accumulated since the reset"
    step(r, cam, 4)
    assert c.update()["known"] > 0
    r.resize(48, 27); cam.update_resolution(48, 27)
    step(r, cam, 4)
    info = c.update()
    assert info["pixels"] == 48 * 27 and info["known"] == 0 and c.state().shape == (27, 48)
    # without an event in between nothing restarts
    step(r, cam, 4)
    assert c.update()["known"] > 0
    r.close(); sb.close(); cam.close()


def test_a_render_with_updates_leaves_the_renderer_untouched(pkg, device, shipped_kernel, cornell_scene):
    W, H, P = 48, 27, 4096
    runs = []
    for with_updates in (False, True):
        r, sb, cam = make(pkg, device, cornell_scene, W, H, pool=P)
        c = pkg.capi.Converge(r)
        for it in range(12):
            step(r, cam, 1)
            if with_updates and it % 3 == 1:
                c.update(error=True, threshold=0.05)
        r.synchronize()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), r.stats().as_dict(), r.read_travtables()))
        r.close(); sb.close(); cam.close()
    (fa, sa, qa, ca, ta, va), (fb, sbb, qb, cb, tb, vb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb and all(np.array_equal(va[k], vb[k]) for k in va)
    assert int(fa[..., 3].view(np.uint32).sum()) > 0


def test_render_until_stops_on_the_estimate(pkg, device, shipped_kernel, cornell_scene):
    W, H = 32, 18
    # the threshold: what the same scene reaches after 64 iterations
    r, sb, cam = make(pkg, device, cornell_scene, W, H)
    c = pkg.capi.Converge(r)
    for _ in range(8):
        step(r, cam, 8); first = c.update()
    threshold = first["max_error"]
    unknown = first["pixels"] - first["known"]
    print("after 64 iterations: max_error %.6g, mean_error %.6g, %d of %d pixels known" % (threshold, first["mean_error"], first["known"], first["pixels"]))
    assert threshold > 0 and first["known"] > 0
    assert unknown == first["unsampled"], "only pixels that never got a sample stay unknown after eight batches"
    r.close(); sb.close(); cam.close()
    # the loop stops before max_iterations (pixels that never become known -- nothing is ever accumulated there -- are allowed for)
    r, sb, cam = make(pkg, device, cornell_scene, W, H)
    c = pkg.capi.Converge(r)
    info = r.render_until(cam, c, check_every=8, max_iterations=4096, threshold=threshold, allow_pixels=unknown)
    print("render_until: %d iterations, below %d of %d, max_error %.6g" % (info["iterations"], info["below"], info["pixels"], info["max_error"]))
    assert info["converged"] and 16 <= info["iterations"] < 4096 and info["iterations"] % 8 == 0
    assert info["pixels"] - info["below"] <= unknown
    # threshold 0: to max_iterations
    info = r.render_until(cam, c, check_every=8, max_iterations=40, threshold=0.0)
    assert not info["converged"] and info["iterations"] == 40 and info["pixels"] == W * H
    # no check ran: the info stays zero
    assert r.render_until(cam, c, check_every=8, max_iterations=3)["pixels"] == 0
    # the session's loop does the same on the real renderer
    cam.reset_accumulation()
    s = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    out = s.run_until(threshold, check_every=8, max_frames=4096, allow_pixels=unknown)
    print("run_until: %d frames, max_error %.6g" % (out["frames"], out["max_error"]))
    assert out["converged"] and 16 <= out["frames"] < 4096 and s.frames == out["frames"]
    out = s.run_until(0.0, check_every=8, max_frames=24)
    assert not out["converged"] and out["frames"] == 24
    s.close()
    # refusals
    lib = pkg.capi.lib()
    ci = pkg.capi.ConvergeInfo()
    C.memset(C.byref(ci), 0xAB, C.sizeof(ci))
    before = bytes(ci)
    n = C.c_uint32(77)
    prm = pkg.capi.converge_params()
    assert lib.gmupt_render_until(r.h, cam.h, c.h, C.byref(prm), 0, 8, C.byref(n), C.byref(ci)) == pkg.capi.ERR_INVALID_ARGUMENT
    assert b"check_every" in lib.gmupt_last_error() and n.value == 77 and bytes(ci) == before
    few = pkg.capi.converge_params(min_batches=1)
    assert lib.gmupt_render_until(r.h, cam.h, c.h, C.byref(few), 8, 8, C.byref(n), C.byref(ci)) == pkg.capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_update(c.h, C.byref(few), None, C.byref(ci)) == pkg.capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_update(c.h, C.byref(prm), C.c_void_p(2), C.byref(ci)) == pkg.capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_update(c.h, C.byref(prm), None, None) == pkg.capi.ERR_INVALID_ARGUMENT
    img = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    assert lib.gmupt_converge_update_image(c.h, C.c_void_p(img.data_ptr() + 4), 2, 2, C.byref(prm), None, C.byref(ci)) == pkg.capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_update_image(c.h, C.c_void_p(img.data_ptr()), 0, 2, C.byref(prm), None, C.byref(ci)) == pkg.capi.ERR_INVALID_ARGUMENT
    small = np.zeros(4, pkg.capi.converge_pixel_dtype)
    assert lib.gmupt_converge_read_state(c.h, small.ctypes.data_as(C.c_void_p), small.nbytes) == pkg.capi.ERR_INVALID_ARGUMENT
    assert bytes(ci) == before and n.value == 77 and not small.view(np.uint8).any()
    assert c.state().shape == (H, W), "the refused calls left the monitor as it was"
    r.close(); sb.close(); cam.close()

"""GPU tests of motion-aware temporal reuse (include/gmupt.h, "motion"): k_mv_resolve against gmupt_motion_host, the AOV output against
gmupt_render_aovs, k_tp_integrate_mv and the handle's pose bookkeeping against the host chain (gmupt_motion_host ->
gmupt_temporal_integrate_motion_host -> gmupt_denoise_host), all bit for bit; isolation; the session; and the quality on an animation."""
import json
import os

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

from test_temporal_gpu import SPATIAL, assert_same, bits, make_camera, moved, surface_mask

pytestmark = pytest.mark.gpu

# MSE(spatial only) / MSE(motion-aware) on the last frame of the animation of test_quality_on_an_animation.  Measured: 2.29 (MSE 0.111190
# -> 0.048476); 60 % of that is below the floor of 1.5, which is therefore the threshold.
QUALITY_GAIN = 1.5


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def scenes(pkg):
    return {"soup": pkg.scenes.build_scene(pkg.scenes.random_triangles_mesh(2000, seed=1)),
            "cornell": pkg.scenes.build_scene(pkg.scenes.cornell_mesh()),
            "textured": pkg.scenes.build_scene(pkg.scenes.textured_mesh())}


def centre_hits(pkg, r, cam_buffer, W, H, x0=0, y0=0, pixels=None):
    """The gmupt_hit records of the centre rays (k = 0 of gmupt_aov_ray) through gmupt_trace_rays: the AOV's own hits."""
    if pixels is None:
        ys, xs = np.mgrid[y0:y0 + H, x0:x0 + W]
        xs, ys = xs.ravel(), ys.ravel()
    else:
        xs, ys = pixels
    rays = pkg.capi.aov_rays(cam_buffer, xs, ys, 1)[:, 0, :]
    return r.trace(closest=rays, light_count=int(cam_buffer.lightCount))[0]


def host_motion(pkg, r, scene, cam_buffer, aov, now, prev, W, H, x0=0, y0=0):
    hits = centre_hits(pkg, r, cam_buffer, W, H, x0, y0)
    return pkg.capi.motion_host(hits, aov.cpu().numpy(), scene["tris"], now, prev).reshape(H, W)


# ---------------------------------------------------------------------------------------------------- 5: the motion plane
@pytest.mark.parametrize("name", ["cornell", "textured", "soup"])
def test_motion_plane_matches_the_host_rule(pkg, device, wide, scenes, name):
    capi, scene = pkg.capi, scenes[name]
    W, H = 96, 54
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=2048)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    r.set_camera(cam.buffer)
    prev = scene["verts"]
    moved_some = 0
    for phase in (0.0, 0.3, 0.7):
        now = pkg.scenes.wobble(scene, phase, 0.05)
        sb.verts.update(now); r.refit()
        pv = torch.from_numpy(prev).cuda()
        for s in (1, 2, 3):
            aov, mv = r.aovs_motion(pv, s)
            assert_same(aov, r.aovs(s), (name, phase, s, "the AOV output is gmupt_render_aovs'"))
            want = host_motion(pkg, r, scene, cam.buffer, aov, now, prev, W, H)
            assert_same(mv, want.view(np.float32).reshape(H, W, 4), (name, phase, s, "motion plane"))
        f = capi.motion_fields(mv)
        surf = surface_mask(aov)
        assert np.array_equal(f["flags"], surf.astype(np.uint32))
        if phase == 0.0:
            assert np.array_equal(bits(f["prev_position"])[surf], bits(aov.cpu().numpy()[..., 8:11])[surf]), "nothing moved: bit for bit"
        else:
            moved_some += int((f["prev_position"] != aov.cpu().numpy()[..., 8:11]).any(-1).sum())
        prev = now
    assert moved_some > W * H // 8
    with pytest.raises(capi.GmuptError) as e:
        r.aovs_motion(torch.from_numpy(prev[:-1].copy()).cuda(), 1)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    r.close(); sb.close(); cam.close()


def test_motion_plane_in_chunks_and_tiles(pkg, device, wide, scenes):
    """s = 8 at 512 px per row is 33 280 rays per row: 63 rows per chunk, several chunks; and tiles of the frame."""
    capi, scene = pkg.capi, scenes["textured"]
    prev, now = scene["verts"], pkg.scenes.wobble(scenes["textured"], 0.3, 0.05)
    sb = capi.SceneBuffers(device, scene)
    for (FW, FH, x0, y0, tw, th, s) in [(512, 160, 0, 0, 512, 160, 8), (96, 54, 17, 5, 30, 11, 2), (96, 54, 0, 20, 96, 18, 1)]:
        r = capi.Renderer(device, tw, th, pool_paths=2048, tile=None if (tw, th) == (FW, FH) else (x0, y0))
        r.bind_scene(sb)
        sb.verts.update(now); r.refit()
        cam = make_camera(pkg, scene, FW, FH)
        r.set_camera(cam.buffer)
        aov, mv = r.aovs_motion(torch.from_numpy(prev).cuda(), s)
        assert_same(aov, r.aovs(s), ("aov", tw, th, s))
        want = host_motion(pkg, r, scene, cam.buffer, aov, now, prev, tw, th, x0, y0)
        assert_same(mv, want.view(np.float32).reshape(th, tw, 4), ("motion", tw, th, s))
        assert (want["flags"] == 1).mean() > 0.2
        r.close(); cam.close()
    sb.close()


def test_motion_plane_of_the_bench_scene(pkg, device, wide):
    """1920x1080 on the bench scene: the whole plane's flags against the AOV records, and 65 536 pixels against the host rule."""
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    W, H = 1920, 1080
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=1 << 16)
    r.bind_scene(sb)
    prev, now = scene["verts"], pkg.scenes.wobble(scene, 0.3, 0.01)
    sb.verts.update(now); r.refit()
    cam = make_camera(pkg, scene, W, H)
    r.set_camera(cam.buffer)
    aov, mv = r.aovs_motion(torch.from_numpy(prev).cuda(), 1)
    assert_same(aov, r.aovs(1), "aov")
    assert np.array_equal(capi.motion_fields(mv)["flags"], surface_mask(aov).astype(np.uint32))
    rng = np.random.default_rng(5)
    idx = rng.choice(W * H, 65536, replace=False)
    xs, ys = idx % W, idx // W
    hits = centre_hits(pkg, r, cam.buffer, W, H, pixels=(xs, ys))
    want = capi.motion_host(hits, aov.cpu().numpy()[ys, xs], scene["tris"], now, prev)
    got = mv.cpu().numpy()[ys, xs]
    assert np.array_equal(bits(got), want.view(np.uint32).reshape(-1, 4))
    assert (want["flags"] == 1).mean() > 0.3
    r.close(); sb.close(); cam.close()


# ---------------------------------------------------------------------------------------------------- 6: the handle against the host chain
class MotionChain:
    """The handle's semantics on the host: two record sets, each with camera, origin, vertex pose and geometry generation; a fold swaps
    them; a set of another generation than the renderer's is integrated against through the motion plane of its pose."""

    def __init__(self, pkg, scene):
        self.pkg, self.capi, self.scene, self.frozen, self.last = pkg, pkg.capi, scene, None, None
        self.used_motion = 0

    def call(self, r, cam, verts, gen, new, s, origin=(0, 0), **params):
        if new:
            self.frozen, self.last = self.last, self.frozen
        beauty, aov = r.framebuffer(), r.aovs(s)
        H, W = beauty.shape[:2]
        mv, prev = None, (None, None, (0, 0))
        if self.frozen:
            prev = self.frozen[:3]
            if self.frozen[4] != gen:
                mv = host_motion(self.pkg, r, self.scene, cam, aov, verts, self.frozen[3], W, H, *origin)
                self.used_motion += 1
        integrated, hist = self.capi.temporal_integrate_motion_host(beauty, aov, mv, *prev, **params)
        self.last = (hist, cam, origin, verts, gen)
        return self.capi.denoise_host(integrated, aov, **{k: v for k, v in params.items() if k in SPATIAL})


def test_animation_matches_the_host_chain(pkg, device, wide, scenes):
    """Seven refits with calls inside and across accumulations, a camera move, a resize, and a refit with no call in between."""
    capi, scene = pkg.capi, scenes["textured"]
    W, H = 64, 36
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=2048)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    chain = MotionChain(pkg, scene)
    cam = make_camera(pkg, scene, W, H)
    state = {"verts": scene["verts"], "gen": 0}

    def frames(n):
        for _ in range(n):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()

    def refit(phase, restart=True):
        state["verts"] = pkg.scenes.wobble(scene, phase, 0.03); state["gen"] += 1
        sb.verts.update(state["verts"]); assert r.refit()["rebuilt"] == 0
        if restart:
            cam.reset_accumulation()

    def check(new, what, s=1, **params):
        got = r.denoise_temporal_motion(t, s, **params)
        assert_same(got, chain.call(r, cam.buffer_copy(), state["verts"], state["gen"], new, s, **params), what)
        return got

    frames(4); check(True, "first call")
    refit(0.1); frames(3); check(True, "after refit 1")
    assert chain.used_motion == 1
    frames(2); check(False, "same accumulation, frozen set of the old pose", s=2)
    assert chain.used_motion == 2
    refit(0.2, restart=False); frames(1); check(False, "refit 2 inside an accumulation")
    refit(0.3); cam.set_pose(*moved(scene["camera"], yaw=2.0)); frames(3); check(True, "refit 3 with a camera move", passes=3)
    refit(0.4); frames(2)                                     # no call at this pose
    refit(0.5); frames(2); check(True, "refits 4 and 5 without a call in between: the snapshot is the frozen set's")
    r.resize(80, 45); cam.update_resolution(80, 45)
    frames(2); c = check(True, "after a resize")
    assert c.shape == (45, 80, 4)
    refit(0.6); frames(2); got = check(True, "refit 6 after the resize")
    assert chain.used_motion >= 6
    assert (bits(got)[..., 3] != bits(r.framebuffer())[..., 3]).mean() > 0.2, "the history is used"
    # the image entry with a caller's motion plane
    refit(0.7); frames(2)
    aov, mv = r.aovs_motion(torch.from_numpy(chain.last[3]).cuda(), 1)
    got = capi.temporal_denoise_image(t, torch.from_numpy(r.framebuffer()).cuda(), aov, cam.buffer_copy(), True, motion=mv)
    chain.frozen, chain.last = chain.last, chain.frozen
    integrated, hist = capi.temporal_integrate_motion_host(r.framebuffer(), aov, mv, *chain.frozen[:3])
    assert_same(got, capi.denoise_host(integrated, aov), "gmupt_temporal_denoise_image_motion")
    # reset: the spatial denoise again
    t.reset()
    assert_same(r.denoise_temporal_motion(t, 1), r.denoise(1), "after a reset")
    r.close(); sb.close(); cam.close()


# ---------------------------------------------------------------------------------------------------- 7: equal generation
def test_equal_generation_is_the_plain_temporal_call(pkg, device, wide, scenes):
    capi, scene = pkg.capi, scenes["cornell"]
    W, H = 48, 27
    sb = capi.SceneBuffers(device, scene)
    outs = []
    for variant in ("plain", "motion", "motion_refit_unchanged"):
        r = capi.Renderer(device, W, H, pool_paths=2048)
        r.bind_scene(sb)
        t = capi.Temporal(r)
        cam = make_camera(pkg, scene, W, H)
        call = r.denoise_temporal if variant == "plain" else r.denoise_temporal_motion
        got = []
        for it in range(12):
            if it == 5:
                cam.set_pose(*moved(scene["camera"], yaw=3.0)); cam.reset_accumulation()
                if variant == "motion_refit_unchanged":
                    r.refit()
            if it == 9:
                r.resize(40, 30); cam.update_resolution(40, 30)
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if it % 2 == 1:
                got.append(call(t, 1 + it % 3).cpu().numpy())
        outs.append(got)
        r.close(); cam.close()
    sb.close()
    for k, (a, b, c) in enumerate(zip(*outs)):
        assert np.array_equal(bits(a), bits(b)), ("no refit", k)
        assert np.array_equal(bits(a), bits(c)), ("a refit with unchanged vertices", k)


# ---------------------------------------------------------------------------------------------------- 8: isolation, snapshots
def test_motion_calls_leave_the_renderer_untouched(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H, P = 48, 27, 4096
    runs = []
    for with_motion in (False, True):
        sb = pkg.capi.SceneBuffers(device, scene)
        r = pkg.capi.Renderer(device, W, H, pool_paths=P)
        r.bind_scene(sb)
        t = pkg.capi.Temporal(r)
        cam = make_camera(pkg, scene, W, H)
        for it in range(12):
            if it == 6:
                sb.verts.update(pkg.scenes.wobble(scene, 0.3, 0.03)); r.refit(); cam.reset_accumulation()
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if with_motion and it % 3 == 1:
                r.denoise_temporal_motion(t, 1); r.denoise_temporal_motion(t, 2, passes=2)
                r.aovs_motion(torch.from_numpy(scene["verts"]).cuda(), 1)
        r.synchronize()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), r.stats().as_dict()))
        r.close(); cam.close(); sb.close()
    (fa, sa, qa, ca, ta), (fb, sbb, qb, cb, tb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb


def test_snapshots_do_not_grow_and_are_freed(pkg, device, wide):
    """A mesh whose snapshot is large enough to see (4 M vertices = 48 MB): 50 refit + call rounds keep two snapshots, reset frees them."""
    capi = pkg.capi
    base = pkg.scenes.build_scene(pkg.scenes.cornell_mesh())
    nv = len(base["verts"])
    scene = dict(base)
    pad = 4_000_000
    scene["verts"] = np.concatenate([base["verts"], np.zeros((pad, 3), np.float32)])      # vertices no triangle uses
    scene["props"] = np.concatenate([base["props"], np.zeros(pad, base["props"].dtype)])
    W, H = 32, 18
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=1024)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    cam = make_camera(pkg, scene, W, H)
    snap = scene["verts"].nbytes

    def round_(k):
        v = scene["verts"].copy(); v[:nv] = pkg.scenes.wobble(base, (k % 10) / 10.0, 0.02)
        sb.verts.update(v); r.refit(); cam.reset_accumulation()
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        r.denoise_temporal_motion(t, 1)

    for k in range(3):
        round_(k)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for k in range(3, 53):
        round_(k)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < snap // 2, "50 rounds allocate no further snapshot (%d bytes gone)" % (free0 - free1)
    t.reset()
    free2 = torch.cuda.mem_get_info()[0]
    assert free2 - free1 > snap, "reset frees both snapshots (%d bytes back, one snapshot is %d)" % (free2 - free1, snap)
    round_(0); round_(1)
    t.close()
    free3 = torch.cuda.mem_get_info()[0]
    assert free3 >= free2 - snap // 2, "destroy frees them too"
    r.close(); sb.close(); cam.close()


# ---------------------------------------------------------------------------------------------------- 9: the session
def test_session_keeps_the_history_across_set_vertices(pkg, device, wide, scenes):
    capi, scene = pkg.capi, scenes["cornell"]
    W, H = 48, 27
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=512)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    sess.set_vertices(sb, pkg.scenes.wobble(scene, 0.05, 0.03), keep_history=True)
    sess.run(12)
    sess.denoised_temporal()
    sess.set_vertices(sb, pkg.scenes.wobble(scene, 0.1, 0.03), keep_history=True)
    assert cam.buffer.iterationCounter == -1, "the accumulation restarts"
    sess.run(2)
    kept, spatial = sess.denoised_temporal(), sess.denoised()
    assert not np.array_equal(kept.view(np.uint32)[..., :3], spatial.view(np.uint32)[..., :3]), "the history is kept"
    surf = surface_mask(r.aovs(1))
    assert (surf & (kept[..., :3].max(-1) == 0)).sum() < (surf & (spatial[..., :3].max(-1) == 0)).sum()
    # the default still drops it
    sess.set_vertices(sb, pkg.scenes.wobble(scene, 0.15, 0.03))
    sess.run(2)
    assert np.array_equal(sess.denoised_temporal().view(np.uint32)[..., :3], sess.denoised().view(np.uint32)[..., :3])
    r.close(); sb.close(); cam.close()


# ---------------------------------------------------------------------------------------------------- 10: quality
def test_quality_on_an_animation(pkg, device, wide, scenes):
    """Cornell 96x54, 12 wobble frames of phase step 0.01 (amplitude 0.05), 3 iterations of a 512-path pool each; reference: 1024 spp of
    the last pose.  Arms on the last frame: (A) the spatial denoise, (B) the motion-aware call, (C) the plain temporal call kept across
    the refits.  Measured on the MI355X (profiles/motion/motion_quality.json, DESIGN.md "Motion"): MSE A 0.111190, B 0.048476, C 0.069528, gain
    A / B 2.29; of the 4975 surface pixels without a sample of the last frame, 4694 show history in B, 3117 in C (and 1427 are not
    black in A: the frame holds colour there from paths that were in flight at the restart).  60 % of the gain is 1.38, so the
    threshold is the floor, 1.5."""
    capi, scene = pkg.capi, scenes["cornell"]
    W, H, N, ITERS = 96, 54, 12, 3
    pose = lambda k: pkg.scenes.wobble(scene, 0.01 * (k + 1), 0.05)
    sb_ref = capi.SceneBuffers(device, pkg.scenes.refit_scene(scene, pose(N - 1)))
    rr = capi.Renderer(device, W, H, pool_paths=1 << 16, path_budget=W * H * 1024)
    rr.bind_scene(sb_ref)
    cr = capi.Camera(W, H); cr.set_pose(*scene["camera"]); cr.buffer.lightCount = scene["light_count"]
    rr.render_budget(cr, 1 << 20)
    ref = rr.framebuffer()
    assert np.all(ref[..., 3].view(np.uint32) == 1024)
    rr.close(); cr.close(); sb_ref.close()

    out = {}
    for arm in ("B", "C"):
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, W, H, pool_paths=512)
        r.bind_scene(sb)
        t = capi.Temporal(r)
        cam = make_camera(pkg, scene, W, H)
        call = r.denoise_temporal_motion if arm == "B" else r.denoise_temporal
        for k in range(N):
            sb.verts.update(pose(k)); r.refit(); cam.reset_accumulation()
            for _ in range(ITERS):
                cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            out[arm] = call(t, 2).cpu().numpy()
        if arm == "B":
            out["A"] = r.denoise(2).cpu().numpy()
            fb, surf = r.framebuffer(), surface_mask(r.aovs(2))
        r.close(); sb.close(); cam.close()
    mse = {k: float(((v[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean()) for k, v in out.items()}
    zero = surf & (fb[..., 3].view(np.uint32) == 0)
    filled = {k: int((zero & (out[k][..., :3].max(-1) > 0)).sum()) for k in "ABC"}
    result = {"scene": "cornell", "width": W, "height": H, "frames": N, "iterations_per_frame": ITERS, "mse": mse,
              "gain_A_over_B": mse["A"] / mse["B"], "surface_pixels_without_sample": int(zero.sum()), "of_them_not_black": filled}
    print("motion quality: " + json.dumps(result))
    if os.environ.get("GMUPT_MOTION_QUALITY_JSON"):
        with open(os.environ["GMUPT_MOTION_QUALITY_JSON"], "w") as f:
            json.dump(result, f, indent=1)
    assert mse["B"] < mse["A"] and mse["B"] <= mse["C"], mse
    assert mse["A"] / mse["B"] >= QUALITY_GAIN, mse
    assert zero.sum() > W * H // 4 and filled["B"] > 0.5 * zero.sum() and filled["B"] > filled["A"] and filled["B"] >= filled["C"], (int(zero.sum()), filled)


def test_session_preview_before_the_first_keep_history(pkg, device, wide, scenes):
    """preview -> set_vertices(keep_history=True) -> preview: the record sets of the plain entry point carry no pose, so they are dropped
    once (the spatial denoise, not a static reprojection onto the moved surface); from then on the history is kept.  A session made
    with motion=True previews through the motion entry point from the start and keeps the history across the first refit too."""
    capi, scene = pkg.capi, scenes["cornell"]
    W, H = 48, 27
    for from_start in (False, True):
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, W, H, pool_paths=512)
        r.bind_scene(sb)
        cam = make_camera(pkg, scene, W, H)
        sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0, motion=from_start)
        sess.run(12)
        sess.denoised_temporal()
        sess.set_vertices(sb, pkg.scenes.wobble(scene, 0.05, 0.03), keep_history=True)
        sess.run(2)
        first, spatial = sess.denoised_temporal(), sess.denoised()
        assert np.array_equal(first.view(np.uint32)[..., :3], spatial.view(np.uint32)[..., :3]) == (not from_start)
        sess.set_vertices(sb, pkg.scenes.wobble(scene, 0.1, 0.03), keep_history=True)
        sess.run(2)
        assert not np.array_equal(sess.denoised_temporal().view(np.uint32)[..., :3], sess.denoised().view(np.uint32)[..., :3]), "kept from then on"
        r.close(); sb.close(); cam.close()

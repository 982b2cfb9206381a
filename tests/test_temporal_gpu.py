"""GPU tests of temporal reuse: k_tp_integrate + the denoiser's launches (gmupt_temporal_denoise_image, gmupt_render_denoised_temporal)
against the host chain gmupt_temporal_integrate_host -> gmupt_denoise_host, bit for bit, the epoch rule of the two record sets, the
renderer left untouched, and the quality gain after a camera move.  The host integration itself is checked against a float64
restatement in test_temporal_cpu.py."""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

from test_temporal_cpu import BASE, camera, noisy_beauty, room_aov

pytestmark = pytest.mark.gpu

# MSE(spatial denoise of B) / MSE(temporal denoise of B given A) against B at 1024 spp; Cornell 96x54, A = the scene pose at 64 spp,
# B = A with yaw + 2 degrees at 2 spp, AOVs at s = 2, default parameters.  Measured: 4.72 (MSE 0.003178 -> 0.000673).
QUALITY_GAIN = 3.0
SPATIAL = ("passes", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo")


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def scenes(pkg):
    return {"soup": pkg.scenes.build_scene(pkg.scenes.random_triangles_mesh(2000, seed=1)),
            "cornell": pkg.scenes.build_scene(pkg.scenes.cornell_mesh()),
            "textured": pkg.scenes.build_scene(pkg.scenes.textured_mesh())}


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, exp, what):
    g, e = bits(got), bits(exp)
    bad = np.nonzero((g != e).any(axis=-1))
    assert len(bad[0]) == 0, "%s: %d pixels differ, first %r" % (what, len(bad[0]), tuple(int(b[0]) for b in bad))


class HostChain:
    """The handle's semantics on the host: two record sets, each with camera and origin; new_accumulation swaps them first."""

    def __init__(self, capi):
        self.capi, self.frozen, self.last = capi, None, None

    def call(self, beauty, aov, cam, origin, new_accumulation, **params):
        if new_accumulation:
            self.frozen, self.last = self.last, self.frozen
        prev = self.frozen or (None, None, (0, 0))
        integrated, hist = self.capi.temporal_integrate_host(beauty, aov, *prev, **params)
        self.last = (hist, cam, origin)
        self.integrated = integrated
        return self.capi.denoise_host(integrated, aov, **{k: v for k, v in params.items() if k in SPATIAL})

    def reset(self):
        self.frozen = self.last = None


def test_synthetic_sequences_match_the_host_chain(pkg, device):
    capi = pkg.capi
    r = capi.Renderer(device, 8, 8, pool_paths=1024)          # no scene needed: the renderer's stream and scratch
    t = capi.Temporal(r)
    chain = HostChain(capi)
    FW, FH = 96, 54
    poses = [BASE, (0.6, 1.5, 1.0, -5.0, 198.0), (0.4, 1.4, 1.2, -4.0, 203.0), (0.5, 1.6, 0.9, -6.0, 201.0)]
    # (pose, rectangle W, H, x0, y0, new_accumulation, params): sizes and origins change, so do the flags
    seq = [(0, 96, 54, 0, 0, 1, {}), (1, 96, 54, 0, 0, 1, {}), (2, 96, 54, 0, 0, 0, {"passes": 3}), (2, 70, 40, 13, 9, 1, {}),
           (3, 50, 30, 20, 12, 1, {"history_cap": 4.0, "min_normal_cos": 0.5, "plane_dist": 0.1}), (0, 96, 54, 0, 0, 0, {})]
    for k, (pi, W, H, x0, y0, new, params) in enumerate(seq):
        cam = camera(pkg, FW, FH, poses[pi])
        aov = room_aov(cam, W, H, x0, y0, seed=10 + k)
        beauty = noisy_beauty(W, H, 20 + k)
        ms = []
        got = capi.temporal_denoise_image(t, torch.from_numpy(beauty).cuda(), torch.from_numpy(aov).cuda(), cam, new, (x0, y0), ms=ms, **params)
        assert got.shape == (H, W, 4) and ms[0] > 0
        exp = chain.call(beauty, aov, cam, (x0, y0), new, **params)
        assert_same(got, exp, ("call", k))
        # consequence (b): the device output is the device denoiser on the integrated image
        assert_same(got, capi.denoise_image(r, torch.from_numpy(chain.integrated).cuda(), torch.from_numpy(aov).cuda(),
                                            **{k2: v for k2, v in params.items() if k2 in SPATIAL}), ("b", k))
        if k == 1:
            assert (bits(got)[..., 3] != bits(beauty)[..., 3]).mean() > 0.3, "the second call uses history"
    r.close()


def make_camera(pkg, scene, W, H, pose=None):
    cam = pkg.capi.Camera(W, H)
    cam.set_pose(*(pose or scene["camera"])); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    return cam


def moved(pose, yaw=0.0, dx=0.0):
    x, y, z, pitch, yw = pose
    return (x + dx, y, z, pitch, yw + yaw)


@pytest.mark.parametrize("name", ["cornell", "textured", "soup"])
@pytest.mark.parametrize("move", ["yaw", "translation"])
def test_rendered_pairs_match_the_host_chain(pkg, device, wide, scenes, name, move):
    capi = pkg.capi
    scene = scenes[name]
    W, H = 96, 54
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=4096)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    chain = HostChain(capi)
    pose = scene["camera"]
    for k, p in enumerate([pose, moved(pose, yaw=3.0) if move == "yaw" else moved(pose, dx=0.3), pose]):
        cam = make_camera(pkg, scene, W, H, p)
        cam.reset_accumulation()
        for _ in range(6 if k == 0 else 2):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        got = r.denoise_temporal(t, 2)
        exp = chain.call(r.framebuffer(), r.aovs(2), cam.buffer_copy(), (0, 0), True)
        assert_same(got, exp, (name, move, k))
        if k == 0:
            assert_same(got, r.denoise(2), "consequence (a): the first call is the spatial denoise")
        cam.close()
    r.close(); sb.close()


def test_tiles_keep_their_own_history(pkg, device, wide, scenes):
    capi = pkg.capi
    scene = scenes["textured"]
    W, H = 96, 54
    sb = capi.SceneBuffers(device, scene)
    for (x0, y0, tw, th) in [(0, 20, 96, 18), (17, 5, 30, 11)]:
        rt = capi.Renderer(device, tw, th, pool_paths=4096, tile=(x0, y0))
        rt.bind_scene(sb)
        t = capi.Temporal(rt)
        chain = HostChain(capi)
        for k, p in enumerate([scene["camera"], moved(scene["camera"], yaw=2.0)]):
            cam = make_camera(pkg, scene, W, H, p)
            cam.reset_accumulation()
            for _ in range(4):
                cam.update(0.0); rt.set_camera(cam.buffer); rt.iterate()
            got = rt.denoise_temporal(t, 1)
            assert got.shape == (th, tw, 4)
            assert_same(got, chain.call(rt.framebuffer(), rt.aovs(1), cam.buffer_copy(), (x0, y0), True), (x0, y0, k))
            cam.close()
        rt.close()
    sb.close()


def test_bench_scene_pair_matches_the_host_chain(pkg, device, wide):
    """1920x1080: the bench scene's AOVs at two poses (yaw + 2 degrees) with noisy beauty images made from their albedo."""
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    W, H = 1920, 1080
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=1 << 16)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    chain = HostChain(capi)
    rng = np.random.default_rng(3)
    for k, p in enumerate([scene["camera"], moved(scene["camera"], yaw=2.0)]):
        cam = make_camera(pkg, scene, W, H, p)
        r.set_camera(cam.buffer)
        aov = r.aovs(1)
        alb = aov.cpu().numpy()[..., 0:3]
        b = np.empty((H, W, 4), np.float32)
        b[..., :3] = np.clip(alb * 0.6 + rng.normal(0, 0.15, alb.shape), 0, 1)
        b[..., 3] = rng.integers(0, 3, (H, W)).astype(np.uint32).view(np.float32)
        got = capi.temporal_denoise_image(t, torch.from_numpy(b).cuda(), aov, cam.buffer_copy(), True)
        assert_same(got, chain.call(b, aov, cam.buffer_copy(), (0, 0), True), ("1920x1080", k))
        cam.close()
    assert (bits(got)[..., 3] != 0).mean() > 0.5
    r.close(); sb.close()


def test_epoch_rule(pkg, device, wide, scenes):
    """Folds happen at the first call after an iteration that cleared the frame, or after a resize; nowhere else."""
    capi = pkg.capi
    scene = scenes["textured"]
    W, H = 48, 27
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=2048)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    chain = HostChain(capi)
    cam = make_camera(pkg, scene, W, H)

    def frames(n):
        for _ in range(n):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()

    def check(new, what, s=1):
        got = r.denoise_temporal(t, s)
        assert_same(got, chain.call(r.framebuffer(), r.aovs(s), cam.buffer_copy(), (0, 0), new), what)
        return got

    frames(4)
    a = check(True, "first call")
    assert_same(r.denoise_temporal(t, 1), a, "no iteration in between: the same output")
    chain.call(r.framebuffer(), r.aovs(1), cam.buffer_copy(), (0, 0), False)
    frames(3)
    check(False, "iterations without a restart do not fold")
    cam.set_pose(*moved(scene["camera"], yaw=4.0)); cam.reset_accumulation()
    frames(2)
    b = check(True, "the restart folds once")
    assert (bits(b)[..., 3] != bits(r.framebuffer())[..., 3]).any(), "the new accumulation uses the old history"
    frames(2)
    check(False, "later iterations of the same accumulation do not fold again")
    check(False, "nor do repeated calls")
    # a resize folds, and the output uses the history of the old size
    r.resize(64, 36); cam.update_resolution(64, 36)
    frames(2)
    c = check(True, "gmupt_resize folds")
    assert c.shape == (36, 64, 4)
    assert (bits(c)[..., 3] != bits(r.framebuffer())[..., 3]).any(), "the resized frame uses the history"
    # reset: consequence (a)
    frames(1)
    t.reset(); chain.reset()
    assert_same(check(False, "after a reset"), r.denoise(1), "a reset gives the spatial denoise")
    assert_same(r.denoise_temporal(t, 1, history_cap=0.0), r.denoise(1), "history_cap = 0 gives the spatial denoise")
    r.close(); sb.close(); cam.close()


def test_temporal_calls_leave_the_renderer_untouched(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H, P = 48, 27, 4096
    sb = pkg.capi.SceneBuffers(device, scene)
    runs = []
    for with_temporal in (False, True):
        r = pkg.capi.Renderer(device, W, H, pool_paths=P)
        r.bind_scene(sb)
        t = pkg.capi.Temporal(r)
        cam = make_camera(pkg, scene, W, H)
        for it in range(12):
            if it == 6:
                cam.set_pose(*moved(scene["camera"], yaw=3.0)); cam.reset_accumulation()
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if with_temporal and it % 3 == 1:
                r.denoise_temporal(t, 1); r.denoise_temporal(t, 2, passes=2)
                pkg.capi.temporal_denoise_image(t, torch.from_numpy(r.framebuffer()).cuda(), r.aovs(1), cam.buffer_copy(), it == 7)
        r.synchronize()
        st = r.stats().as_dict()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), st))
        r.close(); cam.close()
    sb.close()
    (fa, sa, qa, ca, ta), (fb, sbb, qb, cb, tb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb


def test_errors(pkg, device, wide, scenes):
    capi = pkg.capi
    W, H = 32, 18
    r = capi.Renderer(device, W, H, pool_paths=1024)
    other = capi.Renderer(device, W, H, pool_paths=1024)
    t = capi.Temporal(r)
    with pytest.raises(capi.GmuptError) as e:
        r.denoise_temporal(t, 1)
    assert e.value.code == capi.ERR_NOT_BOUND
    with pytest.raises(capi.GmuptError, match="another renderer") as e:
        other.denoise_temporal(t, 1)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    sb = capi.SceneBuffers(device, scenes["cornell"])
    r.bind_scene(sb)
    cam = make_camera(pkg, scenes["cornell"], W, H)
    r.set_camera(cam.buffer)
    for bad in ({"history_cap": -1.0}, {"min_normal_cos": 2.0}, {"plane_dist": float("nan")}, {"passes": 0}):
        with pytest.raises(capi.GmuptError) as e:
            r.denoise_temporal(t, 1, **bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, bad
    bt = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.GmuptError):
        capi.temporal_denoise_image(t, bt, torch.zeros((H, W, 8), dtype=torch.float32, device="cuda"), cam.buffer_copy(), True)
    assert_same(r.denoise_temporal(t, 1), r.denoise(1), "still usable; the refused calls kept no records")
    other.close(); r.close(); sb.close(); cam.close()


def surface_mask(aov):
    f = aov.cpu().numpy().view(np.uint32) if hasattr(aov, "cpu") else aov.view(np.uint32)
    return (f[..., 12].view(np.int32) != -1) & (f[..., 14] == 0)


def test_quality_after_a_camera_move(pkg, device, wide, scenes):
    """Cornell 96x54: history from pose A at 64 spp helps pose B (yaw + 2 degrees) at 2 spp; pixels B has not reached yet show it."""
    capi = pkg.capi
    scene = scenes["cornell"]
    W, H = 96, 54
    sb = capi.SceneBuffers(device, scene)
    poseB = moved(scene["camera"], yaw=2.0)

    def render(spp, pose):
        r = capi.Renderer(device, W, H, pool_paths=min(1 << 16, W * H * spp // 2), path_budget=W * H * spp)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*pose); cam.buffer.lightCount = scene["light_count"]
        r.render_budget(cam, 1 << 20)
        fb = r.framebuffer()
        assert np.all(fb[..., 3].view(np.uint32) == spp)
        return r, cam, fb

    rr, cr, ref = render(1024, poseB)
    rr.close(); cr.close()
    ra, ca, fa = render(64, scene["camera"])
    aovA, camA = ra.aovs(2), ca.buffer_copy()
    ra.close(); ca.close()
    rb, cb, fbB = render(2, poseB)
    aovB, camB = rb.aovs(2), cb.buffer_copy()
    t = capi.Temporal(rb)
    capi.temporal_denoise_image(t, torch.from_numpy(fa).cuda(), aovA, camA, True)
    tem = capi.temporal_denoise_image(t, torch.from_numpy(fbB).cuda(), aovB, camB, True).cpu().numpy()
    spa = capi.denoise_image(rb, torch.from_numpy(fbB).cuda(), aovB).cpu().numpy()
    mse = lambda a: float(((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean())
    gain = mse(spa) / mse(tem)
    print("cornell %dx%d yaw +2: MSE spatial %.6f, temporal %.6f, gain %.2f" % (W, H, mse(spa), mse(tem), gain))
    assert gain >= QUALITY_GAIN, gain
    # a progressive start of B: few paths, most pixels without a sample yet
    rp = capi.Renderer(device, W, H, pool_paths=512)
    rp.bind_scene(sb)
    cp = make_camera(pkg, scene, W, H, poseB)
    for _ in range(3):
        cp.update(0.0); rp.set_camera(cp.buffer); rp.iterate()
    fp, aovP = rp.framebuffer(), rp.aovs(2)
    t.reset()
    capi.temporal_denoise_image(t, torch.from_numpy(fa).cuda(), aovA, camA, True)
    tp = capi.temporal_denoise_image(t, torch.from_numpy(fp).cuda(), aovP, cp.buffer_copy(), True).cpu().numpy()
    sp = capi.denoise_image(rp, torch.from_numpy(fp).cuda(), aovP).cpu().numpy()
    zero = surface_mask(aovP) & (fp[..., 3].view(np.uint32) == 0)
    consistent = zero & (tp[..., 3].view(np.uint32) > 0)
    print("progressive B: %d surface pixels without samples, %d with consistent history" % (zero.sum(), consistent.sum()))
    assert zero.sum() > W * H // 4 and consistent.sum() > 0.5 * zero.sum()
    assert np.all(sp[zero][:, :3] == 0), "the spatial filter leaves them black"
    assert np.all(tp[consistent][:, :3].max(-1) > 0), "temporal reuse fills them"
    rp.close(); cp.close(); rb.close(); cb.close(); sb.close()


def test_session_preview_under_motion(pkg, device, wide, scenes):
    """A session whose camera turns every frame: denoised_temporal leaves fewer black surface pixels than denoised; set_lights resets."""
    scene = scenes["cornell"]
    W, H = 64, 36
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=512)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    for _ in range(8):                                     # a converged start
        sess.frame()
    sess.denoised_temporal()
    black_s = black_t = 0
    for _ in range(16):
        sess.move_camera(mouse_dx=0.5)
        sess.frame()
        surf = surface_mask(r.aovs(1))
        s, t = sess.denoised(), sess.denoised_temporal()
        assert isinstance(t, np.ndarray) and t.shape == (H, W, 4) and t.dtype == np.float32
        black_s += int((surf & (s[..., :3].max(-1) == 0)).sum())
        black_t += int((surf & (t[..., :3].max(-1) == 0)).sum())
    print("black surface pixels over 16 moving frames: denoised %d, denoised_temporal %d" % (black_s, black_t))
    assert black_s > 0 and black_t < 0.75 * black_s        # measured: 21879 -> 11741 (0.54)
    # a light edit drops the history: the next preview is the spatial one
    lights = scene["lights"].copy()
    sess.set_lights(sb.lights, lights, scene["light_count"])
    sess.frame()
    assert np.array_equal(sess.denoised_temporal().view(np.uint32), sess.denoised().view(np.uint32))
    r.close(); sb.close(); cam.close()

"""GPU tests of the a-trous denoiser: k_dn_prepare, k_dn_variance and k_dn_atrous (gmupt_denoise_image / gmupt_render_denoised) against
the host filter gmupt_denoise_host, bit for bit.  The host filter itself is checked against a float64 restatement in test_denoise_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

from test_denoise_cpu import random_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gmu-path-tracer_amd", "host")
QUALITY_GAIN = 4.0   # MSE(4 spp) / MSE(4 spp denoised) against 1024 spp, Cornell 96x54, AOVs at s = 2: measured 9.25


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
    assert len(bad[0]) == 0, "%s: %d pixels differ, first %r: got %r expected %r" % (what, len(bad[0]), tuple(int(b[0]) for b in bad),
                                                                                   g[tuple(b[0] for b in bad)].view(np.float32), e[tuple(b[0] for b in bad)].view(np.float32))


def make_camera(pkg, scene, W, H):
    cam = pkg.capi.Camera(W, H)
    cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    return cam


def rendered(pkg, device, scene, W, H, frames=6, pool=4096, **kw):
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=pool, **kw)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    for _ in range(frames):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    r.synchronize()
    return r, sb, cam


def test_synthetic_images_match_the_host_filter(pkg, device):
    capi = pkg.capi
    r = capi.Renderer(device, 8, 8, pool_paths=1024)          # the filter needs no scene: any renderer's stream and scratch
    for (W, H, seed) in [(1, 1, 1), (7, 3, 2), (100, 37, 3), (64, 48, 4), (193, 5, 5)]:
        beauty, aov = random_inputs(W, H, seed)
        bt, at = torch.from_numpy(beauty).cuda(), torch.from_numpy(aov).cuda()
        for params in ({}, {"sigma_color": 1.5, "sigma_normal": 16.0, "sigma_plane": 0.5, "sigma_albedo": 0.8}):
            for passes in range(1, 6):
                ms = []
                got = capi.denoise_image(r, bt, at, ms=ms, passes=passes, **params)
                assert got.shape == (H, W, 4) and got.dtype == torch.float32 and got.is_cuda and ms[0] > 0
                assert_same(got, capi.denoise_host(beauty, aov, threads=16, passes=passes, **params), (W, H, passes, params))
    r.close()


@pytest.mark.parametrize("name", ["cornell", "textured", "soup"])
def test_rendered_frames_match_the_host_filter(pkg, device, wide, scenes, name):
    capi = pkg.capi
    W, H = 96, 54
    r, sb, cam = rendered(pkg, device, scenes[name], W, H)
    fb = r.framebuffer()
    for s in (1, 2):
        aov = r.aovs(s)
        exp = capi.denoise_host(fb, aov)
        assert_same(capi.denoise_image(r, torch.from_numpy(fb).cuda(), aov), exp, (name, s, "denoise_image"))
        info = capi.TraceInfo()
        got = r.denoise(s, info=info)
        assert info.flags & capi.STAT_CAST_WIDE and info.ms > 0
        assert_same(got, exp, (name, s, "render_denoised"))
        valid = (bits(fb)[..., 3] > 0) & (capi.aov_fields(aov)["coverage"] > 0)
        assert (np.abs(got.cpu().numpy()[..., :3] - fb[..., :3]).max(-1) > 0)[valid].mean() > 0.5, "most surface pixels change"
    r.close(); sb.close(); cam.close()


def test_tile_renderer_filters_its_own_tile(pkg, device, wide, scenes):
    capi = pkg.capi
    scene = scenes["textured"]
    W, H = 96, 54
    sb = capi.SceneBuffers(device, scene)
    cam = make_camera(pkg, scene, W, H)
    for (x0, y0, tw, th) in [(0, 20, 96, 18), (17, 5, 30, 11)]:
        rt = capi.Renderer(device, tw, th, pool_paths=4096, tile=(x0, y0))
        rt.bind_scene(sb)
        for _ in range(5):
            cam.update(0.0); rt.set_camera(cam.buffer); rt.iterate()
        for s in (1, 2):
            got = rt.denoise(s)
            assert got.shape == (th, tw, 4)
            assert_same(got, capi.denoise_host(rt.framebuffer(), rt.aovs(s)), (x0, y0, s))
        rt.close()
    sb.close(); cam.close()


def noisy_beauty(aov, seed):
    """A beauty image for real AOVs: albedo * 0.6 plus seeded noise, one sample everywhere."""
    alb = aov.cpu().numpy()[..., 0:3]
    b = np.empty(alb.shape[:2] + (4,), np.float32)
    b[..., :3] = np.clip(alb * 0.6 + np.random.default_rng(seed).normal(0, 0.15, alb.shape), 0, 1)
    b[..., 3] = np.uint32(1).view(np.float32)
    return b


def test_bench_scene_frame_matches_the_host_filter(pkg, device, wide):
    """1920x1080: the bench scene's AOVs (s = 1) with a noisy beauty image made from their albedo."""
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    W, H = 1920, 1080
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=1 << 16)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    r.set_camera(cam.buffer)
    aov = r.aovs(1)
    beauty = noisy_beauty(aov, 1)
    got = capi.denoise_image(r, torch.from_numpy(beauty).cuda(), aov)
    assert_same(got, capi.denoise_host(beauty, aov, threads=16), "1920x1080")
    assert (capi.aov_fields(aov)["coverage"] > 0).mean() > 0.5
    r.close(); sb.close(); cam.close()


def test_denoise_leaves_the_renderer_untouched(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H, P = 48, 27, 4096
    sb = pkg.capi.SceneBuffers(device, scene)
    runs = []
    for with_denoise in (False, True):
        r = pkg.capi.Renderer(device, W, H, pool_paths=P)
        r.bind_scene(sb)
        cam = make_camera(pkg, scene, W, H)
        for it in range(12):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if with_denoise and it % 3 == 1:
                r.denoise(1); r.denoise(3, passes=2)
                pkg.capi.denoise_image(r, torch.from_numpy(r.framebuffer()).cuda(), r.aovs(1))
        r.synchronize()
        st = r.stats().as_dict()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), st))
        r.close(); cam.close()
    sb.close()
    (fa, sa, qa, ca, ta), (fb, sbb, qb, cb, tb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb
    assert int(fa[..., 3].view(np.uint32).sum()) > 0


def test_scratch_grows_with_the_image(pkg, device):
    capi = pkg.capi
    r = capi.Renderer(device, 8, 8, pool_paths=1024)
    for (W, H, seed) in [(16, 8, 1), (300, 200, 2), (16, 8, 1), (40, 30, 3)]:
        beauty, aov = random_inputs(W, H, seed)
        assert_same(capi.denoise_image(r, torch.from_numpy(beauty).cuda(), torch.from_numpy(aov).cuda(), passes=3),
                    capi.denoise_host(beauty, aov, passes=3), (W, H))
    r.close()


def test_errors(pkg, device, monkeypatch, scenes):
    capi = pkg.capi
    lib = capi.lib()
    P = C.c_void_p
    scene = scenes["cornell"]
    W, H = 32, 18
    beauty, aov = random_inputs(W, H, 9)
    bt, at = torch.from_numpy(beauty).cuda(), torch.from_numpy(aov).cuda()
    out = torch.empty_like(bt)
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    r = capi.Renderer(device, W, H, pool_paths=1024)
    dp = capi.denoise_params()
    n = out.numel() * 4
    call = lambda b=bt.data_ptr(), a=at.data_ptr(), o=out.data_ptr(), nbytes=n, p=dp, w=W, h=H: lib.gmupt_denoise_image(
        r.h, P(b), P(a), w, h, C.byref(p), P(o), nbytes, None)
    assert call() == 0
    assert call(o=bt.data_ptr()) == capi.ERR_INVALID_ARGUMENT and b"beauty" in lib.gmupt_last_error()     # in place is refused
    assert np.array_equal(bits(bt), bits(beauty)), "the refused call wrote nothing"
    for kw in ({"b": 0}, {"a": 0}, {"o": 0}, {"o": out.data_ptr() + 4}, {"a": at.data_ptr() + 8}, {"nbytes": n - 16}, {"w": 0},
               {"p": capi.denoise_params(passes=0)}, {"p": capi.denoise_params(passes=6)}, {"p": capi.denoise_params(sigma_plane=float("nan"))}):
        assert call(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(capi.GmuptError) as e:
        capi.denoise_image(r, bt, at[:, :5])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    # gmupt_render_denoised: the errors of gmupt_render_aovs, then its own
    o2 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    assert lib.gmupt_render_denoised(r.h, 1, C.byref(dp), P(o2.data_ptr()), o2.numel() * 4, None) == capi.ERR_NOT_BOUND   # no scene
    sb = capi.SceneBuffers(device, scene)
    r.bind_scene(sb)
    with pytest.raises(capi.GmuptError, match="camera") as e:
        r.denoise(1)
    assert e.value.code == capi.ERR_NOT_BOUND
    cam = make_camera(pkg, scene, W, H)
    r.set_camera(cam.buffer)
    assert lib.gmupt_render_denoised(r.h, 1, C.byref(dp), P(o2.data_ptr() + 4), o2.numel() * 4, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_denoised(r.h, 1, C.byref(dp), P(o2.data_ptr()), o2.numel() * 4 - 16, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_denoised(r.h, 9, C.byref(dp), P(o2.data_ptr()), o2.numel() * 4, None) == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.GmuptError) as e:
        r.denoise(1, sigma_color=0.0)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    r.denoise(2)                                                                       # still usable
    r.close(); sb.close()
    monkeypatch.setenv("GMUPT_TRAVERSAL", "cast0")
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=1024)
    r.bind_scene(sb); r.set_camera(cam.buffer)
    with pytest.raises(capi.GmuptError, match="wide collapse") as e:
        r.denoise(1)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert_same(capi.denoise_image(r, bt, at), capi.denoise_host(beauty, aov), "the image filter needs no wide collapse")
    r.close(); sb.close(); cam.close()


def test_session_denoised(pkg, device, wide, scenes):
    scene = scenes["cornell"]
    W, H = 64, 36
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=4096)
    r.bind_scene(sb)
    cam = make_camera(pkg, scene, W, H)
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    for _ in range(4):
        sess.frame()
    img = sess.denoised(2, passes=4)
    assert isinstance(img, np.ndarray) and img.shape == (H, W, 4) and img.dtype == np.float32
    assert np.array_equal(img.view(np.uint32), bits(pkg.capi.denoise_host(r.framebuffer(), r.aovs(2), passes=4)))
    assert pkg.progressive.to_rgba8(img).shape == (H, W, 4)
    r.close(); sb.close(); cam.close()


def read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert kind == b"PF" and scale == b"-1.0"
    return np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1]


def test_cpp_driver_writes_the_denoised_files(pkg, device, wide, tmp_path):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    exe = os.path.join(HOST, "gmupt_render")
    W, H, s = 64, 36, 2
    prefix = str(tmp_path / "dn")
    subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", "5", "--pool", "4096", "--live", "4096",
                    "--aov", str(tmp_path / "aov"), "--aov-samples", str(s), "--denoise", prefix, "--dump", str(tmp_path / "fb.f32")],
                   check=True, cwd=str(tmp_path))
    fb = np.fromfile(str(tmp_path / "fb.f32"), dtype=np.float32).reshape(H, W, 4)
    aov = np.fromfile(str(tmp_path / "aov.aov"), dtype=np.float32).reshape(H, W, 16)
    exp = pkg.capi.denoise_host(fb, aov)
    assert np.array_equal(read_pfm(prefix + ".pfm").view(np.uint32), exp[..., :3].view(np.uint32))
    png = pkg.capi.decode_png(open(prefix + ".png", "rb").read())
    assert np.array_equal(png, pkg.progressive.to_rgba8(exp))
    assert (fb[..., 3].view(np.uint32) > 0).sum() > W * H // 4


def test_denoise_quality_on_cornell(pkg, device, wide, scenes):
    """4 spp denoised is much nearer to 1024 spp than 4 spp is (both budgeted renders of Cornell at 96x54)."""
    capi = pkg.capi
    scene = scenes["cornell"]
    W, H = 96, 54
    sb = capi.SceneBuffers(device, scene)

    def render(spp):
        r = capi.Renderer(device, W, H, pool_paths=min(1 << 16, W * H * spp // 2), path_budget=W * H * spp)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        r.render_budget(cam, 1 << 20)
        fb = r.framebuffer()
        assert np.all(fb[..., 3].view(np.uint32) == spp)
        return r, cam, fb

    rr, cr, ref = render(1024)
    rr.close(); cr.close()
    r, cam, noisy = render(4)
    den = r.denoise(2).cpu().numpy()
    r.close(); cam.close(); sb.close()
    mse = lambda a: float(((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean())
    gain = mse(noisy) / mse(den)
    print("cornell %dx%d: MSE 4 spp %.6f, denoised %.6f, gain %.2f" % (W, H, mse(noisy), mse(den), gain))
    assert gain >= QUALITY_GAIN, gain

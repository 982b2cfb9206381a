"""GPU tests of the lens-filtered AOV planes (gmupt_render_aovs_lens, gmupt_render_denoised_lens; include/gmupt_lens_aov.h): k_laov_raygen,
the QueryIO walk and k_laov_resolve against the CPU oracle.

Truth is made as in test_aov_gpu.py: the rays of gmupt_aov_lens_ray go through the oracle's own extension and logic stages on a frozen
state (oracle_rays / per_ray of that module), and the record rule of the header is restated in numpy with float32 running sums in k
order (lens_aov_util.reduce_records).
"""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the records are a torch tensor)

import lens_aov_util as LA
from test_aov_gpu import categories, compare_records, make_camera, oracle_rays, per_ray, pixels, renderer

pytestmark = pytest.mark.gpu

DOF_POSE = (-3.5, 8.0, 7.0, 0.0, 270.0)      # test_lens_gpu.py: outside the Cornell room's opening, high and to the left, looking at the back wall


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def scenes(pkg):
    return {"cornell": pkg.scenes.build_scene(pkg.scenes.cornell_mesh()),
            "spheres": pkg.scenes.build_scene(pkg.scenes.spheres_mesh(n_spheres=12, subdiv=2, seed=7, floor_quads=4)),
            "textured": pkg.scenes.build_scene(pkg.scenes.textured_mesh())}


def lens_of(pkg, aperture, focus):
    return pkg.capi.lens.lens_params(aperture_radius=aperture, focus_distance=focus)


def camera_at(pkg, scene, W, H, pose=None):
    cam = make_camera(pkg, scene, W, H)
    if pose is not None:
        cam.set_pose(*pose); cam.update(0.0)
    return cam


def expected(pkg, scene, cb, lens, xs, ys, s):
    """(records, triangle records, which name a triangle, per-ray values, the oracle's truth) of the pixels (xs, ys)."""
    rays = pkg.capi.lens_aov.aov_lens_rays(cb, lens, xs, ys, s)
    assert rays.shape == (len(xs), s * s, 8)
    truth = oracle_rays(scene, rays.reshape(-1, 8), cb)
    v = per_ray(scene, rays.reshape(-1, 8), truth, cb)
    return LA.reduce_records(v, rays) + (v, truth)


# the views were checked on the CPU with the oracle alone: what each must contain is asserted below from the oracle's per-ray results
@pytest.mark.parametrize("name, s, pose, aperture, focus", [("textured", 2, None, 0.3, 4.0), ("textured", 3, None, 0.3, 4.0), ("cornell", 2, DOF_POSE, 0.5, 12.0)])
def test_records_match_the_oracle(pkg, device, wide, scenes, name, s, pose, aperture, focus):
    scene = scenes[name]
    W, H = 40, 24
    cam = camera_at(pkg, scene, W, H, pose)
    lens = lens_of(pkg, aperture, focus)
    exp, rec, names, v, truth = expected(pkg, scene, cam.buffer, lens, *pixels(W, H), s)
    # the precondition: every branch of the record rule runs
    c = categories(scene, truth)
    cov = v["surface"].reshape(-1, s * s).sum(axis=1)
    have = dict(c, cov0=int((cov == 0).sum()), partly=int(((cov > 0) & (cov < s * s)).sum()), full=int((cov == s * s).sum()))
    print(name, s, have)
    assert have["cov0"] > 0 and have["partly"] > 0 and have["full"] > 0 and have["light"] > 0, have
    if name == "textured":
        assert have["textured"] > 0 and have["normal_mapped"] > 0, have
    else:
        assert have["miss"] > 0, have
    first_not_zero = (v["surface"].reshape(-1, s * s)[:, 0] == 0) & (cov > 0)
    assert first_not_zero.any(), "a pixel whose first surface sample is not ray 0"
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    info = pkg.capi.TraceInfo()
    got = pkg.capi.lens_aov.aovs(r, s, lens, info=info)
    assert got.shape == (H, W, 16) and got.dtype == torch.float32 and got.is_cuda
    assert info.flags & pkg.capi.STAT_CAST_WIDE and info.ms > 0
    compare_records(scene, got.cpu().numpy(), exp, rec, names)
    f = pkg.capi.aov_fields(got)
    assert np.array_equal(f["coverage"].ravel(), cov) and ((f["coverage"] > 0) == ((f["triangle"] >= 0) & (f["light"] == 0))).all()
    r.close(); sb.close(); cam.close()


def test_one_sample_is_the_single_ray_record(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H = 17, 5
    cam = camera_at(pkg, scene, W, H)
    lens = lens_of(pkg, 0.3, 4.0)
    exp, rec, names, v, _ = expected(pkg, scene, cam.buffer, lens, *pixels(W, H), 1)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    got = pkg.capi.lens_aov.aovs(r, 1, lens).cpu().numpy()
    compare_records(scene, got, exp, rec, names)
    # one ray: the record is that ray's own values
    g = got.reshape(-1, 16)
    assert np.array_equal(g[:, 3].view(np.uint32), v["t"].view(np.uint32)) and np.array_equal(g[:, 0:3].view(np.uint32), v["albedo"].view(np.uint32))
    assert v["surface"].any()
    r.close(); sb.close(); cam.close()


def test_tile_renderer_returns_its_sub_rectangle(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H = 96, 54
    cam = camera_at(pkg, scene, W, H)
    lens = lens_of(pkg, 0.3, 4.0)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    whole = {s: pkg.capi.lens_aov.aovs(r, s, lens).cpu().numpy().view(np.uint32) for s in (1, 2)}
    for (x0, y0, tw, th) in [(0, 20, 96, 18), (17, 5, 30, 11)]:
        rt = pkg.capi.Renderer(device, tw, th, pool_paths=4096, tile=(x0, y0))
        rt.bind_scene(sb); rt.set_camera(cam.buffer)
        for s in (1, 2):
            tile = pkg.capi.lens_aov.aovs(rt, s, lens).cpu().numpy().view(np.uint32)
            assert tile.shape == (th, tw, 16) and np.array_equal(tile, whole[s][y0:y0 + th, x0:x0 + tw]), (x0, y0, s)
        rt.close()
    r.close(); sb.close(); cam.close()


def test_a_frame_of_two_chunks_equals_single_chunk_tiles(pkg, device, wide, scenes):
    scene = scenes["spheres"]
    s = pkg.capi.AOV_MAX_SAMPLES
    W = 256
    rows = pkg.capi.AOV_CHUNK_RAYS // (W * s * s)            # 128 rows of 256 * 64 rays fill a chunk
    H = rows + 1                                             # one more: a second chunk of one row
    assert rows * W * s * s == pkg.capi.AOV_CHUNK_RAYS and W * H * s * s > pkg.capi.AOV_CHUNK_RAYS
    cam = camera_at(pkg, scene, W, H)
    lens = lens_of(pkg, 0.2, 9.0)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    whole = pkg.capi.lens_aov.aovs(r, s, lens).cpu().numpy().view(np.uint32)
    assert (pkg.capi.aov_fields(whole.view(np.float32))["coverage"] > 0).sum() > 1000
    for y0, th in [(0, 64), (64, 64), (rows, 1)]:            # the last tile is the second chunk's row
        rt = pkg.capi.Renderer(device, W, th, pool_paths=4096, tile=(0, y0))
        rt.bind_scene(sb); rt.set_camera(cam.buffer)
        assert np.array_equal(pkg.capi.lens_aov.aovs(rt, s, lens).cpu().numpy().view(np.uint32), whole[y0:y0 + th]), y0
        rt.close()
    r.close(); sb.close(); cam.close()


def test_the_call_leaves_the_renderer_untouched(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H, P = 48, 27, 4096
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    attached = lens_of(pkg, 0.2, 5.0)
    runs = []
    for with_calls in (False, True):
        r = capi.Renderer(device, W, H, pool_paths=P)
        r.bind_scene(sb)
        capi.lens.set_lens(r, attached)
        cam = make_camera(pkg, scene, W, H)
        pinhole = []
        for it in range(12):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if it % 3 == 1:
                pinhole.append(r.aovs(2).cpu().numpy().view(np.uint32))
                if with_calls:
                    capi.lens_aov.aovs(r, 1); capi.lens_aov.aovs(r, 3, lens_of(pkg, 0.4, 3.0)); capi.lens_aov.denoise(r, 2)
                    assert np.array_equal(r.aovs(2).cpu().numpy().view(np.uint32), pinhole[-1]), "gmupt_render_aovs returns the bytes it returned before"
        r.synchronize()
        got = capi.lens.get_lens(r)
        assert (got.aperture_radius, got.focus_distance) == (attached.aperture_radius, attached.focus_distance)
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), r.stats().as_dict(), pinhole))
        r.close(); cam.close()
    sb.close()
    (fa, sa, qa, ca, ta, pa), (fb, sbb, qb, cb, tb, pb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert int(fa[..., 3].view(np.uint32).sum()) > 0


def test_null_lens_is_the_attached_lens(pkg, device, wide, scenes):
    scene = scenes["cornell"]
    W, H = 40, 24
    capi = pkg.capi
    cam = camera_at(pkg, scene, W, H, DOF_POSE)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    none = capi.lens.get_lens(r)                              # { 0, the focus of gmupt_lens_default_params }: what the call uses when none is attached
    assert none.aperture_radius == 0.0
    closed = bits(capi.lens_aov.aovs(r, 2, none))
    assert np.array_equal(bits(capi.lens_aov.aovs(r, 2)), closed), "none attached: aperture 0"
    lens = lens_of(pkg, 0.5, 12.0)
    explicit = bits(capi.lens_aov.aovs(r, 2, lens))
    assert not np.array_equal(explicit, closed)
    capi.lens.set_lens(r, lens)
    assert np.array_equal(bits(capi.lens_aov.aovs(r, 2)), explicit)
    assert np.array_equal(bits(capi.lens_aov.aovs(r, 2, none)), closed), "a given lens wins over the attached one"
    r.close(); sb.close(); cam.close()


def test_errors(pkg, device, monkeypatch, scenes):
    capi = pkg.capi
    lib = capi.lib()
    scene = scenes["cornell"]
    W, H = 32, 18
    out = torch.full((H, W, 16), 7.0, dtype=torch.float32, device="cuda")
    img = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    P = C.c_void_p
    ptr, nbytes = P(out.data_ptr()), out.numel() * 4
    iptr, ibytes = P(img.data_ptr()), img.numel() * 4
    ok = lens_of(pkg, 0.3, 4.0)
    L = C.byref(ok)
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    r = capi.Renderer(device, W, H, pool_paths=1024)
    cam = make_camera(pkg, scene, W, H)
    assert lib.gmupt_render_aovs_lens(r.h, L, 1, ptr, nbytes, None) == capi.ERR_NOT_BOUND          # no scene
    assert lib.gmupt_render_denoised_lens(r.h, L, 1, None, iptr, ibytes, None) == capi.ERR_NOT_BOUND
    sb = capi.SceneBuffers(device, scene)
    r.bind_scene(sb)
    assert lib.gmupt_render_aovs_lens(r.h, L, 1, ptr, nbytes, None) == capi.ERR_NOT_BOUND          # no camera
    with pytest.raises(capi.GmuptError, match="camera") as e:
        capi.lens_aov.aovs(r, 1, ok)
    assert e.value.code == capi.ERR_NOT_BOUND
    r.set_camera(cam.buffer)
    assert lib.gmupt_render_aovs_lens(r.h, L, 1, None, nbytes, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_aovs_lens(r.h, L, 1, P(out.data_ptr() + 4), nbytes, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_aovs_lens(r.h, L, 1, ptr, nbytes - 64, None) == capi.ERR_INVALID_ARGUMENT
    for s in (0, 9):
        assert lib.gmupt_render_aovs_lens(r.h, L, s, ptr, nbytes, None) == capi.ERR_INVALID_ARGUMENT
        assert lib.gmupt_render_denoised_lens(r.h, L, s, None, iptr, ibytes, None) == capi.ERR_INVALID_ARGUMENT
    # the lens checks of gmupt_renderer_set_lens, on a lens that is given
    nan, inf = float("nan"), float("inf")
    for a, f in [(nan, 1.0), (inf, 1.0), (-1.0, 1.0), (0.1, nan), (0.1, inf), (0.1, 0.0), (0.1, -2.0)]:
        bad = lens_of(pkg, a, f)
        assert lib.gmupt_render_aovs_lens(r.h, C.byref(bad), 1, ptr, nbytes, None) == capi.ERR_INVALID_ARGUMENT, (a, f)
        assert b"gmupt_render_aovs_lens" in lib.gmupt_last_error()
        assert lib.gmupt_render_denoised_lens(r.h, C.byref(bad), 1, None, iptr, ibytes, None) == capi.ERR_INVALID_ARGUMENT, (a, f)
    assert lib.gmupt_render_denoised_lens(r.h, L, 1, None, None, ibytes, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_denoised_lens(r.h, L, 1, None, iptr, ibytes - 16, None) == capi.ERR_INVALID_ARGUMENT
    dp = capi.denoise_params(passes=0)
    assert lib.gmupt_render_denoised_lens(r.h, L, 1, C.byref(dp), iptr, ibytes, None) == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == 7.0).all()), "no error path writes an output"
    info = capi.TraceInfo()
    assert lib.gmupt_render_aovs_lens(r.h, L, 2, ptr, nbytes, C.byref(info)) == 0 and info.flags & capi.STAT_CAST_WIDE   # still usable
    r.close(); sb.close()
    # a row wider than one chunk: 40 000 pixels * 64 rays at s = 8; 40 000 * 49 fit (and 2^21 / 64 = 32 768 pixels is the widest row at s = 8)
    wide_r = capi.Renderer(device, 40000, 1, pool_paths=1024)
    sb = capi.SceneBuffers(device, scene)
    wide_r.bind_scene(sb); wide_r.set_camera(cam.buffer)
    big = torch.empty((1, 40000, 16), dtype=torch.float32, device="cuda")
    assert lib.gmupt_render_aovs_lens(wide_r.h, L, 8, P(big.data_ptr()), big.numel() * 4, None) == capi.ERR_INVALID_ARGUMENT
    assert b"2^21" in lib.gmupt_last_error()
    capi.lens_aov.aovs(wide_r, 7, ok)
    wide_r.close(); sb.close()
    monkeypatch.setenv("GMUPT_TRAVERSAL", "cast0")
    r, sb = renderer(pkg, device, scene, W, H, pool=1024)
    r.set_camera(cam.buffer)
    with pytest.raises(capi.GmuptError, match="wide collapse") as e:
        capi.lens_aov.aovs(r, 1, ok)
    assert e.value.code == capi.ERR_UNSUPPORTED
    r.close(); sb.close(); cam.close()


def surface_pixels(f):
    """gd_prepare's surface pixel (csrc/pt_guides.hpp) from the fields of a record: a triangle, no light, a non-zero normal."""
    return (f["triangle"] >= 0) & (f["light"] == 0) & (np.abs(f["normal"]).sum(axis=-1) > 0)


def dof_frame(pkg, device, sb, scene, spp, pool, aperture=0.5, W=64, H=36):
    """The Cornell view of the lens image test (test_lens_gpu.py): the camera outside the opening, the lens focused on the back wall
    through focus_at on the centre pixel, `spp` samples in every pixel.  Returns (renderer, camera, lens); the renderer holds the frame."""
    capi = pkg.capi
    r = capi.Renderer(device, W, H, pool_paths=pool, path_budget=W * H * spp)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*DOF_POSE); cam.buffer.lightCount = scene["light_count"]
    cam.update(0.0); r.set_camera(cam.buffer)
    lens = capi.lens.focus_at(r, W / 2, H / 2, 0, aperture_radius=aperture)
    cam.reset_accumulation()
    capi.lens.set_lens(r, lens)
    r.render_budget(cam, 100000)
    assert np.all(r.framebuffer()[..., 3].view(np.uint32) == spp)
    cam.update(0.0); r.set_camera(cam.buffer)
    return r, cam, lens


def test_lens_guides_reach_the_pixels_the_pinhole_guides_leave_alone(pkg, device, wide, scenes):
    """What the lens records are for.  H = the pixels that are not surface pixels in the pinhole record but are in the lens record
    (s = 4): their centre ray misses, blurred foreground reaches them.  gmupt_render_denoised copies them through bit for bit;
    gmupt_render_denoised_lens filters them, and still copies every pixel that is no surface pixel of the lens record."""
    capi = pkg.capi
    scene = scenes["cornell"]
    sb = capi.SceneBuffers(device, scene)
    r, cam, lens = dof_frame(pkg, device, sb, scene, 4, 4096)
    assert abs(lens.focus_distance - 12.0) < 1e-3
    beauty = r.framebuffer().view(np.uint32)
    pin = surface_pixels(capi.aov_fields(r.aovs(4)))
    lf = capi.aov_fields(capi.lens_aov.aovs(r, 4))
    lns = surface_pixels(lf)
    Hset = ~pin & lns
    print("H: %d pixels; pinhole surface pixels %d, lens surface pixels %d, partly covered %d" % (Hset.sum(), pin.sum(), lns.sum(), ((lf["coverage"] > 0) & (lf["coverage"] < 16)).sum()))
    assert Hset.sum() > 0, "the view is wrong: no pixel outside the pinhole silhouette that a lens ray reaches"
    a = r.denoise(4).cpu().numpy().view(np.uint32)
    assert np.array_equal(a[Hset], beauty[Hset]), "the pinhole guides leave H as the beauty holds it"
    b = capi.lens_aov.denoise(r, 4).cpu().numpy().view(np.uint32)
    assert (b[Hset][:, :3] != beauty[Hset][:, :3]).any(), "the lens guides filter H"
    assert np.array_equal(b[~lns], beauty[~lns]), "what no lens ray sees a surface in is copied through"
    assert np.array_equal(r.framebuffer().view(np.uint32), beauty)
    r.close(); cam.close(); sb.close()


def test_session_lens_guides(pkg, device, wide, scenes):
    """ProgressiveSession.denoised / denoised_temporal(lens_guides=True) with a lens set are the filter and the temporal chain on the
    lens records; without a lens they are the default's bits."""
    capi = pkg.capi
    scene = scenes["cornell"]
    W, H = 64, 36
    r, sb = renderer(pkg, device, scene, W, H)
    cam = capi.Camera(W, H); cam.set_pose(*DOF_POSE); cam.buffer.lightCount = scene["light_count"]
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    sess.run(4)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(sess.denoised(2, lens_guides=True)), bits(sess.denoised(2)))
    sess.set_lens(0.5, focus=12.0)
    sess.run(4)
    beauty, aov = capi.lens_aov.guided_inputs(r, 2)
    want = capi.denoise_image(r, beauty, aov).cpu().numpy()
    got = sess.denoised(2, lens_guides=True)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(sess.denoised(2)))
    filled = sess.denoised(2, lens_guides=True, infill=True)
    assert filled.shape == (H, W, 4) and np.isfinite(filled[..., :3]).all()
    t1 = sess.denoised_temporal(2, lens_guides=True)
    t2 = sess.denoised_temporal(2, lens_guides=True)
    assert t1.shape == (H, W, 4) and np.isfinite(t1[..., :3]).all() and np.array_equal(bits(t1), bits(t2)), "the same frame and records twice: nothing folded in between"
    sess.close(); r.close(); sb.close(); cam.close()


def test_lens_guides_lower_the_error_where_the_beauty_is_blurred(pkg, device, wide, scenes):
    """The image-level figure, in the view of the test above.  Reference: the lens beauty at 4096 spp (two such references with other
    seeds differ by an MSE of 2.7e-5 over the frame, under a tenth of every error below; the 4 spp input's own is 1.4e-2).  Inputs: the
    lens beauty at 4 spp for three seeds (pool sizes), denoised with default parameters (a) with the pinhole records and (b) with the
    lens records, both at s = 4.  Region: the pixels with 0 < coverage < 16 in the lens record together with H (366 pixels, 180 in H).
    MSE over rgb against the reference, values clamped at 4.0 as the lens image test does.

    Measured on the MI355X over four seeds (tools/lens_aov_quality.py, profiles/lens_aov/quality.txt): region (a) 0.00500, 0.00428,
    0.00556, 0.00530 -- spread (max - min) 0.00128 -- and (b) 0.00102, 0.00093, 0.00102, 0.00073; whole frame (a) 0.00226, 0.00211,
    0.00238, 0.00227 -- spread 0.00028 -- and (b) 0.00163, 0.00159, 0.00173, 0.00152.
    Asserted, per seed, with those two spreads of (a) as the margins: over the region (b) beats (a) by more than 0.00128; over the
    whole frame (b) is not worse than (a) by more than 0.00028."""
    SPREAD_REGION, SPREAD_FRAME = 0.00128, 0.00028
    capi = pkg.capi
    scene = scenes["cornell"]
    sb = capi.SceneBuffers(device, scene)
    clamp = lambda x: np.minimum(np.asarray(x)[..., :3].astype(np.float64), 4.0)
    r, cam, _ = dof_frame(pkg, device, sb, scene, 4096, 8192)
    ref = clamp(r.framebuffer())
    r.close(); cam.close()
    for pool in (4096, 3072, 2048):
        r, cam, _ = dof_frame(pkg, device, sb, scene, 4, pool)
        pin = surface_pixels(capi.aov_fields(r.aovs(4)))
        lf = capi.aov_fields(capi.lens_aov.aovs(r, 4))
        region = ((lf["coverage"] > 0) & (lf["coverage"] < 16)) | (~pin & surface_pixels(lf))
        a, b = clamp(r.denoise(4).cpu().numpy()), clamp(capi.lens_aov.denoise(r, 4).cpu().numpy())
        r.close(); cam.close()
        mse = lambda x, m: float(((x - ref) ** 2)[m].mean())
        every = np.ones_like(region)
        fig = dict(region_a=mse(a, region), region_b=mse(b, region), frame_a=mse(a, every), frame_b=mse(b, every))
        print("seed (pool %d): region of %d pixels (a) %.6f (b) %.6f; frame (a) %.6f (b) %.6f" % (pool, region.sum(), fig["region_a"], fig["region_b"], fig["frame_a"], fig["frame_b"]))
        assert region.sum() > 100
        assert fig["region_a"] - fig["region_b"] > SPREAD_REGION, (pool, fig)
        assert fig["frame_b"] - fig["frame_a"] <= SPREAD_FRAME, (pool, fig)
    sb.close()

"""GPU tests of the AOV buffers (gmupt_render_aovs): k_aov_raygen, the QueryIO walk and k_aov_resolve against the CPU oracle.

Truth is the oracle's own extension and logic stages on a frozen state: the AOV rays (gmupt_aov_ray) are written into rayOrigin /
rayDirection with identity queues, orc.stage("extension") runs, then throughput / lightThroughput = 1, radiance / directLight = 0,
pathLength = 0, inShadow = 1 and an iterationCounter >= 1, and orc.stage("logic") runs.  matColor, matMR, normal, surfacePoint,
hitDistance, triangle and isEmitter are then the truth of every ray; a light-sphere hit and a miss follow include/gmupt.h in numpy float32.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the records are a torch tensor)

import oracle_lib as O

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
NO_TRI = 0xFFFFFFFF
ENV = (0.3125, 0.55, 0.8)   # a non-default envColor: the albedo of a miss
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gmu-path-tracer_amd", "host")
f32 = np.float32


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


def make_camera(pkg, scene, W, H):
    cam = pkg.capi.Camera(W, H)
    cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    for i, v in enumerate(ENV):
        cam.buffer.envColor[i] = v
    return cam


def pixels(W, H, origin=(0, 0)):
    ys, xs = np.mgrid[0:H, 0:W]
    return (xs.ravel() + origin[0]).tolist(), (ys.ravel() + origin[1]).tolist()


def oracle_rays(scene, rays, cb, threads=16):
    """The oracle's extension + logic stages on (N, 8) rays: dict of per-ray fields (uint32 bit patterns)."""
    N = len(rays)
    P = max(N, 64)
    orc = O.Renderer(scene, 32, 18, P, threads=threads)
    st = orc.path_state()
    fld = lambda name: O.state_field(st, P, name)
    fld("triangle")[:] = NO_TRI
    fld("baryCoord")[:] = 0
    fld("hitDistance").view(np.float32)[:] = FLT_MAX   # the slots beyond N are misses for the logic stage
    fld("isEmitter")[:] = 0
    fld("rayOrigin").view(np.float32)[:N] = rays[:, 0:3]
    fld("rayDirection").view(np.float32)[:N] = rays[:, 4:7]
    q = orc.queues(); q[3][:] = np.arange(P, dtype=np.uint32)
    qc = orc.counters(); qc[:] = 0; qc[7] = N
    ocb = O.CameraBuffer()
    C.memmove(C.byref(ocb), C.byref(cb), 112)
    ocb.sampleCounter = max(1, ocb.sampleCounter)       # logic must not take the clearTexture branch
    orc.set_camera(ocb)
    orc.stage("extension")
    st = orc.path_state()
    for name, v in (("throughput", 1.0), ("lightThroughput", 1.0), ("radiance", 0.0), ("directLight", 0.0)):
        fld(name).view(np.float32)[:] = v
    fld("pathLength")[:] = 0
    fld("inShadow")[:] = 1
    orc.stage("logic")
    st = orc.path_state()
    out = {k: fld(k)[:N].copy() for k in ("matColor", "matMR", "normal", "surfacePoint", "hitDistance", "triangle", "isEmitter")}
    orc.close()
    return out


def per_ray(scene, rays, truth, cb):
    """include/gmupt.h per ray from the oracle's truth: dict of float32 / uint32 arrays over the N rays."""
    t = truth["hitDistance"][:, 0].view(np.float32)
    light = truth["isEmitter"][:, 0]
    rec = truth["triangle"]
    hit_tri = rec[:, 0] != NO_TRI
    surface = hit_tri & (light == 0)
    lit = light > 0
    n = len(rays)
    albedo = np.tile(np.array([cb.envColor[0], cb.envColor[1], cb.envColor[2]], np.float32), (n, 1))
    if lit.any():
        em = scene["lights"]["emission"].astype(np.float32)[np.minimum(light[lit] - 1, 127)]
        emax = em.max(axis=1, keepdims=True)
        albedo[lit] = em / emax
    albedo[surface] = truth["matColor"][surface].view(np.float32)
    normal = np.zeros((n, 3), np.float32); normal[surface] = truth["normal"][surface].view(np.float32)
    mr = np.zeros((n, 2), np.float32); mr[surface] = truth["matMR"][surface].view(np.float32)
    pos = np.zeros((n, 3), np.float32)
    pos[surface] = truth["surfacePoint"][surface].view(np.float32)
    pos[lit] = rays[lit, 0:3] + rays[lit, 4:7] * t[lit, None]          # surfacePoint still holds the triangle's point there
    material = np.where(hit_tri, rec[:, 3], 0).astype(np.uint32)
    return {"t": t, "light": light, "rec": rec, "hit_tri": hit_tri, "surface": surface, "albedo": albedo, "normal": normal,
            "metallic": mr[:, 0], "roughness": mr[:, 1], "position": pos, "material": material}


def expected(scene, rays, truth, s, cb):
    """(N pixels, 16) uint32 records from the oracle's per-ray truth; rays (N, R, 8).  Word 12 (triangle) is left 0: compare_records checks it."""
    N, R = rays.shape[0], rays.shape[1]
    v = per_ray(scene, rays.reshape(-1, 8), truth, cb)
    g = lambda k: v[k].reshape((N, R) + v[k].shape[1:])
    exp = np.zeros((N, 16), np.float32)
    if s == 1:
        albedo, normal, cov = g("albedo")[:, 0], g("normal")[:, 0], g("surface")[:, 0].astype(np.uint32)
    else:
        sa = np.zeros((N, 3), np.float32); sn = np.zeros((N, 3), np.float32)
        for k in range(1, R):                                              # sum = 0.0f, += in k order, / (float)(s*s)
            sa = (sa + g("albedo")[:, k]).astype(np.float32); sn = (sn + g("normal")[:, k]).astype(np.float32)
        albedo, normal = sa / f32(s * s), sn / f32(s * s)
        cov = g("surface")[:, 1:].sum(axis=1).astype(np.uint32)
    exp[:, 0:3] = albedo; exp[:, 3] = g("t")[:, 0]
    exp[:, 4:7] = normal; exp[:, 7] = g("roughness")[:, 0]
    exp[:, 8:11] = g("position")[:, 0]; exp[:, 11] = g("metallic")[:, 0]
    e = exp.view(np.uint32)
    e[:, 13] = g("material")[:, 0]; e[:, 14] = g("light")[:, 0]; e[:, 15] = cov
    return e, g("rec")[:, 0], g("hit_tri")[:, 0]


def compare_records(scene, got, exp, exp_rec, exp_hit):
    """got (N, 16) float32 from the GPU against expected(): every word bit for bit; the triangle id names the oracle's triangle record
    (its lowest reference, as gmupt_hit)."""
    g = np.ascontiguousarray(got, dtype=np.float32).reshape(-1, 16).view(np.uint32)
    cols = [c for c in range(16) if c != 12]
    bad = np.nonzero((g[:, cols] != exp[:, cols]).any(axis=1))[0]
    assert len(bad) == 0, "%d records differ, first %d: got %r expected %r" % (len(bad), bad[0], g[bad[0]].view(np.float32), exp[bad[0]].view(np.float32))
    tri = g[:, 12].view(np.int32)
    hit = tri >= 0
    assert np.array_equal(hit, exp_hit), "which pixels hit a triangle"
    recs = scene["tris"].view(np.uint32).reshape(-1, 4)
    assert np.array_equal(recs[tri[hit]], exp_rec[hit]), "triangle record"
    assert (tri[~hit] == -1).all()


def categories(scene, truth):
    v_light = truth["isEmitter"][:, 0] > 0
    hit_tri = truth["triangle"][:, 0] != NO_TRI
    surface = hit_tri & ~v_light
    mats = scene["materials"]
    mid = np.where(surface, truth["triangle"][:, 3], 0)
    tex = mats["textureIndices"][mid]
    return {"miss": int((~hit_tri & ~v_light).sum()), "light": int(v_light.sum()), "surface": int(surface.sum()),
            "textured": int((surface & (tex >= 0).any(axis=1)).sum()), "normal_mapped": int((surface & (tex[:, 2] >= 0)).sum())}


def renderer(pkg, device, scene, W, H, pool=4096, **kw):
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=pool, **kw)
    r.bind_scene(sb)
    return r, sb


@pytest.fixture(scope="module")
def scenes(pkg):
    return {"soup": pkg.scenes.build_scene(pkg.scenes.random_triangles_mesh(2000, seed=1)),
            "cornell": pkg.scenes.build_scene(pkg.scenes.cornell_mesh()),
            "spheres": pkg.scenes.build_scene(pkg.scenes.spheres_mesh(n_spheres=12, subdiv=2, seed=7, floor_quads=4)),
            "textured": pkg.scenes.build_scene(pkg.scenes.textured_mesh())}


def test_one_sample_matches_the_oracle(pkg, device, wide, scenes):
    W, H = 96, 54
    seen = {}
    for name in ("soup", "cornell", "spheres", "textured"):
        scene = scenes[name]
        cam = make_camera(pkg, scene, W, H)
        r, sb = renderer(pkg, device, scene, W, H)
        r.set_camera(cam.buffer)
        info = pkg.capi.TraceInfo()
        got = r.aovs(1, info=info)
        assert got.shape == (H, W, 16) and got.dtype == torch.float32 and got.is_cuda
        assert info.flags & pkg.capi.STAT_CAST_WIDE and info.ms > 0
        rays = pkg.capi.aov_rays(cam.buffer, *pixels(W, H), 1)
        truth = oracle_rays(scene, rays.reshape(-1, 8), cam.buffer)
        compare_records(scene, got.cpu().numpy(), *expected(scene, rays, truth, 1, cam.buffer))
        c = categories(scene, truth)
        for k, v in c.items():
            seen[k] = seen.get(k, 0) + v
        if name == "textured":
            assert c["textured"] > 0 and c["normal_mapped"] > 0, c
        f = pkg.capi.aov_fields(got)
        assert f["albedo"].shape == (H, W, 3) and ((f["coverage"] == 1) == ((f["triangle"] >= 0) & (f["light"] == 0))).all()
        r.close(); sb.close(); cam.close()
    assert all(seen[k] > 0 for k in ("miss", "light", "surface", "textured", "normal_mapped")), seen


@pytest.mark.parametrize("s", [2, 3])
def test_filtered_planes_are_the_ordered_mean(pkg, device, wide, scenes, s):
    scene = scenes["textured"]
    W, H = 40, 24
    cam = make_camera(pkg, scene, W, H)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    got = r.aovs(s).cpu().numpy()
    rays = pkg.capi.aov_rays(cam.buffer, *pixels(W, H), s)
    assert rays.shape == (W * H, s * s + 1, 8)
    truth = oracle_rays(scene, rays.reshape(-1, 8), cam.buffer)
    exp = expected(scene, rays, truth, s, cam.buffer)
    compare_records(scene, got, *exp)
    cov = pkg.capi.aov_fields(got)["coverage"].ravel()
    assert cov.max() == s * s and ((cov > 0) & (cov < s * s)).sum() > 0, "edges: partly covered pixels"
    # the centre fields are the one-sample call's
    one = r.aovs(1).cpu().numpy().reshape(-1, 16).view(np.uint32)
    g = got.reshape(-1, 16).view(np.uint32)
    assert np.array_equal(g[:, [3, 7, 8, 9, 10, 11, 12, 13, 14]], one[:, [3, 7, 8, 9, 10, 11, 12, 13, 14]])
    r.close(); sb.close(); cam.close()


def test_tile_renderer_returns_its_sub_rectangle(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H = 96, 54
    cam = make_camera(pkg, scene, W, H)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    whole = {s: r.aovs(s).cpu().numpy().view(np.uint32) for s in (1, 2)}
    for (x0, y0, tw, th) in [(0, 20, 96, 18), (17, 5, 30, 11)]:
        rt = pkg.capi.Renderer(device, tw, th, pool_paths=4096, tile=(x0, y0))
        rt.bind_scene(sb); rt.set_camera(cam.buffer)
        for s in (1, 2):
            tile = rt.aovs(s).cpu().numpy().view(np.uint32)
            assert tile.shape == (th, tw, 16) and np.array_equal(tile, whole[s][y0:y0 + th, x0:x0 + tw]), (x0, y0, s)
        rt.close()
    r.close(); sb.close(); cam.close()


def test_frames_beyond_one_chunk_equal_single_chunk_tiles(pkg, device, wide, scenes):
    scene = scenes["spheres"]
    W = H = 256
    s = 8                                                   # 256 * 256 * 65 rays: chunks of 126, 126 and 4 rows (2^21 rays at most)
    assert W * H * (s * s + 1) > pkg.capi.AOV_CHUNK_RAYS
    cam = make_camera(pkg, scene, W, H)
    r, sb = renderer(pkg, device, scene, W, H)
    r.set_camera(cam.buffer)
    whole = r.aovs(s).cpu().numpy().view(np.uint32)
    assert (pkg.capi.aov_fields(whole.view(np.float32))["coverage"] > 0).sum() > 1000
    # tiles of 64 x 64 pixels: 266 240 rays each, one chunk
    for y0 in range(0, H, 64):
        for x0 in range(0, W, 64):
            rt = pkg.capi.Renderer(device, 64, 64, pool_paths=4096, tile=(x0, y0))
            rt.bind_scene(sb); rt.set_camera(cam.buffer)
            assert np.array_equal(rt.aovs(s).cpu().numpy().view(np.uint32), whole[y0:y0 + 64, x0:x0 + 64]), (x0, y0)
            rt.close()
    r.close(); sb.close(); cam.close()


def test_bench_scene_sample_matches_the_oracle(pkg, device, wide):
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    W, H = 1920, 1080
    cam = make_camera(pkg, scene, W, H)
    r, sb = renderer(pkg, device, scene, W, H, pool=1 << 16)
    r.set_camera(cam.buffer)
    got = r.aovs(1).cpu().numpy().reshape(-1, 16)
    pick = np.sort(np.random.default_rng(1234).choice(W * H, 65536, replace=False))
    xs, ys = (pick % W).tolist(), (pick // W).tolist()
    rays = pkg.capi.aov_rays(cam.buffer, xs, ys, 1)
    truth = oracle_rays(scene, rays.reshape(-1, 8), cam.buffer)
    compare_records(scene, got[pick], *expected(scene, rays, truth, 1, cam.buffer))
    c = categories(scene, truth)
    assert c["surface"] > 30000, c
    r.close(); sb.close(); cam.close()


def test_aovs_leave_the_renderer_untouched(pkg, device, wide, scenes):
    scene = scenes["textured"]
    W, H, P = 48, 27, 4096
    sb = pkg.capi.SceneBuffers(device, scene)
    runs = []
    for with_aovs in (False, True):
        r = pkg.capi.Renderer(device, W, H, pool_paths=P)
        r.bind_scene(sb)
        cam = make_camera(pkg, scene, W, H)
        for it in range(12):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if with_aovs and it % 3 == 1:
                r.aovs(1); r.aovs(3)
        r.synchronize()
        st = r.stats().as_dict()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), st))
        r.close(); cam.close()
    sb.close()
    (fa, sa, qa, ca, ta), (fb, sbb, qb, cb, tb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb
    assert int(fa[..., 3].view(np.uint32).sum()) > 0


def test_session_aovs(pkg, device, wide, scenes):
    scene = scenes["cornell"]
    W, H = 64, 36
    r, sb = renderer(pkg, device, scene, W, H)
    cam = make_camera(pkg, scene, W, H)
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    sess.frame()
    f = sess.aovs(2)
    direct = r.aovs(2).cpu().numpy().view(np.uint32)
    assert f["normal"].shape == (H, W, 3) and f["depth"].shape == (H, W)
    assert np.array_equal(f["albedo"].view(np.uint32), direct[..., 0:3]) and np.array_equal(f["triangle"].view(np.uint32), direct[..., 12])
    r.close(); sb.close(); cam.close()


def test_errors(pkg, device, monkeypatch, scenes):
    capi = pkg.capi
    lib = capi.lib()
    scene = scenes["cornell"]
    W, H = 32, 18
    out = torch.empty((H, W, 16), dtype=torch.float32, device="cuda")
    P = C.c_void_p
    ptr = P(out.data_ptr())
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    r = capi.Renderer(device, W, H, pool_paths=1024)
    cam = make_camera(pkg, scene, W, H)
    assert lib.gmupt_render_aovs(r.h, 1, ptr, out.numel() * 4, None) == capi.ERR_NOT_BOUND     # no scene
    sb = capi.SceneBuffers(device, scene)
    r.bind_scene(sb)
    assert lib.gmupt_render_aovs(r.h, 1, ptr, out.numel() * 4, None) == capi.ERR_NOT_BOUND     # no camera
    with pytest.raises(capi.GmuptError, match="camera") as e:
        r.aovs(1)
    assert e.value.code == capi.ERR_NOT_BOUND
    r.set_camera(cam.buffer)
    nbytes = out.numel() * 4
    assert lib.gmupt_render_aovs(r.h, 1, None, nbytes, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_aovs(r.h, 1, P(out.data_ptr() + 4), nbytes, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_aovs(r.h, 1, ptr, nbytes - 64, None) == capi.ERR_INVALID_ARGUMENT
    for s in (0, 9):
        assert lib.gmupt_render_aovs(r.h, s, ptr, nbytes, None) == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.GmuptError) as e:
        r.aovs(12)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    info = capi.TraceInfo()
    assert lib.gmupt_render_aovs(r.h, 2, ptr, nbytes, C.byref(info)) == 0 and info.flags & capi.STAT_CAST_WIDE   # still usable
    r.close(); sb.close()
    # a row wider than one chunk at s = 8: 40 000 pixels * 65 rays
    wide_r = capi.Renderer(device, 40000, 1, pool_paths=1024)
    sb = capi.SceneBuffers(device, scene)
    wide_r.bind_scene(sb); wide_r.set_camera(cam.buffer)
    big = torch.empty((1, 40000, 16), dtype=torch.float32, device="cuda")
    assert lib.gmupt_render_aovs(wide_r.h, 8, P(big.data_ptr()), big.numel() * 4, None) == capi.ERR_INVALID_ARGUMENT
    assert b"2^21" in lib.gmupt_last_error()
    wide_r.aovs(7)                                          # 40 000 * 50 rays fit one chunk
    wide_r.close(); sb.close()
    monkeypatch.setenv("GMUPT_TRAVERSAL", "cast0")
    r, sb = renderer(pkg, device, scene, W, H, pool=1024)
    r.set_camera(cam.buffer)
    with pytest.raises(capi.GmuptError, match="wide collapse") as e:
        r.aovs(1)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.GmuptError) as e2:
        r.trace(torch.zeros((4, 8), dtype=torch.float32, device="cuda"), None)
    assert e2.value.code == capi.ERR_UNSUPPORTED                                  # the same condition as the ray queries
    r.close(); sb.close(); cam.close()


def read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert scale == b"-1.0"
    c = 3 if kind == b"PF" else 1
    assert kind in (b"PF", b"Pf")
    return np.frombuffer(body, "<f4").reshape(h, w, c)[::-1]


def test_cpp_driver_writes_the_aov_files(pkg, device, wide, tmp_path):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    exe = os.path.join(HOST, "gmupt_render")
    W, H, frames, s = 64, 36, 3, 2
    prefix = str(tmp_path / "cb")
    subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", "4096", "--live", "4096",
                    "--aov", prefix, "--aov-samples", str(s)], check=True, cwd=str(tmp_path))
    raw = np.fromfile(prefix + ".aov", dtype=np.float32).reshape(H, W, 16)
    # the same scene through the C-ABI: the C++ loader's mesh with the cornell scene's lights and camera; camera and lights as the driver has them
    dump = str(tmp_path / "cornell.gmesh")
    subprocess.run([exe, "--build-only", "--scene", "cornell", "--dump-mesh", dump], check=True, capture_output=True)
    mesh = dict(pkg.scenes.load_gmesh(dump))
    like = pkg.scenes.cornell_mesh()
    for k in ("lights", "light_count", "camera", "name"):
        mesh[k] = like[k]
    scene = pkg.scenes.build_scene(mesh)
    r, sb = renderer(pkg, device, scene, W, H)
    cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = max(2, scene["light_count"])
    for _ in range(frames):
        cam.update(0.0)
    r.set_camera(cam.buffer)
    ref = r.aovs(s).cpu().numpy()
    assert np.array_equal(raw.view(np.uint32), ref.view(np.uint32))
    f = pkg.capi.aov_fields(ref)
    assert np.array_equal(read_pfm(prefix + "_albedo.pfm").view(np.uint32), f["albedo"].view(np.uint32))
    assert np.array_equal(read_pfm(prefix + "_normal.pfm").view(np.uint32), f["normal"].view(np.uint32))
    assert np.array_equal(read_pfm(prefix + "_depth.pfm")[..., 0].view(np.uint32), f["depth"].view(np.uint32))
    assert (f["triangle"] >= 0).sum() > W * H // 2
    r.close(); sb.close(); cam.close()

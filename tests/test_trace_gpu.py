"""GPU tests of the ray-query API (gmupt_trace_rays / gmupt_pick): k_cast_w with the QueryIO policy on caller rays.

Truth is the CPU oracle's own extension / shadow stages on a frozen state (trace_util.oracle_truth), compared bit for bit
(trace_util.assert_matches_oracle).
"""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the query's rays and outputs are torch tensors)

import oracle_lib as O
from trace_util import FLT_MAX, NO_TRI, assert_matches_oracle, make_rays, oracle_truth, random_rays

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


def renderer(pkg, device, scene, pool=4096, **kw):
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, 32, 18, pool_paths=pool, **kw)
    r.bind_scene(sb)
    return r, sb


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scenes(pkg):
    return {"soup": pkg.scenes.build_scene(pkg.scenes.random_triangles_mesh(2000, seed=1)),
            "cornell": pkg.scenes.build_scene(pkg.scenes.cornell_mesh()),
            "spheres": pkg.scenes.build_scene(pkg.scenes.spheres_mesh(n_spheres=12, subdiv=2, seed=7, floor_quads=4))}


@pytest.mark.parametrize("name", ["soup", "cornell", "spheres"])
def test_random_rays_match_the_oracle(pkg, device, wide, scenes, name):
    scene = scenes[name]
    rng = np.random.default_rng(5)
    closest, any_rays = random_rays(scene, 4096, rng)
    r, sb = renderer(pkg, device, scene)
    for lc in (0, scene["light_count"]):
        info = pkg.capi.TraceInfo()
        hits, occ = r.trace(gpu(closest), gpu(any_rays), light_count=lc, info=info)
        torch.cuda.synchronize()
        assert hits.shape == (4096, 8) and occ.shape == (4096,) and hits.is_cuda
        assert info.flags & pkg.capi.STAT_CAST_WIDE and info.ms > 0
        h, o = hits.cpu().numpy(), occ.cpu().numpy()
        assert_matches_oracle(scene, closest, any_rays, h, o, lc)
        f = pkg.capi.hit_fields(h)
        assert (f["triangle"] >= 0).sum() > 100 and o.sum() > 100 and (o == 0).sum() > 100
        if lc:
            assert name != "cornell" or (f["light"] > 0).sum() > 0
        else:
            assert (f["light"] == 0).all()
    r.close(); sb.close()


def grid_scene(pkg, seed):
    rng = np.random.default_rng(seed)
    n_tris = int(rng.integers(20, 400)); grid = int(rng.choice([3, 5, 9])); nv = max(4, n_tris // 2)
    verts = (rng.integers(0, grid, (nv, 3)) * (8.0 / (grid - 1)) - 4.0).astype(np.float32)
    idx = rng.integers(0, nv, (n_tris, 3)).astype(np.int32)
    idx[: n_tris // 5] = idx[n_tris // 5: 2 * (n_tris // 5)][: n_tris // 5]
    mesh = pkg.scenes.cornell_mesh()
    mesh.update({"verts": verts, "normals": np.tile(np.array([0.0, 1.0, 0.0], np.float32), (nv, 1)), "indices": idx,
                 "vertex_material": rng.integers(0, 3, nv).astype(np.uint32), "name": "grid%d" % seed})
    mesh.pop("uv", None)
    scene = pkg.scenes.build_scene(mesh)
    P = 4096
    pts = (rng.integers(0, grid, (P, 3)) * (8.0 / (grid - 1)) - 4.0).astype(np.float32)
    dirs = rng.integers(-2, 3, (P, 3)).astype(np.float32); dirs[(dirs == 0).all(axis=1)] = (1.0, 0.0, 0.0)
    nz = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), (P, 3))
    dirs[np.arange(P) % 3 == 0] = nz[np.arange(P) % 3 == 0]
    dirs[: P // 2] /= np.linalg.norm(dirs[: P // 2], axis=1, keepdims=True)
    o = (pts - dirs * rng.integers(1, 4, (P, 1)).astype(np.float32)).astype(np.float32)
    return scene, make_rays(o, dirs, FLT_MAX), make_rays(o, dirs, rng.uniform(0.5, 12.0, P).astype(np.float32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_grid_meshes_with_exact_ties(pkg, device, wide, seed):
    # coplanar duplicates, zero direction components, origins on box planes: ties go to the exact walk, whose ray re-fetch is the policy's
    scene, closest, any_rays = grid_scene(pkg, seed)
    r, sb = renderer(pkg, device, scene)
    info = pkg.capi.TraceInfo()
    hits, occ = r.trace(gpu(closest), gpu(any_rays), light_count=scene["light_count"], info=info)
    assert info.redo_rays > 0, "exact ties must go to the exact walk"
    assert_matches_oracle(scene, closest, any_rays, hits.cpu().numpy(), occ.cpu().numpy(), scene["light_count"])
    r.close(); sb.close()


def test_ties_without_zero_components(pkg, device, wide):
    mesh = pkg.scenes.cornell_mesh()
    verts = np.array([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2], [-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2],
                      [0, 1, 0], [1, 1, 0], [0, 1, 1], [-1, 1, 0], [0, 1, -1]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [8, 9, 10], [8, 10, 11], [8, 11, 12], [8, 12, 9]], np.int32)
    mesh.update({"verts": verts, "normals": np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(verts), 1)), "indices": idx,
                 "vertex_material": np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2], np.uint32), "name": "ties"})
    mesh.pop("uv", None)
    scene = pkg.scenes.build_scene(mesh)
    P = 2048
    rng = np.random.default_rng(11)
    target = np.zeros((P, 3), np.float32)
    target[:, 0] = rng.integers(-7, 8, P) * 0.25; target[:, 2] = rng.integers(-7, 8, P) * 0.25
    target[P // 2:] = (0.0, 1.0, 0.0); target[P // 2:, 0] += rng.integers(-2, 3, P - P // 2) * 0.25
    dirs = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0], np.float32), (P, 3)); dirs[:, 1] = -np.abs(dirs[:, 1])
    o = (target - dirs * rng.integers(1, 5, (P, 1)).astype(np.float32)).astype(np.float32)
    closest, any_rays = make_rays(o, dirs, FLT_MAX), make_rays(o, dirs, rng.uniform(0.5, 12.0, P).astype(np.float32))
    r, sb = renderer(pkg, device, scene)
    info = pkg.capi.TraceInfo()
    hits, occ = r.trace(gpu(closest), gpu(any_rays), info=info)
    assert info.redo_rays > P // 8
    assert_matches_oracle(scene, closest, any_rays, hits.cpu().numpy(), occ.cpu().numpy(), 0)
    r.close(); sb.close()


@pytest.mark.parametrize("name", ["soup", "spheres"])
def test_tiny_stacks_park_rays_for_the_exact_walk(pkg, monkeypatch, scenes, name):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    scene = scenes[name]
    closest, any_rays = random_rays(scene, 4096, np.random.default_rng(9))
    with pkg.capi.use_build("wides8"):
        dev = pkg.capi.Device(0)
        r, sb = renderer(pkg, dev, scene)
        info = pkg.capi.TraceInfo()
        hits, occ = r.trace(gpu(closest), gpu(any_rays), light_count=scene["light_count"], info=info)
        assert info.redo_rays > (500 if name == "soup" else 0) and not (info.flags & (pkg.capi.STAT_STACK_OVERFLOW | pkg.capi.STAT_CAST_ABORTED))
        h, o = hits.cpu().numpy(), occ.cpu().numpy()
        r.close(); sb.close(); dev.close()
    assert_matches_oracle(scene, closest, any_rays, h, o, scene["light_count"])


def test_finite_tmax_for_closest_hits(pkg, device, wide, scenes):
    scene = scenes["spheres"]
    rng = np.random.default_rng(21)
    closest, _ = random_rays(scene, 4096, rng)
    lc = scene["light_count"]
    truth = oracle_truth(scene, closest, closest[:0], lc)
    t_ref = truth["hitDistance"][:, 0].view(np.float32)[:4096]
    limited = closest.copy()
    with np.errstate(over="ignore"):
        limited[:, 3] = np.where(rng.random(4096) < 0.5, t_ref * np.float32(rng.uniform(0.3, 0.99)), t_ref * np.float32(1.5)).astype(np.float32)
    limited[:64, 3] = t_ref[:64]            # exactly the oracle's t: strict `t < distance` makes it a miss
    limited[~np.isfinite(limited[:, 3]), 3] = FLT_MAX
    r, sb = renderer(pkg, device, scene)
    hits, _ = r.trace(gpu(limited), None, light_count=lc)
    f = pkg.capi.hit_fields(hits)
    below = t_ref < limited[:, 3]
    assert below.sum() > 500 and (~below).sum() > 500
    ref_tri = truth["triangle"][:4096, 0] != NO_TRI
    # below tmax: the oracle's hit (its triangle part: a light sphere can only be nearer); not below: a miss at t = tmax -- unless a light sphere is
    hu = hits.cpu().numpy().view(np.uint32)
    sel = below & (truth["isEmitter"][:4096, 0] == 0)
    assert np.array_equal(hu[sel, 0], truth["hitDistance"][:4096, 0][sel])
    assert np.array_equal(f["triangle"][sel] >= 0, ref_tri[sel])
    miss = ~below & (f["light"] == 0)
    assert (f["triangle"][miss] == -1).all() and np.array_equal(f["t"][miss], limited[miss, 3]) and not f["u"][miss].any() and not f["v"][miss].any()
    r.close(); sb.close()


def test_batch_shapes_and_a_batch_larger_than_the_pool(pkg, device, wide, scenes):
    scene = scenes["soup"]
    rng = np.random.default_rng(2)
    r, sb = renderer(pkg, device, scene, pool=1 << 12)
    info = pkg.capi.TraceInfo()
    h, o = r.trace(None, None, info=info)
    assert h.shape == (0, 8) and o.shape == (0,) and info.redo_rays == 0
    closest, any_rays = random_rays(scene, 3 << 20, rng)
    c, a = gpu(closest), gpu(any_rays)
    hits, occ = r.trace(c, a, light_count=2)
    h_only, none = r.trace(c[:5000], None, light_count=2)
    bits = lambda t: t.view(torch.int32)      # (the triangle word of a miss, -1, is a NaN pattern as float32: compare bits)
    assert none.shape == (0,) and torch.equal(bits(h_only), bits(hits[:5000]))
    nothing, o_only = r.trace(None, a[:7000], light_count=2)
    assert nothing.shape == (0, 8) and torch.equal(o_only, occ[:7000])
    parts = [r.trace(c[k:k + (1 << 20)], a[k:k + (1 << 20)], light_count=2) for k in range(0, 3 << 20, 1 << 20)]
    assert torch.equal(bits(torch.cat([p[0] for p in parts])), bits(hits)) and torch.equal(torch.cat([p[1] for p in parts]), occ)
    # numpy in, numpy out
    hn, on = r.trace(closest[:1000], any_rays[:1000], light_count=2)
    assert isinstance(hn, np.ndarray) and on.dtype == np.uint32 and np.array_equal(hn.view(np.uint32), hits[:1000].cpu().numpy().view(np.uint32))
    sub = np.r_[0:200, (3 << 20) - 200:(3 << 20)]
    assert_matches_oracle(scene, closest[sub], any_rays[sub], hits.cpu().numpy()[sub], occ.cpu().numpy()[sub], 2)
    r.close(); sb.close()


def test_queries_leave_the_renderer_untouched(pkg, device, wide, scenes):
    scene = scenes["cornell"]
    W, H, P = 48, 27, 4096
    sb = pkg.capi.SceneBuffers(device, scene)
    runs = []
    closest, any_rays = random_rays(scene, 20000, np.random.default_rng(4))
    c, a = gpu(closest), gpu(any_rays)
    for with_queries in (False, True):
        r = pkg.capi.Renderer(device, W, H, pool_paths=P)
        r.bind_scene(sb)
        cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        for it in range(12):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if with_queries and it % 3 == 1:
                r.trace(c, a, light_count=2)
                r.pick(10, 20, 2)
        r.synchronize()
        st = r.stats().as_dict()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), st))
        r.close(); cam.close()
    sb.close()
    (fa, sa, qa, ca, ta), (fb, sbb, qb, cb, tb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb
    assert int(fa[..., 3].view(np.uint32).sum()) > 0


def test_pipeline_rays_equal_the_renderers_own_cast(pkg, device, wide):
    # the bench scene (~260k triangles) at pool 2^16: one iteration's extension and shadow rays, read after the shading stage, traced as one
    # call; k_cast_w then casts the same rays for the renderer: the two answers are the same bits
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    P, W, H = 1 << 16, 1920, 1080
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=P)
    r.bind_scene(sb)
    cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    for _ in range(6):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    cam.update(0.0); r.set_camera(cam.buffer)
    r.run_stage(pkg.capi.STAGE_SHADE)
    st, q, qc = r.read_path_state(), r.read_queues(), r.counters()
    ext = q[3][: qc[7]]; ext = ext[ext != 0xFFFFFFFF]
    sh = q[4][: qc[6]]
    f32 = lambda name: O.state_field(st, P, name).view(np.float32)
    closest = make_rays(f32("rayOrigin")[ext], f32("rayDirection")[ext], FLT_MAX)
    any_rays = make_rays(f32("shadowrayOrigin")[sh], f32("shadowrayDirection")[sh], f32("lightDistance")[sh, 0])
    assert len(ext) > 10000 and len(sh) > 1000
    hits, occ = r.trace(gpu(closest), gpu(any_rays), light_count=scene["light_count"])
    r.run_stage(pkg.capi.STAGE_RAYCASTS)
    after = r.read_path_state()
    u = lambda name: O.state_field(after, P, name)
    h = hits.cpu().numpy().view(np.uint32)
    assert np.array_equal(h[:, 0], u("hitDistance")[ext, 0]) and np.array_equal(h[:, 4], u("isEmitter")[ext, 0])
    tri = h[:, 3].view(np.int32); hit = tri >= 0
    recs = scene["tris"].view(np.uint32).reshape(-1, 4)
    assert np.array_equal(recs[tri[hit]], u("triangle")[ext][hit]) and np.array_equal(h[hit, 1:3], u("baryCoord")[ext][hit, 1:3])
    assert np.array_equal(occ.cpu().numpy().astype(np.uint32), u("inShadow")[sh, 0])
    r.close(); sb.close(); cam.close()


def test_pick(pkg, device, wide, scenes):
    scene = scenes["cornell"]
    W, H = 96, 54
    lc = scene["light_count"]
    r, sb = renderer(pkg, device, scene)
    cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = lc; cam.update(0.0)
    with pytest.raises(pkg.capi.GmuptError) as e:
        r.pick(3, 4, lc)                                    # no camera set yet
    assert e.value.code == pkg.capi.ERR_NOT_BOUND
    r.set_camera(cam.buffer)
    # every pixel centre through the query; the pick call agrees with it and with the oracle
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.stack([np.frombuffer(bytes(pkg.capi.camera_pick_ray(cam.buffer, x, y)), np.float32) for x, y in zip(xs.ravel(), ys.ravel())])
    hits, _ = r.trace(gpu(rays), None, light_count=lc)
    hits = hits.cpu().numpy()
    assert_matches_oracle(scene, rays, rays[:0], hits, np.zeros(0, np.uint32), lc)
    f = pkg.capi.hit_fields(hits)
    lit = np.nonzero(f["light"] > 0)[0]
    assert len(lit) > 0, "the Cornell camera sees a light sphere"
    for k in [0, 1, W * 20 + 33, int(lit[0]), int(lit[-1])]:
        ray, hit = r.pick(xs.ravel()[k], ys.ravel()[k], lc)
        assert bytes(ray) == rays[k].tobytes() and bytes(hit) == hits[k].tobytes()
    ray, hit = r.pick(xs.ravel()[lit[0]], ys.ravel()[lit[0]], lc)
    assert hit.light > 0
    # tile mode: a band renderer shares the whole frame's camera, the same pixel gives the same answer
    sb2 = pkg.capi.SceneBuffers(device, scene)
    rt = pkg.capi.Renderer(device, W, 18, pool_paths=4096, tile=(0, 30))
    rt.bind_scene(sb2); rt.set_camera(cam.buffer)
    for k in [5, int(lit[0]), W * 40 + 7]:
        assert bytes(rt.pick(xs.ravel()[k], ys.ravel()[k], lc)[1]) == hits[k].tobytes()
    # the session's pick: the editor's selection and the world-space point
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    sel = sess.pick(xs.ravel()[lit[0]], ys.ravel()[lit[0]])
    assert sel["light"] == hits[lit[0]].view(np.uint32)[4] and sel["point"] is not None
    k = W * 27 + 48
    sel = sess.pick(48, 27)
    assert sel["triangle"] == f["triangle"][k] and sel["material"] == f["material"][k]
    assert np.array_equal(sel["point"], rays[k, 0:3] + rays[k, 4:7] * np.float32(f["t"][k]))
    rt.close(); sb2.close(); r.close(); sb.close(); cam.close()


def test_errors(pkg, device, monkeypatch, scenes):
    capi = pkg.capi
    lib = capi.lib()
    scene = scenes["soup"]
    rays = gpu(np.tile(np.array([0, 0, 0, 1, 0, 0, 1, 0], np.float32), (4, 1))); out = torch.empty((4, 8), dtype=torch.float32, device="cuda")
    occ = torch.empty(4, dtype=torch.int32, device="cuda")
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    r = capi.Renderer(device, 32, 18, pool_paths=1024)
    with pytest.raises(capi.GmuptError) as e:
        r.trace(rays, None)
    assert e.value.code == capi.ERR_NOT_BOUND
    sb = capi.SceneBuffers(device, scene)
    r.bind_scene(sb)
    P = C.c_void_p
    assert lib.gmupt_trace_rays(r.h, None, 4, P(out.data_ptr()), None, 0, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_trace_rays(r.h, P(rays.data_ptr()), 4, None, None, 0, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_trace_rays(r.h, None, 0, None, P(rays.data_ptr()), 4, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_trace_rays(r.h, P(rays.data_ptr() + 4), 3, P(out.data_ptr()), None, 0, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    big = capi.MAX_TRACE_BATCH + 1
    assert lib.gmupt_trace_rays(r.h, P(rays.data_ptr()), big, P(out.data_ptr()), None, 0, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_trace_rays(r.h, None, 0, None, P(rays.data_ptr()), big, P(occ.data_ptr()), 0, None) == capi.ERR_INVALID_ARGUMENT
    assert b"2^26" in lib.gmupt_last_error()
    r.trace(rays, rays)                                      # still usable
    r.close(); sb.close()
    monkeypatch.setenv("GMUPT_TRAVERSAL", "cast0")
    r, sb = renderer(pkg, device, scene, pool=1024)
    with pytest.raises(capi.GmuptError, match="wide collapse") as e:
        r.trace(rays, rays)
    assert e.value.code == capi.ERR_UNSUPPORTED
    r.close(); sb.close()

"""GPU tests of the refit (gmupt_renderer_refit): a renderer bound to the ORIGINAL scene, its vertex buffer updated, refitted -- against
  - gmupt_bvh_refit_host for the node buffer, bit for bit;
  - the CPU oracle on scenes.refit_scene(scene, moved) for frames and path state, bit for bit (parity_util);
  - a fresh renderer bound to scenes.refit_scene(scene, moved) for ray queries, AOVs, the denoiser and picking, record for record.
"""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the query's rays and outputs are torch tensors)

import oracle_lib as O
import parity_util as PU

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
SCENES = ["cornell", "soup", "spheres", "chain", "textured"]


@pytest.fixture(scope="module")
def scenes5(pkg, cornell_scene, soup_scene, spheres_small_scene):
    S = pkg.scenes
    return {"cornell": cornell_scene, "soup": soup_scene, "spheres": spheres_small_scene,
            "chain": S.build_scene(S.deep_chain_mesh()), "textured": S.build_scene(S.textured_mesh())}


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


def make_rays(origins, dirs, tmax):
    r = np.zeros((len(origins), 8), np.float32)
    r[:, 0:3] = origins; r[:, 3] = tmax; r[:, 4:7] = dirs
    return r


def query_rays(scene, n=4096, seed=11):
    """Random rays, rays with zero direction components, and rays that start in and run along face planes of leaf boxes of `scene`."""
    rng = np.random.default_rng(seed)
    lo, hi = scene["verts"].min(axis=0), scene["verts"].max(axis=0)
    ext = (hi - lo).max()
    o = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (n, 3)).astype(np.float32)
    target = scene["verts"][rng.integers(0, len(scene["verts"]), n)] + rng.normal(0, 0.02 * ext, (n, 3))
    d = (target - o).astype(np.float32)
    rays = [make_rays(o, d, FLT_MAX)]
    dz = d.copy()
    dz[np.arange(n), rng.integers(0, 3, n)] = 0.0
    dz[: n // 4, 0] = 0.0; dz[: n // 4, 1] = 0.0; dz[: n // 4, 2] = np.where(rng.random(n // 4) < 0.5, -1.0, 1.0)
    rays.append(make_rays(o, dz, FLT_MAX))
    nodes = scene["nodes"]
    leaves = np.flatnonzero((nodes["isLeaf"] != 0) & (nodes["right"] > nodes["left"]))
    pick = leaves[rng.integers(0, len(leaves), n)]
    axis = rng.integers(0, 3, n)
    bmin, bmax = nodes["min"][pick], nodes["max"][pick]
    size = np.maximum(bmax - bmin, 1e-3 * ext)
    po = (bmin + rng.uniform(-0.5, 1.5, (n, 3)) * size).astype(np.float32)
    face = np.where(rng.random(n) < 0.5, bmin[np.arange(n), axis], bmax[np.arange(n), axis])
    po[np.arange(n), axis] = face                          # in the plane of a face of the leaf's box
    pd = rng.normal(0, 1, (n, 3)).astype(np.float32)
    pd[: n // 2] = ((bmin + rng.uniform(0, 1, (n, 3)) * size) - po)[: n // 2]   # half of them aimed at the box
    pd[np.arange(n), axis] = 0.0                           # and running along it
    rays.append(make_rays(po, pd, FLT_MAX))
    return np.concatenate(rays)


def shadow_rays(rays, seed=3):
    rng = np.random.default_rng(seed)
    a = rays.copy()
    a[:, 3] = rng.uniform(0.5, 40.0, len(a)).astype(np.float32)
    return a


def refitted_renderer(pkg, device, scene, moved_verts, W=48, H=27, P=2048, normals=None):
    """A renderer bound to `scene`, then given the moved vertices and refitted: (renderer, buffers, info)."""
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=P)
    r.bind_scene(sb)
    sb.verts.update(moved_verts)
    if normals is not None:
        props = scene["props"].copy(); props["normal"] = normals
        sb.props.update(props)
    info = r.refit()
    return r, sb, info


def fresh_renderer(pkg, device, scene, W=48, H=27, P=2048):
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=P)
    r.bind_scene(sb)
    return r, sb


def assert_nodes(pkg, sb, scene, moved_verts, what=""):
    got = sb.nodes.read(pkg.capi.bvh_node_dtype)
    want = pkg.capi.bvh_refit_host(scene["nodes"], scene["tris"], moved_verts)
    assert got.tobytes() == want.tobytes(), "%s: the refitted node buffer differs from gmupt_bvh_refit_host in %d nodes" % (
        what, int(np.sum(np.any(got.view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12), axis=1))))
    return want


def assert_same_queries(a, b, rays, light_count, what=""):
    sh = shadow_rays(rays)
    ha, oa = a.trace(closest=rays, any=sh, light_count=light_count)
    hb, ob = b.trace(closest=rays, any=sh, light_count=light_count)
    ha, hb = ha.view(np.uint32)[:, :6], hb.view(np.uint32)[:, :6]
    assert np.array_equal(ha, hb), "%s: %d of %d hit records differ from the fresh renderer's" % (what, int(np.any(ha != hb, axis=1).sum()), len(ha))
    assert np.array_equal(oa, ob), "%s: %d occlusion words differ" % (what, int((oa != ob).sum()))
    assert int((ha[:, 3].view(np.int32) >= 0).sum()) > len(rays) // 100, "%s: the query rays hit next to nothing" % what   # (a sanity check of the rays, not of the code: the chain scene is mostly empty space)


def wide_shape(r, cam_buffer):
    r.reset_stats(); r.set_camera(cam_buffer); r.iterate()
    s = r.stats()
    return s.flags, s.wide_nodes, s.wide_pairs, s.wide_top_nodes


# ---- 1, 3: boxes bit for bit, the tables' shape kept, ray queries equal to a fresh bind
@pytest.mark.parametrize("name", SCENES)
def test_refit_boxes_and_queries(pkg, device, wide, scenes5, name):
    capi = pkg.capi
    scene = scenes5[name]
    cam = capi.Camera(48, 27); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    for phase in (0, 0.3):
        w = pkg.scenes.wobble(scene, phase, 0.05)
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, 48, 27, pool_paths=2048)
        r.bind_scene(sb)
        before = wide_shape(r, cam.buffer)
        sb.verts.update(w)
        info = r.refit()
        print("refit %s phase %s: %r" % (name, phase, info))
        assert info["rebuilt"] == 0 and info["reason"] == 0, info
        assert info["levels"] >= 1 and info["opened_nodes"] >= 1 and info["ms"] > 0
        moved_nodes = assert_nodes(pkg, sb, scene, w, name)
        after = wide_shape(r, cam.buffer)
        assert before[0] & capi.STAT_CAST_WIDE and after[0] & capi.STAT_CAST_WIDE, (before, after)
        assert before[1:] == after[1:] and before[1] > 0, "the collapse must keep its shape: %r -> %r" % (before, after)
        moved = pkg.scenes.refit_scene(scene, w)
        assert moved["nodes"].tobytes() == moved_nodes.tobytes()
        fr, fsb = fresh_renderer(pkg, device, moved)
        assert_same_queries(r, fr, query_rays(moved), scene["light_count"], "%s phase %s" % (name, phase))
        info2 = r.refit()                                  # again on the same vertices: the same bytes
        assert info2["rebuilt"] == 0
        assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == moved_nodes.tobytes()
        assert_same_queries(r, fr, query_rays(moved, seed=12), scene["light_count"], "%s phase %s, second refit" % (name, phase))
        fr.close(); fsb.close(); r.close(); sb.close()
    cam.close()


# ---- 2: frames and path state against the oracle on the refitted scene, with each shipped ray cast and the tiny-stack build
def _parity_after_refit(pkg, dev, scene, W, H, P, L, iters):
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    normals = pkg.scenes.vertex_normals(w, scene["tris"]["v"])
    moved = pkg.scenes.refit_scene(scene, w, normals)
    orc, hip, ocam, hcam, sb = PU.make_pair(pkg, dev, scene, W, H, P, live=L)
    orc.close()
    orc = O.Renderer(moved, W, H, P, live=L, threads=8)
    sb.verts.update(w)
    sb.props.update(moved["props"])
    info = hip.refit()
    live = L or P
    for it in range(iters):
        PU.step_both(orc, hip, ocam, hcam)
        if it < 4 or it % 10 == 9 or it == iters - 1:
            bad = PU.compare_state(orc, hip, P, live)
            assert not bad, "iteration %d: path state differs: %r" % (it, bad[:4])
            assert np.array_equal(orc.counters(), hip.counters()), it
            assert np.array_equal(orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32)), "iteration %d: framebuffer differs" % it
    assert int(hip.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    st = hip.stats()
    hip.close(); sb.close(); orc.close()
    return info, st


PARITY = [("cornell", 64, 36, 4096, 0, 30), ("cornell", 32, 18, 8192, 6144, 12), ("soup", 48, 27, 2048, 0, 40),
          ("spheres", 48, 27, 2048, 0, 120), ("textured", 48, 27, 2048, 0, 40), ("chain", 48, 27, 2048, 0, 20)]


@pytest.mark.parametrize("kernel", ["wide", "cast0"])
@pytest.mark.parametrize("scene_name,W,H,P,L,iters", PARITY)
def test_refit_parity_with_the_oracle(pkg, device, monkeypatch, scenes5, kernel, scene_name, W, H, P, L, iters):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    info, st = _parity_after_refit(pkg, device, scenes5[scene_name], W, H, P, L, iters)
    assert info["rebuilt"] == 0, info
    assert bool(st.flags & pkg.capi.STAT_CAST_WIDE) == (kernel == "wide")
    assert (info["opened_nodes"] > 0) == (kernel == "wide")


@pytest.mark.parametrize("scene_name", ["soup", "spheres"])
def test_refit_parity_with_tiny_stacks(pkg, monkeypatch, scenes5, scene_name):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    with pkg.capi.use_build("wides8"):
        dev = pkg.capi.Device(0)
        info, st = _parity_after_refit(pkg, dev, scenes5[scene_name], 48, 27, 4096, 0, 20)
        dev.close()
    assert info["rebuilt"] == 0 and st.flags & pkg.capi.STAT_CAST_WIDE
    assert st.cast_redo_rays > 0 and not (st.flags & (pkg.capi.STAT_STACK_OVERFLOW | pkg.capi.STAT_CAST_ABORTED))


def test_refit_in_the_variants_build_rebuilds_on_the_host(pkg, monkeypatch, soup_scene):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    with pkg.capi.use_build("variants"):
        dev = pkg.capi.Device(0)
        info, st = _parity_after_refit(pkg, dev, soup_scene, 48, 27, 2048, 0, 12)
        dev.close()
    assert info["rebuilt"] == 1 and info["reason"] & pkg.capi.REFIT_VARIANTS_BUILD, info


# ---- 4: an animation and back to the first pose
def test_animation_three_steps_and_back(pkg, device, wide, soup_scene):
    capi = pkg.capi
    scene = soup_scene
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    r.bind_scene(sb)
    boxes = []
    for phase in (0.2, 0.45, 0.8, 0.2):
        w = pkg.scenes.wobble(scene, phase, 0.05)
        sb.verts.update(w)
        info = r.refit()
        assert info["rebuilt"] == 0, (phase, info)
        boxes.append(assert_nodes(pkg, sb, scene, w, "phase %s" % phase))
        moved = pkg.scenes.refit_scene(scene, w)
        fr, fsb = fresh_renderer(pkg, device, moved)
        assert_same_queries(r, fr, query_rays(moved), scene["light_count"], "phase %s" % phase)
        fr.close(); fsb.close()
    assert boxes[0].tobytes() == boxes[3].tobytes() and boxes[0].tobytes() != boxes[1].tobytes()
    r.close(); sb.close()


# ---- 5: the flat-child flag and the host fallback
def test_flat_child_falls_back_to_the_host_pass(pkg, device, wide, soup_scene):
    capi = pkg.capi
    scene = soup_scene
    v = scene["verts"].copy()
    t = scene["tris"]["v"]
    cz = v[t][:, :, 2].mean(axis=1)
    low = np.unique(t[cz < np.median(cz)])
    v[low, 2] = v[:, 2].min()                              # the lower half of the soup, by centroid, snapped onto the plane z = min z
    r, sb, info = refitted_renderer(pkg, device, scene, v)
    print("fallback refit: %r" % (info,))
    assert info["rebuilt"] == 1 and info["reason"] & capi.REFIT_FLAT_CHILD, info
    assert_nodes(pkg, sb, scene, v, "snapped")
    moved = pkg.scenes.refit_scene(scene, v)
    fr, fsb = fresh_renderer(pkg, device, moved)
    assert_same_queries(r, fr, query_rays(moved), scene["light_count"], "snapped")
    fr.close(); fsb.close()
    # back to a wobbled pose: the refit now works from the rebuilt tables
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    sb.verts.update(w)
    info = r.refit()
    assert_nodes(pkg, sb, scene, w, "after the fallback")
    moved = pkg.scenes.refit_scene(scene, w)
    fr, fsb = fresh_renderer(pkg, device, moved)
    assert_same_queries(r, fr, query_rays(moved), scene["light_count"], "after the fallback (rebuilt %d)" % info["rebuilt"])
    fr.close(); fsb.close(); r.close(); sb.close()


# ---- 6: errors
def test_refit_errors_write_nothing(pkg, device, wide, cornell_scene):
    capi = pkg.capi
    scene = cornell_scene
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    with pytest.raises(capi.GmuptError) as e:
        r.refit()
    assert e.value.code == capi.ERR_NOT_BOUND
    # a vertex no triangle record uses rides at the end of the vertex array
    spare = dict(scene)
    spare["verts"] = np.concatenate([scene["verts"], np.zeros((1, 3), np.float32)])
    spare["props"] = np.concatenate([scene["props"], np.zeros(1, capi.tri_props_dtype)])
    sb = capi.SceneBuffers(device, spare)
    r.bind_scene(sb)
    rays = query_rays(spare, n=1024)
    nodes0 = sb.nodes.read(capi.bvh_node_dtype).tobytes()
    hits0, _ = r.trace(closest=rays, light_count=0)
    used = int(scene["tris"]["v"][3, 1])
    for bad in (np.nan, np.inf, -np.inf):
        v = pkg.scenes.wobble(spare, 0.3, 0.05)
        v[used, 1] = bad
        sb.verts.update(v)
        with pytest.raises(capi.GmuptError) as e:
            r.refit()
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, e.value
        assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == nodes0, "a refused refit must not write the node buffer"
        hits1, _ = r.trace(closest=rays, light_count=0)
        assert np.array_equal(hits0.view(np.uint32), hits1.view(np.uint32)), "a refused refit must not write the traversal tables"
    v = pkg.scenes.wobble(spare, 0.3, 0.05)
    v[-1] = (np.nan, np.inf, -np.inf)                      # the unused vertex may hold anything
    sb.verts.update(v)
    info = r.refit()
    assert info["rebuilt"] == 0
    assert_nodes(pkg, sb, spare, v, "unused non-finite vertex")
    r.close(); sb.close()


# ---- 7: what rides on the same tables
def test_aovs_denoise_and_pick_after_refit(pkg, device, wide, spheres_small_scene):
    capi = pkg.capi
    scene = spheres_small_scene
    W, H, P = 64, 36, 4096
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    normals = pkg.scenes.vertex_normals(w, scene["tris"]["v"])
    moved = pkg.scenes.refit_scene(scene, w, normals)
    a, asb, info = refitted_renderer(pkg, device, scene, w, W, H, P, normals=normals)
    assert info["rebuilt"] == 0
    b, bsb = fresh_renderer(pkg, device, moved, W, H, P)
    cams = []
    for r in (a, b):
        cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        for _ in range(16):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        cams.append(cam)
    assert np.array_equal(a.framebuffer().view(np.uint32), b.framebuffer().view(np.uint32))
    for s in (1, 2):
        assert torch.equal(a.aovs(s).view(torch.int32), b.aovs(s).view(torch.int32)), "AOVs at %d samples" % s
    assert torch.equal(a.denoise().view(torch.int32), b.denoise().view(torch.int32))
    found = 0
    for px, py in [(5, 5), (32, 18), (20, 30), (50, 12), (63, 35)]:
        (_, ha), (_, hb) = a.pick(px, py, scene["light_count"]), b.pick(px, py, scene["light_count"])
        assert bytes(ha)[:24] == bytes(hb)[:24]
        found += ha.triangle >= 0
    assert found >= 3
    for c in cams:
        c.close()
    a.close(); asb.close(); b.close(); bsb.close()


# ---- 8: the progressive front-end's event
def test_progressive_session_set_vertices(pkg, device, wide, cornell_scene):
    capi = pkg.capi
    scene = cornell_scene
    W, H, P = 48, 27, 2048
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=P)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    sess = pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0)
    sess.run(10)
    first = sess.denoised_temporal()
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    info = sess.set_vertices(sb, w)
    assert info["rebuilt"] == 0
    assert cam.buffer.iterationCounter == -1, "the accumulation restarts"
    # a history existed and was dropped: the next temporal output is the plain denoiser's (consequence (a) of include/gmupt.h)
    assert first.shape == (H, W, 4)
    sess.run(6)
    assert_nodes(pkg, sb, scene, w, "session")
    assert np.array_equal(sess.denoised_temporal().view(np.uint32)[..., :3], sess.denoised().view(np.uint32)[..., :3])
    cam.close(); r.close(); sb.close()


def test_progressive_session_frame_equals_the_oracle(pkg, device, wide, cornell_scene):
    """set_vertices before the first frame: the N frames after it are the oracle's on the refitted scene, bit for bit."""
    capi = pkg.capi
    scene = cornell_scene
    W, H, P, N = 48, 27, 2048, 24
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    moved = pkg.scenes.refit_scene(scene, w)
    orc, hip, ocam, hcam, sb = PU.make_pair(pkg, device, scene, W, H, P)
    orc.close()
    orc = O.Renderer(moved, W, H, P, threads=8)
    sess = pkg.progressive.ProgressiveSession(hip, hcam, W, H, preview_every=0)
    sess.set_vertices(sb, w)
    ocam.buffer.iterationCounter = -1
    for it in range(N):
        sess.frame()
        ocam.update(); orc.set_camera(ocam.buffer); orc.iterate()
        assert bytes(ocam.buffer) == bytes(hcam.buffer), "host camera streams diverged"
    assert not PU.compare_state(orc, hip, P, P)
    assert np.array_equal(orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32))
    hip.close(); sb.close(); orc.close()


# ---- 9: full size (config 5: the tree is deeper than the LDS part of the stacks; the tables are the largest the project binds)
def test_refit_at_config5_size(pkg, device, wide):
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(1953, 4, seed=1234))
    assert 9_900_000 < scene["num_triangles"] < 10_100_000 and scene["depth"] + 2 > 24
    w = pkg.scenes.wobble(scene, 0.3, 0.01)
    r, sb, info = refitted_renderer(pkg, device, scene, w, 64, 36, 4096)
    print("config 5 refit: %r" % (info,))
    assert info["rebuilt"] == 0, info
    moved_nodes = assert_nodes(pkg, sb, scene, w, "config 5")
    moved = dict(scene); moved["verts"] = w; moved["nodes"] = moved_nodes
    rays = query_rays(moved, n=1 << 16, seed=5)[: 1 << 16]
    rays = np.concatenate([rays[: 1 << 15], query_rays(moved, n=1 << 14, seed=6)[1 << 14:]])   # random rays, then the special ones
    sh = shadow_rays(rays)
    ha, oa = r.trace(closest=rays, any=sh, light_count=scene["light_count"])
    r.close(); sb.close()
    fr, fsb = fresh_renderer(pkg, device, moved, 64, 36, 4096)
    hb, ob = fr.trace(closest=rays, any=sh, light_count=scene["light_count"])
    fr.close(); fsb.close()
    assert len(rays) == 1 << 16
    assert np.array_equal(ha.view(np.uint32)[:, :6], hb.view(np.uint32)[:, :6]) and np.array_equal(oa, ob)
    assert int((ha.view(np.int32)[:, 3] >= 0).sum()) > 1 << 12

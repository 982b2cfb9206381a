"""The GPU LBVH builder (gmupt_lbvh_build, csrc/pt_lbvh.hip) against its host reference gmupt_lbvh_build_host, bit for bit, and the built
tree under everything that takes a tree: bind, both shipped ray casts against the oracle, ray queries, AOVs, refit, the progressive
session's rebuild."""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the builder's indices are torch tensors)

import lbvh_util as LU
import oracle_lib as O
import parity_util as PU
from test_refit_gpu import assert_same_queries, query_rays, shadow_rays
from trace_util import assert_matches_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def builder(pkg, device):
    b = pkg.capi.Lbvh(device)
    yield b
    b.close()


def device_build(pkg, device, builder, mesh, L, with_material=True):
    """(nodes, tris, info with ref_triangle) of the device build of a mesh, read back."""
    capi = pkg.capi
    vb = capi.Buffer(device, capi.BUFFER_VERTICES, np.ascontiguousarray(mesh["verts"], np.float32))
    try:
        nb, tb, info = builder.build(vb, mesh["indices"], mesh["vertex_material"] if with_material else None, max_leaf_size=L, ref_triangle=True)
        try:
            return nb.read(capi.bvh_node_dtype), tb.read(capi.triangle_dtype), info
        finally:
            nb.close(); tb.close()
    finally:
        vb.close()


def assert_equals_host(pkg, device, builder, mesh, L, what, with_material=True):
    nodes, tris, info = device_build(pkg, device, builder, mesh, L, with_material)
    want = pkg.capi.lbvh_build_host(mesh["verts"], mesh["indices"], mesh["vertex_material"] if with_material else None, L)
    what = "%s, L = %d" % (what, L)
    assert len(nodes) == len(want["nodes"]) and len(tris) == len(want["tris"]), what
    assert np.array_equal(info["ref_triangle"], want["ref_triangle"]), what
    assert tris.tobytes() == want["tris"].tobytes(), what
    assert nodes.tobytes() == want["nodes"].tobytes(), "%s: %d of %d nodes differ" % (
        what, int(np.any(nodes.view(np.uint32).reshape(-1, 12) != want["nodes"].view(np.uint32).reshape(-1, 12), axis=1).sum()), len(nodes))
    for k in ("num_nodes", "num_leaves", "depth", "num_tris"):
        assert info[k] == want["info"][k], (what, k)
    assert info["root_min"].tobytes() == want["info"]["root_min"].tobytes() and info["root_max"].tobytes() == want["info"]["root_max"].tobytes()
    assert info["ms"] > 0
    return info


@pytest.mark.parametrize("L", [1, 4])
def test_device_build_equals_the_host_reference(pkg, device, builder, L):
    meshes = LU.crafted_meshes(4)
    for n in (63, 64, 65, 257, 5000):                       # around one wave, one block, several blocks
        meshes["soup%d" % n] = LU.soup(n, n)
    meshes["cornell"] = pkg.scenes.cornell_mesh()
    for name, mesh in meshes.items():
        assert_equals_host(pkg, device, builder, mesh, L, name)
    assert_equals_host(pkg, device, builder, meshes["soup257"], L, "no vertex_material", with_material=False)


def test_scratch_is_reused_and_grown(pkg, device):
    b = pkg.capi.Lbvh(device)
    for n in (300, 40, 300, 2100, 7):                       # smaller (the front of each part), the same again, larger (a new allocation), tiny
        assert_equals_host(pkg, device, b, LU.soup(n, 1000 + n), 4, "handle reused, %d triangles" % n)
    b.close()


def test_indices_as_a_device_tensor(pkg, device, builder):
    capi = pkg.capi
    mesh = LU.soup(130, 9)
    vb = capi.Buffer(device, capi.BUFFER_VERTICES, mesh["verts"])
    idx = torch.from_numpy(mesh["indices"]).cuda()
    vm = torch.from_numpy(mesh["vertex_material"].astype(np.int32)).cuda()
    nb, tb, info = builder.build(vb, idx, vm)
    want = capi.lbvh_build_host(mesh["verts"], mesh["indices"], mesh["vertex_material"])
    assert nb.read(capi.bvh_node_dtype).tobytes() == want["nodes"].tobytes() and tb.read(capi.triangle_dtype).tobytes() == want["tris"].tobytes()
    assert int(capi.lib().gmupt_buffer_size(nb.h)) == info["num_nodes"] * 48 and int(capi.lib().gmupt_buffer_size(tb.h)) == 130 * 16
    assert "ref_triangle" not in info
    nb.close(); tb.close(); vb.close()


class DeviceBuiltScene:
    """Scene buffers whose tree comes from the GPU builder: the mesh's vertices are uploaded, the nodes and triangle records are built on
    the device.  `scene` is the host-reference scene dict of the same mesh (what the oracle renders)."""

    def __init__(self, pkg, device, builder, mesh, L=4):
        capi = pkg.capi
        self.scene = pkg.scenes.build_scene(mesh, builder="lbvh", max_leaf_size=L)
        self.sb = capi.SceneBuffers(device, self.scene)
        self.sb.nodes.close(); self.sb.tris.close()
        self.sb.nodes, self.sb.tris, self.info = builder.build(self.sb.verts, mesh["indices"], mesh["vertex_material"], max_leaf_size=L)

    def close(self):
        self.sb.close()


@pytest.mark.parametrize("kernel", ["wide", "cast0"])
@pytest.mark.parametrize("scene_name,W,H,P,iters", [("cornell", 64, 36, 4096, 12), ("soup", 48, 27, 2048, 12)])
def test_frames_on_the_device_built_tree_equal_the_oracle(pkg, device, builder, monkeypatch, kernel, scene_name, W, H, P, iters):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    mesh = pkg.scenes.cornell_mesh() if scene_name == "cornell" else pkg.scenes.random_triangles_mesh(2000, seed=1)
    d = DeviceBuiltScene(pkg, device, builder, mesh)
    scene = d.scene
    orc = O.Renderer(scene, W, H, P, threads=8)
    hip = pkg.capi.Renderer(device, W, H, pool_paths=P)
    hip.bind_scene(d.sb)
    ocam = O.Camera(W, H); ocam.set_pose(*scene["camera"]); ocam.buffer.lightCount = scene["light_count"]
    hcam = pkg.capi.Camera(W, H); hcam.set_pose(*scene["camera"]); hcam.buffer.lightCount = scene["light_count"]
    for it in range(iters):
        PU.step_both(orc, hip, ocam, hcam)
        if it < 3 or it == iters - 1:
            bad = PU.compare_state(orc, hip, P, P)
            assert not bad, "iteration %d: path state differs: %r" % (it, bad[:4])
            assert np.array_equal(orc.counters(), hip.counters()), it
            assert np.array_equal(orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32)), "iteration %d: framebuffer differs" % it
    assert int(hip.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    assert bool(hip.stats().flags & pkg.capi.STAT_CAST_WIDE) == (kernel == "wide")
    hip.close(); hcam.close(); orc.close(); d.close()


def test_queries_and_aovs_on_the_device_built_tree(pkg, device, builder, wide, soup_scene):
    capi = pkg.capi
    mesh = pkg.scenes.random_triangles_mesh(2000, seed=1)                     # the mesh of soup_scene
    d = DeviceBuiltScene(pkg, device, builder, mesh)
    lb = capi.Renderer(device, 48, 27, pool_paths=2048); lb.bind_scene(d.sb)
    ssb = capi.SceneBuffers(device, soup_scene)
    sb = capi.Renderer(device, 48, 27, pool_paths=2048); sb.bind_scene(ssb)
    rays = query_rays(d.scene, n=4096)                                        # random rays, zero direction components, rays along leaf faces
    sh = shadow_rays(rays)
    lc = d.scene["light_count"]
    hits, occ = lb.trace(closest=rays, any=sh, light_count=lc)
    assert_matches_oracle(d.scene, rays, sh, hits, occ, lc)
    hits_s, occ_s = sb.trace(closest=rays, any=sh, light_count=lc)
    assert np.array_equal(hits.view(np.uint32)[:, 0], hits_s.view(np.uint32)[:, 0]), "closest-hit t must not depend on the tree"
    assert np.array_equal(hits.view(np.uint32)[:, 4], hits_s.view(np.uint32)[:, 4]) and np.array_equal(occ, occ_s)
    assert int((hits.view(np.int32)[:, 3] >= 0).sum()) > len(rays) // 10
    # AOVs: every field but the reference index is the tree's business of neither builder
    cam = capi.Camera(48, 27); cam.set_pose(*d.scene["camera"]); cam.buffer.lightCount = lc; cam.update(0.0)
    lb.set_camera(cam.buffer); sb.set_camera(cam.buffer)
    a, b = capi.aov_fields(lb.aovs(2).cpu().numpy()), capi.aov_fields(sb.aovs(2).cpu().numpy())
    for k in ("depth", "material", "light"):
        assert a[k].tobytes() == b[k].tobytes(), k
    hit = a["triangle"] >= 0
    assert hit.any() and np.array_equal(hit, b["triangle"] >= 0)
    # the centre ray's AOV record against the oracle's answer to gmupt_aov_ray
    xs, ys = np.meshgrid(np.arange(48), np.arange(27))
    centre = capi.aov_rays(cam.buffer, xs.ravel(), ys.ravel(), 2)[:, 0]
    h2, _ = lb.trace(closest=centre, light_count=lc)
    assert_matches_oracle(d.scene, centre, centre[:0], h2, np.zeros(0, np.uint32), lc)
    assert np.array_equal(a["depth"].ravel().view(np.uint32), h2.view(np.uint32)[:, 0]) and np.array_equal(a["triangle"].ravel(), h2.view(np.int32)[:, 3])
    cam.close(); lb.close(); sb.close(); ssb.close(); d.close()


def test_refit_after_a_bind_of_the_device_built_tree(pkg, device, builder, wide):
    capi = pkg.capi
    mesh = pkg.scenes.random_triangles_mesh(2000, seed=1)
    d = DeviceBuiltScene(pkg, device, builder, mesh)
    r = capi.Renderer(device, 48, 27, pool_paths=2048); r.bind_scene(d.sb)
    w = pkg.scenes.wobble(d.scene, 0.3, 0.05)
    d.sb.verts.update(w)
    info = r.refit()
    assert info["rebuilt"] == 0, info
    moved = pkg.scenes.refit_scene(d.scene, w)
    assert d.sb.nodes.read(capi.bvh_node_dtype).tobytes() == moved["nodes"].tobytes()
    fsb = capi.SceneBuffers(device, moved)
    f = capi.Renderer(device, 48, 27, pool_paths=2048); f.bind_scene(fsb)
    assert_same_queries(r, f, query_rays(moved), moved["light_count"], "refit of an LBVH")
    cam = capi.Camera(48, 27); cam.set_pose(*moved["camera"]); cam.buffer.lightCount = moved["light_count"]
    for _ in range(3):
        cam.update(0.0)
        r.set_camera(cam.buffer); f.set_camera(cam.buffer); r.iterate(); f.iterate()
    assert np.array_equal(r.framebuffer().view(np.uint32), f.framebuffer().view(np.uint32))
    assert np.array_equal(r.read_path_state(), f.read_path_state())
    cam.close(); f.close(); fsb.close(); r.close(); d.close()


def test_progressive_session_rebuild_with_a_changed_index_list(pkg, device, wide):
    capi, S = pkg.capi, pkg.scenes
    W, H, P = 48, 27, 2048
    mesh = S.cornell_mesh()
    cut = dict(mesh)
    cut["indices"] = np.ascontiguousarray(mesh["indices"][np.arange(len(mesh["indices"])) % 3 != 2])      # every third triangle dropped

    def session(m, builder_name):
        scene = S.build_scene(m, builder=builder_name)
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, W, H, pool_paths=P); r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        return pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0), sb, scene

    a, asb, _ = session(mesh, "sbvh")
    info = a.rebuild(asb, indices=cut["indices"], vertex_material=mesh["vertex_material"])   # before the first frame: both cameras draw the same seeds
    assert a.camera.buffer.iterationCounter == -1, "the accumulation restarts"
    b, bsb, bscene = session(cut, "lbvh")
    b.camera.reset_accumulation()
    assert info["num_tris"] == len(cut["indices"]) and info["num_nodes"] == len(bscene["nodes"]) and info["depth"] == bscene["depth"]
    assert asb.nodes.read(capi.bvh_node_dtype).tobytes() == bscene["nodes"].tobytes() and asb.tris.read(capi.triangle_dtype).tobytes() == bscene["tris"].tobytes()
    for _ in range(8):
        a.frame(); b.frame()
        assert bytes(a.camera.buffer) == bytes(b.camera.buffer), "host camera streams diverged"
    fa, fb = a.renderer.framebuffer(), b.renderer.framebuffer()
    assert int(fb[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), "after rebuild() the frames are those of a fresh session on the new mesh"
    assert np.array_equal(a.renderer.read_path_state(), b.renderer.read_path_state())
    # moved vertices, the remembered index list: the tree of the host reference; the history of the old geometry is dropped, so the next
    # temporal output is the plain denoiser's (consequence (a) of include/gmupt.h)
    assert a.denoised_temporal().shape == (H, W, 4)
    w = S.wobble(cut, 0.3, 0.05)
    a.rebuild(asb, verts=w)
    assert a.camera.buffer.iterationCounter == -1
    want = capi.lbvh_build_host(w, cut["indices"], mesh["vertex_material"])
    assert asb.nodes.read(capi.bvh_node_dtype).tobytes() == want["nodes"].tobytes() and asb.tris.read(capi.triangle_dtype).tobytes() == want["tris"].tobytes()
    a.run(6)
    assert np.array_equal(a.denoised_temporal().view(np.uint32)[..., :3], a.denoised().view(np.uint32)[..., :3])
    for s_, sbuf in ((a, asb), (b, bsb)):
        s_.close()
        s_.renderer.close(); s_.camera.close(); sbuf.close()


def test_errors_create_no_buffer(pkg, device, builder):
    capi = pkg.capi
    mesh = LU.soup(300, 77)
    v, t = mesh["verts"].copy(), mesh["indices"].copy()
    vb = capi.Buffer(device, capi.BUFFER_VERTICES, v)
    import ctypes as C

    def refused(indices, L=4, verts_h=vb.h):
        idx = torch.from_numpy(np.ascontiguousarray(indices, np.int32)).cuda()
        nodes, tris = C.c_void_p(0xDEAD), C.c_void_p(0xDEAD)
        p = capi.LbvhParams(L)
        torch.cuda.synchronize()
        rc = capi.lib().gmupt_lbvh_build(builder.h, verts_h, idx.data_ptr(), len(indices), None, C.byref(p), C.byref(nodes), C.byref(tris), None, None)
        assert not nodes.value and not tris.value, "an error hands out no buffer"
        return rc

    INVALID = -1
    t2 = t.copy(); t2[299, 1] = len(v)
    assert refused(t2) == INVALID
    t2[299, 1] = -5
    assert refused(t2) == INVALID
    assert refused(t, L=0) == INVALID and refused(t, L=65) == INVALID
    assert refused(t, verts_h=None) == INVALID
    v2 = v.copy(); v2[t[150, 2], 1] = np.inf
    vb.update(v2)
    assert refused(t) == INVALID
    with pytest.raises(capi.GmuptError) as e:
        builder.build(vb, t)
    assert e.value.code == INVALID and "finite" in str(e.value)
    # a vertex no triangle uses may hold anything; and the handle still builds after the errors
    unused = np.concatenate([v, [[np.nan, 0.0, np.inf]]]).astype(np.float32)
    vb2 = capi.Buffer(device, capi.BUFFER_VERTICES, unused)
    nb, tb, info = builder.build(vb2, t)
    want = capi.lbvh_build_host(v, t)
    assert nb.read(capi.bvh_node_dtype).tobytes() == want["nodes"].tobytes()
    nb.close(); tb.close(); vb2.close(); vb.close()

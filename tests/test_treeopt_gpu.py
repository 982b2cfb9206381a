"""The GPU treelet optimiser (gmupt_treeopt_run, csrc/pt_treeopt.hip) against its host reference gmupt_tree_optimize_host, byte for byte,
and the optimised tree under everything that takes a tree: the tree cost, bind, both shipped ray casts against the oracle, ray queries,
AOVs, refit, the progressive session's rebuild and its refit-or-rebuild policy."""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the session's builder takes torch tensors)

import oracle_lib as O
import parity_util as PU
import treecost_util as TU
import treeopt_util as TO
from test_refit_gpu import assert_same_queries, query_rays, shadow_rays
from trace_util import assert_matches_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def inputs(pkg):
    return TO.input_scenes(pkg.scenes, pkg.capi)


@pytest.fixture(scope="module")
def optimizer(pkg, device):
    o = pkg.capi.TreeOptimizer(device)
    yield o
    o.close()


def device_run(pkg, device, optimizer, nodes, passes):
    """(nodes, info) of the device run on a host array, read back."""
    capi = pkg.capi
    buf = capi.Buffer(device, capi.BUFFER_BVH_NODES, nodes)
    try:
        out, info = optimizer.run(buf, passes=passes)
        try:
            assert buf.read(capi.bvh_node_dtype).tobytes() == np.ascontiguousarray(nodes).tobytes(), "the input buffer is not modified"
            assert int(capi.lib().gmupt_buffer_size(out.h)) == len(nodes) * 48
            return out.read(capi.bvh_node_dtype), info
        finally:
            out.close()
    finally:
        buf.close()


def assert_equals_host(pkg, device, optimizer, nodes, passes, what):
    got, info = device_run(pkg, device, optimizer, nodes, passes)
    want, winfo = pkg.capi.tree_optimize_host(nodes, passes)
    what = "%s, %d passes" % (what, passes)
    assert not TO.info_differs(info, winfo), "%s: %r differ: device %r, host %r" % (what, TO.info_differs(info, winfo), info, winfo)
    assert got.tobytes() == want.tobytes(), "%s: %d of %d nodes differ" % (
        what, int(np.any(got.view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12), axis=1).sum()), len(got))
    assert info["ms"] > 0, what
    return got, info


@pytest.mark.parametrize("passes", [1, 3])
def test_device_equals_the_host_reference_on_the_crafted_inputs(pkg, device, optimizer, inputs, passes):
    rewritten = 0
    for key, scene in inputs.items():
        rewritten += assert_equals_host(pkg, device, optimizer, scene["nodes"], passes, "%s, L = %d" % key)[1]["treelets_rewritten"]
    assert rewritten > 0


@pytest.mark.parametrize("passes", [1, 3])
def test_device_equals_the_host_reference_on_40000_nodes(pkg, device, optimizer, passes):
    """20 000 triangles at L = 1: 39 999 nodes, several workgroups at every lower level -- the smallest size at which a missed ordering
    between two levels could show."""
    mesh = pkg.scenes.random_triangles_mesh(20000, seed=3)
    nodes = pkg.capi.lbvh_build_host(mesh["verts"], mesh["indices"], mesh["vertex_material"], 1)["nodes"]
    assert len(nodes) == 39999
    _, info = assert_equals_host(pkg, device, optimizer, nodes, passes, "soup20000, L = 1")
    print("soup20000, L = 1, %d passes: %.3f ms, %d treelets rewritten, depth %d -> %d, cost %.6g -> %.6g" % (
        passes, info["ms"], info["treelets_rewritten"], info["depth_before"], info["depth_after"], info["cost_before"], info["cost_after"]))
    assert info["treelets_rewritten"] > 1000 and info["cost_after"] < info["cost_before"]


def test_scratch_is_reused_and_grown(pkg, device, inputs):
    o = pkg.capi.TreeOptimizer(device)
    order = [("soup2000", 4), ("soup8", 1), ("soup2000", 4), ("soup2000", 1), ("soup1", 1), ("cornell", 1)]   # smaller, the same again, larger, one record
    for key in order:
        assert_equals_host(pkg, device, o, inputs[key]["nodes"], 2, "handle reused, %s L = %d" % key)
    o.close()


def test_refusals_create_no_buffer_and_leave_the_handle_usable(pkg, device, optimizer, inputs):
    capi = pkg.capi
    good = inputs[("soup2000", 4)]["nodes"]
    deep = TO.chain_nodes(66, capi.bvh_node_dtype)
    inner = np.flatnonzero(good["isLeaf"] == 0)
    bad_link = good.copy(); bad_link["right"][inner[-1]] = int(inner[-1])
    shared = good.copy(); shared["right"][inner[0]] = shared["left"][inner[0]]
    info = capi.TreeoptInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    keep = bytes(info)

    def refused(nodes, passes=3):
        buf = capi.Buffer(device, capi.BUFFER_BVH_NODES, nodes)
        out = C.c_void_p(0xDEAD)
        p = capi.TreeoptParams(passes)
        rc = capi.lib().gmupt_treeopt_run(optimizer.h, buf.h, C.byref(p), C.byref(out), C.byref(info))
        assert not out.value and bytes(info) == keep, "an error hands out no buffer and leaves the info alone"
        buf.close()
        return rc

    for nodes, code in ((deep, capi.ERR_UNSUPPORTED), (bad_link, capi.ERR_INVALID_ARGUMENT), (shared, capi.ERR_INVALID_ARGUMENT)):
        assert refused(nodes) == code
        assert_equals_host(pkg, device, optimizer, good, 1, "after a refusal")        # refused and accepted runs interleaved
    assert refused(good, passes=0) == capi.ERR_INVALID_ARGUMENT and refused(good, passes=9) == capi.ERR_INVALID_ARGUMENT
    verts = capi.Buffer(device, capi.BUFFER_VERTICES, np.zeros((16, 3), np.float32))
    out = C.c_void_p(0xDEAD)
    assert capi.lib().gmupt_treeopt_run(optimizer.h, verts.h, None, C.byref(out), None) == capi.ERR_INVALID_ARGUMENT and not out.value
    verts.close()
    with pytest.raises(capi.GmuptError) as e:
        device_run(pkg, device, optimizer, deep, 3)
    assert e.value.code == capi.ERR_UNSUPPORTED and "66" in str(e.value)
    ok = TO.chain_nodes(64, capi.bvh_node_dtype)
    assert_equals_host(pkg, device, optimizer, ok, 3, "the deepest chain that is accepted")


def test_a_tree_that_grows_too_deep_in_a_pass_is_refused_like_on_the_host(pkg, device, optimizer, inputs, wide):
    """The deep chain at L = 1 passes 64 levels in its fourth pass: the device refuses it with the host's status and message, hands out no
    buffer, Lbvh.build(optimize=4) leaves none behind, and a session's rebuild(optimize=4) keeps the tree it is bound to."""
    capi, S = pkg.capi, pkg.scenes
    nodes = inputs[("chain", 1)]["nodes"]
    assert_equals_host(pkg, device, optimizer, nodes, 3, "chain, L = 1: 64 levels after the third pass")
    with pytest.raises(capi.GmuptError) as host:
        capi.tree_optimize_host(nodes, 4)
    for passes in (4, 8):
        with pytest.raises(capi.GmuptError) as e:
            device_run(pkg, device, optimizer, nodes, passes)
        assert e.value.code == host.value.code == capi.ERR_UNSUPPORTED
        assert str(e.value).split(":", 2)[2] == str(host.value).split(":", 2)[2], (str(e.value), str(host.value))
    assert_equals_host(pkg, device, optimizer, inputs[("soup2000", 4)]["nodes"], 1, "after the refusal")
    mesh = S.deep_chain_mesh()
    scene = S.build_scene(mesh)
    sess, sb = make_session(pkg, device, scene)
    bound = sb.nodes
    with pytest.raises(capi.GmuptError) as e:
        sess.rebuild(sb, indices=mesh["indices"], vertex_material=mesh["vertex_material"], max_leaf_size=1, optimize=4)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert sb.nodes is bound and bound.h and sb.nodes.read(capi.bvh_node_dtype).tobytes() == scene["nodes"].tobytes()
    sess.run(2)                                                            # and the session still renders on the tree it kept
    info = sess.rebuild(sb, indices=mesh["indices"], vertex_material=mesh["vertex_material"], max_leaf_size=1, optimize=3)
    assert info["depth"] == 64 and sb.nodes.read(capi.bvh_node_dtype).tobytes() == S.build_scene(mesh, builder="lbvh", max_leaf_size=1, optimize=3)["nodes"].tobytes()
    sess.run(2)
    close_session(sess, sb)


def test_tree_cost_of_the_new_buffer_equals_the_hosts(pkg, device, optimizer, inputs):
    capi = pkg.capi
    r = capi.Renderer(device, 16, 16, pool_paths=1024)
    for key in (("soup2000", 1), ("cornell", 4), ("cornell_sbvh", 0)):
        buf = capi.Buffer(device, capi.BUFFER_BVH_NODES, inputs[key]["nodes"])
        out, info = optimizer.run(buf)
        want, _ = capi.tree_optimize_host(inputs[key]["nodes"], 3)
        got = r.tree_cost(nodes=out)
        assert not TU.differing(got, capi.tree_cost_host(want)), key
        assert got["sah"] < capi.tree_cost_host(inputs[key]["nodes"])["sah"], key
        out.close(); buf.close()
    r.close()


class OptimisedScene:
    """Scene buffers whose tree was built and optimised on the device; `scene` is the host-reference scene dict (what the oracle renders)."""

    def __init__(self, pkg, device, mesh, L=4, passes=3):
        capi = pkg.capi
        self.scene = pkg.scenes.build_scene(mesh, builder="lbvh", max_leaf_size=L, optimize=passes)
        self.sb = capi.SceneBuffers(device, self.scene)
        self.sb.nodes.close(); self.sb.tris.close()
        b = capi.Lbvh(device)
        self.sb.nodes, self.sb.tris, self.info = b.build(self.sb.verts, mesh["indices"], mesh["vertex_material"], max_leaf_size=L, optimize=passes)
        b.close()
        assert self.sb.nodes.read(capi.bvh_node_dtype).tobytes() == self.scene["nodes"].tobytes()
        assert self.info["depth"] == self.scene["depth"] and self.info["optimize"]["treelets_rewritten"] > 0

    def close(self):
        self.sb.close()


@pytest.mark.parametrize("kernel", ["wide", "cast0"])
@pytest.mark.parametrize("scene_name", ["cornell", "soup"])
def test_frames_on_the_optimised_tree_equal_the_oracle(pkg, device, monkeypatch, kernel, scene_name):
    W, H, P, iters = 32, 18, 1024, 10
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    mesh = pkg.scenes.cornell_mesh() if scene_name == "cornell" else pkg.scenes.random_triangles_mesh(2000, seed=1)
    d = OptimisedScene(pkg, device, mesh)
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


def test_queries_aovs_and_refit_on_the_optimised_tree(pkg, device, wide):
    capi = pkg.capi
    mesh = pkg.scenes.random_triangles_mesh(2000, seed=1)
    d = OptimisedScene(pkg, device, mesh)
    r = capi.Renderer(device, 48, 27, pool_paths=2048); r.bind_scene(d.sb)
    rays = query_rays(d.scene, n=4096)
    sh = shadow_rays(rays)
    lc = d.scene["light_count"]
    hits, occ = r.trace(closest=rays, any=sh, light_count=lc)
    assert_matches_oracle(d.scene, rays, sh, hits, occ, lc)
    assert int((hits.view(np.int32)[:, 3] >= 0).sum()) > len(rays) // 10
    cam = capi.Camera(48, 27); cam.set_pose(*d.scene["camera"]); cam.buffer.lightCount = lc; cam.update(0.0)
    r.set_camera(cam.buffer)
    a = capi.aov_fields(r.aovs(2).cpu().numpy())
    xs, ys = np.meshgrid(np.arange(48), np.arange(27))
    centre = capi.aov_rays(cam.buffer, xs.ravel(), ys.ravel(), 2)[:, 0]
    h2, _ = r.trace(closest=centre, light_count=lc)
    assert_matches_oracle(d.scene, centre, centre[:0], h2, np.zeros(0, np.uint32), lc)
    assert np.array_equal(a["depth"].ravel().view(np.uint32), h2.view(np.uint32)[:, 0]) and np.array_equal(a["triangle"].ravel(), h2.view(np.int32)[:, 3])
    # refit after the bind
    w = pkg.scenes.wobble(d.scene, 0.3, 0.05)
    d.sb.verts.update(w)
    info = r.refit()
    assert info["rebuilt"] == 0, info
    moved = pkg.scenes.refit_scene(d.scene, w)
    assert d.sb.nodes.read(capi.bvh_node_dtype).tobytes() == moved["nodes"].tobytes()
    fsb = capi.SceneBuffers(device, moved)
    f = capi.Renderer(device, 48, 27, pool_paths=2048); f.bind_scene(fsb)
    assert_same_queries(r, f, query_rays(moved), moved["light_count"], "refit of an optimised LBVH")
    for _ in range(3):
        cam.update(0.0)
        r.set_camera(cam.buffer); f.set_camera(cam.buffer); r.iterate(); f.iterate()
    assert np.array_equal(r.framebuffer().view(np.uint32), f.framebuffer().view(np.uint32))
    assert np.array_equal(r.read_path_state(), f.read_path_state())
    cam.close(); f.close(); fsb.close(); r.close(); d.close()


W_, H_, P_ = 48, 27, 2048


def make_session(pkg, device, scene):
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W_, H_, pool_paths=P_); r.bind_scene(sb)
    cam = capi.Camera(W_, H_); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return pkg.progressive.ProgressiveSession(r, cam, W_, H_, preview_every=0), sb


def close_session(sess, sb):
    sess.close(); sess.renderer.close(); sess.camera.close(); sb.close()


def test_session_rebuild_binds_the_optimised_tree(pkg, device, wide):
    capi, S = pkg.capi, pkg.scenes
    mesh = S.cornell_mesh()
    a, asb = make_session(pkg, device, S.build_scene(mesh))
    info = a.rebuild(asb, indices=mesh["indices"], vertex_material=mesh["vertex_material"], optimize=3)
    want = S.build_scene(mesh, builder="lbvh", optimize=3)
    assert asb.nodes.read(capi.bvh_node_dtype).tobytes() == want["nodes"].tobytes() and asb.tris.read(capi.triangle_dtype).tobytes() == want["tris"].tobytes()
    assert not TO.info_differs(info["optimize"], want["optimize"]) and info["depth"] == want["depth"]
    assert not TU.differing(a.renderer.tree_cost(), capi.tree_cost_host(want["nodes"])), "the optimised tree is the bound one"
    b, bsb = make_session(pkg, device, want)
    b.camera.reset_accumulation()
    for _ in range(6):
        a.frame(); b.frame()
    assert int(b.renderer.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(a.renderer.framebuffer().view(np.uint32), b.renderer.framebuffer().view(np.uint32))
    # without the argument: the tree of the parent commit
    a.rebuild(asb)
    assert asb.nodes.read(capi.bvh_node_dtype).tobytes() == S.build_scene(mesh, builder="lbvh")["nodes"].tobytes()
    close_session(a, asb); close_session(b, bsb)


def test_session_policy_compares_and_binds_the_optimised_candidate(pkg, device, wide):
    capi, S = pkg.capi, pkg.scenes
    scene = S.build_scene(S.cornell_mesh())
    w = TU.pose(scene, "scatter")
    base, refitted, cand, plain_cost = TU.host_policy_figures(capi, scene, w)
    opt, oinfo = capi.tree_optimize_host(cand["nodes"], 3)
    opt_cost = capi.tree_cost_host(opt)["sah"]
    assert opt_cost < plain_cost and refitted > 1.01 * base
    sess, sb = make_session(pkg, device, scene)
    info = sess.set_vertices(sb, w, rebuild_above=1.01, optimize=3)
    assert info["tree_rebuilt"] is True
    assert [TU.bits(info[k]) for k in ("baseline", "cost", "candidate_cost")] == [TU.bits(x) for x in (base, refitted, opt_cost)]
    assert TU.bits(sess.baseline) == TU.bits(opt_cost)
    assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == opt.tobytes() and sb.tris.read(capi.triangle_dtype).tobytes() == cand["tris"].tobytes()
    assert not TU.differing(sess.renderer.tree_cost(), capi.tree_cost_host(opt))
    close_session(sess, sb)

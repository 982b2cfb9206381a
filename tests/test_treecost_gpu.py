"""The device tree cost (gmupt_renderer_tree_cost, csrc/pt_treecost.hip) against its host reference gmupt_tree_cost_host, bit for bit in
every field but ms: crafted record arrays around the wave, block and level boundaries, the bound tree before and after a refit, calls in
a row on reused scratch, the renderer left untouched, the errors -- and the refit-or-rebuild policy of ProgressiveSession.set_vertices
against the host rule's figures and the oracle's frames."""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the session's builder takes torch tensors)

import oracle_lib as O
import parity_util as PU
import treecost_util as TU

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def library(pkg):
    return TU.library_scenes(pkg.scenes)


@pytest.fixture(scope="module")
def unbound(pkg, device):
    """A renderer without a scene: a node buffer passed as nodes= needs none."""
    r = pkg.capi.Renderer(device, 16, 16, pool_paths=1024)
    yield r
    r.close()


def device_cost(pkg, device, r, nodes):
    buf = pkg.capi.Buffer(device, pkg.capi.BUFFER_BVH_NODES, nodes)
    try:
        return r.tree_cost(nodes=buf)
    finally:
        buf.close()


def assert_equals_host(pkg, got, nodes, what):
    want = pkg.capi.tree_cost_host(nodes)
    assert not TU.differing(got, want), "%s: %r differ: device %r, host %r" % (what, TU.differing(got, want), got, want)
    assert got["ms"] > 0, what


# ---- 1: crafted arrays
@pytest.mark.parametrize("n", TU.SIZES_GPU)
def test_device_equals_the_host_rule_on_crafted_records(pkg, device, unbound, n):
    nodes = TU.random_records(n, n, pkg.capi.bvh_node_dtype)
    assert_equals_host(pkg, device_cost(pkg, device, unbound, nodes), nodes, "%d records" % n)


@pytest.mark.parametrize("kind", TU.SPECIAL)
def test_device_equals_the_host_rule_on_the_edge_cases(pkg, device, unbound, kind):
    nodes = TU.special_records(kind, pkg.capi.bvh_node_dtype)
    got = device_cost(pkg, device, unbound, nodes)
    assert_equals_host(pkg, got, nodes, kind)
    if kind == "zero_root":
        assert TU.bits(got["sah"]) == 0
    if kind == "inf":
        assert got["sah"] == np.inf


# ---- 2: the bound tree, before and after a refit
@pytest.mark.parametrize("builder", ["sbvh", "lbvh"])
@pytest.mark.parametrize("name", ["cornell", "soup", "spheres_small"])
def test_bound_tree_before_and_after_a_refit(pkg, device, wide, library, name, builder):
    capi = pkg.capi
    scene = library[name][1 if builder == "sbvh" else 2]
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    r.bind_scene(sb)
    first = r.tree_cost()
    assert_equals_host(pkg, first, scene["nodes"], "%s %s as bound" % (name, builder))
    assert not TU.differing(r.tree_cost(), first), "a second call returns the same bits"
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    sb.verts.update(w)
    r.refit()
    moved = r.tree_cost()                       # on the renderer's stream, behind the refit's launches
    assert_equals_host(pkg, moved, capi.bvh_refit_host(scene["nodes"], scene["tris"], w), "%s %s refitted" % (name, builder))
    assert TU.bits(moved["sah"]) != TU.bits(first["sah"]), "the wobble changes the cost"
    assert not TU.differing(r.tree_cost(), moved)
    assert not TU.differing(r.tree_cost(nodes=sb.nodes), moved), "the bound buffer passed explicitly"
    r.close(); sb.close()


# ---- 3: calls in a row
def test_stale_partials_and_a_rebind(pkg, device, wide, library):
    capi = pkg.capi
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    big = TU.random_records(65537, 99, capi.bvh_node_dtype)
    two = TU.random_records(2, 98, capi.bvh_node_dtype)
    assert_equals_host(pkg, device_cost(pkg, device, r, big), big, "65537 records")
    assert_equals_host(pkg, device_cost(pkg, device, r, two), two, "2 records over the partials of 65537")
    assert_equals_host(pkg, device_cost(pkg, device, r, big), big, "65537 records again")
    sbs = []
    for name in ("soup", "cornell"):            # the first call after a bind, and after a bind of another scene
        scene = library[name][1]
        sbs.append(capi.SceneBuffers(device, scene))
        r.bind_scene(sbs[-1])
        assert_equals_host(pkg, r.tree_cost(), scene["nodes"], "first call after binding %s" % name)
    r.close()
    for sb in sbs:
        sb.close()


# ---- 4: the renderer is left as it was
def test_renderer_state_is_untouched(pkg, device, wide, library):
    capi = pkg.capi
    scene = library["soup"][1]
    W, H, P = 48, 27, 2048
    sb = capi.SceneBuffers(device, scene)
    a = capi.Renderer(device, W, H, pool_paths=P); a.bind_scene(sb)
    b = capi.Renderer(device, W, H, pool_paths=P); b.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    nodes_before = sb.nodes.read(np.uint8).tobytes()
    for it in range(6):
        cam.update(0.0)
        a.set_camera(cam.buffer); b.set_camera(cam.buffer)
        a.iterate(); b.iterate()
        got = a.tree_cost()                     # between the iterations of a only, without a synchronise of the caller's
        assert_equals_host(pkg, got, scene["nodes"], "iteration %d" % it)
    assert int(b.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(a.framebuffer().view(np.uint32), b.framebuffer().view(np.uint32))
    assert np.array_equal(a.read_path_state(), b.read_path_state())
    assert np.array_equal(a.read_queues(), b.read_queues()) and np.array_equal(a.counters(), b.counters())
    assert sb.nodes.read(np.uint8).tobytes() == nodes_before
    for k, v in a.read_travtables().items():
        assert v.tobytes() == b.read_travtables()[k].tobytes(), k
    cam.close(); a.close(); b.close(); sb.close()


# ---- 5: errors
def test_errors_write_nothing(pkg, device, unbound, library):
    capi = pkg.capi
    lib = capi.lib()
    info = capi.TreeCostInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    before = bytes(info)
    assert lib.gmupt_renderer_tree_cost(unbound.h, None, C.byref(info)) == capi.ERR_NOT_BOUND and bytes(info) == before
    assert b"gmupt_renderer_tree_cost" in lib.gmupt_last_error()
    verts = capi.Buffer(device, capi.BUFFER_VERTICES, np.zeros((16, 3), np.float32))      # 192 bytes: four records' worth, of another kind
    assert lib.gmupt_renderer_tree_cost(unbound.h, verts.h, C.byref(info)) == capi.ERR_INVALID_ARGUMENT and bytes(info) == before
    nodes = capi.Buffer(device, capi.BUFFER_BVH_NODES, TU.random_records(5, 1, capi.bvh_node_dtype))
    assert lib.gmupt_renderer_tree_cost(unbound.h, nodes.h, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_renderer_tree_cost(None, nodes.h, C.byref(info)) == capi.ERR_INVALID_ARGUMENT and bytes(info) == before
    with pytest.raises(capi.GmuptError) as e:
        unbound.tree_cost()
    assert e.value.code == capi.ERR_NOT_BOUND
    # and the renderer still answers afterwards
    assert_equals_host(pkg, unbound.tree_cost(nodes=nodes), nodes.read(capi.bvh_node_dtype), "after the errors")
    verts.close(); nodes.close()


# ---- 6: the session's policy (the Cornell box; the poses are checked on the host rule by test_treecost_cpu.py)
W_, H_, P_ = 48, 27, 2048


def make_session(pkg, device, scene):
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W_, H_, pool_paths=P_); r.bind_scene(sb)
    cam = capi.Camera(W_, H_); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return pkg.progressive.ProgressiveSession(r, cam, W_, H_, preview_every=0), sb


def close_session(sess, sb):
    sess.close(); sess.renderer.close(); sess.camera.close(); sb.close()


def assert_frames_equal_the_oracle(sess, oracle_scene, frames, what):
    """The session's next `frames` frames against the oracle on `oracle_scene`, from a restarted accumulation."""
    orc = O.Renderer(oracle_scene, W_, H_, P_, threads=8)
    ocam = O.Camera(W_, H_); ocam.set_pose(*oracle_scene["camera"]); ocam.buffer.lightCount = oracle_scene["light_count"]
    ocam.buffer.iterationCounter = -1
    assert sess.camera.buffer.iterationCounter == -1, what
    for _ in range(frames):
        sess.frame()
        ocam.update(); orc.set_camera(ocam.buffer); orc.iterate()
        assert bytes(ocam.buffer) == bytes(sess.camera.buffer), "host camera streams diverged"
    assert not PU.compare_state(orc, sess.renderer, P_, P_), what
    fb = sess.renderer.framebuffer()
    assert int(fb[..., 3].view(np.uint32).sum()) > 0, what
    assert np.array_equal(orc.framebuffer().view(np.uint32), fb.view(np.uint32)), what
    orc.close()


def test_session_without_a_threshold_is_todays_call(pkg, device, wide, library):
    scene = library["cornell"][1]
    sess, sb = make_session(pkg, device, scene)
    w = TU.pose(scene, "scatter")               # even the pose that would trigger: None computes no cost and never rebuilds
    info = sess.set_vertices(sb, w)
    assert sorted(info) == sorted(k for k, _ in pkg.capi.RefitInfo._fields_)
    assert sess.baseline is None and sess.lbvh is None
    assert sb.nodes.read(pkg.capi.bvh_node_dtype).tobytes() == pkg.capi.bvh_refit_host(scene["nodes"], scene["tris"], w).tobytes()
    assert_frames_equal_the_oracle(sess, pkg.scenes.refit_scene(scene, w), 12, "rebuild_above=None")
    close_session(sess, sb)


def test_session_jitter_keeps_the_refitted_tree(pkg, device, wide, library):
    capi = pkg.capi
    scene = library["cornell"][1]
    w = TU.pose(scene, "jitter")
    base, refitted, _, _ = TU.host_policy_figures(capi, scene, w)
    sess, sb = make_session(pkg, device, scene)
    info = sess.set_vertices(sb, w, rebuild_above=TU.POLICY_THRESHOLD)
    assert info["tree_rebuilt"] is False and info["candidate_cost"] is None
    assert TU.bits(info["baseline"]) == TU.bits(base) and TU.bits(info["cost"]) == TU.bits(refitted)
    assert TU.bits(sess.baseline) == TU.bits(base) and sess.lbvh is None
    assert info["rebuilt"] == 0 and "levels" in info
    assert_frames_equal_the_oracle(sess, pkg.scenes.refit_scene(scene, w), 8, "jitter")
    close_session(sess, sb)


def test_session_scatter_adopts_the_candidate(pkg, device, wide, library):
    capi = pkg.capi
    scene = library["cornell"][1]
    w = TU.pose(scene, "scatter")
    base, refitted, cand, cand_cost = TU.host_policy_figures(capi, scene, w)
    sess, sb = make_session(pkg, device, scene)             # (no frame before the event: session and oracle cameras draw the same seeds)
    old_nodes = sb.nodes
    info = sess.set_vertices(sb, w, rebuild_above=TU.POLICY_THRESHOLD)
    assert info["tree_rebuilt"] is True and info["candidate_cost"] < info["cost"]
    assert [TU.bits(info[k]) for k in ("baseline", "cost", "candidate_cost")] == [TU.bits(x) for x in (base, refitted, cand_cost)]
    assert TU.bits(sess.baseline) == TU.bits(cand_cost)
    assert sb.nodes is not old_nodes and not old_nodes.h, "the old node buffer is closed, the candidate is in its place"
    assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == cand["nodes"].tobytes() and sb.tris.read(capi.triangle_dtype).tobytes() == cand["tris"].tobytes()
    assert not TU.differing(sess.renderer.tree_cost(), capi.tree_cost_host(cand["nodes"])), "the adopted tree is the bound one"
    adopted = dict(scene, verts=w, nodes=cand["nodes"], tris=cand["tris"])
    assert_frames_equal_the_oracle(sess, adopted, 12, "scatter, adopted LBVH")
    # the same pose again: a refit of the fresh LBVH changes no byte, its cost is the baseline, no candidate
    again = sess.set_vertices(sb, w, rebuild_above=TU.POLICY_THRESHOLD)
    assert again["tree_rebuilt"] is False and again["candidate_cost"] is None
    assert TU.bits(again["cost"]) == TU.bits(cand_cost) == TU.bits(again["baseline"])
    # rebuild() forgets the baseline
    sess.rebuild(sb)
    assert sess.baseline is None
    close_session(sess, sb)


def test_session_adoption_drops_normals_and_history(pkg, device, wide, library):
    capi = pkg.capi
    scene = library["cornell"][1]
    w = TU.pose(scene, "scatter")
    sess, sb = make_session(pkg, device, scene)
    sess.run(6)
    assert sess.denoised_temporal().shape == (H_, W_, 4)          # a history exists
    info = sess.set_vertices(sb, w, normals="smooth", keep_history=True, rebuild_above=TU.POLICY_THRESHOLD)
    assert info["tree_rebuilt"] is True
    assert sess.normals is None, "the adjacency of the old triangle records is dropped with them, as by rebuild()"
    assert sess.camera.buffer.iterationCounter == -1
    sess.run(6)
    # a new binding is a new geometry: the next temporal output is the plain denoiser's (consequence (a) of include/gmupt.h)
    assert np.array_equal(sess.denoised_temporal().view(np.uint32)[..., :3], sess.denoised().view(np.uint32)[..., :3])
    close_session(sess, sb)


def test_session_candidate_that_may_lose(pkg, device, wide, library):
    """A threshold just below cost / baseline on "jitter" builds a candidate; the host rule says which of the two trees is cheaper, and the
    session must do what that says."""
    capi = pkg.capi
    scene = library["cornell"][1]
    w = TU.pose(scene, "jitter")
    base, refitted, cand, cand_cost = TU.host_policy_figures(capi, scene, w)
    threshold = 1.0 + 0.5 * (refitted / base - 1.0)
    assert 1.0 < threshold and refitted > threshold * base
    sess, sb = make_session(pkg, device, scene)
    info = sess.set_vertices(sb, w, rebuild_above=threshold)
    assert TU.bits(info["cost"]) == TU.bits(refitted) and TU.bits(info["candidate_cost"]) == TU.bits(cand_cost)
    wins = cand_cost < refitted
    print("jitter: refitted %.17g, candidate %.17g: the candidate %s" % (refitted, cand_cost, "wins" if wins else "loses"))
    assert info["tree_rebuilt"] is wins
    if wins:
        assert TU.bits(sess.baseline) == TU.bits(cand_cost) and sb.nodes.read(capi.bvh_node_dtype).tobytes() == cand["nodes"].tobytes()
        expect = dict(scene, verts=w, nodes=cand["nodes"], tris=cand["tris"])
    else:
        assert TU.bits(sess.baseline) == TU.bits(refitted)
        assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == capi.bvh_refit_host(scene["nodes"], scene["tris"], w).tobytes()
        expect = pkg.scenes.refit_scene(scene, w)
    again = sess.set_vertices(sb, w, rebuild_above=threshold)
    assert again["candidate_cost"] is None and again["tree_rebuilt"] is False, "a candidate that lost is not built again for the same pose"
    assert_frames_equal_the_oracle(sess, expect, 8, "jitter, threshold just below the ratio")
    close_session(sess, sb)

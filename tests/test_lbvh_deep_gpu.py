"""The LBVH builder and everything that takes its tree at rule 9's depth limit of 64 levels (include/gmupt.h "LBVH"), on the Morton key
chains of tests/lbvh_util.py: the device build on both sides of the limit against the host reference and the independent builder; the
deepest accepted tree under bind, both shipped ray casts, refit and the tree cost, against the CPU oracle and the host rules bit for bit;
the progressive session when the candidate of its rebuild policy is refused.  tests/test_lbvh_cpu.py holds the CPU half: the depth table,
the refused host builds and the oracle's stack depth on these scenes."""
import ctypes as C
import re

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the builder's indices are torch tensors)

import lbvh_util as LU
import oracle_lib as O
import parity_util as PU
import treecost_util as TU
from test_lbvh_gpu import DeviceBuiltScene, assert_equals_host, builder   # noqa: F401 (builder is a fixture)
from test_refit_gpu import assert_same_queries, shadow_rays
from trace_util import NO_TRI, assert_matches_oracle, oracle_truth

pytestmark = pytest.mark.gpu
KERNELS = ["wide", "cast0"]
DEEP_TREES = {"leaf1": (2, 1), "leaf4": (8, 4)}            # name -> (copies, L) of key_chain(copies, 0.125): both 64 levels deep
CAST_FIELDS = ["surfacePoint", "baryCoord", "triangle", "isEmitter", "hitDistance", "inShadow"]   # what the two ray-cast stages write


_RULE_DEPTH = {}


def rule_depth(pkg, copies, half, L):
    """The depth of key_chain(copies, half)'s tree by the independent builder, which has no limit; never the library's."""
    key = (copies, half, L)
    if key not in _RULE_DEPTH:
        m = LU.key_chain(copies, half)
        _RULE_DEPTH[key] = LU.build(m["verts"], m["indices"], None, L, pkg.capi.bvh_node_dtype, pkg.capi.triangle_dtype)[3]
    return _RULE_DEPTH[key]


def depth_in(message):
    """The numbers of the library's depth message: [depth found, 64]."""
    return [int(x) for x in re.findall(r"\d+", message.replace("gmupt error -5", ""))]


def try_build(pkg, builder, vb, indices, L):
    """gmupt_lbvh_build through ctypes: (return code, nodes handle, triangles handle, gmupt_last_error)."""
    capi = pkg.capi
    idx = torch.from_numpy(np.ascontiguousarray(indices, np.int32)).cuda()
    nodes, tris = C.c_void_p(0xDEAD), C.c_void_p(0xDEAD)
    p = capi.LbvhParams(L)
    torch.cuda.synchronize()
    rc = capi.lib().gmupt_lbvh_build(builder.h, vb.h, idx.data_ptr(), len(indices), None, C.byref(p), C.byref(nodes), C.byref(tris), None, None)
    return rc, nodes.value, tris.value, capi.lib().gmupt_last_error().decode()


def assert_refused(pkg, device, builder, copies, half, L, depth):
    capi = pkg.capi
    what = "key_chain(%d, %r), L = %d" % (copies, half, L)
    assert rule_depth(pkg, copies, half, L) == depth > LU.MAX_DEPTH, what
    mesh = LU.key_chain(copies, half)
    vb = capi.Buffer(device, capi.BUFFER_VERTICES, mesh["verts"])
    try:
        rc, nodes, tris, message = try_build(pkg, builder, vb, mesh["indices"], L)
        assert rc == capi.ERR_UNSUPPORTED == -5, (what, rc, message)
        assert not nodes and not tris, "%s: an error hands out no buffer" % what
        assert depth_in(message) == [depth, LU.MAX_DEPTH], (what, message)
        with pytest.raises(capi.GmuptError) as e:
            builder.build(vb, mesh["indices"], mesh["vertex_material"], max_leaf_size=L)
        assert e.value.code == capi.ERR_UNSUPPORTED and depth_in(str(e.value)) == [depth, LU.MAX_DEPTH], str(e.value)
    finally:
        vb.close()


def assert_accepted(pkg, device, builder, copies, half, L, depth):
    what = "key_chain(%d, %r)" % (copies, half)
    assert rule_depth(pkg, copies, half, L) == depth <= LU.MAX_DEPTH, (what, L)
    info = assert_equals_host(pkg, device, builder, LU.key_chain(copies, half), L, what)
    assert info["depth"] == depth, (what, L)


# ---- a. the device build on both sides of the limit
@pytest.mark.parametrize("half", LU.KEY_CHAIN_HALVES)
def test_device_build_up_to_depth_64_equals_the_host_reference(pkg, device, builder, half):
    cases = LU.key_chain_cases(accepted=True)
    assert {L for _, L, d in cases if d == LU.MAX_DEPTH} == set(LU.KEY_CHAIN_LEAF_SIZES), "a tree of exactly 64 levels at every leaf size"
    for copies, L, depth in cases:
        assert_accepted(pkg, device, builder, copies, half, L, depth)


@pytest.mark.parametrize("half", LU.KEY_CHAIN_HALVES)
def test_device_build_beyond_depth_64_is_refused(pkg, device, builder, half):
    cases = LU.key_chain_cases(accepted=False)
    assert len(cases) == 12 and {65, 72} <= {d for _, _, d in cases}
    for copies, L, depth in cases:
        assert_refused(pkg, device, builder, copies, half, L, depth)


def test_refused_and_accepted_builds_share_a_handle(pkg, device):
    """The scratch is reused from the front, and the level offsets of a 72-level build must not reach the next one."""
    b = pkg.capi.Lbvh(device)
    table = {(c, L): d for c, row in LU.KEY_CHAIN_DEPTH.items() for L, d in zip(LU.KEY_CHAIN_LEAF_SIZES, row)}
    for copies, half, L in ((300, 0.125, 1), (2, 0.125, 1), (9, 0.0, 4), (8, 0.0, 4), (300, 0.0, 4), (1, 0.0, 1), (3, 0.125, 1), (3, 0.125, 2),
                            (300, 0.125, 2), (4, 0.125, 2), (5, 0.0, 1), (5, 0.0, 4)):
        depth = table[copies, L]
        (assert_accepted if depth <= LU.MAX_DEPTH else assert_refused)(pkg, device, b, copies, half, L, depth)
    assert_equals_host(pkg, device, b, LU.soup(300, 1300), 4, "an ordinary mesh after the chains")
    b.close()


# ---- b. everything that takes a tree, on the two trees of 64 levels
class Frozen:
    """The oracle with a batch of rays in its path state and identity queues, after its extension and shadow stages (the truth of the
    renderer's own ray-cast stage), and the state before them."""

    def __init__(self, pkg, scene, closest, any_rays):
        P = len(closest)
        self.orc = orc = O.Renderer(scene, 32, 18, P, threads=8)
        st = orc.path_state()
        f32 = lambda name: O.state_field(st, P, name).view(np.float32)
        f32("rayOrigin")[:] = closest[:, 0:3]; f32("rayDirection")[:] = closest[:, 4:7]
        f32("shadowrayOrigin")[:] = any_rays[:, 0:3]; f32("shadowrayDirection")[:] = any_rays[:, 4:7]
        f32("lightDistance")[:, 0] = any_rays[:, 3]
        orc.queues()[3][:] = np.arange(P, dtype=np.uint32); orc.queues()[4][:] = np.arange(P, dtype=np.uint32)
        qc = orc.counters(); qc[:] = 0; qc[6] = P; qc[7] = P
        cam = pkg.capi.Camera(32, 18); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
        self.cam = cam.buffer_copy(); cam.close()
        orc.set_camera(self.cam)
        self.before = (orc.path_state().copy(), orc.queues().copy(), orc.counters().copy())
        orc.reset_stats()
        orc.stage("extension"); orc.stage("shadow")
        self.max_stack = orc.stats().maxStack

    def assert_cast_matches(self, pkg, device, sb, what):
        """A renderer bound to `sb` runs its ray-cast stage on the state before: the fields the casts write equal the oracle's."""
        capi = pkg.capi
        P = self.orc.pool
        hip = capi.Renderer(device, 32, 18, pool_paths=P, collect_stats=True)
        try:
            hip.bind_scene(sb); hip.set_camera(self.cam)
            hip.write_path_state(self.before[0]); hip.write_queues(self.before[1]); hip.write_counters(self.before[2])
            hip.run_stage(capi.STAGE_RAYCASTS)
            bad = PU.compare_state(self.orc, hip, P, P, fields=CAST_FIELDS)
            st = hip.stats()
        finally:
            hip.close()
        assert not bad, (what, bad[:3])
        assert not (st.flags & (capi.STAT_STACK_OVERFLOW | capi.STAT_CAST_ABORTED)), "%s: flags %#x" % (what, st.flags)
        return st

    def close(self):
        self.orc.close()


@pytest.fixture(scope="module")
def deep_trees(pkg):
    """name -> a tree of 64 levels: its mesh, the host-reference scene (what the oracle renders), the query rays and the oracle's answers,
    computed once and left unchanged."""
    out = {name: deep_tree(pkg, name) for name in DEEP_TREES}
    yield out
    for t in out.values():
        t["frozen"].close()


def deep_tree(pkg, name):
    copies, L = DEEP_TREES[name]
    mesh = LU.key_chain_render_mesh(pkg.scenes, copies, 0.125)
    scene = pkg.scenes.build_scene(mesh, builder="lbvh", max_leaf_size=L)
    assert rule_depth(pkg, copies, 0.125, L) == scene["depth"] == LU.MAX_DEPTH
    rays = LU.key_chain_rays(4096, seed=0)
    sh = shadow_rays(rays)
    lc = scene["light_count"]
    truth = oracle_truth(scene, rays, sh, lc)
    assert int((truth["triangle"][:len(rays), 0] != NO_TRI).sum()) > len(rays) // 2, "more than half of the rays hit the chain"
    frozen = Frozen(pkg, scene, rays, sh)
    usable = pkg.capi.travtables(scene["nodes"], scene["tris"], scene["verts"], want_wide=True)["wnode"].size > 0
    return {"name": name, "L": L, "mesh": mesh, "scene": scene, "rays": rays, "shadow": sh, "lc": lc, "truth": truth, "frozen": frozen,
            "wide_usable": usable}


def bound(pkg, device, builder, deep, W=48, H=27, P=2048):
    """The tree built on the device and a renderer bound to it: (DeviceBuiltScene, renderer)."""
    d = DeviceBuiltScene(pkg, device, builder, deep["mesh"], L=deep["L"])
    assert d.info["depth"] == LU.MAX_DEPTH
    assert d.sb.nodes.read(pkg.capi.bvh_node_dtype).tobytes() == deep["scene"]["nodes"].tobytes()
    r = pkg.capi.Renderer(device, W, H, pool_paths=P, collect_stats=True)
    r.bind_scene(d.sb)
    return d, r


def wide_in_use(pkg, r, deep, kernel):
    """Does this renderer hold a wide collapse of the tree?  What bind built on the device must be what the host table build says."""
    have = r.stats().wide_nodes > 0
    assert have == (kernel == "wide" and deep["wide_usable"])
    return have


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("tree", sorted(DEEP_TREES))
def test_ray_queries_on_the_depth_64_tree(pkg, device, builder, monkeypatch, deep_trees, tree, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    deep = deep_trees[tree]
    capi = pkg.capi
    d, r = bound(pkg, device, builder, deep)
    rays, sh, lc = deep["rays"], deep["shadow"], deep["lc"]
    if wide_in_use(pkg, r, deep, kernel):
        hits, occ = r.trace(closest=rays, any=sh, light_count=lc)
        assert_matches_oracle(deep["scene"], rays, sh, hits, occ, lc, truth=deep["truth"])
        assert int((hits.view(np.int32)[:, 3] >= 0).sum()) > len(rays) // 2
    else:                                                   # the API's contract: no wide collapse, no ray query
        with pytest.raises(capi.GmuptError, match="wide collapse") as e:
            r.trace(closest=rays, any=sh, light_count=lc)
        assert e.value.code == capi.ERR_UNSUPPORTED
    r.close()
    # the same rays through the renderer's own ray-cast stage, which every kernel has
    frozen = deep["frozen"]
    print("%s, %s: the oracle's walk of the query rays stacks %d entries" % (deep["name"], kernel, frozen.max_stack))
    assert 59 <= frozen.max_stack <= LU.MAX_DEPTH, "the rays must take the walk close to the stacks' limit (it measured 61)"
    st = frozen.assert_cast_matches(pkg, device, d.sb, "%s, %s" % (deep["name"], kernel))
    assert bool(st.flags & capi.STAT_CAST_WIDE) == (kernel == "wide" and deep["wide_usable"])
    if kernel == "cast0":
        assert st.flags & capi.STAT_STACK_SPILL, "depth 64 needs the spilling instantiation of k_cast_f"
    d.close()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("tree", sorted(DEEP_TREES))
def test_frames_on_the_depth_64_tree_equal_the_oracle(pkg, device, builder, monkeypatch, deep_trees, tree, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    deep = deep_trees[tree]
    capi = pkg.capi
    W, H, P = 48, 27, 2048
    scene = deep["scene"]
    d, hip = bound(pkg, device, builder, deep, W, H, P)
    wide = wide_in_use(pkg, hip, deep, kernel)
    orc = O.Renderer(scene, W, H, P, threads=8)
    ocam = O.Camera(W, H); ocam.set_pose(*scene["camera"]); ocam.buffer.lightCount = scene["light_count"]
    hcam = capi.Camera(W, H); hcam.set_pose(*scene["camera"]); hcam.buffer.lightCount = scene["light_count"]
    for it in range(4):
        PU.step_both(orc, hip, ocam, hcam)
        bad = PU.compare_state(orc, hip, P, P)
        assert not bad, "iteration %d: path state differs: %r" % (it, bad[:4])
        assert np.array_equal(orc.counters(), hip.counters()), it
        assert np.array_equal(orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32)), "iteration %d: framebuffer differs" % it
    max_stack = orc.stats().maxStack
    print("%s, %s: oracle maxStack %d over 4 iterations of %dx%d" % (deep["name"], kernel, max_stack, W, H))
    if deep["name"] == "leaf1":                             # the condition of tests/test_lbvh_cpu.py::test_key_chain_oracle_stack_depth
        assert LU.KEY_CHAIN_MIN_STACK <= max_stack <= LU.MAX_DEPTH
    assert int(hip.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    flags = hip.stats().flags
    assert not (flags & (capi.STAT_STACK_OVERFLOW | capi.STAT_CAST_ABORTED)), "flags %#x" % flags
    assert bool(flags & capi.STAT_CAST_WIDE) == wide
    if kernel == "cast0":
        assert flags & capi.STAT_STACK_SPILL, "flags %#x" % flags
    hip.close(); hcam.close(); orc.close(); d.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_refit_and_tree_cost_on_the_depth_64_tree(pkg, device, builder, monkeypatch, deep_trees, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    deep = deep_trees["leaf1"]                              # (the second tree runs the ray queries and the frames only)
    capi, S = pkg.capi, pkg.scenes
    scene = deep["scene"]
    d, r = bound(pkg, device, builder, deep)
    wide = wide_in_use(pkg, r, deep, kernel)
    got, want = r.tree_cost(), capi.tree_cost_host(scene["nodes"])
    assert not TU.differing(got, want) and not TU.differing(want, TU.rule(scene["nodes"])), (got, want)
    w = S.wobble(scene, 0.3, 0.01)
    d.sb.verts.update(w)
    info = r.refit()
    assert info["rebuilt"] == 0, info
    moved = S.refit_scene(scene, w)
    assert moved["nodes"].tobytes() != scene["nodes"].tobytes()
    assert d.sb.nodes.read(capi.bvh_node_dtype).tobytes() == moved["nodes"].tobytes(), "the refitted node buffer differs from gmupt_bvh_refit_host"
    got, want = r.tree_cost(), capi.tree_cost_host(moved["nodes"])
    assert not TU.differing(got, want) and not TU.differing(want, TU.rule(moved["nodes"])), (got, want)
    fsb = capi.SceneBuffers(device, moved)
    if wide:
        f = capi.Renderer(device, 48, 27, pool_paths=2048); f.bind_scene(fsb)
        assert_same_queries(r, f, deep["rays"], moved["light_count"], "refit of the depth-64 tree")
        f.close()
    r.close()
    # the refitted tables under the renderer's own cast, which every kernel has: a renderer bound before the move and refitted, and a
    # fresh bind of the moved scene, against the oracle on the moved scene
    frozen = Frozen(pkg, moved, deep["rays"], deep["shadow"])
    try:
        P = frozen.orc.pool
        hip = capi.Renderer(device, 32, 18, pool_paths=P, collect_stats=True)
        d.sb.verts.update(scene["verts"]); d.sb.nodes.update(scene["nodes"])
        hip.bind_scene(d.sb)
        d.sb.verts.update(w)
        assert hip.refit()["rebuilt"] == 0
        hip.set_camera(frozen.cam)
        hip.write_path_state(frozen.before[0]); hip.write_queues(frozen.before[1]); hip.write_counters(frozen.before[2])
        hip.run_stage(capi.STAGE_RAYCASTS)
        bad = PU.compare_state(frozen.orc, hip, P, P, fields=CAST_FIELDS)
        flags = hip.stats().flags
        hip.close()
        assert not bad, bad[:3]
        assert not (flags & (capi.STAT_STACK_OVERFLOW | capi.STAT_CAST_ABORTED)), "flags %#x" % flags
        frozen.assert_cast_matches(pkg, device, fsb, "a fresh bind of the moved scene, %s" % kernel)
    finally:
        frozen.close()
    fsb.close(); d.close()


# ---- c. the session when the candidate of the rebuild policy is refused
def test_session_keeps_the_refitted_tree_when_the_candidate_is_refused(pkg, device, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    capi, S = pkg.capi, pkg.scenes
    W, H, P = 48, 27, 2048
    # two poses of one list of 73 triangles: a soup, and the key chain whose LBVH at the policy's leaf size of 4 is 65 levels deep
    pose_b = LU.key_chain(9, 0.125)
    mesh_a = LU.render_mesh(S, dict(pose_b, verts=LU.soup(73, 5)["verts"].astype(np.float32)), "soup73")
    b_verts = pose_b["verts"]
    assert rule_depth(pkg, 9, 0.125, 4) == 65
    scene_a = S.build_scene(mesh_a, builder="lbvh")
    refitted = S.refit_scene(scene_a, b_verts)
    base, cost = capi.tree_cost_host(scene_a["nodes"])["sah"], capi.tree_cost_host(refitted["nodes"])["sah"]
    threshold = 1.0001
    assert base > 0 and cost > threshold * base, "the refit to pose B must cross the threshold, or no candidate is built"
    with pytest.raises(capi.GmuptError) as e:               # the candidate the session will ask for, by the host rule
        capi.lbvh_build_host(b_verts, scene_a["tris"]["v"], np.ascontiguousarray(scene_a["props"]["materialID"]))
    assert e.value.code == capi.ERR_UNSUPPORTED

    def session(scene):
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, W, H, pool_paths=P); r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        return pkg.progressive.ProgressiveSession(r, cam, W, H, preview_every=0), sb

    a, asb = session(scene_a)
    first = a.set_vertices(asb, b_verts, rebuild_above=threshold)
    assert first["tree_rebuilt"] is False and first["candidate_cost"] is None
    assert depth_in(first["candidate_refused"]) == [65, LU.MAX_DEPTH], first
    assert TU.bits(first["cost"]) == TU.bits(cost) and TU.bits(first["baseline"]) == TU.bits(base) and first["rebuilt"] == 0
    assert TU.bits(a.baseline) == TU.bits(cost), "a refused candidate moves the baseline like one that lost"
    second = a.set_vertices(asb, b_verts, rebuild_above=threshold)
    assert second["tree_rebuilt"] is False and second["candidate_cost"] is None and "candidate_refused" not in second, "no hopeless candidate on every call"
    assert TU.bits(second["cost"]) == TU.bits(cost) and TU.bits(second["baseline"]) == TU.bits(cost) and second["rebuilt"] == 0
    assert asb.nodes.read(capi.bvh_node_dtype).tobytes() == refitted["nodes"].tobytes() and asb.tris.read(capi.triangle_dtype).tobytes() == scene_a["tris"].tobytes()

    b, bsb = session(refitted)
    b.camera.reset_accumulation()

    def same_frames(n):
        for _ in range(n):
            a.frame(); b.frame()
            assert bytes(a.camera.buffer) == bytes(b.camera.buffer), "host camera streams diverged"
        fa, fb = a.renderer.framebuffer(), b.renderer.framebuffer()
        assert int(fb[..., 3].view(np.uint32).sum()) > 0
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), "the frames are those of a fresh session on the refitted scene"
        assert np.array_equal(a.renderer.read_path_state(), b.renderer.read_path_state())

    same_frames(4)
    # an explicit rebuild of pose B is the caller's own request and still fails -- before anything of the session has changed
    handles = (asb.nodes.h.value, asb.tris.h.value)
    with pytest.raises(capi.GmuptError) as e:
        a.rebuild(asb)
    assert e.value.code == capi.ERR_UNSUPPORTED and depth_in(str(e.value)) == [65, LU.MAX_DEPTH]
    assert (asb.nodes.h.value, asb.tris.h.value) == handles and all(handles), "the old buffers stay open and in place"
    assert asb.nodes.read(capi.bvh_node_dtype).tobytes() == refitted["nodes"].tobytes()
    same_frames(1)
    for s_, sbuf in ((a, asb), (b, bsb)):
        s_.close()
        s_.renderer.close(); s_.camera.close(); sbuf.close()

"""gmupt_tree_optimize_host (the host reference of the GPU treelet optimiser) against the independent restatement of the rule in
tests/treeopt_util.py, bit for bit; the structure bind, refit and the oracle rely on; the errors; the cost on the library meshes.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import treeopt_util as TO
from test_lbvh_cpu import interior_rays
from trace_util import oracle_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_treeopt_default_params", "gmupt_tree_optimize_host", "gmupt_treeopt_create", "gmupt_treeopt_destroy", "gmupt_treeopt_run"]


@pytest.fixture(scope="module")
def inputs(pkg):
    return TO.input_scenes(pkg.scenes, pkg.capi)


@pytest.fixture(scope="module")
def restated(inputs):
    """(name, L) -> {passes: (nodes, info) or Refused} by the Python restatement, computed once."""
    return {key: TO.optimize(scene["nodes"], max(TO.PASSES)) for key, scene in inputs.items()}


def host(pkg, nodes, passes):
    try:
        return pkg.capi.tree_optimize_host(nodes, passes)
    except pkg.capi.GmuptError as e:
        return e


def check_structure(pkg, scene, nodes, info, what):
    capi = pkg.capi
    src = scene["nodes"]
    # bind's validation and table build accept it; the depth is what the info says
    tables = capi.travtables(nodes, scene["tris"], scene["verts"], want_wide=True)
    assert tables["scalars"].view(np.uint32)[2] == info["depth_after"], what
    # the leaf set is unchanged, record for record
    leaf_bytes = lambda a: sorted(a[a["isLeaf"] != 0].tobytes()[i:i + 48] for i in range(0, 48 * int((a["isLeaf"] != 0).sum()), 48))
    assert leaf_bytes(nodes) == leaf_bytes(src), what
    inner = np.flatnonzero(nodes["isLeaf"] == 0)
    assert np.all(nodes["left"][inner] > inner) and np.all(nodes["right"][inner] > inner) and len(nodes) == len(src), what
    # every inner box is the union of its children's; a refit changes no byte
    l, r = nodes[nodes["left"][inner]], nodes[nodes["right"][inner]]
    assert np.array_equal(nodes["min"][inner], np.minimum(l["min"], r["min"])) and np.array_equal(nodes["max"][inner], np.maximum(l["max"], r["max"])), what
    assert capi.bvh_refit_host(nodes, scene["tris"], scene["verts"]).tobytes() == nodes.tobytes(), what
    # the costs
    assert info["cost_after"] <= info["cost_before"], what
    assert TO.bits(info["cost_before"]) == TO.bits(TO.post_order_cost(src)), what
    assert TO.bits(info["cost_after"]) == TO.bits(TO.post_order_cost(nodes)), what
    tc = capi.tree_cost_host(nodes)
    total = tc["sum_inner"] + tc["sum_leaf"]
    assert abs(total - info["cost_after"]) <= (len(nodes) + 8) * 2.0**-52 * total, what      # the same terms in another order


def test_host_equals_the_restatement_bit_for_bit(pkg, inputs, restated):
    assert {n for n, _ in inputs} >= {"soup1", "soup2", "soup3", "soup7", "soup8", "copies37", "plane", "cornell", "soup2000", "chain", "textured",
                                      "cornell_sbvh"} and any(n.startswith("key_chain") for n, _ in inputs)
    rewritten = 0
    for key, scene in inputs.items():
        for passes in TO.PASSES:
            what = "%s, L = %d, %d passes" % (key + (passes,))
            want, got = restated[key][passes], host(pkg, scene["nodes"], passes)
            if isinstance(want, TO.Refused):
                assert isinstance(got, pkg.capi.GmuptError) and got.code == want.code, what
                print("%s: refused (%s)" % (what, want))
                continue
            assert not isinstance(got, Exception), "%s: %s" % (what, got)
            nodes, info = got
            assert not TO.info_differs(info, want[1]), "%s: %r differ: host %r, restatement %r" % (what, TO.info_differs(info, want[1]), info, want[1])
            assert nodes.tobytes() == want[0].tobytes(), "%s: %d of %d nodes differ" % (
                what, int(np.any(nodes.view(np.uint32).reshape(-1, 12) != want[0].view(np.uint32).reshape(-1, 12), axis=1).sum()), len(nodes))
            assert info["ms"] == 0.0
            check_structure(pkg, scene, nodes, info, what)
            rewritten += info["treelets_rewritten"]
            if key[0] in ("soup1", "soup2"):
                assert info["treelets_rewritten"] == 0 and nodes.tobytes() == scene["nodes"].tobytes(), what
    assert rewritten > 0


# (key chain, L) -> (depth after, treelets rewritten) for 1, 2 and 3 passes
KEY_CHAIN_PINNED = {("key_chain1", 1): ((19, 60), (23, 64), (21, 66)), ("key_chain1", 4): ((19, 58), (24, 65), (22, 69)),
                    ("key_chain2", 1): ((19, 60), (23, 64), (21, 66)), ("key_chain2", 4): ((20, 59), (24, 65), (22, 68)),
                    ("key_chain3", 4): ((20, 59), (25, 65), (23, 67)), ("key_chain4", 4): ((20, 59), (25, 64), (23, 66)),
                    ("key_chain5", 4): ((20, 59), (25, 64), (23, 66)), ("key_chain8", 4): ((20, 59), (25, 64), (23, 66))}


def test_key_chain_cells_are_pinned(pkg, inputs, restated):
    """What the rule gives on the accepted key chain cells, as the host rule gave it when this test was written: every cell is accepted at
    every pass count, and the chain only gets shallower."""
    cells = [k for k in inputs if k[0].startswith("key_chain")]
    assert len(cells) == 8
    for key in cells:
        for passes in TO.PASSES:
            got = host(pkg, inputs[key]["nodes"], passes)
            assert not isinstance(got, Exception), (key, passes, got)
            info = got[1]
            print("%s L = %d, %d passes: depth %d -> %d, %d rewritten, cost %.6g -> %.6g" % (key + (passes, info["depth_before"], info["depth_after"],
                  info["treelets_rewritten"], info["cost_before"], info["cost_after"])))
            assert info["depth_after"] <= info["depth_before"] <= TO.MAX_DEPTH
            assert (info["depth_after"], info["treelets_rewritten"]) == KEY_CHAIN_PINNED[key][passes - 1], (key, passes)


def test_oracle_renders_and_hits_the_same_triangles(pkg, inputs):
    for key, scene in inputs.items():
        nodes, _ = pkg.capi.tree_optimize_host(scene["nodes"], 3)
        opt = dict(scene, nodes=nodes)
        orc = O.Renderer(opt, 32, 18, 1024, threads=4)
        cam = O.Camera(32, 18); cam.set_pose(*opt["camera"]); cam.buffer.lightCount = opt["light_count"]
        for _ in range(3):
            cam.update(); orc.set_camera(cam.buffer); orc.iterate()
        assert 0 <= orc.stats().maxStack <= 64, key
        orc.close()
        mesh = {"verts": scene["verts"], "indices": scene["tris"]["v"]}
        if np.ptp(scene["verts"], axis=0).min() > 0:
            rays = interior_rays(mesh, 256, 11)
            a, b = oracle_truth(scene, rays, rays[:0], 0), oracle_truth(opt, rays, rays[:0], 0)
            n = len(rays)
            assert np.array_equal(a["hitDistance"][:n], b["hitDistance"][:n]), key
            if key[0] not in ("copies37", "cornell_sbvh") and not key[0].startswith("key_chain"):      # no coincident triangles: the hit record is a function of the geometry
                assert np.array_equal(a["triangle"][:n], b["triangle"][:n]), key


def test_cost_falls_on_the_library_meshes(pkg, inputs):
    for name in TO.library_meshes(pkg.scenes):
        for L in TO.LEAF_SIZES:
            scene = inputs[(name, L)]
            before = pkg.capi.tree_cost_host(scene["nodes"])["sah"]
            nodes, info = pkg.capi.tree_optimize_host(scene["nodes"], 3)
            after = pkg.capi.tree_cost_host(nodes)["sah"]
            print("%s L = %d: sah %.4f -> %.4f (%.1f %%), depth %d -> %d, %d treelets rewritten" % (
                name, L, before, after, 100.0 * (after / before - 1.0), info["depth_before"], info["depth_after"], info["treelets_rewritten"]))
            assert after < before, (name, L)


def call_host(pkg, nodes, n, passes, out, info):
    p = pkg.capi.TreeoptParams(passes)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return pkg.capi.lib().gmupt_tree_optimize_host(ptr(nodes), n, C.byref(p), ptr(out), C.byref(info) if info is not None else None)


def test_errors_leave_the_outputs_untouched(pkg, inputs):
    capi = pkg.capi
    good = inputs[("soup8", 1)]["nodes"]
    deep = TO.chain_nodes(66, capi.bvh_node_dtype)
    room = max(len(good), len(deep))
    out = np.full(room * 48, 0x5A, np.uint8).view(capi.bvh_node_dtype)
    info = capi.TreeoptInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    keep = (out.tobytes(), bytes(info))

    def refused(code, nodes, n, passes, o=out):
        assert call_host(pkg, nodes, n, passes, o, info) == code
        assert (out.tobytes(), bytes(info)) == keep, "an error must leave the outputs alone"

    INVALID, UNSUPPORTED = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    refused(INVALID, None, len(good), 3)
    refused(INVALID, good, 0, 3)
    refused(INVALID, good, len(good), 3, None)
    for passes in (0, 9):
        refused(INVALID, good, len(good), passes)
    refused(UNSUPPORTED, deep, len(deep), 1)
    assert re.findall(r"\d+", capi.lib().gmupt_last_error().decode().split(":", 1)[1]) == ["66", "64"]
    with pytest.raises(TO.Refused) as e:
        TO.optimize(deep, 1)
    assert e.value.code == UNSUPPORTED
    ok = TO.chain_nodes(64, capi.bvh_node_dtype)                               # the deepest chain that is accepted
    assert call_host(pkg, ok, len(ok), 1, np.zeros(len(ok), capi.bvh_node_dtype), None) == 0
    inner = np.flatnonzero(good["isLeaf"] == 0)
    for bad in (int(inner[-1]), int(inner[-1]) - 1, 0, -1, len(good), 1 << 30):     # at and below its parent, outside the array
        x = good.copy(); x["right"][inner[-1]] = bad
        refused(INVALID, x, len(x), 2)
        with pytest.raises(TO.Refused):
            TO.optimize(x, 1)
    x = good.copy(); x["right"][inner[0]] = x["left"][inner[0]]                # one child twice, its sibling an orphan
    refused(INVALID, x, len(x), 2)
    # and a good call still works, into the same array
    assert call_host(pkg, good, len(good), 3, out, info) == 0
    want, winfo = capi.tree_optimize_host(good, 3)
    assert out[:len(good)].tobytes() == want.tobytes() and out[len(good):].tobytes() == keep[0][len(good) * 48:]
    assert info.num_nodes == len(good) and info.ms == 0.0 and TO.bits(info.cost_after) == TO.bits(winfo["cost_after"])


def test_bindings_default_to_off(pkg):
    import inspect
    capi, S = pkg.capi, pkg.scenes
    p = capi.TreeoptParams(0)
    capi.lib().gmupt_treeopt_default_params(C.byref(p))
    assert p.passes == 3
    mesh = S.cornell_mesh()
    plain, opt = S.build_scene(mesh, builder="lbvh"), S.build_scene(mesh, builder="lbvh", optimize=3)
    assert S.build_scene(mesh, builder="lbvh", optimize=0)["nodes"].tobytes() == plain["nodes"].tobytes() and "optimize" not in plain
    want, info = capi.tree_optimize_host(plain["nodes"], 3)
    assert opt["nodes"].tobytes() == want.tobytes() and opt["tris"].tobytes() == plain["tris"].tobytes()
    assert opt["depth"] == info["depth_after"] and opt["optimize"]["treelets_rewritten"] == info["treelets_rewritten"] > 0 and opt["sah"] < plain["sah"]
    with pytest.raises(ValueError):
        S.build_scene(mesh, optimize=3)
    sess = pkg.progressive.ProgressiveSession
    for fn, name in ((capi.Lbvh.build, "optimize"), (sess.rebuild, "optimize"), (sess.set_vertices, "optimize"), (sess.set_pose, "optimize"),
                     (S.build_scene, "optimize")):
        assert inspect.signature(fn).parameters[name].default == 0, fn
    assert inspect.signature(capi.TreeOptimizer.run).parameters["passes"].default == 3
    assert inspect.signature(capi.tree_optimize_host).parameters["passes"].default == 3


def test_a_tree_that_grows_too_deep_in_a_pass_is_refused(pkg, inputs):
    """The library's deep chain at L = 1: 35 levels as built, 45, 55 and 64 after one, two and three passes, beyond 64 in the fourth --
    GMUPT_ERR_UNSUPPORTED from the host rule and from the restatement alike, for every pass count from 4 on, nothing written."""
    capi = pkg.capi
    nodes = inputs[("chain", 1)]["nodes"]
    assert [capi.tree_optimize_host(nodes, p)[1]["depth_after"] for p in (1, 2, 3)] == [45, 55, 64]
    want = TO.optimize(nodes, 5)
    assert isinstance(want[4], TO.Refused) and want[4].code == capi.ERR_UNSUPPORTED and isinstance(want[5], TO.Refused) and not isinstance(want[3], TO.Refused)
    out = np.full(len(nodes) * 48, 0x5A, np.uint8).view(capi.bvh_node_dtype)
    keep = out.tobytes()
    for passes in (4, 5, 8):
        assert call_host(pkg, nodes, len(nodes), passes, out, None) == capi.ERR_UNSUPPORTED and out.tobytes() == keep
        assert b"after pass 4" in capi.lib().gmupt_last_error()
    with pytest.raises(capi.GmuptError) as e:
        pkg.scenes.build_scene(pkg.scenes.deep_chain_mesh(), builder="lbvh", max_leaf_size=1, optimize=4)
    assert e.value.code == capi.ERR_UNSUPPORTED


class _Stub:
    """A buffer / renderer / camera / builder stand-in for the session's policy: the calls set_vertices makes, recorded."""

    def __init__(self, pkg, costs, refuse_code):
        self.pkg, self.costs, self.refuse_code, self.calls = pkg, list(costs), refuse_code, []
        self.verts = self.tris = self.props = self.nodes = self

    def update(self, *a):
        self.calls.append("update")

    def read(self, dtype):
        return np.zeros(4, dtype)

    def refit(self):
        return {"rebuilt": 0}

    def tree_cost(self, nodes=None):
        self.calls.append("tree_cost")
        return {"sah": self.costs.pop(0)}

    def reset_accumulation(self):
        pass

    def build(self, verts, indices, vertex_material, max_leaf_size=4, optimize=0):
        self.calls.append(("build", optimize))
        if optimize:
            raise self.pkg.capi.GmuptError("gmupt error: the tree is 65 levels deep after pass 2", self.refuse_code)
        return self, self, {"depth": 3}

    def bind_scene(self, sb):
        self.calls.append("bind")

    def close(self):
        self.calls.append("close")


def test_an_optimiser_refusal_for_depth_is_a_candidate_that_lost(pkg):
    """set_vertices(rebuild_above=, optimize=N): GMUPT_ERR_UNSUPPORTED out of Lbvh.build(optimize=N) raises nothing, keeps the refitted tree
    and makes its cost the baseline; any other error propagates.  The builder, renderer and buffers are stand-ins: no device."""
    capi = pkg.capi
    stub = _Stub(pkg, [10.0, 20.0], capi.ERR_UNSUPPORTED)                     # baseline 10, refitted 20: beyond 1.5 x
    sess = pkg.progressive.ProgressiveSession(stub, stub, 4, 4)
    sess.lbvh = stub
    info = sess.set_vertices(stub, np.zeros((3, 3), np.float32), rebuild_above=1.5, optimize=3)
    assert ("build", 3) in stub.calls and "bind" not in stub.calls
    assert info["tree_rebuilt"] is False and info["candidate_cost"] is None and "65 levels" in info["candidate_refused"]
    assert info["cost"] == 20.0 and info["baseline"] == 10.0 and sess.baseline == 20.0
    # the same pose again: the refitted tree is the baseline now, no candidate is built
    stub.costs = [20.0]
    n = len(stub.calls)
    again = sess.set_vertices(stub, np.zeros((3, 3), np.float32), rebuild_above=1.5, optimize=3)
    assert again["candidate_cost"] is None and "candidate_refused" not in again and not [c for c in stub.calls[n:] if isinstance(c, tuple)]
    # without optimize the same stand-in builds, and the cheaper candidate is bound
    stub2 = _Stub(pkg, [10.0, 20.0, 12.0], capi.ERR_UNSUPPORTED)
    sess2 = pkg.progressive.ProgressiveSession(stub2, stub2, 4, 4)
    sess2.lbvh = stub2
    info2 = sess2.set_vertices(stub2, np.zeros((3, 3), np.float32), rebuild_above=1.5)
    assert ("build", 0) in stub2.calls and "bind" in stub2.calls and info2["tree_rebuilt"] is True and info2["candidate_cost"] == 12.0
    # another error is not swallowed
    stub3 = _Stub(pkg, [10.0, 20.0], capi.ERR_HIP)
    sess3 = pkg.progressive.ProgressiveSession(stub3, stub3, 4, 4)
    sess3.lbvh = stub3
    with pytest.raises(capi.GmuptError) as e:
        sess3.set_vertices(stub3, np.zeros((3, 3), np.float32), rebuild_above=1.5, optimize=3)
    assert e.value.code == capi.ERR_HIP


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in pkg.capi.SYMBOLS, name
        assert getattr(lib, name, None) is not None, name
    assert C.sizeof(pkg.capi.TreeoptInfo) == 40 and pkg.capi.TreeoptInfo.ms.offset == 32 and pkg.capi.TreeoptInfo.cost_before.offset == 16
    assert "Tree optimisation" in header

"""gmupt_lbvh_build_host (the host reference of the GPU LBVH builder) against an independent builder written from the rule in
include/gmupt.h (tests/lbvh_util.py), bit for bit; the structure bind, refit and the oracle rely on; the errors of rule 9.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import lbvh_util as LU
import oracle_lib as O
from trace_util import FLT_MAX, NO_TRI, make_rays, oracle_truth

LEAF_SIZES = [1, 2, 4, 64]


def library_meshes(pkg):
    S = pkg.scenes
    return {"cornell": S.cornell_mesh(), "soup2000": S.random_triangles_mesh(2000), "chain": S.deep_chain_mesh(), "textured": S.textured_mesh()}


@pytest.fixture(scope="module")
def meshes(pkg):
    m = library_meshes(pkg)
    m.update(LU.crafted_meshes(4))
    m.update({"soup64": LU.soup(64, 164), "soup65": LU.soup(65, 165)})       # L and L + 1 triangles for L = 64
    return m


def check_tree(pkg, mesh, L, name, want_depth=None):
    capi = pkg.capi
    v, t, vm = mesh["verts"], mesh["indices"], mesh["vertex_material"]
    got = capi.lbvh_build_host(v, t, vm, L)
    nodes, tris, ref, depth, leaves = LU.build(v, t, vm, L, capi.bvh_node_dtype, capi.triangle_dtype)
    what = "%s, L = %d" % (name, L)
    assert want_depth is None or depth == want_depth, "%s: the independent builder finds depth %d, the construction states %d" % (what, depth, want_depth)
    assert np.array_equal(got["ref_triangle"], ref), what
    assert got["tris"].tobytes() == tris.tobytes(), what
    assert len(got["nodes"]) == len(nodes), what
    assert got["nodes"].tobytes() == nodes.tobytes(), "%s: %d of %d nodes differ" % (
        what, int(np.any(got["nodes"].view(np.uint32).reshape(-1, 12) != nodes.view(np.uint32).reshape(-1, 12), axis=1).sum()), len(nodes))
    # info describes the arrays
    info = got["info"]
    n = len(t)
    assert (info["num_nodes"], info["num_leaves"], info["depth"], info["num_tris"], info["ms"]) == (len(nodes), leaves, depth, n, 0.0), what
    assert info["num_nodes"] == 2 * info["num_leaves"] - 1 and got["depth"] == depth
    assert info["root_min"].tobytes() == nodes[0]["min"].tobytes() and info["root_max"].tobytes() == nodes[0]["max"].tobytes()
    # structure: every source triangle once, leaves no larger than L and tiling the records, siblings adjacent, children above
    assert np.array_equal(np.sort(got["ref_triangle"]), np.arange(n)), what
    g = got["nodes"]
    leaf = g["isLeaf"] != 0
    assert np.all(g["right"][leaf] - g["left"][leaf] <= L) and np.all(g["right"][leaf] > g["left"][leaf])
    assert np.array_equal(np.sort(g["left"][leaf])[1:], np.sort(g["right"][leaf])[:-1]) and g["right"][leaf].max() == n
    assert np.all(g["right"][~leaf] == g["left"][~leaf] + 1) and np.all(g["left"][~leaf] > np.flatnonzero(~leaf))
    assert (len(g) == 1) == (n <= L)
    for pad in ("pad0", "pad1", "pad2"):
        assert not g[pad].view(np.uint32).any()
    # a refit of the fresh tree changes no byte; bind's validation and table build (wide collapse included) accept it
    assert capi.bvh_refit_host(g, got["tris"], v).tobytes() == g.tobytes(), what
    tables = capi.travtables(g, got["tris"], v, want_wide=True)
    assert tables["scalars"].view(np.uint32)[2] == depth, what
    assert tables["tri48"].size == (n + 1) * 48
    return got


@pytest.mark.parametrize("L", LEAF_SIZES)
def test_host_build_equals_the_rule(pkg, meshes, L):
    for name, mesh in meshes.items():
        got = check_tree(pkg, mesh, L, name)
        if name == "copies37":
            assert np.array_equal(got["ref_triangle"], np.arange(37)), "equal keys keep index order"
        if name == "grid16":
            assert len(set(LU.morton_keys(mesh["verts"], mesh["indices"]))) == 2, "the grid lies in one cell of the key space"


@pytest.mark.parametrize("half", [0.0, 2.0**-23, 0.125, 0.25])
def test_key_chain_keys(half):
    """The construction of lbvh_util.key_chain: 65 distinct keys, every single bit 0..62 among them, whatever the triangles' size."""
    for copies in (1, 2, 9):
        mesh = LU.key_chain(copies, half)
        keys = LU.morton_keys(mesh["verts"], mesh["indices"])
        assert keys == [0] * copies + [1 << j for j in range(63)] + [(1 << 63) - 1], (copies, half)


@pytest.mark.parametrize("half", LU.KEY_CHAIN_HALVES)
def test_key_chain_trees_up_to_the_depth_limit(pkg, half):
    """Every accepted cell of the depth table, the largest accepted depth 64 among them: the highest differing bit takes every position
    62..0 in one tree, then delta continues into the position tie-break."""
    cases = LU.key_chain_cases(accepted=True)
    assert sorted(d for _, _, d in cases)[-1] == LU.MAX_DEPTH and len(cases) == 12
    for copies, L, depth in cases:
        got = check_tree(pkg, LU.key_chain(copies, half), L, "key_chain(%d, %r)" % (copies, half), want_depth=depth)
        assert got["depth"] == depth


def test_key_chain_oracle_stack_depth(pkg):
    """What makes the GPU frames on the depth-64 tree (test_lbvh_deep_gpu.py) mean something: the oracle's walk of that scene stacks far
    beyond the 24-entry LDS part of the casts' stacks and close to the limit of 64.  Measured: 46 (48 with half = 0.25)."""
    scene = pkg.scenes.build_scene(LU.key_chain_render_mesh(pkg.scenes, 2, 0.125), builder="lbvh", max_leaf_size=1)
    assert scene["depth"] == LU.MAX_DEPTH
    orc = O.Renderer(scene, 32, 18, 1024, threads=4)
    cam = O.Camera(32, 18); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    for _ in range(4):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    max_stack = orc.stats().maxStack
    samples = int(orc.framebuffer()[..., 3].view(np.uint32).sum())
    orc.close()
    print("key_chain(2, 0.125), L = 1: oracle maxStack %d" % max_stack)
    assert samples > 0 and LU.KEY_CHAIN_MIN_STACK <= max_stack <= LU.MAX_DEPTH


def test_default_leaf_size_and_scene_builder(pkg):
    capi, S = pkg.capi, pkg.scenes
    p = capi.LbvhParams(0)
    capi.lib().gmupt_lbvh_default_params(C.byref(p))
    assert p.max_leaf_size == 4
    mesh = S.cornell_mesh()
    a = S.build_scene(mesh, builder="lbvh")
    b = capi.lbvh_build_host(mesh["verts"], mesh["indices"], mesh["vertex_material"])
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["tris"].tobytes() == b["tris"].tobytes()
    assert a["depth"] == b["depth"] and a["sah"] == b["sah"] > 0
    d = S.build_scene(mesh)
    assert d["nodes"].tobytes() == S.build_scene(mesh, builder="sbvh")["nodes"].tobytes()      # the default is the SBVH, as before
    assert abs(capi.tree_sah(d["nodes"]) - d["sah"]) < 1e-4 * d["sah"]                        # tree_sah is the SBVH builder's measure
    with pytest.raises(ValueError):
        S.build_scene(mesh, builder="kd")


def interior_rays(mesh, n, seed):
    """Rays from random origins through points well inside random triangles: a closest hit on an edge, where two triangles tie in t,
    does not occur, so the hit TRIANGLE is a function of the geometry and not of the tree."""
    rng = np.random.default_rng(seed)
    v, t = mesh["verts"], mesh["indices"]
    lo, hi = v.min(axis=0), v.max(axis=0)
    o = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (n, 3)).astype(np.float32)
    w = rng.uniform(0.15, 1.0, (n, 3)); w /= w.sum(axis=1, keepdims=True)
    tri = t[rng.integers(0, len(t), n)]
    target = (v[tri] * w[:, :, None]).sum(axis=1)
    return make_rays(o, (target - o).astype(np.float32), FLT_MAX)


def test_oracle_renders_and_answers_queries_on_the_lbvh_scene(pkg):
    S = pkg.scenes
    mesh = S.cornell_mesh()
    sbvh, lbvh = S.build_scene(mesh), S.build_scene(mesh, builder="lbvh")
    orc = O.Renderer(lbvh, 32, 18, 1024, threads=4)
    cam = O.Camera(32, 18); cam.set_pose(*lbvh["camera"]); cam.buffer.lightCount = lbvh["light_count"]
    for _ in range(6):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    assert int(orc.framebuffer()[..., 3].view(np.uint32).sum()) > 0 and 0 < orc.stats().maxStack <= 64
    orc.close()
    rays = interior_rays(mesh, 2048, 7)
    a = oracle_truth(sbvh, rays, rays[:0], 0)
    b = oracle_truth(lbvh, rays, rays[:0], 0)
    n = len(rays)
    assert np.array_equal(a["hitDistance"][:n], b["hitDistance"][:n]), "closest-hit t must not depend on the tree"
    hit = a["triangle"][:n, 0] != NO_TRI
    assert hit.sum() > n // 2
    assert np.array_equal(a["triangle"][:n], b["triangle"][:n]) and np.array_equal(a["baryCoord"][:n], b["baryCoord"][:n])
    # the record the oracle reports is the source triangle's: through ref_triangle both trees name the same one
    for scene, truth in ((sbvh, a), (lbvh, b)):
        recs = scene["tris"].view(np.uint32).reshape(-1, 4)
        src = np.asarray(mesh["indices"], np.uint32)[scene["ref_triangle"]]
        assert np.array_equal(recs[:, :3], src)


def call_host(pkg, verts, num_verts, indices, num_tris, L, nodes, tris, ref):
    p = pkg.capi.LbvhParams(L)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return pkg.capi.lib().gmupt_lbvh_build_host(ptr(verts), num_verts, ptr(indices), num_tris, None, C.byref(p), ptr(nodes), ptr(tris), ptr(ref), None)


def test_errors_write_nothing(pkg):
    capi = pkg.capi
    mesh = LU.soup(9, 5)
    v, t = mesh["verts"].copy(), mesh["indices"].copy()
    n = len(t)
    deep = LU.key_chain_cases(accepted=False)
    room = max(n, max(c for c, _, _ in deep) + 64)                            # the outputs hold the largest refused mesh too
    nodes = np.full(2 * room - 1, 0x5A, np.uint8).repeat(48).view(capi.bvh_node_dtype)
    tris = np.full(room * 16, 0x5A, np.uint8).view(capi.triangle_dtype)
    ref = np.full(room, 0x5A5A5A5A, np.int32)
    keep = (nodes.tobytes(), tris.tobytes(), ref.tobytes())

    def refused(code, *args):
        assert call_host(pkg, *args) == code
        assert (nodes.tobytes(), tris.tobytes(), ref.tobytes()) == keep, "an error must leave the outputs alone"

    INVALID, UNSUPPORTED = -1, -5
    refused(INVALID, None, len(v), t, n, 4, nodes, tris, ref)
    refused(INVALID, v, len(v), None, n, 4, nodes, tris, ref)
    refused(INVALID, v, len(v), t, n, 4, None, tris, ref)
    refused(INVALID, v, len(v), t, n, 4, nodes, None, ref)
    refused(INVALID, v, 0, t, n, 4, nodes, tris, ref)
    refused(INVALID, v, len(v), t, 0, 4, nodes, tris, ref)
    for L in (0, 65, 1 << 20):
        refused(INVALID, v, len(v), t, n, L, nodes, tris, ref)
    for bad in (-1, len(v), 1 << 30):
        t2 = t.copy(); t2[n - 1, 2] = bad                                       # the LAST triangle: everything before it has been read
        refused(INVALID, v, len(v), t2, n, 4, nodes, tris, ref)
    for bad in (np.nan, np.inf, -np.inf):
        v2 = v.copy(); v2[t[n - 1, 1], 2] = bad
        refused(INVALID, v2, len(v2), t, n, 4, nodes, tris, ref)
    # rule 9's depth error: every cell of the key chain's depth table beyond 64, the nearest (65) and the farthest (72) among them
    assert UNSUPPORTED == capi.ERR_UNSUPPORTED and len(deep) == 12 and {65, 72} <= {d for _, _, d in deep}
    for copies, L, depth in deep:
        for half in LU.KEY_CHAIN_HALVES:
            m = LU.key_chain(copies, half)
            kv, kt = m["verts"], np.ascontiguousarray(m["indices"], np.int32)
            assert LU.build(kv, kt, None, L, capi.bvh_node_dtype, capi.triangle_dtype)[3] == depth, (copies, L, half)
            refused(UNSUPPORTED, kv, len(kv), kt, len(kt), L, nodes, tris, ref)
            with pytest.raises(capi.GmuptError) as e:
                capi.lbvh_build_host(kv, kt, m["vertex_material"], L)
            assert e.value.code == UNSUPPORTED and re.findall(r"\d+", str(e.value).split(":", 1)[1]) == [str(depth), "64"], str(e.value)
    # a vertex no triangle uses may hold anything
    v3 = np.concatenate([v, [[np.nan, np.inf, 0.0]]]).astype(np.float32)
    assert call_host(pkg, v3, len(v3), t, n, 4, nodes, tris, ref) == 0
    want = capi.lbvh_build_host(v, t, None, 4)
    assert nodes[:len(want["nodes"])].tobytes() == want["nodes"].tobytes() and tris[:n].tobytes() == want["tris"].tobytes() and np.array_equal(ref[:n], want["ref_triangle"])
    assert (nodes[len(want["nodes"]):].tobytes(), tris[n:].tobytes(), ref[n:].tobytes()) == (keep[0][len(want["nodes"]) * 48:], keep[1][n * 16:], keep[2][n * 4:])
    # ref_triangle_out may be NULL
    assert call_host(pkg, v, len(v), t, n, 4, nodes, tris, None) == 0

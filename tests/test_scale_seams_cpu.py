"""CPU checks behind test_scale_seams_gpu.py: the helpers of scale_util, and -- from the host references and the mirrored constants alone,
never from a device result -- that every input of the GPU tests reaches the seam it is there for."""
import collections
import os
import re

import numpy as np
import pytest

import lbvh_util as LU
import normals_util as NU
import pose_util as PS
import scale_util as SU

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "csrc")


def test_mirrored_constants_equal_the_sources():
    for name, constants in SU.MIRRORED.items():
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for k, want in constants.items():
            found = re.findall(r"\b%s\s*=\s*(\d+)\b" % k, text)
            assert found == [str(want)], (name, k, found)
    assert SU.LB_LEVEL_STRIDE == 262144 and SU.TO_LEVEL_STRIDE == 8192
    with open(os.path.join(CSRC, "pt_normals.hip")) as f:
        assert "unsigned b = 1; while (b < 32 && (numVerts >> b)) b++; return b;" in f.read(), "nm_key_bits changed: scale_util restates it"
    # every sort of the library is rocprim::radix_sort_pairs with the default configuration: what SORT_ONE_BLOCK / SORT_MERGE_LIMIT describe
    for name in ("pt_lbvh.hip", "pt_levels.hpp", "pt_normals.hip"):
        with open(os.path.join(CSRC, name)) as f:
            calls = re.findall(r"rocprim::(\w+)\s*(<?)", f.read())
        assert calls and all(c == ("radix_sort_pairs", "") for c in calls), (name, calls)
    with open(os.path.join(CSRC, "pt_treeopt.hip")) as f:                  # its sorts are level_sort of pt_levels.hpp
        assert "rocprim::" not in f.read()
    assert [SU.sort_path(n) for n in (1024, 1025, 1 << 20, (1 << 20) + 1)] == ["block", "merge", "merge", "onesweep"]


# ---- pose
def test_pose_seam_sizes_reach_the_second_trip():
    cap = SU.PS_MAX_GRID * SU.PS_BLOCK
    assert SU.POSE_SEAM_VERTS == (cap, cap + 1, cap + SU.PS_BLOCK + 1) and cap + SU.PS_BLOCK + 1 == 524545
    assert SU.pose_trips(cap) == ({1: 2048}, 2048)                                   # no second trip anywhere
    assert SU.pose_trips(cap + 1) == ({2: 1, 1: 2047}, 2049)                         # block 0 alone
    assert SU.pose_trips(cap + SU.PS_BLOCK + 1) == ({2: 2, 1: 2046}, 2050)           # blocks 0 and 1; the last tile holds one vertex
    assert (cap + SU.PS_BLOCK + 1) - 2049 * SU.PS_BLOCK == 1
    assert SU.pose_trips(257) == ({1: 2}, 2), "what the kernel-level pose tests reach"
    lds = [J for _, J, _ in SU.POSE_SEAM_RIGS]
    assert lds == [3, 640, 641], "a few matrices in LDS, the most that fit, one more (global memory)"


def test_flat_scene_binds_any_vertex_count(pkg):
    scene = SU.flat_scene(pkg.capi, 1000)
    assert scene["verts"].shape == (1000, 3) and len(scene["props"]) == 1000 and len(scene["nodes"]) == 1 and len(scene["tris"]) == 1
    assert scene["nodes"][0]["isLeaf"] == 1 and scene["tris"]["v"].max() < 1000


def test_target_weight_patterns():
    for T in SU.ACTIVE_TARGETS:
        p = SU.target_weight_patterns(T)
        assert sorted(p) == sorted(["all", "third_zero", "wave0_zero", "only_last"] + (["nan70"] if T > SU.NAN_TARGET else []))
        assert all(w.dtype == np.float32 and w.shape == (T,) for w in p.values())
        assert np.count_nonzero(p["all"]) == T
        z = np.flatnonzero(p["third_zero"] == 0)
        assert np.array_equal(z, np.arange(0, T, 3)) and np.signbit(p["third_zero"][z]).any() and not np.signbit(p["third_zero"][z]).all()
        assert not p["wave0_zero"][:64].any() and np.count_nonzero(p["wave0_zero"]) == T - 64
        assert np.flatnonzero(p["only_last"]).tolist() == [T - 1]
        if "nan70" in p:
            assert np.isnan(p["nan70"][70]) and int(np.isnan(p["nan70"]).sum()) == 1
            assert int((p["nan70"] != 0).sum()) == np.count_nonzero(p["third_zero"]) + (1 if p["third_zero"][70] == 0 else 0)
        # every wave of k_ps_active that holds targets holds active ones somewhere among the patterns, and lanes up to 63 are used
        assert np.count_nonzero(p["all"][(T - 1) // 64 * 64:]) > 0 and T <= SU.PS_MAX_TARGETS
    assert max(SU.ACTIVE_TARGETS) == SU.PS_MAX_TARGETS


def test_active_target_cases_are_order_sensitive_and_the_host_agrees(pkg):
    """A target in a wrong slot or a wrong order must change bits: for the deltas and weights of every case with two or more finite
    active weights, the rule with the targets applied in reversed order differs.  And the host reference equals the restatement."""
    checked = 0
    for K, J, T, name, rig in SU.active_cases():
        tw = rig["target_weights"]
        want = PS.restated(rig)
        host = PS.host(pkg.capi, rig)
        if name == "nan70":
            assert np.isnan(want).all() and np.isnan(host).all()
            continue
        assert PS.differing(want, host) == 0, (K, J, T, name)
        if np.count_nonzero(tw) >= 2:
            rev = PS.rule(rig["rest"], rig["joints"], rig["weights"], rig["num_joints"], rig["mats"], rig["deltas"][::-1], tw[::-1])
            assert PS.differing(want, rev) > 0, (K, J, T, name)
            checked += 1
    assert checked == 2 * (3 * len(SU.ACTIVE_TARGETS) - 2)      # all but wave0_zero at T = 64 (nothing active) and T = 65 (one target)


# ---- the meshes
def test_grid_mesh_is_what_it_says():
    m = SU.grid_mesh(4, 3, 2, seed=5, copies=2)
    v, t = m["verts"], m["indices"]
    assert v.dtype == np.float32 and t.dtype == np.int32 and t.shape == (48, 3) and v.shape == (144, 3) and len(m["vertex_material"]) == 144
    tri = np.sort(t[:, 0] // 3)
    assert np.array_equal(tri, np.arange(48)) and np.array_equal(t, t[:, :1] + np.arange(3)) and not np.array_equal(t[:, 0] // 3, np.arange(48))
    p = v[t]                                                               # (n, 3 corners, 3)
    centre = (p.min(axis=1) + p.max(axis=1)) * np.float32(0.5)
    cell = t[:, 0] // 3 // 2
    want = np.stack([cell % 4, cell // 4 % 3, cell // 12], axis=1).astype(np.float32)
    assert np.array_equal(centre, want), "the box centre is the cell centre exactly"
    h = (p.max(axis=1) - p.min(axis=1)) * np.float32(0.5)
    assert np.all(h == h[:, :1]) and set(np.unique(h).tolist()) <= set(SU.GRID_HALVES) and len(np.unique(h)) == 3
    assert np.array_equal((p[:, 1] - p[:, 0]) / h, np.tile([2.0, 0.0, 2.0], (48, 1))) and np.array_equal((p[:, 2] - p[:, 0]) / h, np.tile([0.0, 2.0, 2.0], (48, 1)))
    again = SU.grid_mesh(4, 3, 2, seed=5, copies=2)
    assert all(np.array_equal(m[k], again[k]) for k in m) and not np.array_equal(t, SU.grid_mesh(4, 3, 2, seed=6, copies=2)["indices"])


def test_nodes_per_depth_on_a_small_tree(pkg):
    m = SU.grid_mesh(4, 4, 2)
    nodes = pkg.capi.lbvh_build_host(m["verts"], m["indices"], m["vertex_material"], 1)["nodes"]
    assert SU.nodes_per_depth(nodes) == ([1, 2, 4, 8, 16, 32], [1, 2, 4, 8, 16, 0])
    ref = LU.build(m["verts"], m["indices"], m["vertex_material"], 1, pkg.capi.bvh_node_dtype, pkg.capi.triangle_dtype)
    assert ref[0].tobytes() == nodes.tobytes(), "and the independent builder agrees on a grid mesh"


# ---- the LBVH builder's seams
@pytest.fixture(scope="module")
def grid_1m_tree(pkg):
    m = SU.grid_mesh(128, 128, 64)
    return m, pkg.capi.lbvh_build_host(m["verts"], m["indices"], m["vertex_material"], 1)


def test_the_grid_tree_has_a_level_k_lb_level_strides_over(grid_1m_tree):
    m, built = grid_1m_tree
    n = len(m["indices"])
    kept, inner = SU.nodes_per_depth(built["nodes"])
    assert n == 1 << 20 and len(built["nodes"]) == 2 * n - 1 and built["info"]["depth"] == 20
    assert inner[19] == 524288 > SU.LB_LEVEL_STRIDE and kept[20] == 1 << 20, "two trips over the inner nodes of depth 19, four over the leaves"
    assert max(kept[:19]) <= SU.LB_LEVEL_STRIDE
    assert SU.bounds_partials(n) == 4096 > SU.LB_BLOCK
    assert SU.sort_path(n) == "merge" and n == SU.SORT_MERGE_LIMIT and SU.sort_path(2 * n - 1) == "onesweep"
    # what the single-stage tests reach: 5000 triangles
    assert SU.bounds_partials(5000) < SU.LB_BLOCK and 2 * 5000 - 1 < SU.LB_LEVEL_STRIDE and SU.sort_path(2 * 5000 - 1) == "merge"


def test_the_other_builder_inputs_sit_where_they_should():
    assert SU.bounds_partials(70_000) == 274 > SU.LB_BLOCK
    assert SU.bounds_partials(65_536) == SU.LB_BLOCK and SU.bounds_partials(65_537) == SU.LB_BLOCK + 1
    assert SU.sort_path(128 * 128 * 65) == "onesweep"
    assert SU.sort_path(64 * 64 * 16 * 4) == "merge" and SU.sort_path(64 * 64 * 65 * 4) == "onesweep"
    assert len(LU.soup(65_537, 2)["indices"]) == 65_537


@pytest.mark.parametrize("nz", [16, 65])
def test_the_duplicated_grid_has_four_triangles_per_key(nz):
    m = SU.grid_mesh(64, 64, nz, seed=1, copies=4)
    t = m["indices"]
    cell = t[:, 0] // 3 // 4
    assert len(t) == 64 * 64 * nz * 4 and np.all(np.bincount(cell) == 4)
    rng = np.random.default_rng(nz)
    chosen = rng.choice(64 * 64 * nz, 1024, replace=False)
    rows = np.flatnonzero(np.isin(cell, chosen))                           # 4096 triangles: all four of 1024 cells, in index-list order
    assert len(rows) == 4096
    keys = LU.morton_keys(m["verts"], t[rows])
    count = collections.Counter(keys)
    assert len(count) == 1024 and set(count.values()) == {4}
    # the four of a cell are not in storage order in the index list (else index order and storage order could not be told apart) ...
    by_cell = collections.defaultdict(list)
    for r in rows.tolist():
        by_cell[int(cell[r])].append(int(t[r, 0]))
    assert sum(1 for v in by_cell.values() if v != sorted(v)) > 512
    # ... and their records differ: each has vertices of its own
    assert len(np.unique(t[rows, 0])) == 4096


# ---- the treelet optimiser's seam
@pytest.mark.parametrize("name", ["soup70000", "grid64x32x32"])
def test_treeopt_inputs_have_a_level_past_the_grid_cap_and_are_rewritten(pkg, name):
    mesh = LU.soup(70_000, 3) if name == "soup70000" else SU.grid_mesh(64, 32, 32)
    nodes = pkg.capi.lbvh_build_host(mesh["verts"], mesh["indices"], mesh["vertex_material"], 1)["nodes"]
    kept, inner = SU.nodes_per_depth(nodes)
    assert max(inner) > SU.TO_LEVEL_STRIDE, (name, max(inner))
    if name == "grid64x32x32":
        assert inner[15] == 32768 == 4 * SU.TO_LEVEL_STRIDE
    for passes in (1, 3):
        out, info = pkg.capi.tree_optimize_host(nodes, passes)
        assert info["treelets_rewritten"] > 0 and info["cost_after"] < info["cost_before"], (name, passes, info)
        # the rewritten tree still has such a level: the later passes stride too
        assert max(SU.nodes_per_depth(out)[1]) > SU.TO_LEVEL_STRIDE
    small = pkg.capi.lbvh_build_host(*[pkg.scenes.random_triangles_mesh(20000, seed=3)[k] for k in ("verts", "indices", "vertex_material")], 1)["nodes"]
    print("widest inner level of the 40 000-node test of test_treeopt_gpu.py: %d" % max(SU.nodes_per_depth(small)[1]))


# ---- the normals' seams
def test_normals_inputs_sit_past_the_small_sorts(pkg):
    S = pkg.scenes
    for n_spheres, path in ((12, "merge"), (70, "onesweep")):
        mesh = S.spheres_mesh(n_spheres=n_spheres, subdiv=4, seed=7, floor_quads=4)
        t = np.ascontiguousarray(mesh["indices"], np.int32)
        assert SU.sort_path(t.size) == path, (n_spheres, t.size)
        valence = np.bincount(t.reshape(-1))
        assert np.count_nonzero((valence == 5) | (valence == 6)) > 0.99 * len(valence), "shared vertices of valence 5 and 6"
    assert SU.sort_path(3 * 1000) == "merge" and SU.sort_path(3 * 257) == "block", "what the single-stage tests reach"
    assert [SU.nm_key_bits(n) for n in (1, 2, 3, (1 << 17) - 1, 1 << 17, (1 << 17) + 1)] == [1, 2, 2, 17, 18, 18]
    v, t = NU.strip(1 << 17)
    assert len(v) == 1 << 17 and t.max() == (1 << 17) - 1 and SU.sort_path(t.size) == "merge"
    assert (1 << 17) >> 17 == 1 and int(t.max()) >> 17 == 0, "the key numVerts alone has bit 17"


def test_normals_of_the_large_strip_are_order_sensitive(pkg):
    """The sums of the strip's vertices depend on the corner order, so an unstable sort would show."""
    v, t = NU.strip(1 << 17)
    want = pkg.capi.vertex_normals_host(v, t)
    assert np.array_equal(want.view(np.uint32), NU.rule(v, t).view(np.uint32))
    assert not np.array_equal(want.view(np.uint32), NU.rule(v, t, descending=True).view(np.uint32))

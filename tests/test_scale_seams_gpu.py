"""The mesh-update kernels past their grid caps and past the small paths of the sort library: each against its host reference, bit for bit,
at the smallest size that reaches the seam.  test_scale_seams_cpu.py proves from the host references and the mirrored constants alone
that every seam named here is reached by its input; nothing in this file reads that off the device result.

  pose      k_ps_pose runs on at most PS_MAX_GRID blocks: the second trip of its tile loop (the LDS stage written again behind the trailing
            barrier, the joint matrices in LDS read again after it), and k_ps_active with targets in all four waves
  LBVH      k_lb_bounds2 striding over more than 256 block partials, k_lb_level striding over a depth of more than 262 144 kept nodes,
            both sorts on each path of the sort library, equal keys on the large paths
  treelets  k_to_level striding (four block barriers per trip) over a depth of more than 8192 entries
  normals   the adjacency build -- k_nm_keys, the sort on nm_key_bits(numVerts) bits, k_nm_offsets -- on the large sort paths, and the key
            numVerts itself where it needs a bit more than every vertex

The sort library: rocprim::radix_sort_pairs with its default configuration (rocPRIM 4.2, device_radix_sort.hpp) sorts up to 1024 items
(256 threads x 4 items, for 4-byte and for 8-byte keys alike) in one block, up to 1 048 576 (merge_sort_limit) by block sorts and merge
passes, and only above that by the onesweep radix sort.  The tests of the single stages stop at 9999 keys: one block and the lower end
of the merge path.  scale_util.sort_path names the path of a size; the sizes below are chosen with it."""
import time

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import lbvh_util as LU
import normals_util as NU
import pose_util as PS
import scale_util as SU
from test_lbvh_gpu import assert_equals_host as lbvh_equals_host
from test_normals_gpu import assert_props, expected_props, tree_scene
from test_pose_gpu import make_pose, rig_for
from test_treeopt_gpu import assert_equals_host as treeopt_equals_host

pytestmark = pytest.mark.gpu
PS_MAX_GRID, PS_BLOCK = SU.PS_MAX_GRID, SU.PS_BLOCK      # kPsMaxGrid and kPsBlock of csrc/pt_pose.hip, mirrored in scale_util
NAN_BITS = 0x7FC00000


# ---- 1. pose: the second trip of the tile loop
@pytest.mark.parametrize("V", SU.POSE_SEAM_VERTS)
def test_pose_past_the_grid_cap_equals_the_rule_and_the_host(pkg, device, V):
    """V = PS_MAX_GRID * PS_BLOCK: 2048 tiles, one trip everywhere.  + 1: block 0 makes a second trip for a single vertex.  + PS_BLOCK + 1:
    blocks 0 and 1 make a second trip, block 1's for a single vertex.  (K, J, T) of SU.POSE_SEAM_RIGS: the joint matrices in LDS (3, and
    the 640 that fill it) must survive the reuse of the stage in front of them; 641 are read from global memory.  The vertex buffer holds
    NaN bits before each update, so a vertex that no trip wrote shows."""
    capi = pkg.capi
    assert V >= PS_MAX_GRID * PS_BLOCK
    sb = capi.SceneBuffers(device, SU.flat_scene(capi, V))
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    try:
        r.bind_scene(sb)
        sentinel = np.full(3 * V, NAN_BITS, np.uint32)
        for K, J, T in SU.POSE_SEAM_RIGS:
            what = "V %d K %d J %d T %d" % (V, K, J, T)
            rig = rig_for(V, K, J, T)
            # by the rule a vertex whose weights are all zero keeps its (morphed) rest position: past the cap every vertex gets an influence
            idle = np.flatnonzero(~rig["weights"][PS_MAX_GRID * PS_BLOCK:].any(axis=1)) + PS_MAX_GRID * PS_BLOCK
            rig["weights"][idle, 0] = 0.5; rig["joints"][idle, 0] = idle % J
            t0 = time.perf_counter()
            want = PS.restated(rig)
            t1 = time.perf_counter()
            host = PS.host(capi, rig)
            t2 = time.perf_counter()
            assert PS.differing(want, host) == 0, what + ": gmupt_pose_host differs from the restatement"
            assert not np.isnan(want).any()
            pose = make_pose(capi, r, rig)
            try:
                sb.verts.update(sentinel)
                info = pose.update(rig["mats"], rig["target_weights"], info=True)
                got = sb.verts.read(np.float32).reshape(-1, 3)
            finally:
                pose.close()
            print("%s: restatement %.2f s, host %.2f s, device %.3f ms" % (what, t1 - t0, t2 - t1, info["ms"]))
            assert info["num_verts"] == V and got.shape == (V, 3), what
            assert not (got.view(np.uint32) == NAN_BITS).any(), "%s: %d words were never written" % (what, int((got.view(np.uint32) == NAN_BITS).sum()))
            bad = np.flatnonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
            assert len(bad) == 0, "%s: %d vertices differ from the restatement, the first in tile %d" % (what, len(bad), bad[0] // PS_BLOCK)
            assert PS.differing(got, host) == 0, what + ": differs from gmupt_pose_host"
            for tile in (PS_MAX_GRID, PS_MAX_GRID + 1):      # what a second trip wrote is a pose, not the rest positions
                lo, hi = tile * PS_BLOCK, min((tile + 1) * PS_BLOCK, V)
                if lo < V:
                    for posed in (want, got):
                        assert np.all(np.any(posed[lo:hi].view(np.uint32) != rig["rest"][lo:hi].view(np.uint32), axis=1)), (what, tile)
    finally:
        r.close(); sb.close()


# ---- 2. pose: active targets across the waves of k_ps_active
@pytest.fixture(scope="module")
def active_scene(pkg, device):
    capi = pkg.capi
    sb = capi.SceneBuffers(device, SU.flat_scene(capi, SU.ACTIVE_VERTS))
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    r.bind_scene(sb)
    yield r, sb
    r.close(); sb.close()


@pytest.mark.parametrize("K,J", SU.ACTIVE_RIGS)
def test_pose_active_targets_in_every_wave(pkg, device, active_scene, K, J):
    """T = 64 .. 256 targets: weights in waves 1 to 3 of k_ps_active, so its cross-wave prefix is not zero and its lane mask is taken at
    every lane.  The morph sum is ordered, so a target in a wrong slot or a wrong order changes bits (test_scale_seams_cpu.py shows that
    for these very deltas).  With a NaN weight every vertex is NaN, and IEEE 754 does not say which: there the comparison is of the NaN
    masks and of the bits elsewhere."""
    capi = pkg.capi
    r, sb = active_scene
    V = SU.ACTIVE_VERTS
    seen = 0
    for k, j, T, name, rig in SU.active_cases():
        if (k, j) != (K, J):
            continue
        what = "K %d J %d T %d %s" % (K, J, T, name)
        tw = rig["target_weights"]
        want, host = PS.restated(rig), PS.host(capi, rig)
        pose = make_pose(capi, r, rig)
        try:
            sb.verts.update(np.full(3 * V, NAN_BITS, np.uint32) if name != "nan70" else np.zeros(3 * V, np.float32))
            info = pose.update(rig["mats"], tw, info=True)
            got = sb.verts.read(np.float32).reshape(-1, 3)
        finally:
            pose.close()
        assert info["active_targets"] == int((tw != 0).sum()) and info["num_verts"] == V, (what, info)
        if name == "nan70":
            assert info["active_targets"] == int(np.count_nonzero(tw[~np.isnan(tw)])) + 1
            for other in (want, host):
                assert np.array_equal(np.isnan(got), np.isnan(other)) and np.isnan(got).all(), what
                assert np.array_equal(got.view(np.uint32)[~np.isnan(other)], other.view(np.uint32)[~np.isnan(other)]), what
        else:
            assert PS.differing(got, want) == 0, "%s: %d vertices differ from the restatement" % (what, PS.differing(got, want))
            assert PS.differing(got, host) == 0, "%s: %d vertices differ from gmupt_pose_host" % (what, PS.differing(got, host))
        seen += 1
    assert seen == 4 * len(SU.ACTIVE_TARGETS) + sum(1 for T in SU.ACTIVE_TARGETS if T > SU.NAN_TARGET)


# ---- 3. the LBVH builder
@pytest.fixture(scope="module")
def builder(pkg, device):
    b = pkg.capi.Lbvh(device)
    yield b
    b.close()


@pytest.fixture(scope="module")
def grid_1m():
    return SU.grid_mesh(128, 128, 64)


@pytest.mark.parametrize("L", [1, 4])
def test_lbvh_grid_of_1048576_triangles(pkg, device, builder, grid_1m, L):
    """128 x 128 x 64 cells: 4096 block partials for k_lb_bounds2; at L = 1 a depth of 524 288 inner nodes and one of 1 048 576 leaves for
    k_lb_level (two and four trips); the first sort at merge_sort_limit exactly, the last size of the merge path; the second sort,
    2 097 151 node ids at either L, on the onesweep path."""
    t0 = time.perf_counter()
    info = lbvh_equals_host(pkg, device, builder, grid_1m, L, "grid 128x128x64")
    print("grid 128x128x64, L = %d: device %.3f ms, build + host reference + comparison %.2f s" % (L, info["ms"], time.perf_counter() - t0))
    assert info["num_tris"] == 1 << 20 and info["num_nodes"] == ((1 << 21) - 1 if L == 1 else (1 << 19) - 1)


def test_lbvh_first_sort_on_the_onesweep_path(pkg, device, builder):
    """128 x 128 x 65 cells, 1 064 960 triangles: the first sort, on all 63 key bits, leaves the merge path too."""
    mesh = SU.grid_mesh(128, 128, 65)
    assert SU.sort_path(len(mesh["indices"])) == "onesweep"
    info = lbvh_equals_host(pkg, device, builder, mesh, 4, "grid 128x128x65")
    print("grid 128x128x65, L = 4: device %.3f ms" % info["ms"])


@pytest.mark.parametrize("L", [1, 4])
def test_lbvh_irregular_tree_past_256_partials(pkg, device, builder, L):
    mesh = LU.soup(70_000, 1)
    assert SU.bounds_partials(len(mesh["indices"])) > SU.LB_BLOCK
    lbvh_equals_host(pkg, device, builder, mesh, L, "soup70000")


@pytest.mark.parametrize("n", [65_536, 65_537])
def test_lbvh_on_the_boundary_of_the_partials_loop(pkg, device, builder, n):
    """256 block partials: one per thread of k_lb_bounds2 and no second trip; 257: thread 0 alone makes one."""
    mesh = LU.soup(n, 2)
    assert SU.bounds_partials(n) == SU.LB_BLOCK + (n > 65_536)
    lbvh_equals_host(pkg, device, builder, mesh, 4, "soup%d" % n)


@pytest.mark.parametrize("nz", [16, 65])
def test_lbvh_equal_keys_keep_index_order_at_scale(pkg, device, builder, nz):
    """Four triangles per cell of 64 x 64 x nz, each with vertices and a box of its own, in a permuted index list: the order of the four in
    the records and in ref_triangle is the first sort's order among equal keys.  nz = 16: 262 144 triangles, the merge path; nz = 65:
    1 064 960, the onesweep path."""
    mesh = SU.grid_mesh(64, 64, nz, seed=1, copies=4)
    n = len(mesh["indices"])
    assert SU.sort_path(n) == ("merge" if nz == 16 else "onesweep")
    info = lbvh_equals_host(pkg, device, builder, mesh, 1, "grid 64x64x%d x 4 copies" % nz)
    assert info["num_tris"] == n and info["num_nodes"] == 2 * n - 1


# ---- 4. the treelet optimiser
@pytest.fixture(scope="module")
def optimizer(pkg, device):
    o = pkg.capi.TreeOptimizer(device)
    yield o
    o.close()


@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("name", ["soup70000", "grid64x32x32"])
def test_treeopt_levels_past_the_grid_cap(pkg, device, optimizer, name, passes):
    """The host LBVH at L = 1 of a 70 000-triangle soup (139 999 records, up to 18 243 inner nodes at a depth: three trips of
    k_to_level) and of the 64 x 32 x 32 grid (131 071 records, 32 768 inner nodes at depth 15: four trips).  Both are rewritten by the
    host reference (test_scale_seams_cpu.py): the plain grid needed no jitter beyond grid_mesh's per-triangle extents.
    tree_optimize_host takes 0.15 s (one pass) and 0.40 s (three) on the soup's tree, 0.11 s and 0.30 s on the grid's."""
    mesh = LU.soup(70_000, 3) if name == "soup70000" else SU.grid_mesh(64, 32, 32)
    nodes = pkg.capi.lbvh_build_host(mesh["verts"], mesh["indices"], mesh["vertex_material"], 1)["nodes"]
    assert len(nodes) == 2 * len(mesh["indices"]) - 1
    t0 = time.perf_counter()
    _, info = treeopt_equals_host(pkg, device, optimizer, nodes, passes, name + ", L = 1")
    print("%s, %d passes: device %.3f ms, %d treelets rewritten, device run + host reference + comparison %.2f s" % (
        name, passes, info["ms"], info["treelets_rewritten"], time.perf_counter() - t0))
    assert info["treelets_rewritten"] > 0


# ---- 5. smooth normals
def normals_case(pkg, device, v, t, what):
    capi = pkg.capi
    scene = tree_scene(capi, v, t)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    try:
        r.bind_scene(sb)
        n = capi.Normals(r, t)
        info = n.update(info=True)
        assert info["num_verts"] == len(v) and info["num_tris"] == len(t), (what, info)
        assert info["max_valence"] == int(np.bincount(t.reshape(-1)).max()), (what, info)
        assert_props(sb.props.read(capi.tri_props_dtype), expected_props(capi, scene["props"], v, t), what)
        return info
    finally:
        r.close(); sb.close()


@pytest.mark.parametrize("n_spheres", [12, 70])
def test_normals_of_shared_vertices_past_the_small_sorts(pkg, device, n_spheres):
    """Icospheres at subdivision 4, vertices of valence 5 and 6 whose sums are ordered by the sort's stability: 12 of them are about
    184 000 corners (the merge path), 70 about 1 075 000 (the onesweep path)."""
    S = pkg.scenes
    mesh = S.spheres_mesh(n_spheres=n_spheres, subdiv=4, seed=7, floor_quads=4)
    v, t = S.wobble(mesh, 0.3), np.ascontiguousarray(mesh["indices"], np.int32)
    assert SU.sort_path(t.size) == ("merge" if n_spheres == 12 else "onesweep")
    info = normals_case(pkg, device, v, t, "spheres%d" % n_spheres)
    print("spheres%d: %d vertices, %d corners, device %.3f ms" % (n_spheres, len(v), t.size, info["ms"]))


@pytest.mark.parametrize("nv", [(1 << 17) - 1, 1 << 17, (1 << 17) + 1])
def test_normals_where_the_key_of_a_bad_index_needs_another_bit(pkg, device, nv):
    """nm_key_bits is 17 for 131 071 vertices and 18 from 131 072 on, where the key numVerts itself has a bit no vertex has."""
    v, t = NU.strip(nv)
    assert SU.nm_key_bits(nv) == (17 if nv < 1 << 17 else 18) and SU.sort_path(t.size) == "merge"
    normals_case(pkg, device, v, t, "strip%d" % nv)


def test_normals_refuse_an_index_equal_to_a_power_of_two_vertex_count(pkg, device):
    """One index equal to numVerts = 2^17: its key is the only one with bit 17 set.  create refuses, and the property records stay."""
    capi = pkg.capi
    nv = 1 << 17
    v, t = NU.strip(nv)
    scene = tree_scene(capi, v, t)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    try:
        r.bind_scene(sb)
        bad = t.copy(); bad[len(t) // 2, 1] = nv
        with pytest.raises(capi.GmuptError) as e:
            capi.Normals(r, bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and not r._normals
        r.synchronize()
        assert sb.props.read(capi.tri_props_dtype).tobytes() == scene["props"].tobytes()
        n = capi.Normals(r, t)                                # and the renderer still takes the good list
        n.update()
        assert_props(sb.props.read(capi.tri_props_dtype), expected_props(capi, scene["props"], v, t), "after the refusal")
    finally:
        r.close(); sb.close()

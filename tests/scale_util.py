"""Shared by the scale-seam tests (test_scale_seams_cpu.py, test_scale_seams_gpu.py): the sizes at which the mesh-update kernels change
behaviour -- a grid cap after which a block strides, a loop over block partials, the three paths of the sort library -- as mirrored
constants, the meshes and rigs that reach them, and the level counts that prove from a host tree alone that they are reached."""
import numpy as np

import pose_util as PS

F = np.float32

# ---- mirrors of kernel constants; test_scale_seams_cpu.py reads each one back from its source file
PS_BLOCK = 256                # kPsBlock, csrc/pt_pose.hip: vertices per tile of k_ps_pose
PS_MAX_GRID = 2048            # kPsMaxGrid, csrc/pt_pose.hip: blocks of k_ps_pose; beyond that many tiles a block walks further tiles
PS_MAX_TARGETS = 256          # kPsMaxTargets, csrc/pt_pose.hpp: one thread of k_ps_active per target, four waves
LB_BLOCK = 256                # kLbBlock, csrc/pt_lbvh.hip: triangles per block partial of k_lb_bounds; threads of k_lb_bounds2
LB_LEVEL_BLOCKS = 1024        # kLbLevelBlocks, csrc/pt_lbvh.hip: grid of k_lb_level
TO_BLOCK = 256                # kToBlock, csrc/pt_treeopt.hip
TO_LEVEL_BLOCKS = 2048        # kToLevelBlocks, csrc/pt_treeopt.hip: grid of k_to_level, one wave of 64 per inner node
MIRRORED = {"pt_pose.hip": {"kPsBlock": PS_BLOCK, "kPsMaxGrid": PS_MAX_GRID}, "pt_pose.hpp": {"kPsMaxTargets": PS_MAX_TARGETS},
            "pt_lbvh.hip": {"kLbBlock": LB_BLOCK, "kLbLevelBlocks": LB_LEVEL_BLOCKS},
            "pt_treeopt.hip": {"kToBlock": TO_BLOCK, "kToLevelBlocks": TO_LEVEL_BLOCKS}}
LB_LEVEL_STRIDE = LB_LEVEL_BLOCKS * LB_BLOCK            # 262 144 kept nodes of one depth: beyond it k_lb_level strides
TO_LEVEL_STRIDE = TO_LEVEL_BLOCKS * (TO_BLOCK // 64)    # 8192 entries of one depth: beyond it k_to_level strides

# ---- the paths of rocprim::radix_sort_pairs with the default configuration, which every sort of the library uses (rocPRIM 4.2,
# device_radix_sort.hpp: radix_sort_impl; the same for 4-byte and 8-byte keys with 4-byte values):
#   size <= 1024 (256 threads x 4 items)  one block, radix_sort_block_sort
#   size <= 1 048 576 (merge_sort_limit)  radix_sort_merge_impl: block sorts, then merge passes comparing the bit range
#   above                                 radix_sort_onesweep_impl: the only path that scatters by digit
SORT_ONE_BLOCK = 1024
SORT_MERGE_LIMIT = 1024 * 1024


def sort_path(size):
    return "block" if size <= SORT_ONE_BLOCK else "merge" if size <= SORT_MERGE_LIMIT else "onesweep"


# ---- pose
POSE_SEAM_VERTS = (PS_MAX_GRID * PS_BLOCK, PS_MAX_GRID * PS_BLOCK + 1, PS_MAX_GRID * PS_BLOCK + PS_BLOCK + 1)
POSE_SEAM_RIGS = ((1, 3, 0), (4, 640, 2), (4, 641, 2))          # (K, J, T): matrices in LDS, the most that fit there, in global memory
ACTIVE_VERTS = 65
ACTIVE_TARGETS = (64, 65, 128, 129, 255, 256)
ACTIVE_RIGS = ((0, 0), (4, 3))                                  # (K, J): morph only, and skinned
NAN_TARGET = 70


def pose_trips(V):
    """Trips of k_ps_pose's tile loop per block, as {trips: number of blocks}, and the tile count."""
    tiles = (V + PS_BLOCK - 1) // PS_BLOCK
    grid = min(tiles, PS_MAX_GRID)
    trips = {}
    for b in range(grid):
        k = len(range(b, tiles, grid))
        trips[k] = trips.get(k, 0) + 1
    return trips, tiles


def target_weight_patterns(T, seed=0):
    """name -> (T,) float32 target weights: the patterns that put work into every wave of k_ps_active and every term of its prefix."""
    rng = np.random.default_rng([T, seed])
    full = (rng.uniform(0.25, 1.0, T) * np.where(rng.random(T) < 0.5, -1.0, 1.0)).astype(F)
    out = {"all": full.copy()}
    third = full.copy()
    third[0::6] = F(0.0); third[3::6] = F(-0.0)                  # every third weight zero, both signs
    out["third_zero"] = third
    wave0 = full.copy(); wave0[:64] = F(0.0)                     # nothing in wave 0: base of wave 1 is 0 with a non-empty wave below it
    out["wave0_zero"] = wave0
    last = np.zeros(T, F); last[T - 1] = full[T - 1]
    out["only_last"] = last
    if T > NAN_TARGET:
        nan = third.copy(); nan[NAN_TARGET] = np.nan             # a NaN weight is active (k_ps_active: w != 0; the rule: a[t] != 0)
        out["nan70"] = nan
    return out


def active_cases():
    """(K, J, T, pattern name, rig) of every case of the active-target tests; the rig's target weights are the pattern."""
    for K, J in ACTIVE_RIGS:
        for T in ACTIVE_TARGETS:
            for name, tw in target_weight_patterns(T).items():
                rig = PS.random_rig(ACTIVE_VERTS, K, J, T, 7)
                rig["target_weights"] = tw
                yield K, J, T, name, rig


def flat_scene(capi, V):
    """A scene dict the renderer binds whose vertex buffer holds V vertices: one triangle on the first three, a one-leaf tree, V zeroed
    property records.  What the pose stage needs of a binding is the vertex buffer alone."""
    verts = np.zeros((V, 3), F)
    verts[:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    built = capi.lbvh_build_host(verts[:3], np.array([[0, 1, 2]], np.int32))
    return {"nodes": built["nodes"], "tris": built["tris"], "verts": verts, "props": np.zeros(V, capi.tri_props_dtype),
            "lights": np.zeros(1, capi.light_dtype), "materials": np.zeros(1, capi.material_dtype)}


# ---- trees
GRID_HALVES = (2.0 ** -4, 2.0 ** -3, 2.0 ** -2)


def grid_mesh(nx, ny, nz, seed=0, copies=1):
    """One triangle per cell of an nx x ny x nz grid (`copies` of them per cell), each with vertices of its own: the cell's integer
    coordinates plus (-h, -h, -h), (h, -h, h), (-h, h, h) -- the corners of lbvh_util.key_chain -- with h a per-triangle power of two
    from GRID_HALVES.  The box centre is the cell centre exactly, so the copies of a cell share one Morton key, and the leaf boxes
    differ.  The vertices are stored in cell order (z slowest, copies adjacent); the index list is a seeded permutation of the triangles,
    so the first sort has work to do and the order among equal keys is that of the permuted list."""
    rng = np.random.default_rng([nx, ny, nz, seed, copies])
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = np.repeat(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F), copies, axis=0)
    n = len(c)
    h = np.array(GRID_HALVES, F)[rng.integers(0, len(GRID_HALVES), n)]
    corners = np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], F)
    v = c[:, None, :] + h[:, None, None] * corners[None, :, :]
    assert v.dtype == np.float32
    idx = np.arange(3 * n, dtype=np.int32).reshape(n, 3)[rng.permutation(n)]
    return {"verts": v.reshape(-1, 3), "indices": np.ascontiguousarray(idx), "vertex_material": rng.integers(0, 3, 3 * n).astype(np.uint32)}


def nodes_per_depth(nodes):
    """(kept, inner): the number of records and of inner records at each depth of a record array, by walking left / right level by level."""
    left, right, leaf = nodes["left"].astype(np.int64), nodes["right"].astype(np.int64), nodes["isLeaf"] != 0
    level = np.zeros(1, np.int64)
    kept, inner = [], []
    while len(level):
        x = level[~leaf[level]]
        kept.append(len(level)); inner.append(len(x))
        level = np.concatenate([left[x], right[x]])
    assert sum(kept) == len(nodes)
    return kept, inner


def bounds_partials(n):
    """Block partials k_lb_bounds2 reduces for n triangles; its 256 threads stride once there are more than 256."""
    return (n + LB_BLOCK - 1) // LB_BLOCK


# ---- normals
def nm_key_bits(num_verts):
    """nm_key_bits of csrc/pt_normals.hip: the bits of the keys 0 .. numVerts."""
    b = 1
    while b < 32 and (num_verts >> b):
        b += 1
    return b

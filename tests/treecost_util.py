"""The tree-cost rule of include/gmupt.h ("Tree cost") restated in numpy, written from the header alone, and the inputs the tree-cost tests
share: crafted record arrays (no tree needed: the rule follows no link), the library meshes, and the two seeded poses of the policy tests."""
import numpy as np

import lbvh_util as LU

RUN = 256
INT_FIELDS = ("num_inner", "num_leaves", "num_refs", "max_leaf_refs")
DOUBLE_FIELDS = ("sum_inner", "sum_leaf", "root_half_area", "sah")
SIZES_CPU = (1, 2, 255, 256, 257, 65536, 65537)                   # 65537: the first size with a third level
SIZES_GPU = (1, 2, 63, 64, 65, 255, 256, 257, 65536, 65537)       # wave, block and level boundaries
SPECIAL = ("max_below_min", "nan", "inf", "zero_root", "wrap")


def ordered_sum(terms):
    """The summation order of the rule: runs of 256 (padded with +0.0), stride halving inside a run, level by level."""
    x = np.asarray(terms, np.float64)
    while True:
        runs = (len(x) + RUN - 1) // RUN
        x = np.concatenate([x, np.zeros(runs * RUN - len(x), np.float64)]).reshape(runs, RUN)
        s = RUN // 2
        while s >= 1:
            x = x[:, :s] + x[:, s:2 * s]
            s //= 2
        x = x[:, 0]
        if len(x) == 1:
            return float(x[0])


def rule(nodes):
    """The gmupt_tree_cost_info fields (without ms) of a record array, by the header's sentences."""
    nodes = np.asarray(nodes)
    with np.errstate(invalid="ignore", over="ignore"):
        d = nodes["max"].astype(np.float64) - nodes["min"].astype(np.float64)
        e = np.where(d > 0, d, 0.0)
        a = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]
        leaf = nodes["isLeaf"] != 0
        refs = (nodes["right"].astype(np.uint32) - nodes["left"].astype(np.uint32)).astype(np.uint32)      # wraps
        w = np.where(leaf, refs.astype(np.float64), 2.0)
        term = a * w
        sum_inner = ordered_sum(np.where(leaf, 0.0, term))
        sum_leaf = ordered_sum(np.where(leaf, term, 0.0))
        root = float(a[0])
        sah = (sum_inner + sum_leaf) / root if root > 0 else 0.0
    leaf_refs = refs[leaf].astype(np.uint64)
    return {"sum_inner": sum_inner, "sum_leaf": sum_leaf, "root_half_area": root, "sah": float(sah),
            "num_inner": int((~leaf).sum()), "num_leaves": int(leaf.sum()), "num_refs": int(leaf_refs.sum(dtype=np.uint64)),
            "max_leaf_refs": int(leaf_refs.max()) if len(leaf_refs) else 0}


def bits(x):
    return np.float64(x).view(np.uint64)


def differing(got, want):
    """The fields (ms aside) in which two results differ: integers by value, doubles by bit pattern."""
    return [k for k in INT_FIELDS if got[k] != want[k]] + [k for k in DOUBLE_FIELDS if bits(got[k]) != bits(want[k])]


def random_records(n, seed, node_dtype):
    """n records with random boxes of positive extent and random kind / links: isLeaf any value (0 in about half), left / right any
    int32, so that about half of the leaves have right < left."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros(n, node_dtype)
    nodes["min"] = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    nodes["max"] = nodes["min"] + rng.uniform(0.01, 5, (n, 3)).astype(np.float32)
    nodes["isLeaf"] = np.where(rng.random(n) < 0.5, 0, rng.integers(-3, 4, n))
    nodes["left"] = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    nodes["right"] = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    small = rng.random(n) < 0.5                                     # the other half: the small ranges of a real leaf
    nodes["left"][small] = rng.integers(0, 1000, n)[small]
    nodes["right"][small] = nodes["left"][small] + rng.integers(0, 9, n)[small]
    for k in ("pad0", "pad1", "pad2"):
        nodes[k] = rng.uniform(-1, 1, n).astype(np.float32)         # ignored by the rule
    return nodes


def special_records(kind, node_dtype, n=300):
    """The edge cases of the rule inside n random records.  None of them produces inf * 0, the one NaN the rule leaves unspecified."""
    nodes = random_records(n, 1000 + SPECIAL.index(kind), node_dtype)
    pick = np.arange(3, n, 7)                # (record 0, the root, stays an ordinary box except in zero_root)
    if kind == "max_below_min":              # every second picked record on all axes, the others on one
        nodes["max"][pick[::2]] = nodes["min"][pick[::2]] - 1.0
        nodes["max"][pick[1::2], 1] = nodes["min"][pick[1::2], 1] - 0.5
    elif kind == "nan":
        nodes["min"][pick[::2], 0] = np.nan
        nodes["max"][pick[1::2], 2] = np.nan
        nodes["max"][pick[0]] = np.nan; nodes["min"][pick[0]] = np.nan
    elif kind == "inf":                      # an infinite extent next to positive ones, on an inner node and on a leaf of three references
        nodes["max"][7, 0] = np.inf; nodes["isLeaf"][7] = 0
        nodes["min"][14, 1] = -np.inf; nodes["isLeaf"][14] = 1; nodes["left"][14] = 5; nodes["right"][14] = 8
    elif kind == "zero_root":                # a root that is a segment: no area, sah == 0.0
        nodes["max"][0, :2] = nodes["min"][0, :2]
    elif kind == "wrap":                     # right < left on every picked record, all of them leaves
        nodes["isLeaf"][pick] = 1
        nodes["left"][pick] = 10; nodes["right"][pick] = np.arange(len(pick)) % 10
    else:
        raise ValueError(kind)
    return nodes


def library_scenes(scenes):
    """name -> (mesh, sbvh scene, lbvh scene) of the three library meshes the GPU tests bind, and of the Morton key chain whose LBVH (leaf
    size 4) is 64 levels deep, the deepest tree the builder accepts."""
    meshes = {"cornell": scenes.cornell_mesh(), "soup": scenes.random_triangles_mesh(2000, seed=1),
              "spheres_small": scenes.spheres_mesh(n_spheres=12, subdiv=2, seed=7, floor_quads=4),
              "key_chain": LU.key_chain_render_mesh(scenes, 8, 0.125)}
    return {k: (m, scenes.build_scene(m), scenes.build_scene(m, builder="lbvh")) for k, m in meshes.items()}


# ---- the poses of the policy tests (the Cornell box): checked on the host rule by test_treecost_cpu.py, used on the device by
# test_treecost_gpu.py.  A seed that fails the conditions there is replaced HERE; the conditions stay.
POLICY_THRESHOLD = 1.5
POSE_SEEDS = {"scatter": 1, "jitter": 2}


def pose(scene, kind):
    """scatter: every vertex at a uniform random point of the scene's bounds.  jitter: every vertex displaced by 1e-3 of the largest
    extent (a uniform random offset per component)."""
    v = np.asarray(scene["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    rng = np.random.default_rng(POSE_SEEDS[kind])
    if kind == "scatter":
        return rng.uniform(lo, hi, v.shape).astype(np.float32)
    return (v + rng.uniform(-1.0, 1.0, v.shape) * (1e-3 * float((hi - lo).max()))).astype(np.float32)


def host_policy_figures(capi, scene, verts):
    """What the policy sees for a pose, by the host rule: (bind-time sah, sah of the refitted tree, the LBVH candidate of the pose as
    lbvh_build_host returns it, its sah).  The candidate uses what rebuild() picks before any rebuild: the bound triangle records'
    index triples and the materialID column of the property records."""
    base = capi.tree_cost_host(scene["nodes"])["sah"]
    refitted = capi.tree_cost_host(capi.bvh_refit_host(scene["nodes"], scene["tris"], verts))["sah"]
    cand = capi.lbvh_build_host(verts, scene["tris"]["v"], np.ascontiguousarray(scene["props"]["materialID"]))
    return base, refitted, cand, capi.tree_cost_host(cand["nodes"])["sah"]

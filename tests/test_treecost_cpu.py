"""gmupt_tree_cost_host, the reference of the device tree cost (include/gmupt.h "Tree cost"), against the independent numpy restatement of
the rule in treecost_util.py -- bit for bit, on crafted record arrays -- and against capi.tree_sah on the library meshes within the bound
of a reordered sum.  The two poses the GPU policy test uses are checked here on the host rule.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import treecost_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_tree_cost_host", "gmupt_renderer_tree_cost"]


@pytest.fixture(scope="module")
def library(pkg):
    return TU.library_scenes(pkg.scenes)


@pytest.mark.parametrize("n", TU.SIZES_CPU)
def test_host_rule_equals_the_restatement_bit_for_bit(pkg, n):
    nodes = TU.random_records(n, n, pkg.capi.bvh_node_dtype)
    got, want = pkg.capi.tree_cost_host(nodes), TU.rule(nodes)
    assert not TU.differing(got, want), (n, TU.differing(got, want), got, want)
    assert got["ms"] == 0.0 and got["num_inner"] + got["num_leaves"] == n


@pytest.mark.parametrize("kind", TU.SPECIAL)
def test_edge_cases_equal_the_restatement_bit_for_bit(pkg, kind):
    nodes = TU.special_records(kind, pkg.capi.bvh_node_dtype)
    got, want = pkg.capi.tree_cost_host(nodes), TU.rule(nodes)
    assert not TU.differing(got, want), (kind, TU.differing(got, want), got, want)
    if kind == "zero_root":
        assert got["root_half_area"] == 0.0 and TU.bits(got["sah"]) == 0 and got["sum_inner"] > 0
    elif kind == "inf":
        assert got["sum_inner"] == np.inf and got["sum_leaf"] == np.inf and got["sah"] == np.inf
    elif kind == "wrap":
        assert got["max_leaf_refs"] == 2**32 - 1                        # right = 9, left = 10
    else:
        assert np.isfinite(got["sah"]) and got["sah"] > 0


def test_nan_and_inverted_boxes_count_as_flat(pkg):
    """Extent: a NaN or max < min gives 0 -- the record contributes what the same record with that axis flat contributes."""
    dt = pkg.capi.bvh_node_dtype
    for kind in ("nan", "max_below_min"):
        nodes = TU.special_records(kind, dt)
        flat = nodes.copy()
        with np.errstate(invalid="ignore"):
            bad = ~(flat["max"] > flat["min"])
        flat["max"][bad] = 0.0; flat["min"][bad] = 0.0
        assert bad.any() and not TU.differing(pkg.capi.tree_cost_host(nodes), pkg.capi.tree_cost_host(flat)), kind


def test_thread_counts_give_the_same_bits(pkg):
    for n in (257, 65537, 300000):                                      # 300000: several runs per thread at every count
        nodes = TU.random_records(n, 7 * n, pkg.capi.bvh_node_dtype)
        one = pkg.capi.tree_cost_host(nodes, threads=1)
        for threads in (3, 16):
            assert not TU.differing(pkg.capi.tree_cost_host(nodes, threads=threads), one), (n, threads)


def test_library_meshes_agree_with_tree_sah(pkg, library):
    """Reordering N non-negative double terms moves their sum by at most N * 2^-53 relative per addition chain end to end, i.e. well within
    N * 2^-52; tree_sah's 2 * area and int count differ from the rule's half area and uint32 weight by exact factors, its final
    division and the handful of roundings per term by a few ulp more: (N + 8) * 2^-52."""
    assert library["key_chain"][2]["depth"] == 64, "the key chain's LBVH is the deepest tree the builder accepts"
    for name, (_, sbvh, lbvh) in library.items():
        for what, scene in (("sbvh", sbvh), ("lbvh", lbvh)):
            nodes = scene["nodes"]
            N = len(nodes)
            got, ref = pkg.capi.tree_cost_host(nodes), pkg.capi.tree_sah(nodes)
            rel = abs(got["sah"] - ref) / ref
            print("%s %s: %d nodes, sah %.17g, tree_sah %.17g, relative difference %.3g (bound %.3g)" % (name, what, N, got["sah"], ref, rel, (N + 8) * 2.0**-52))
            assert ref > 0 and rel <= (N + 8) * 2.0**-52, (name, what)
            leaf = nodes["isLeaf"] != 0
            refs = (nodes["right"][leaf].astype(np.int64) - nodes["left"][leaf])
            assert got["num_inner"] == int((~leaf).sum()) and got["num_leaves"] == int(leaf.sum())
            assert got["num_refs"] == int(refs.sum()) == len(scene["tris"]) and got["max_leaf_refs"] == int(refs.max())
            assert not TU.differing(got, TU.rule(nodes)), (name, what)


def test_errors_leave_the_info_untouched(pkg):
    capi = pkg.capi
    lib = capi.lib()
    nodes = TU.random_records(10, 3, capi.bvh_node_dtype)
    info = capi.TreeCostInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    before = bytes(info)
    p = nodes.ctypes.data_as(C.c_void_p)
    for args in ((None, 10, C.byref(info)), (p, 0, C.byref(info)), (p, 10, None)):
        assert lib.gmupt_tree_cost_host(*args, 4) == capi.ERR_INVALID_ARGUMENT
        assert bytes(info) == before
    assert b"gmupt_tree_cost_host" in lib.gmupt_last_error()
    with pytest.raises(capi.GmuptError) as e:
        capi.tree_cost_host(nodes[:0])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_renderer_tree_cost(None, None, C.byref(info)) == capi.ERR_INVALID_ARGUMENT and bytes(info) == before   # before any device is touched


def test_policy_poses_meet_their_conditions(pkg, library):
    """What tests/test_treecost_gpu.py relies on, on the host rule: "scatter" degrades the refitted tree beyond the threshold and its LBVH
    is cheaper than the refitted tree; "jitter" stays below the threshold."""
    capi = pkg.capi
    scene = library["cornell"][1]
    base, refitted, _, cand = TU.host_policy_figures(capi, scene, TU.pose(scene, "scatter"))
    print("scatter: bind %.6g, refitted %.6g (x %.4f), LBVH of the pose %.6g" % (base, refitted, refitted / base, cand))
    assert base > 0 and refitted > TU.POLICY_THRESHOLD * base and cand < refitted
    base, refitted, _, cand = TU.host_policy_figures(capi, scene, TU.pose(scene, "jitter"))
    print("jitter: bind %.6g, refitted %.6g (x %.6f), LBVH of the pose %.6g" % (base, refitted, refitted / base, cand))
    assert refitted < TU.POLICY_THRESHOLD * base
    assert refitted > base * 1.0000001, "the just-below threshold of the GPU test needs a ratio above 1"
    extent = float((scene["verts"].max(axis=0) - scene["verts"].min(axis=0)).max())
    assert np.abs(TU.pose(scene, "jitter").astype(np.float64) - scene["verts"]).max() <= 1.001e-3 * extent


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in pkg.capi.SYMBOLS, name
        assert getattr(lib, name, None) is not None, name
    assert C.sizeof(pkg.capi.TreeCostInfo) == 64 and pkg.capi.TreeCostInfo.ms.offset == 56
    assert "Tree cost" in header


def test_session_signature_keeps_the_default(pkg):
    import inspect
    sig = inspect.signature(pkg.progressive.ProgressiveSession.set_vertices)
    assert sig.parameters["rebuild_above"].default is None
    with pytest.raises(ValueError):
        pkg.progressive.ProgressiveSession(None, None, 4, 4).set_vertices(None, None, rebuild_above=1.0)

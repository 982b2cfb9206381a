"""CPU tests of the restated refit rule (tests/refit_tables_util.py), the expected value of tests/test_refit_tables_gpu.py: no device.

The host-built tables of a tree are what the rule gives for that tree's own boxes and vertices, so the restatement applied to them must
change no byte (fixed point).  That pins the restatement against build_trav_tables, which the golden digests of test_travtables_cpu.py
pin in turn; the GPU tests then compare the k_rf_* kernels with the restatement.
"""
import contextlib

import numpy as np
import pytest

import refit_tables_util as RT

NONE = RT.NONE
FIXTURES = ("cornell", "soup", "spheres", "chain", "textured")
CRAFTED = ("empty_leaf", "lbvh1", "lbvh2", "lbvh3", "lbvh257")
ALL = FIXTURES + CRAFTED


@pytest.fixture(scope="module")
def scenes(pkg, cornell_scene, soup_scene, spheres_small_scene):
    S = pkg.scenes
    out = {"cornell": cornell_scene, "soup": soup_scene, "spheres": spheres_small_scene,
           "chain": S.build_scene(S.deep_chain_mesh()), "textured": S.build_scene(S.textured_mesh()),
           "empty_leaf": RT.empty_leaf_scene(pkg)}
    for n in (1, 2, 3, 257):
        out["lbvh%d" % n] = RT.lbvh_scene(pkg, n, 500 + n, 1)
    return out


@pytest.fixture(scope="module")
def tables(pkg, scenes):
    cache = {}

    def get(name, want_wide=True):
        if (name, want_wide) not in cache:
            s = scenes[name]
            cache[name, want_wide] = pkg.capi.travtables(s["nodes"], s["tris"], s["verts"], want_wide=want_wide)
        return cache[name, want_wide]
    return get


@pytest.mark.parametrize("want_wide", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_the_host_built_tables_are_a_fixed_point_of_the_rule(scenes, tables, name, want_wide):
    s, T = scenes[name], tables(name, want_wide)
    RT.assert_tables(RT.refit_tables(T, s["nodes"], s["tris"], s["verts"]), T, "%s, want_wide=%s" % (name, want_wide))


@pytest.mark.parametrize("name", ALL)
def test_moved_vertices_change_the_tables_and_every_box_is_its_nodes(pkg, scenes, tables, name):
    s, T = scenes[name], tables(name)
    w = pkg.scenes.wobble(s, 0.3, 0.05)
    nodes = pkg.capi.bvh_refit_host(s["nodes"], s["tris"], w)
    E = RT.refit_tables(T, nodes, s["tris"], w)
    changed = [k for k in RT.KINDS if not np.array_equal(E[k], T[k])]
    assert "tri48" in changed and "scalars" in changed, "the wobble moves nothing: %r" % (changed,)
    if len(T["wnode"]):
        assert {"tripair", "node64", "wnode"} <= set(changed), changed
    assert not set(changed) & set(RT.MAPS) and "pair_ref" not in changed, "the rule writes no map"
    n_packed, n_slots = RT.assert_tight(E, nodes)
    assert n_packed == int((nodes["isLeaf"] == 0).sum())
    assert n_slots == (len(nodes) - 1 - len(T["opened"]) // 4 if len(T["wnode"]) else 0)
    # what the rule keeps: flag and first-equal words, the sentinel, w[18] / w[19], descriptors, link and aux rows, NaN slots, fillers
    tri_e, tri_t = E["tri48"].view(np.uint32).reshape(-1, 12), T["tri48"].view(np.uint32).reshape(-1, 12)
    assert np.array_equal(tri_e[:, 9:], tri_t[:, 9:]) and np.array_equal(tri_e[-1], tri_t[-1])
    assert np.array_equal(E["node64"].view(np.uint32).reshape(-1, 16)[:, 12:], T["node64"].view(np.uint32).reshape(-1, 16)[:, 12:])
    if len(T["wnode"]):
        assert np.array_equal(E["tripair"].view(np.uint32).reshape(-1, 20)[:, 18:], T["tripair"].view(np.uint32).reshape(-1, 20)[:, 18:])
        assert np.array_equal(E["wnode"].view(np.uint32).reshape(-1, 32)[:, 24:], T["wnode"].view(np.uint32).reshape(-1, 32)[:, 24:])
    # and the boxes are tight for the moved vertices, not the old ones: the restatement of the ORIGINAL nodes fails the same check
    with pytest.raises(AssertionError) if n_packed else contextlib.nullcontext():
        RT.assert_tight(RT.refit_tables(T, s["nodes"], s["tris"], w), nodes)


@pytest.mark.parametrize("name", ["soup", "spheres"])
def test_a_fresh_build_of_the_refitted_tree_is_not_the_expected_value(pkg, scenes, tables, name):
    """The numbering and the collapse follow the surface areas: the fresh build's WNode or Node64 differ from the tables refit leaves."""
    s, T = scenes[name], tables(name)
    w = pkg.scenes.wobble(s, 0.3, 0.05)
    nodes = pkg.capi.bvh_refit_host(s["nodes"], s["tris"], w)
    E = RT.refit_tables(T, nodes, s["tris"], w)
    fresh = pkg.capi.travtables(nodes, s["tris"], w)
    assert not RT.table_diffs(fresh, E, ("tri48", "tripair", "pair_ref")), "the triangle tables do not depend on the boxes"
    assert RT.table_diffs(fresh, E, ("wnode", "node64")), "%s: a fresh build happens to equal the refitted tables" % name


def test_the_scenes_hold_every_record_kind_the_kernels_branch_on(scenes, tables):
    T = {n: tables(n) for n in ALL}
    pair_ref = lambda n: T[n]["pair_ref"].view(np.uint32)
    assert any((pair_ref(n)[1::2] == NONE).any() for n in ALL), "no padding pair slot"
    assert any((T[n]["wide_map"].view(np.uint32) == NONE).any() for n in ALL), "no empty WNode slot"
    nan = np.float32(np.nan).view(np.uint32)
    for n in ALL:                                             # ... and such a slot is six quiet NaNs
        wm = T[n]["wide_map"].view(np.uint32).reshape(-1, 4)
        w, k = np.nonzero(wm == NONE)
        assert (T[n]["wnode"].view(np.uint32).reshape(-1, 8, 4)[w, :6, k] == nan).all(), n
    assert (T["chain"]["node_map"].view(np.uint32) == NONE).sum() == 1, "the chain scene has no filler Node64"
    # an empty leaf: its all-zero pair with two padding slots, and a descriptor that names the sentinel record R
    e = scenes["empty_leaf"]["nodes"]
    empty = np.flatnonzero((e["isLeaf"] != 0) & (e["right"] == e["left"]))
    assert len(empty) == 1, "the hand-made tree has no empty leaf"
    assert not any(((s["nodes"]["isLeaf"] != 0) & (s["nodes"]["right"] == s["nodes"]["left"])).any() for n, s in scenes.items() if n != "empty_leaf")
    R = len(scenes["empty_leaf"]["tris"])
    pr = pair_ref("empty_leaf").reshape(-1, 2)
    assert ((pr == NONE).all(axis=1)).sum() == 1, "the empty leaf's pair"
    assert (T["empty_leaf"]["node64"].view(np.int32).reshape(-1, 16)[:, 12:14] == ~R).sum() == 1, "no descriptor of the sentinel record"
    sentinel = T["empty_leaf"]["tri48"].view(np.uint32).reshape(-1, 12)[R]
    assert sentinel.tolist() == [0] * 9 + [1, NONE, 0]
    assert int(empty[0]) in T["empty_leaf"]["wide_map"].view(np.uint32).tolist(), "the empty leaf has no WNode slot"
    # a reference shared by two leaves: the first-equal-reference word of a duplicate names an earlier record
    first = T["soup"]["tri48"].view(np.uint32).reshape(-1, 12)[:-1, 10]
    assert (first != np.arange(len(first))).any(), "the soup has no duplicated references"
    # a one-leaf root: no wide copy at all
    assert len(scenes["lbvh1"]["nodes"]) == 1 and scenes["lbvh1"]["nodes"]["isLeaf"][0]
    assert len(T["lbvh1"]["wnode"]) == len(T["lbvh1"]["wide_map"]) == len(T["lbvh1"]["opened"]) == 0 and len(T["lbvh1"]["tripair"]) > 0
    assert (T["lbvh1"]["node_map"].view(np.uint32) == NONE).all()
    # without the wide copy: no pairs, no tie words
    assert all(len(tables(n, False)[k]) == 0 for n in ALL for k in ("tripair", "pair_ref", "wnode", "wide_map", "opened"))


def test_device_view_drops_the_pairs_without_a_wide_copy(tables):
    d = RT.device_view(tables("lbvh1"))
    assert len(d["tripair"]) == len(d["pair_ref"]) == 0 and len(d["tri48"]) == 2 * 48
    d = RT.device_view(tables("lbvh2"))
    assert len(d["tripair"]) == 2 * 80 and len(d["wnode"]) == 128


def test_table_diffs_names_the_table_the_count_and_the_first_record(tables):
    T = tables("soup")
    bad = {k: v.copy() for k, v in T.items()}
    bad["wnode"].view(np.uint32).reshape(-1, 32)[[3, 5], 7] ^= 1
    bad["tri48"] = bad["tri48"][:-48]
    lines = RT.table_diffs(bad, T)
    assert len(lines) == 2 and lines[0].startswith("tri48: ") and "bytes" in lines[0]
    assert lines[1].startswith("wnode: 2 of %d records differ, the first is record 3 (words [7])" % (len(T["wnode"]) // 128))
    nan_t = {k: v.copy() for k, v in T.items()}
    nan_t["wnode"].view(np.uint32)[:6] = 0x7FC00001          # another NaN: equal as a float to none, different bits
    assert RT.table_diffs(nan_t, nan_t) == [] and RT.table_diffs(nan_t, T)

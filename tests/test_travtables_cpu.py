"""CPU tests of the traversal-table builder (csrc/pt_travtables.cpp) through gmupt_debug_travtables_*: no device involved.

Byte identity: a SHA-256 of every table, every refit map and the scalar block, per scene and option set, against
tests/golden/travtables_digests.json.  The digests were recorded from the body of the former build_traversal_copy moved into the module
unchanged, before it was taken apart into steps; `python tests/test_travtables_cpu.py` rewrites the file from the library in the tree (a
deliberate change of a table only).

Invariants: what the ray-cast kernels and the k_rf_* kernels rely on, recomputed here from the reference-layout tree with numpy.
"""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "travtables_digests.json")
NONE = 0xFFFFFFFF                 # kRfNone, and a padding slot of pairRef
EMPTY_LINK = -0x80000000          # link of an empty WNode slot
TOP_TREE_NODES = 768              # GMUPT_TOP_NODES of the shipped build (pt_device.hpp)
DEF_STACK = 24                    # GMUPT_DEF_STACK (pt_traverse_deferred.hpp): a tree with maxDepth + 2 above it gets the deep top capacity
OPTION_SETS = {"default": {}, "bfs": {"top_order_bfs": True}, "unpaired": {"node_pairing": False}, "no_wide": {"want_wide": False}}
SCENES = ("cornell", "soup", "spheres_small", "deep_chain_mesh", "textured", "deep_chain_large")
DIGESTED = ("node64", "tri48", "tripair", "pair_ref", "wnode", "scalars", "level_nodes", "level_off", "node_map", "wide_map", "opened")
SCALARS = ("topCount", "topCountDeep", "maxDepth", "rootDesc", "rootMin0", "rootMin1", "rootMin2", "rootMax0", "rootMax1", "rootMax2",
           "triBase", "wideTopCount", "wideStackBound", "numPairs", "wideCount")
NODE64 = np.dtype([("box", "<f4", 12), ("d", "<i4", 4)])
WNODE = np.dtype([("p", "<f4", (6, 4)), ("link", "<i4", 4), ("aux", "<i4", 4)])


def make_scenes(pkg):
    S = pkg.scenes
    return {"cornell": S.build_scene(S.cornell_mesh()), "soup": S.build_scene(S.random_triangles_mesh(2000, seed=1)),
            "spheres_small": S.build_scene(S.spheres_mesh(n_spheres=12, subdiv=2, seed=7, floor_quads=4)),
            "deep_chain_mesh": S.build_scene(S.deep_chain_mesh()), "textured": S.build_scene(S.textured_mesh()),
            # the five scenes above hold no tree that is deep AND has more inner nodes than the plain top capacity: this one has
            "deep_chain_large": S.build_scene(S.deep_chain_mesh(n=2000, factor=0.97, per=4))}


def digests(raw):
    return {k: hashlib.sha256(raw[k].tobytes()).hexdigest() for k in DIGESTED}


class Tables:
    def __init__(self, pkg, scene, **opt):
        self.raw = raw = pkg.capi.travtables(scene["nodes"], scene["tris"], scene["verts"], **opt)
        self.nodes, self.R = scene["nodes"], len(scene["tris"])
        self.node64 = raw["node64"].view(NODE64)
        self.tri48 = raw["tri48"].view(np.uint32).reshape(-1, 12)
        self.pairs = raw["tripair"].view(np.uint32).reshape(-1, 20)
        self.wnode = raw["wnode"].view(WNODE)
        for k in ("pair_ref", "level_nodes", "level_off", "node_map", "wide_map", "opened"):
            setattr(self, k, raw[k].view(np.uint32))
        words = raw["scalars"].view(np.uint32)
        self.s = {n: int(w) for n, w in zip(SCALARS, words)}
        self.s["rootDesc"] = int(words[3:4].view(np.int32)[0])
        self.is_leaf = self.nodes["isLeaf"] != 0
        self.inner = np.flatnonzero(~self.is_leaf)


@pytest.fixture(scope="module")
def scenes6(pkg):
    return make_scenes(pkg)


@pytest.fixture(scope="module")
def built(pkg, scenes6):
    cache = {}

    def get(scene, optset="default"):
        if (scene, optset) not in cache:
            cache[scene, optset] = Tables(pkg, scenes6[scene], **OPTION_SETS[optset])
        return cache[scene, optset]
    return get


def child_ok(nodes, p, c):
    """rf_child_ok of pt_refit.hpp: False when c is flat on an axis on which p is not, in the plane of one of p's faces."""
    cmn, cmx, pmn, pmx = nodes["min"][c][:3], nodes["max"][c][:3], nodes["min"][p][:3], nodes["max"][p][:3]
    return not np.any((cmn == cmx) & (pmn != pmx) & ((cmn == pmn) | (cmx == pmx)))


def opens(nodes, p):
    return child_ok(nodes, p, nodes["left"][p]) and child_ok(nodes, p, nodes["right"][p])


# ------------------------------------------------------------------------------------------------ byte identity
@pytest.mark.parametrize("optset", sorted(OPTION_SETS))
@pytest.mark.parametrize("scene", SCENES)
def test_tables_match_the_recorded_digests(built, scene, optset):
    want = json.load(open(GOLDEN))[scene][optset]
    got = digests(built(scene, optset).raw)
    assert sorted(got) == sorted(want)
    assert {k: got[k] for k in got if got[k] != want[k]} == {}, "these tables changed their bytes"


def test_option_sets_change_what_they_should(built):
    """bfs and unpaired renumber Node64 (results do not depend on it); no_wide builds no pairs, no WNodes, no wide maps, no tie words."""
    for scene in ("soup", "deep_chain_large"):
        d = {o: digests(built(scene, o).raw) for o in OPTION_SETS}
        assert d["bfs"]["node_map"] != d["default"]["node_map"] and d["unpaired"]["node_map"] != d["default"]["node_map"]
        for o in ("bfs", "unpaired"):
            assert all(d[o][k] == d["default"][k] for k in ("tripair", "pair_ref", "wnode", "wide_map", "opened", "level_nodes", "level_off", "tri48"))
        t = built(scene, "no_wide")
        assert len(t.wnode) == len(t.pairs) == len(t.pair_ref) == len(t.wide_map) == len(t.opened) == 0
        assert t.s["numPairs"] == t.s["wideCount"] == t.s["wideTopCount"] == t.s["wideStackBound"] == 0
        assert not t.tri48[:, 10].any(), "word 10 of Tri48 stays zero when the wide copy is not wanted"
        assert d["no_wide"]["node64"] == d["default"]["node64"] and d["no_wide"]["level_nodes"] == d["default"]["level_nodes"]


def test_variants_build_makes_the_same_tables_and_the_unified_records(pkg, scenes6):
    scene = scenes6["soup"]
    want = digests(pkg.capi.travtables(scene["nodes"], scene["tris"], scene["verts"]))
    with pkg.capi.use_build("variants"):
        raw = pkg.capi.travtables(scene["nodes"], scene["tris"], scene["verts"])
    assert digests(raw) == want
    recs = raw["rec64"].view(np.uint32).reshape(-1, 16)
    n64, t48 = raw["node64"].view(np.uint32).reshape(-1, 16), raw["tri48"].view(np.uint32).reshape(-1, 12)
    assert len(recs) == len(n64) + len(t48) and np.array_equal(recs[:len(n64)], n64) and np.array_equal(recs[len(n64):, :12], t48)
    tri_words = np.ascontiguousarray(scene["tris"]).view(np.uint32).reshape(-1, 4)
    assert np.array_equal(recs[len(n64):-1, 12:], tri_words) and not recs[-1, 12:].any()


# ------------------------------------------------------------------------------------------------ the cases the scenes must hold
def test_the_scenes_exercise_every_case(built):
    ts = {s: built(s) for s in SCENES}
    assert any(t.s["maxDepth"] + 2 > DEF_STACK for t in ts.values()), "no tree deep enough for the deep top capacity"
    assert any(t.s["topCountDeep"] > t.s["topCount"] for t in ts.values()), "no deep tree that fills more than the plain top capacity"
    assert any(t.s["topCountDeep"] % 2 == 1 and (t.node_map == NONE).sum() == 1 and len(t.node_map) > t.s["topCountDeep"] for t in ts.values()), \
        "no odd top count with a filler record in front of the paired lines"
    sizes = lambda t: (t.nodes["right"] - t.nodes["left"])[t.is_leaf]
    assert any((sizes(t) % 2 == 1).any() for t in ts.values()), "no odd-sized leaf"
    assert any((t.wnode["aux"][:, 1] < 4).any() for t in ts.values()), "no WNode with an empty slot"
    assert any((t.tri48[:-1, 10] != np.arange(t.R)).any() for t in ts.values()), "no references duplicated by spatial splits"
    refused = 0
    for t in ts.values():
        for w in np.flatnonzero(t.wnode["aux"][:, 1] < 4):           # a wide node with room left ...
            for k in range(t.wnode["aux"][w, 1]):
                n = t.wide_map[4 * w + k]
                refused += (not t.is_leaf[n]) and not opens(t.nodes, n)   # ... and an inner slot it could not open
    assert refused, "no inner node that the flat-child rule refuses to open"


# ------------------------------------------------------------------------------------------------ invariants
WIDE_CASES = [(s, o) for s in SCENES for o in ("default", "bfs", "unpaired")]
ALL_CASES = WIDE_CASES + [(s, "no_wide") for s in SCENES]


def leaf_first_pair(t):
    """first pair of every leaf (an empty leaf has one all-zero pair), and the number of pairs"""
    size = np.where(t.is_leaf, t.nodes["right"] - t.nodes["left"], 0)
    npairs = np.where(t.is_leaf, np.maximum((size + 1) // 2, 1), 0)
    return np.cumsum(npairs) - npairs, int(npairs.sum())


@pytest.mark.parametrize("scene,optset", WIDE_CASES)
def test_every_reference_is_in_exactly_one_pair_slot(built, scene, optset):
    t = built(scene, optset)
    first, total = leaf_first_pair(t)
    assert len(t.pairs) == total == t.s["numPairs"] and len(t.pair_ref) == 2 * total
    refs = t.pair_ref[t.pair_ref != NONE]
    assert np.array_equal(np.sort(refs), np.arange(t.R)), "a reference is missing or in two slots"
    comp = [0, 1, 2, 3, 4, 5, 6, 7, 8]                                # v0.xyz, e1.xyz, e2.xyz: words 0..8 of Tri48
    for leaf in np.flatnonzero(t.is_leaf):
        a, b = int(t.nodes["left"][leaf]), int(t.nodes["right"][leaf])
        n = max((b - a + 1) // 2, 1)
        pr = t.pairs[first[leaf]:first[leaf] + n]
        want = list(range(a, b)) + [NONE] * (2 * n - (b - a))
        assert t.pair_ref[2 * first[leaf]:2 * (first[leaf] + n)].tolist() == want
        assert pr[:-1, 18].tolist() == [0] * (n - 1) and pr[-1, 18] == 1, "word 18: the last pair of the leaf, and only it"
        assert pr[:, 19].tolist() == [2] * (n - 1) + [b - a - 2 * (n - 1)], "word 19: references in the pair"
        for j in range(n):
            for slot in range(2):
                ref = want[2 * j + slot]
                assert np.array_equal(pr[j, slot:18:2], t.tri48[ref, comp] if ref != NONE else np.zeros(9, np.uint32))


@pytest.mark.parametrize("scene,optset", WIDE_CASES)
def test_wide_walk_reaches_every_leaf_once_and_slots_hold_their_nodes_boxes(built, scene, optset):
    t = built(scene, optset)
    W = len(t.wnode)
    assert W == t.s["wideCount"] and W > 0 and len(t.wide_map) == 4 * W
    first, _ = leaf_first_pair(t)
    depth = np.zeros(len(t.nodes), np.int64)
    for i in t.inner:
        depth[t.nodes["left"][i]] = depth[t.nodes["right"][i]] = depth[i] + 1
    seen_wide, seen_leaf, stack = [], [], [(0, 0)]
    while stack:
        w, grown_from = stack.pop()
        seen_wide.append(w)
        o = t.wnode[w]
        n = int(o["aux"][1])
        assert 2 <= n <= 4 and o["aux"][0] == depth[grown_from] and o["aux"][2] == o["aux"][3] == 0
        for k in range(4):
            node = int(t.wide_map[4 * w + k])
            if k >= n:
                assert node == NONE and o["link"][k] == EMPTY_LINK and np.isnan(o["p"][:, k]).all()
                assert (o["p"][:, k].view(np.uint32) == np.float32(np.nan).view(np.uint32)).all(), "an empty slot is the quiet NaN"
                continue
            rows = np.concatenate([t.nodes["min"][node][:3], t.nodes["max"][node][:3][::-1]])   # min x, y, z, max z, y, x
            assert np.array_equal(o["p"][:, k].view(np.uint32), rows.view(np.uint32)), (w, k)
            if t.is_leaf[node]:
                seen_leaf.append(node)
                assert o["link"][k] == ~int(first[node])
            else:
                assert 0 <= o["link"][k] < W
                stack.append((int(o["link"][k]), node))
    assert sorted(seen_wide) == list(range(W)), "a wide node is unreachable or reached twice"
    assert sorted(seen_leaf) == np.flatnonzero(t.is_leaf).tolist(), "a leaf is unreachable or reached twice"
    assert t.s["wideTopCount"] == min(W, t.s["wideTopCount"]) and t.s["wideTopCount"] > 0


@pytest.mark.parametrize("scene,optset", ALL_CASES)
def test_node_map_inverts_the_inner_numbering(built, scene, optset):
    t = built(scene, optset)
    nm = t.node_map
    assert len(nm) == len(t.node64) == t.s["triBase"]
    named = nm[nm != NONE]
    assert np.array_equal(np.sort(named), t.inner), "every inner node has exactly one packed record"
    assert (nm == NONE).sum() <= 1 and not t.raw["node64"].reshape(-1, 64)[nm == NONE].any(), "a filler record is all zero"
    index = np.full(len(t.nodes), -1, np.int64); index[named] = np.flatnonzero(nm != NONE)
    depth = np.zeros(len(t.nodes), np.int64)
    for i in t.inner:
        depth[t.nodes["left"][i]] = depth[t.nodes["right"][i]] = depth[i] + 1
    assert t.s["maxDepth"] == depth.max()

    def desc(c):
        if not t.is_leaf[c]:
            return index[c]
        return ~(int(t.nodes["left"][c]) if t.nodes["right"][c] > t.nodes["left"][c] else t.R)
    for i in t.inner:
        rec = t.node64[index[i]]
        l, r = t.nodes["left"][i], t.nodes["right"][i]
        box = np.concatenate([t.nodes["min"][l][:3], t.nodes["max"][l][:3], t.nodes["min"][r][:3], t.nodes["max"][r][:3]])
        assert np.array_equal(rec["box"].view(np.uint32), box.view(np.uint32))
        assert rec["d"].tolist() == [desc(l), desc(r), depth[i], 0]
    assert t.s["rootDesc"] == desc(0)
    assert t.s["topCount"] == min(t.s["topCountDeep"], TOP_TREE_NODES)
    assert (nm[:t.s["topCountDeep"]] != NONE).all(), "the LDS-resident top holds no filler"
    # the triangle records: last-of-leaf flags and the sentinel
    assert len(t.tri48) == t.R + 1
    last = np.zeros(t.R + 1, np.uint32); last[t.R] = 1
    nonempty = t.is_leaf & (t.nodes["right"] > t.nodes["left"])
    last[t.nodes["right"][nonempty] - 1] = 1
    assert np.array_equal(t.tri48[:, 9], last) and not t.tri48[t.R, :9].any() and not t.tri48[:, 11].any()


@pytest.mark.parametrize("scene,optset", ALL_CASES)
def test_level_nodes_come_after_their_children(built, scene, optset):
    t = built(scene, optset)
    assert np.array_equal(np.sort(t.level_nodes), t.inner)
    assert t.level_off[0] == 0 and np.all(np.diff(t.level_off.astype(np.int64)) >= 0) and t.level_off[-1] == len(t.level_nodes)
    pos = np.full(len(t.nodes), -1, np.int64); pos[t.level_nodes] = np.arange(len(t.level_nodes))
    level = np.searchsorted(t.level_off, pos, side="right")          # the launch (height) an entry belongs to
    for side in ("left", "right"):
        c = t.nodes[side][t.inner]
        assert np.all(t.is_leaf[c] | (pos[c] < pos[t.inner])), "a node listed before one of its children"
        assert np.all(t.is_leaf[c] | (level[c] < level[t.inner])), "a node in the launch of one of its children"


@pytest.mark.parametrize("scene,optset", WIDE_CASES)
def test_opened_nodes_pass_the_flat_child_rule(built, scene, optset):
    t = built(scene, optset)
    assert len(set(t.opened.tolist())) == len(t.opened) and not t.is_leaf[t.opened].any()
    assert all(opens(t.nodes, n) for n in t.opened)
    kept = set(t.wide_map[t.wide_map != NONE].tolist())
    assert not kept & set(t.opened.tolist()) and kept | set(t.opened.tolist()) | {0} == set(range(len(t.nodes))), \
        "every node but the root either keeps a slot or was opened"


@pytest.mark.parametrize("scene,optset", WIDE_CASES)
def test_wide_stack_bound_covers_an_exhaustive_walk(built, scene, optset):
    """Every slot hit on every level: the inner stack holds the inner slots not taken yet.  Two visiting orders."""
    t = built(scene, optset)
    for order in (1, -1):
        stack, deepest, visited = [0], 0, 0
        while stack:
            w = stack.pop()
            visited += 1
            links = [int(l) for l in t.wnode["link"][w][:t.wnode["aux"][w, 1]] if l >= 0][::order]
            stack.extend(links)
            deepest = max(deepest, len(stack) - 1 if links else len(stack))   # the walk keeps one of the pushed slots in hand
        assert visited == len(t.wnode)
        assert t.s["wideStackBound"] >= deepest, (order, deepest)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gmupt_pkg
    pkg_ = gmupt_pkg.load()
    out = {name: {o: digests(Tables(pkg_, sc, **kw).raw) for o, kw in OPTION_SETS.items()} for name, sc in make_scenes(pkg_).items()}
    json.dump(out, open(GOLDEN, "w"), indent=1, sort_keys=True)
    print("wrote", GOLDEN)

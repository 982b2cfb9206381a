"""Shared by the refit-table tests: the rule by which gmupt_renderer_refit rewrites a renderer's traversal tables, restated from the
text of include/gmupt.h (the refit section) and the layout comments of csrc/pt_device.hpp alone -- numpy float32 arithmetic, no call into
the library.  The expected tables after a refit are refit_tables(tables read after bind, refitted nodes, triangle records, moved
vertices): every word the rule does not name is copied from the bind-time tables, which is how the kept words get checked.

A fresh build of the tables from the refitted tree is NOT the expected value: the numbering and the collapse follow the surface areas of
the boxes, so WNode / Node64 of a fresh build differ ("Refit").
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF                 # a refit-map entry that names no node (filler Node64, empty WNode slot); a padding slot of pairRef
KINDS = ("node64", "tri48", "tripair", "pair_ref", "wnode", "rec64", "scalars", "level_nodes", "level_off", "node_map", "wide_map", "opened")
DEVICE_TABLES = ("node64", "tri48", "tripair", "pair_ref", "wnode", "rec64")
MAPS = ("level_nodes", "level_off", "node_map", "wide_map", "opened")
RECORD_BYTES = {"node64": 64, "tri48": 48, "tripair": 80, "pair_ref": 4, "wnode": 128, "rec64": 64, "scalars": 4, "level_nodes": 4,
                "level_off": 4, "node_map": 4, "wide_map": 4, "opened": 4}
SCALAR_ROOT_MIN, SCALAR_ROOT_MAX = slice(4, 7), slice(7, 10)   # of the 15 words: topCount, topCountDeep, maxDepth, rootDesc, rootMin[3], rootMax[3], ...


def _words(table, per_record):
    return np.ascontiguousarray(table).view(np.uint32).reshape(-1, per_record).copy()


def refit_tables(bind_tables, nodes_refitted, tris, verts_moved):
    """The tables a refit leaves: {kind: uint8 array} like capi.travtables / Renderer.read_travtables."""
    nodes = np.asarray(nodes_refitted)
    v = np.ascontiguousarray(verts_moved, F).reshape(-1, 3)
    t = np.asarray(tris)["v"]
    R = len(t)
    out = {k: np.ascontiguousarray(bind_tables[k]).copy() for k in KINDS}
    mn, mx = nodes["min"].astype(F), nodes["max"].astype(F)

    # Tri48: r0 = (v0.xyz, e1.x) r1 = (e1.yz, e2.xy) r2 = (e2.z, last flag, first equal reference, 0): nine floats written, three words
    # and the sentinel record R kept
    tri = _words(out["tri48"], 12)
    assert len(tri) == R + 1, "Tri48 holds one record per reference and the sentinel"
    if R:
        v0 = v[t[:, 0]]
        nine = np.concatenate([v0, v[t[:, 1]] - v0, v[t[:, 2]] - v0], axis=1)
        assert nine.dtype == F
        tri[:R, :9] = nine.view(np.uint32)
    out["tri48"] = tri.reshape(-1).view(np.uint8)

    have_wide = len(out["wnode"]) > 0                # without a wide copy the TriPair and WNode parts are skipped
    if have_wide:
        # TriPair: w[2c + k] = component c of the Tri48 of pairRef[2p + k], zeros in a padding slot; w[18], w[19] kept
        pairs = _words(out["tripair"], 20)
        ref = np.ascontiguousarray(out["pair_ref"]).view(np.uint32).reshape(-1, 2)
        assert len(ref) == len(pairs)
        for k in range(2):
            has = ref[:, k] != NONE
            comp = np.zeros((len(pairs), 9), np.uint32)
            comp[has] = tri[ref[has, k], :9]
            pairs[:, k:18:2] = comp
        out["tripair"] = pairs.reshape(-1).view(np.uint8)

    # Node64: a = (lmin.xyz, lmax.x) b = (lmax.yz, rmin.xy) c = (rmin.z, rmax.xyz), i.e. the twelve box floats of the two children of
    # nodeMap[q] in a row; d kept; a filler record (nodeMap[q] names no node) kept
    n64 = _words(out["node64"], 16)
    nmap = np.ascontiguousarray(out["node_map"]).view(np.uint32)
    assert len(nmap) == len(n64)
    q = np.flatnonzero(nmap != NONE)
    q = q[nodes["isLeaf"][nmap[q]] == 0]             # (a packed record exists for inner nodes only)
    l, r = nodes["left"][nmap[q]], nodes["right"][nmap[q]]
    n64[q, :12] = np.concatenate([mn[l], mx[l], mn[r], mx[r]], axis=1).view(np.uint32)
    out["node64"] = n64.reshape(-1).view(np.uint8)

    if have_wide:
        # WNode: p[0..5][slot] = min.x, min.y, min.z, max.z, max.y, max.x of wideMap[4 w + slot]; link and aux rows kept; an empty slot
        # (wideMap names no node) keeps its NaN bits
        wn = _words(out["wnode"], 32)
        wmap = np.ascontiguousarray(out["wide_map"]).view(np.uint32).reshape(-1, 4)
        assert len(wmap) == len(wn)
        w, k = np.nonzero(wmap != NONE)
        node = wmap[w, k]
        rows = np.concatenate([mn[node], mx[node][:, ::-1]], axis=1).view(np.uint32)      # min x, y, z, max z, y, x
        for row in range(6):
            wn[w, 4 * row + k] = rows[:, row]
        out["wnode"] = wn.reshape(-1).view(np.uint8)

    # rootMin / rootMax: the refitted root box; the other nine words kept
    s = np.ascontiguousarray(out["scalars"]).view(np.uint32).copy()
    assert len(s) == 15
    s[SCALAR_ROOT_MIN] = mn[0].view(np.uint32)
    s[SCALAR_ROOT_MAX] = mx[0].view(np.uint32)
    out["scalars"] = s.view(np.uint8)
    return out


def device_view(host_tables):
    """What a renderer holds after the bind upload of host-built tables: without a wide copy the pairs stay on the host."""
    out = {k: np.ascontiguousarray(host_tables[k]) for k in KINDS}
    if len(out["wnode"]) == 0:
        out["tripair"] = out["pair_ref"] = np.zeros(0, np.uint8)
    return out


def table_diffs(got, want, kinds=KINDS):
    """[] when every table of `kinds` is equal bit for bit, else one line per differing table: its name, the number of differing records and
    the first one's index.  All comparisons on uint32 words (a NaN must keep its bits)."""
    bad = []
    for k in kinds:
        g, w = np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)
        if g.nbytes != w.nbytes:
            bad.append("%s: %d bytes, expected %d" % (k, g.nbytes, w.nbytes))
            continue
        per = RECORD_BYTES[k] // 4
        rows = np.flatnonzero(np.any(g.view(np.uint32).reshape(-1, per) != w.view(np.uint32).reshape(-1, per), axis=1))
        if len(rows):
            first = int(rows[0])
            words = np.flatnonzero(g.view(np.uint32).reshape(-1, per)[first] != w.view(np.uint32).reshape(-1, per)[first]).tolist()
            bad.append("%s: %d of %d records differ, the first is record %d (words %r)" % (k, len(rows), g.nbytes // RECORD_BYTES[k], first, words))
    return bad


def assert_tables(got, want, what, kinds=KINDS):
    bad = table_diffs(got, want, kinds)
    assert not bad, "%s: %s" % (what, "; ".join(bad))


def assert_tight(tables, nodes):
    """Every occupied WNode slot and every Node64 child box EQUALS the mapped node's box (not merely contains it)."""
    nodes = np.asarray(nodes)
    mn, mx = nodes["min"].astype(F).view(np.uint32), nodes["max"].astype(F).view(np.uint32)
    n64 = _words(tables["node64"], 16)
    nmap = np.ascontiguousarray(tables["node_map"]).view(np.uint32)
    q = np.flatnonzero(nmap != NONE)
    for side, first in (("left", 0), ("right", 6)):
        c = nodes[side][nmap[q]]
        assert np.array_equal(n64[q, first:first + 3], mn[c]) and np.array_equal(n64[q, first + 3:first + 6], mx[c]), "a Node64 %s child box is not its node's" % side
    wn = _words(tables["wnode"], 32).reshape(-1, 8, 4)
    wmap = np.ascontiguousarray(tables["wide_map"]).view(np.uint32).reshape(-1, 4)
    w, k = np.nonzero(wmap != NONE)
    node = wmap[w, k]
    assert np.array_equal(wn[w, 0:3, k], mn[node]) and np.array_equal(wn[w, 3:6, k], mx[node][:, ::-1]), "a WNode slot is not its node's box"
    return len(q), len(w)


# ---- scenes the fixture scenes do not hold
def lbvh_scene(pkg, n, seed, L):
    """build_scene(LU.soup(n, seed), builder="lbvh", max_leaf_size=L); the render-side arrays the soup of lbvh_util lacks (normals,
    materials, lights, camera) come from the scenes module's own soup."""
    import lbvh_util as LU
    S = pkg.scenes
    mesh = dict(LU.soup(n, seed))
    side = S.random_triangles_mesh(1, seed=1)
    mesh["normals"] = S.vertex_normals(mesh["verts"], mesh["indices"])
    for k in ("materials", "lights", "light_count", "camera"):
        mesh[k] = side[k]
    mesh["name"] = "lbvh_soup%d" % n
    return S.build_scene(mesh, builder="lbvh", max_leaf_size=L)


def empty_leaf_scene(pkg):
    """A hand-made valid tree with an empty leaf (right == left), which no builder here produces, over six soup triangles:
         0 -> (1, 2)   1 -> (leaf [0, 2), leaf [2, 3))   2 -> (leaf [3, 3): EMPTY, leaf [3, 6))
    The empty leaf's box is a cube strictly inside the soup's (refit leaves it as it is); the other boxes are the refit rule's."""
    capi = pkg.capi
    scene = lbvh_scene(pkg, 6, 41, 1)
    nodes = np.zeros(7, capi.bvh_node_dtype)
    for i, (l, r, leaf) in enumerate([(1, 2, 0), (3, 4, 0), (5, 6, 0), (0, 2, 1), (2, 3, 1), (3, 3, 1), (3, 6, 1)]):
        nodes[i]["left"], nodes[i]["right"], nodes[i]["isLeaf"] = l, r, leaf
    centre = scene["verts"].mean(axis=0)
    nodes[5]["min"], nodes[5]["max"] = centre - F(0.25), centre + F(0.25)
    scene["nodes"] = capi.bvh_refit_host(nodes, scene["tris"], scene["verts"])
    scene["name"] = "empty_leaf"
    return scene

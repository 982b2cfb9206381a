"""Shared by the LBVH tests: an independent builder written from the rule in include/gmupt.h alone (numpy float32 arithmetic, np.lexsort,
a top-down split at the highest differing bit -- no Karras search, no code of the library), and the crafted meshes."""
import numpy as np

F = np.float32


def _lo(a, b):
    return np.where(b < a, b, a)


def _hi(a, b):
    return np.where(b > a, b, a)


def morton_keys(verts, indices):
    """Rules 1-4: the 63-bit keys as Python ints."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    t = np.asarray(indices).reshape(-1, 3)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    bmin, bmax = _lo(_lo(p0, p1), p2), _hi(_hi(p0, p1), p2)
    c = (bmin + bmax) * F(0.5)
    cmin, cmax = c.min(axis=0), c.max(axis=0)
    ext = cmax - cmin
    q = np.zeros(c.shape, np.uint64)
    for k in range(3):
        if ext[k] > 0:
            x = ((c[:, k] - cmin[k]) / ext[k]) * F(2097152.0)
            assert x.dtype == np.float32
            q[:, k] = np.minimum(np.uint64(2097151), x.astype(np.uint64))
    keys = []
    for qx, qy, qz in q.tolist():
        key = 0
        for b in range(21):
            key |= ((qx >> b) & 1) << (3 * b + 2) | ((qy >> b) & 1) << (3 * b + 1) | ((qz >> b) & 1) << (3 * b)
        keys.append(key)
    return keys


def build(verts, indices, vertex_material, L, node_dtype, tri_dtype):
    """The whole rule: (nodes, tris, ref_triangle, depth, leaves)."""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    t = np.asarray(indices, np.int32).reshape(-1, 3)
    n = len(t)
    keys = morton_keys(v, t)
    src = np.lexsort((np.arange(n), np.array(keys, dtype=np.uint64)))          # by key, then by index
    comb = [(keys[s] << 32) | p for p, s in enumerate(src.tolist())]            # (key, position): the equal-key rule of delta is its low word
    # rules 5-6, top-down: [first, last, depth, left child, right child]
    tree = [[0, n - 1, 0, None, None]]
    todo = [0]
    while todo:
        i = todo.pop()
        first, last, depth = tree[i][:3]
        if last - first + 1 <= L:
            continue
        bit = (comb[first] ^ comb[last]).bit_length() - 1
        s = max(p for p in range(first, last) if not (comb[p] >> bit) & 1)
        tree[i][3], tree[i][4] = len(tree), len(tree) + 1
        tree.append([first, s, depth + 1, None, None]); tree.append([s + 1, last, depth + 1, None, None])
        todo += [len(tree) - 2, len(tree) - 1]
    # rule 7
    order = sorted(range(len(tree)), key=lambda i: (tree[i][2], tree[i][0]))
    number = {i: k for k, i in enumerate(order)}
    # rule 8
    tris = np.zeros(n, tri_dtype)
    tris["v"] = t[src]
    if vertex_material is not None:
        tris["materialID"] = np.asarray(vertex_material, np.uint32)[t[src, 0]]
    nodes = np.zeros(len(tree), node_dtype)
    for k in reversed(range(len(order))):
        first, last, depth, l, r = tree[order[k]]
        if l is None:
            pts = v[tris["v"][first:last + 1].reshape(-1)]
            mn, mx = pts[0].copy(), pts[0].copy()
            for p in pts[1:]:
                mn, mx = _lo(mn, p), _hi(mx, p)
            nodes[k]["left"], nodes[k]["right"], nodes[k]["isLeaf"] = first, last + 1, 1
        else:
            a, b = nodes[number[l]], nodes[number[r]]
            assert number[r] == number[l] + 1 and number[l] > k
            mn, mx = _lo(a["min"], b["min"]), _hi(a["max"], b["max"])
            nodes[k]["left"], nodes[k]["right"], nodes[k]["isLeaf"] = number[l], number[l] + 1, 0
        nodes[k]["min"], nodes[k]["max"] = mn, mx
    depth = max(x[2] for x in tree)
    leaves = sum(1 for x in tree if x[3] is None)
    return nodes, tris, src.astype(np.int32), depth, leaves


def _mesh(verts, indices, seed=0):
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    t = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    return {"verts": v, "indices": t, "vertex_material": rng.integers(0, 3, len(v)).astype(np.uint32)}


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10, 10, (n, 1, 3))
    v = (c + rng.uniform(-1, 1, (n, 3, 3))).reshape(-1, 3)
    return _mesh(v, np.arange(3 * n).reshape(n, 3), seed)


def key_chain(copies, half=0.0):
    """A Morton key chain: the mesh that puts the tree on either side of rule 9's depth limit.  Triangle centres, in this order: `copies`
    at the origin (key 0), one per key bit j = 0..62 at 2^(j // 3) / 2^21 on axis 2 - j % 3 (key 1 << j), one at (1, 1, 1) (cmin = 0 and
    ext = 1 on every axis; the last cell, key all ones).  half == 0: every triangle is its centre three times; half > 0: the centre plus
    (-h, -h, -h), (h, -h, h), (-h, h, h), whose box centre is the centre again -- exactly, for half in {2^-23, 0.125, 0.25}.  Every inner
    node of the chain has one leaf and one inner child: the highest differing bit takes every position 62..0, then the copies continue
    the chain through the position tie-break.  KEY_CHAIN_DEPTH has the depths."""
    c = np.zeros((copies + 64, 3), F)
    for j in range(63):
        c[copies + j, 2 - j % 3] = F(2.0 ** (j // 3 - 21))
    c[copies + 63] = 1.0
    h = F(half)
    corners = np.array([[-h, -h, -h], [h, -h, h], [-h, h, h]], F)
    v = c[:, None, :] + corners[None, :, :]
    assert v.dtype == np.float32
    return _mesh(v.reshape(-1, 3), np.arange(3 * len(c)).reshape(len(c), 3), copies)


# copies -> the depth of key_chain(copies, half)'s tree for L = 1, 2, 4, whatever half is: by the rule, the chain of 63 key bits below the
# root's split, shortened by the leaf size at its lower end and extended by ceil(log2) levels of the position tie-break among the copies
KEY_CHAIN_DEPTH = {1: (63, 62, 60), 2: (64, 63, 61), 3: (65, 64, 62), 4: (65, 64, 63), 5: (66, 65, 64), 8: (66, 65, 64), 9: (67, 66, 65),
                   300: (72, 71, 70)}
KEY_CHAIN_LEAF_SIZES = (1, 2, 4)
KEY_CHAIN_HALVES = (0.0, 0.125)
MAX_DEPTH = 64                                      # rule 9
KEY_CHAIN_MIN_STACK = 40                            # what the oracle's walk of key_chain(2, 0.125), L = 1 must at least stack (it measured 46)


def key_chain_cases(accepted):
    """(copies, L, depth) of every cell of KEY_CHAIN_DEPTH on one side of the limit."""
    return [(c, L, d) for c, row in KEY_CHAIN_DEPTH.items() for L, d in zip(KEY_CHAIN_LEAF_SIZES, row) if (d <= MAX_DEPTH) == accepted]


def key_chain_render_mesh(scenes, copies, half):
    return render_mesh(scenes, key_chain(copies, half), "key_chain%d" % copies)


def render_mesh(scenes, mesh, name):
    """A mesh of this file as one scenes.build_scene takes: face normals, the materials and lights of the library's triangle soup, a
    camera that looks at the key chain's corner from z = 2."""
    m = dict(mesh)
    n = len(m["indices"])
    soup_ = scenes.random_triangles_mesh(n, seed=1)
    v, t = m["verts"], m["indices"]
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    m.update({"normals": np.repeat(fn, 3, axis=0).astype(F), "vertex_material": soup_["vertex_material"], "materials": soup_["materials"],
              "lights": soup_["lights"], "light_count": soup_["light_count"], "camera": (0.3, 0.3, 2.0, 0.0, 270.0),
              "name": name})
    return m


def key_chain_rays(n=4096, seed=0):
    """(n, 8) closest-hit rays (origin, tmax = FLT_MAX, direction, pad) from around the key chain towards its corner at the origin, where
    the deep end of the tree lies: most of them hit, and those walk the chain to its bottom."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.3, 0.8, (n, 3)).astype(F)
    target = rng.uniform(-0.1, 0.1, (n, 3)).astype(F)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = o; rays[:, 3] = np.finfo(F).max; rays[:, 4:7] = target - o
    return rays


def crafted_meshes(L=4):
    """name -> mesh(verts, indices, vertex_material): the edge cases of the rule."""
    out = {}
    for n in sorted({1, 2, 3, L, L + 1}):
        out["soup%d" % n] = soup(n, 100 + n)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    out["copies37"] = _mesh(tri, np.tile([0, 1, 2], (37, 1)), 1)                # one key: the index decides, 37 is no power of two
    rng = np.random.default_rng(2)
    v = rng.uniform(-3, 3, (60, 3, 3)); v[:, :, 1] = 2.5                         # every centre in the plane y = 2.5: ext.y = 0
    out["plane"] = _mesh(v.reshape(-1, 3), np.arange(180).reshape(60, 3), 2)
    v = rng.uniform(-2, 2, (24, 3, 3)).astype(F)
    v[:8, :, 0] = F(-0.0); v[8:16, :, 0] = F(0.0)                                # centres with x = -0.0 and x = +0.0, the rest on either side
    v[:4, :, 2] = F(-0.0)
    out["signed_zero"] = _mesh(v.reshape(-1, 3), np.arange(72).reshape(24, 3), 3)
    gx, gy = np.meshgrid(np.arange(17, dtype=F), np.arange(17, dtype=F))
    gv = np.stack([gx.ravel() * F(1e-6), gy.ravel() * F(1e-6), np.zeros(289, F)], axis=1)
    gv = np.concatenate([gv, [[100.0, 100.0, 0.0], [101.0, 100.0, 0.0], [100.0, 101.0, 0.0]]])   # one far triangle: the grid shares coarse cells
    quads = [(y * 17 + x, y * 17 + x + 1, (y + 1) * 17 + x, (y + 1) * 17 + x + 1) for y in range(16) for x in range(16)]
    gi = [[a, b, c] for a, b, c, d in quads] + [[b, d, c] for a, b, c, d in quads] + [[289, 290, 291]]
    out["grid16"] = _mesh(gv, gi, 4)
    return out

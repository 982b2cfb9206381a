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

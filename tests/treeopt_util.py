"""The treelet optimiser of include/gmupt.h ("Tree optimisation") restated in numpy / Python, written from the header alone: a post-order
recursion (a schedule neither the host reference nor the kernels use), the programme of a treelet size by size with the partitions of
a size as one table, the rewrite as a recursion in pre-order.  And the inputs the optimiser tests share."""
import functools

import numpy as np

import lbvh_util as LU

F = np.float32
INVALID, UNSUPPORTED = -1, -5
MAX_DEPTH = 64
PASSES = (1, 2, 3)
LEAF_SIZES = (1, 4)


class Refused(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _lo(a, b):
    return np.where(b < a, b, a)


def _hi(a, b):
    return np.where(b > a, b, a)


def half_area(mn, mx):
    d = [float(mx[k]) - float(mn[k]) for k in range(3)]
    ex, ey, ez = [x if x > 0 else 0.0 for x in d]
    return (ex * ey + ey * ez) + ez * ex


@functools.lru_cache(maxsize=None)
def _tables(k):
    """For k slots: the membership matrix of the subsets, and per subset size m >= 2 the subsets of that size with, row by row, their
    partitions p in increasing numeric value (every subset of a size has the same number of them)."""
    member = np.array([[(s >> j) & 1 for j in range(k)] for s in range(1 << k)], bool)
    by_size = []
    for m in range(2, k + 1):
        subsets = [s for s in range(1, 1 << k) if bin(s).count("1") == m]
        rows = []
        for s in subsets:
            low = s & -s
            rows.append([p for p in range(1, s) if p & s == p and p & low])
        by_size.append((np.array(subsets), np.array(rows)))
    return member, by_size


class _Tree:
    def __init__(self, nodes):
        self.n = len(nodes)
        self.left = nodes["left"].astype(np.int64).tolist()
        self.right = nodes["right"].astype(np.int64).tolist()
        self.leaf = (nodes["isLeaf"] != 0).tolist()
        self.mn = nodes["min"].astype(F).copy()
        self.mx = nodes["max"].astype(F).copy()
        self.rec = nodes.copy()
        self.cost = [0.0] * self.n
        self.rewritten = 0

    def depths(self):
        depth = [0] * self.n
        todo = [0]
        while todo:
            i = todo.pop()
            if not self.leaf[i]:
                for c in (self.left[i], self.right[i]):
                    depth[c] = depth[i] + 1
                    todo.append(c)
        return depth

    def area(self, i):
        return half_area(self.mn[i], self.mx[i])

    def refresh(self, x):
        l, r = self.left[x], self.right[x]
        self.mn[x], self.mx[x] = _lo(self.mn[l], self.mn[r]), _hi(self.mx[l], self.mx[r])
        self.cost[x] = self.area(x) * 2.0 + (self.cost[l] + self.cost[r])

    def process(self, x):
        """Step 1-4 of the rule for x, after everything below it."""
        if self.leaf[x]:
            self.cost[x] = self.area(x) * float((self.right[x] - self.left[x]) & 0xFFFFFFFF)
            return
        self.process(self.left[x])
        self.process(self.right[x])
        slots, inner = [self.left[x], self.right[x]], []
        while len(slots) < 7:
            best = None
            for j, node in enumerate(slots):
                if self.leaf[node]:
                    continue
                a = self.area(node)
                if best is None or a > best[0] or (a == best[0] and node < best[1]):
                    best = (a, node, j)
            if best is None:
                break
            _, node, j = best
            inner.append(node)
            slots[j] = self.left[node]
            slots.append(self.right[node])
        self.refresh(x)
        k = len(slots)
        if k < 3:
            return
        member, by_size = _tables(k)
        smn, smx = self.mn[slots], self.mx[slots]                      # (k, 3); min / max by value: no NaN in the tests' boxes
        with np.errstate(invalid="ignore"):
            bmn = np.where(member[:, :, None], smn[None], np.inf).min(axis=1).astype(np.float64)
            bmx = np.where(member[:, :, None], smx[None], -np.inf).max(axis=1).astype(np.float64)
            e = bmx - bmn
        e = np.where(e > 0, e, 0.0)
        a = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]
        c = np.zeros(1 << k)
        part = np.zeros(1 << k, np.int64)
        for j, node in enumerate(slots):
            c[1 << j] = self.cost[node]
        for subsets, rows in by_size:
            v = c[rows] + c[subsets[:, None] ^ rows]
            pick = v.argmin(axis=1)                                    # the first of equal minima: "strictly smaller" in increasing p
            c[subsets] = a[subsets] * 2.0 + v[np.arange(len(subsets)), pick]
            part[subsets] = rows[np.arange(len(subsets)), pick]
        full = (1 << k) - 1
        if not c[full] < self.cost[x]:
            return
        self.rewritten += 1
        spare = iter(sorted(inner))

        def build(s, node):
            for side, sub in ((self.left, int(part[s])), (self.right, s ^ int(part[s]))):
                if sub & (sub - 1):
                    child = next(spare)
                    side[node] = child
                    build(sub, child)
                else:
                    side[node] = slots[sub.bit_length() - 1]
            l, r = self.left[node], self.right[node]
            self.mn[node], self.mx[node] = _lo(self.mn[l], self.mn[r]), _hi(self.mx[l], self.mx[r])
            self.cost[node] = float(c[s])

        build(full, x)

    def numbered(self):
        depth = self.depths()
        order = sorted(range(self.n), key=lambda i: (depth[i], i))
        number = {i: p for p, i in enumerate(order)}
        out = np.zeros(self.n, self.rec.dtype)
        for p, i in enumerate(order):
            if self.leaf[i]:
                out[p] = self.rec[i]
            else:
                out[p]["min"], out[p]["max"] = self.mn[i], self.mx[i]
                out[p]["left"], out[p]["right"], out[p]["isLeaf"] = number[self.left[i]], number[self.right[i]], 0
        return out, max(depth)


def post_order_cost(nodes):
    """C(root) of a record array by the header's two cost lines and the boxes as stored."""
    def cost(i):
        n = nodes[i]
        a = half_area(n["min"], n["max"])
        if n["isLeaf"]:
            return a * float((int(n["right"]) - int(n["left"])) & 0xFFFFFFFF)
        return a * 2.0 + (cost(int(n["left"])) + cost(int(n["right"])))
    return cost(0)


def optimize(nodes, passes):
    """{p: (nodes, info) or Refused} for p = 1 .. passes, in one sweep; raises Refused for what the input itself is refused for."""
    nodes = np.asarray(nodes)
    n = len(nodes)
    refs = [0] * n
    for i in range(n):
        if nodes[i]["isLeaf"]:
            continue
        for c in (int(nodes[i]["left"]), int(nodes[i]["right"])):
            if not i < c < n:
                raise Refused(INVALID, "link")
            refs[c] += 1
    if any(refs[i] != (1 if i else 0) for i in range(n)):
        raise Refused(INVALID, "not a tree")
    t = _Tree(nodes)
    depth_before = max(t.depths())
    if depth_before > MAX_DEPTH:
        raise Refused(UNSUPPORTED, "depth %d" % depth_before)
    out = {}
    cost_before = None
    for p in range(1, passes + 1):
        if p == 1:                                                     # C(root) by step 2 alone: the same recursion with no rewrite
            cost_before = _plain_cost(_Tree(nodes), 0)
        t.process(0)
        res, depth = t.numbered()
        if depth > MAX_DEPTH:
            for q in range(p, passes + 1):
                out[q] = Refused(UNSUPPORTED, "depth %d after pass %d" % (depth, p))
            break
        out[p] = (res, {"num_nodes": n, "depth_before": depth_before, "depth_after": depth, "treelets_rewritten": t.rewritten,
                        "cost_before": cost_before, "cost_after": t.cost[0]})
    return out


def _plain_cost(t, x):
    if t.leaf[x]:
        return t.area(x) * float((t.right[x] - t.left[x]) & 0xFFFFFFFF)
    cl, cr = _plain_cost(t, t.left[x]), _plain_cost(t, t.right[x])
    l, r = t.left[x], t.right[x]
    t.mn[x], t.mx[x] = _lo(t.mn[l], t.mn[r]), _hi(t.mx[l], t.mx[r])
    return t.area(x) * 2.0 + (cl + cr)


def bits(x):
    return np.float64(x).view(np.uint64)


def info_differs(got, want):
    """The fields (ms aside) in which two info dicts differ: integers by value, the costs by bit pattern."""
    ints = ("num_nodes", "depth_before", "depth_after", "treelets_rewritten")
    return [k for k in ints if got[k] != want[k]] + [k for k in ("cost_before", "cost_after") if bits(got[k]) != bits(want[k])]


# ---- inputs
def crafted_meshes():
    """name -> mesh: 1, 2, 3, 7 and 8 triangles, 37 copies of one triangle, centres in one plane."""
    out = {"soup%d" % n: LU.soup(n, 100 + n) for n in (1, 2, 3, 7, 8)}
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    out["copies37"] = LU._mesh(np.tile(tri, (37, 1)), np.arange(111).reshape(37, 3), 1)       # every area equal: every tie-break is taken
    out["plane"] = LU.crafted_meshes(4)["plane"]
    return out


def library_meshes(scenes):
    return {"cornell": scenes.cornell_mesh(), "soup2000": scenes.random_triangles_mesh(2000), "chain": scenes.deep_chain_mesh(),
            "textured": scenes.textured_mesh()}


def input_scenes(scenes, capi):
    """(name, L) -> scene dict (nodes, tris, verts, ...; what build_scene returns) of every input tree of the tests: LBVHs of the crafted
    and the library meshes at L = 1 and 4, the accepted key_chain cells, and a host SBVH of the Cornell box whose boxes were refitted (so
    that its leaves follow the refit rule; its spatial splits make duplicate references)."""
    out = {}
    for name, mesh in crafted_meshes().items():
        for L in LEAF_SIZES:
            out[(name, L)] = scenes.build_scene(LU.render_mesh(scenes, mesh, name), builder="lbvh", max_leaf_size=L)
    for name, mesh in library_meshes(scenes).items():
        for L in LEAF_SIZES:
            out[(name, L)] = scenes.build_scene(mesh, builder="lbvh", max_leaf_size=L)
    for copies, L, depth in LU.key_chain_cases(accepted=True):
        if L in LEAF_SIZES:
            out[("key_chain%d" % copies, L)] = scenes.build_scene(LU.key_chain_render_mesh(scenes, copies, 0.125), builder="lbvh", max_leaf_size=L)
    sbvh = scenes.build_scene(scenes.cornell_mesh())
    out[("cornell_sbvh", 0)] = dict(sbvh, nodes=capi.bvh_refit_host(sbvh["nodes"], sbvh["tris"], sbvh["verts"]))
    return out


def chain_nodes(levels, node_dtype):
    """A hand-made chain `levels` deep: inner node 2i has the leaf 2i + 1 and the inner node 2i + 2; 2 * levels + 1 records."""
    n = 2 * levels + 1
    nodes = np.zeros(n, node_dtype)
    for i in range(n):
        nodes[i]["min"], nodes[i]["max"] = (0, 0, 0), (1 + i, 1, 1)
    for d in range(levels):
        nodes[2 * d]["left"], nodes[2 * d]["right"] = 2 * d + 1, 2 * d + 2
        nodes[2 * d + 1]["left"], nodes[2 * d + 1]["right"], nodes[2 * d + 1]["isLeaf"] = d, d + 1, 1
    nodes[n - 1]["left"], nodes[n - 1]["right"], nodes[n - 1]["isLeaf"] = levels, levels + 1, 1
    return nodes

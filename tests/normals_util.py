"""Shared by the tests of the smooth vertex normals (gmupt_vertex_normals_host, gmupt_normals_*): an independent numpy restatement of the
rule of include/gmupt.h ("normals"), binary32 throughout, and the meshes the tests run it on.

Elementwise float32 products, differences and sums, np.sqrt on float32 and a float32 division are exactly the rule's operations (each
rounds once to binary32; numpy never contracts).  The ordered sum is a loop over valence rank: step r adds, for every vertex that has
one, the face vector of its r-th corner in ascending (or, for the control, descending) corner number."""
import numpy as np


def rule(verts, indices, descending=False):
    """The normals of the rule as a (V, 3) float32 array.  descending=True sums every vertex's corners in descending corner number: not
    the rule -- the control that shows a fixture can tell the orders apart."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(indices, np.int64).reshape(-1, 3)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        e1, e2 = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        f = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        assert f.dtype == np.float32
        cv = t.reshape(-1)                                   # vertex of corner c
        corner = np.arange(len(cv))
        order = np.lexsort((-corner if descending else corner, cv))   # by vertex, then by corner number
        start = np.searchsorted(cv[order], np.arange(len(v)))
        rank = np.arange(len(cv)) - start[cv[order]]
        s = np.zeros((len(v), 3), np.float32)
        for r in range(int(rank.max()) + 1 if len(rank) else 0):
            c = order[rank == r]                             # at most one corner per vertex
            s[cv[c]] = s[cv[c]] + f[c // 3]
        l = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        assert l.dtype == np.float32
        ok = (l > 0) & np.isfinite(l)
        n = s * (one / l)[:, None]
    n[~ok] = (0.0, 1.0, 0.0)
    return n.astype(np.float32)


FALLBACK = np.array([0.0, 1.0, 0.0], np.float32)


def fixtures(S):
    """name -> (verts, indices) of the three generated meshes, each at wobble phase 0 and 0.3.  S: the package's scenes module."""
    out = {}
    for name, mesh in (("spheres3", S.spheres_mesh(n_spheres=3, subdiv=2, floor_quads=2)), ("cornell", S.cornell_mesh()),
                       ("soup200", S.random_triangles_mesh(200, seed=3))):
        for phase in (0, 0.3):
            out["%s@%s" % (name, phase)] = (S.wobble(mesh, phase), np.ascontiguousarray(mesh["indices"], np.int32))
    return out


def strip(nv, seed=0):
    """A zigzag triangle strip of nv vertices and nv - 2 triangles with some relief, so that no two normals agree."""
    rng = np.random.default_rng(100 + seed + nv)
    i = np.arange(nv)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.3 * np.sin(0.7 * i)], axis=1) + rng.uniform(-0.1, 0.1, (nv, 3))
    t = np.stack([i[:-2], i[1:-1], i[2:]], axis=1)
    t[1::2] = t[1::2][:, [1, 0, 2]]                          # one winding
    return v.astype(np.float32), t.astype(np.int32)


def hand_made():
    """name -> (verts, indices, fallback) -- fallback: the vertices that must get exactly (0, 1, 0); every other vertex must not."""
    out = {}
    out["one_triangle"] = (np.array([[0, 0, 0], [1, 0.5, 0], [0.25, 0, -1]], np.float32), np.array([[0, 1, 2]], np.int32), [])
    for nv in (255, 256, 257, 258, 259):                      # vertex counts 255..257 and triangle counts 255..257 around the block size
        v, t = strip(nv)
        out["strip%d" % nv] = (v, t, [])
    v, t = strip(40)
    out["unused_vertex"] = (np.concatenate([v, np.array([[3.0, 4.0, 5.0]], np.float32)]), t, [40])
    # a zero-area triangle on two vertices of its own, and one that shares a strip vertex (which then ignores it)
    v, t = strip(30)
    v = np.concatenate([v, np.array([[9, 9, 9], [9, 9, 9]], np.float32)])
    t = np.concatenate([t, np.array([[30, 31, 30], [5, 30, 31]], np.int32)])
    out["zero_area"] = (v, t, [30, 31])
    # two coincident faces of opposite winding: each vertex sums f and -f
    out["opposite_faces"] = (np.array([[0, 0, 0], [1, 0.25, 0], [0.5, 1, 0.75]], np.float32), np.array([[0, 1, 2], [0, 2, 1]], np.int32), [0, 1, 2])
    # a fan of valence 1000
    k = np.arange(1000)
    ring = np.stack([np.cos(2 * np.pi * k / 1000), 0.05 * np.sin(9 * 2 * np.pi * k / 1000), np.sin(2 * np.pi * k / 1000)], axis=1)
    v = np.concatenate([np.array([[0.0, 0.4, 0.0]]), ring]).astype(np.float32)
    t = np.stack([np.zeros(1000, np.int64), 1 + (k + 1) % 1000, 1 + k], axis=1).astype(np.int32)
    out["fan1000"] = (v, t, [])
    v, t = strip(50)
    out["repeated_triangle"] = (v, np.concatenate([t[:20], t[7:8], t[20:], t[7:8]]), [])
    # one NaN and one +inf vertex: exactly the vertices of their fans fall back
    v, t = strip(60)
    v[17, 1] = np.nan
    v[41, 0] = np.inf
    bad = sorted(set(t[np.any((t == 17) | (t == 41), axis=1)].reshape(-1).tolist()))
    out["nan_inf"] = (v, t, bad)
    return out


def all_meshes(S):
    out = dict(fixtures(S))
    out.update({k: (v, t) for k, (v, t, _) in hand_made().items()})
    return out

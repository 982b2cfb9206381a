"""CPU tests of the refit's host statement (gmupt_bvh_refit_host) and of the scene helpers around it (scenes.wobble, scenes.refit_scene,
scenes.vertex_normals).

Truth for the boxes is an independent numpy recomputation of the rule in include/gmupt.h: the box of the whole triangles of a leaf's
references (minimum / maximum.reduceat over the references' vertices), inner nodes by a sweep over falling indices.  Minimum and maximum
of finite floats do not depend on the folding order apart from the sign of a zero, so the comparison is by value (==).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

PHASES = (0, 0.3, 0.71)


def numpy_refit(nodes, tris, verts):
    out = nodes.copy()
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    leaf = (nodes["isLeaf"] != 0) & (nodes["right"] > nodes["left"])
    idx = np.flatnonzero(leaf)
    if len(idx):
        # reduceat over each leaf's own range [left, right) of the reference array: ranges listed as (start, end) pairs, every second
        # result (the one from `end` to the next start) dropped
        pv = verts[tris["v"]]                                    # (R, 3 vertices, 3 components)
        rmin = np.concatenate([pv.min(axis=1), np.zeros((1, 3), np.float32)])
        rmax = np.concatenate([pv.max(axis=1), np.zeros((1, 3), np.float32)])
        order = np.argsort(nodes["left"][idx], kind="stable")
        idx = idx[order]
        bounds = np.stack([nodes["left"][idx], nodes["right"][idx]], axis=1).reshape(-1).astype(np.int64)
        out["min"][idx] = np.minimum.reduceat(rmin, bounds, axis=0)[0::2]
        out["max"][idx] = np.maximum.reduceat(rmax, bounds, axis=0)[0::2]
    for i in range(len(nodes) - 1, -1, -1):
        if not nodes["isLeaf"][i]:
            l, r = nodes["left"][i], nodes["right"][i]
            out["min"][i] = np.minimum(out["min"][l], out["min"][r])
            out["max"][i] = np.maximum(out["max"][l], out["max"][r])
    return out


@pytest.fixture(scope="module")
def scenes5(pkg, cornell_scene, soup_scene, spheres_small_scene):
    S = pkg.scenes
    return {"cornell": cornell_scene, "soup": soup_scene, "spheres": spheres_small_scene,
            "chain": S.build_scene(S.deep_chain_mesh()), "textured": S.build_scene(S.textured_mesh())}


@pytest.mark.parametrize("name", ["cornell", "soup", "spheres", "chain", "textured"])
def test_host_refit_equals_numpy_recomputation(pkg, scenes5, name):
    scene = scenes5[name]
    for phase in PHASES:
        w = pkg.scenes.wobble(scene, phase, 0.05)
        if phase == 0:
            assert np.array_equal(w.view(np.uint32), scene["verts"].view(np.uint32)), "phase 0 must be the identity"
        else:
            assert not np.array_equal(w, scene["verts"])
        got = pkg.capi.bvh_refit_host(scene["nodes"], scene["tris"], w)
        want = numpy_refit(scene["nodes"], scene["tris"], w)
        assert np.array_equal(got["min"], want["min"]) and np.array_equal(got["max"], want["max"]), (name, phase)
        # every child inside its parent, min <= max everywhere
        assert np.all(got["min"] <= got["max"])
        inner = np.flatnonzero(got["isLeaf"] == 0)
        for side in ("left", "right"):
            c = got[side][inner]
            assert np.all(got["min"][c] >= got["min"][inner]) and np.all(got["max"][c] <= got["max"][inner]), (name, phase, side)


@pytest.mark.parametrize("name", ["cornell", "soup", "spheres", "chain", "textured"])
def test_identity_refit_contains_the_builders_boxes_and_keeps_the_topology(pkg, scenes5, name):
    scene = scenes5[name]
    nodes = scene["nodes"].copy()
    nodes["pad0"] = 1.25; nodes["pad1"] = -7.0; nodes["pad2"] = 3.5          # the pad words are the caller's
    got = pkg.capi.bvh_refit_host(nodes, scene["tris"], scene["verts"])
    nonempty = (nodes["isLeaf"] == 0) | (nodes["right"] > nodes["left"])
    assert np.all(got["min"][nonempty] <= nodes["min"][nonempty]) and np.all(got["max"][nonempty] >= nodes["max"][nonempty]), \
        "the builder's boxes are clipped, never larger than the whole triangles'"
    empty = ~nonempty
    assert np.array_equal(got["min"][empty].view(np.uint32), nodes["min"][empty].view(np.uint32))
    assert np.array_equal(got["max"][empty].view(np.uint32), nodes["max"][empty].view(np.uint32))
    for f in ("left", "right", "isLeaf", "pad0", "pad1", "pad2"):
        assert np.array_equal(got[f].view(np.uint32), nodes[f].view(np.uint32)), f
    again = pkg.capi.bvh_refit_host(got, scene["tris"], scene["verts"])
    assert got.tobytes() == again.tobytes(), "a second refit must change no byte"
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    ref = pkg.capi.bvh_refit_host(nodes, scene["tris"], w, threads=1)
    for threads in (0, 2, 5, 16, 64):
        assert pkg.capi.bvh_refit_host(nodes, scene["tris"], w, threads=threads).tobytes() == ref.tobytes(), threads


def test_soup_has_split_references_whose_boxes_grow(pkg, soup_scene):
    """The price of refitting an SBVH: some leaf of a scene with spatial splits gets a strictly looser box than the builder's."""
    got = pkg.capi.bvh_refit_host(soup_scene["nodes"], soup_scene["tris"], soup_scene["verts"])
    assert len(soup_scene["tris"]) > soup_scene["num_triangles"], "the soup fixture has no duplicated references"
    assert np.any(got["min"] < soup_scene["nodes"]["min"]) or np.any(got["max"] > soup_scene["nodes"]["max"])


def test_oracle_renders_the_refitted_scene_and_the_fixture_moves(pkg, oracle, cornell_scene, soup_scene):
    for scene in (cornell_scene, soup_scene):
        w = pkg.scenes.wobble(scene, 0.3, 0.05)
        moved = pkg.scenes.refit_scene(scene, w, pkg.scenes.vertex_normals(w, scene["tris"]["v"]) if scene is soup_scene else None)
        assert moved["nodes"].tobytes() == pkg.capi.bvh_refit_host(scene["nodes"], scene["tris"], w).tobytes()
        assert scene["verts"] is not moved["verts"] and not np.array_equal(scene["verts"], moved["verts"])
        frames = []
        for s in (scene, moved):
            orc = O.Renderer(s, 48, 27, 2048, threads=8)
            cam = O.Camera(48, 27); cam.set_pose(*s["camera"]); cam.buffer.lightCount = s["light_count"]
            for _ in range(24):
                cam.update(); orc.set_camera(cam.buffer); orc.iterate()
            assert 0 < orc.stats().maxStack <= 64, "the walk of the refitted tree must stay inside the 64-entry traversal stack"
            frames.append(orc.framebuffer().copy())
            orc.close()
        assert frames[1][..., 3].view(np.uint32).sum() > 0
        assert not np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32)), "the wobble moves nothing visible"


def test_vertex_normals_are_area_weighted_unit_vectors(pkg):
    mesh = pkg.scenes.spheres_mesh(n_spheres=1, subdiv=2, seed=3, floor_quads=1)
    v, t = pkg.scenes.icosphere(2)
    n = pkg.scenes.vertex_normals(v, t)
    assert n.dtype == np.float32 and n.shape == v.shape
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    assert np.all(np.sum(n * v, axis=1) > 0.99), "the smooth normals of a sphere about the origin point along the radius"
    # a large and a small triangle at one vertex: the large one's normal dominates by its area
    verts = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tri = np.array([[0, 1, 2], [0, 3, 4]], np.int32)
    n = pkg.scenes.vertex_normals(verts, tri)
    want = np.array([1.0, 0.0, 100.0]); want /= np.linalg.norm(want)
    assert np.allclose(n[0], want, atol=1e-6)
    assert mesh["verts"].shape[0] > 0


def test_argument_errors_leave_the_nodes_untouched(pkg, cornell_scene):
    capi = pkg.capi
    lib = capi.lib()
    nodes0 = cornell_scene["nodes"]
    tris0 = np.ascontiguousarray(cornell_scene["tris"])
    verts0 = np.ascontiguousarray(cornell_scene["verts"])
    moved = pkg.scenes.wobble(cornell_scene, 0.3, 0.05)

    def call(nodes, tris, verts, n=None, r=None, v=None):
        return lib.gmupt_bvh_refit_host(capi._ptr(nodes) if nodes is not None else None, len(nodes0) if n is None else n,
                                        capi._ptr(tris) if tris is not None else None, len(tris0) if r is None else r,
                                        capi._ptr(verts) if verts is not None else None, len(verts0) if v is None else v, 4)

    nodes = nodes0.copy()
    assert call(None, tris0, moved) == -1 and call(nodes, None, moved) == -1 and call(nodes, tris0, None) == -1
    assert call(nodes, tris0, moved, n=0) == -1
    assert nodes.tobytes() == nodes0.tobytes()
    inner = int(np.flatnonzero(nodes0["isLeaf"] == 0)[-1])
    leaf = int(np.flatnonzero((nodes0["isLeaf"] != 0) & (nodes0["right"] > nodes0["left"]))[0])
    cases = []
    bad = nodes0.copy(); bad["left"][inner] = inner; cases.append((bad, tris0))                  # a child index not above its parent
    bad = nodes0.copy(); bad["right"][inner] = len(nodes0); cases.append((bad, tris0))          # a child outside the array
    bad = nodes0.copy(); bad["right"][leaf] = len(tris0) + 1; cases.append((bad, tris0))        # a leaf range outside the references
    bad = nodes0.copy(); bad["left"][leaf] = -1; cases.append((bad, tris0))
    badt = tris0.copy(); badt["v"][len(tris0) // 2, 1] = len(verts0); cases.append((nodes0.copy(), badt))   # a vertex index out of range
    badt = tris0.copy(); badt["v"][0, 0] = -1; cases.append((nodes0.copy(), badt))
    for n, t in cases:
        before = n.tobytes()
        assert call(n, t, moved) == capi.GmuptError("", -1).code == -1
        assert n.tobytes() == before, "a refused call must not write"
        assert b"gmupt_bvh_refit_host" in lib.gmupt_last_error()
    with pytest.raises(capi.GmuptError):
        capi.bvh_refit_host(cases[0][0], tris0, moved)
    assert call(nodes, tris0, moved) == 0 and nodes.tobytes() != nodes0.tobytes()
    with pytest.raises(ValueError):
        pkg.scenes.refit_scene(cornell_scene, moved[:-1])

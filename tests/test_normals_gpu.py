"""GPU tests of the smooth vertex normals (gmupt_normals_*, gmupt_buffer_update_device): the property buffer after Normals.update() against
gmupt_vertex_normals_host, word for word; the progressive front-end's set_vertices(normals="smooth") against the CPU oracle on
scenes.refit_scene(scene, moved, vertex_normals_host(moved, indices)), bit for bit."""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import normals_util as NU
import oracle_lib as O
import parity_util as PU

pytestmark = pytest.mark.gpu
EXTRA = 7          # property records beyond the vertices: never written


def tree_scene(capi, verts, indices, seed=0):
    """A scene dict the renderer binds for a bare (verts, indices) mesh: an LBVH over a finite copy of the vertices, and property records
    -- EXTRA more than vertices -- filled with sentinel bits in every field."""
    sane = np.nan_to_num(np.ascontiguousarray(verts, np.float32), nan=0.0, posinf=1.0, neginf=-1.0)
    built = capi.lbvh_build_host(sane, indices)
    rng = np.random.default_rng(77 + seed)
    props = rng.integers(0, 1 << 32, (len(verts) + EXTRA) * 8, dtype=np.uint64).astype(np.uint32).view(capi.tri_props_dtype)
    return {"nodes": built["nodes"], "tris": built["tris"], "verts": sane, "props": props, "lights": np.zeros(1, capi.light_dtype),
            "materials": np.zeros(1, capi.material_dtype)}


def expected_props(capi, props, verts, indices):
    want = props.copy()
    want["normal"][: len(verts)] = capi.vertex_normals_host(verts, indices)
    return want


def assert_props(got, want, what):
    g, w = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    assert g.shape == w.shape
    assert np.array_equal(g, w), "%s: %d of %d property records differ (first: %d)" % (
        what, int(np.any(g != w, axis=1).sum()), len(g), int(np.flatnonzero(np.any(g != w, axis=1))[0]))


@pytest.fixture(scope="module")
def meshes(pkg):
    return NU.all_meshes(pkg.scenes)


def test_update_equals_the_host_rule_on_every_mesh(pkg, device, meshes):
    capi = pkg.capi
    for k, (name, (v, t)) in enumerate(sorted(meshes.items())):
        scene = tree_scene(capi, v, t, k)
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, 16, 9, pool_paths=1024)
        r.bind_scene(sb)
        sb.verts.update(v)                                   # the mesh as it is, non-finite vertices included
        n = capi.Normals(r, t)
        info = n.update(info=True)
        assert info["num_verts"] == len(v) and info["num_tris"] == len(t) and info["ms"] > 0, info
        assert info["max_valence"] == int(np.bincount(t.reshape(-1)).max()), (name, info)
        want = expected_props(capi, scene["props"], v, t)
        assert_props(sb.props.read(capi.tri_props_dtype), want, name)
        assert n.update() is None
        r.synchronize()
        assert_props(sb.props.read(capi.tri_props_dtype), want, name + ", second update")
        r.close(); sb.close()
        assert not n.h, "Renderer.close() closes the handle first"


def test_indices_as_numpy_and_as_a_device_tensor(pkg, device, meshes):
    capi = pkg.capi
    v, t = meshes["spheres3@0.3"]
    scene = tree_scene(capi, v, t)
    results = []
    for as_tensor in (False, True):
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, 16, 9, pool_paths=1024)
        r.bind_scene(sb)
        idx = torch.from_numpy(t).to("cuda:%d" % device.index) if as_tensor else t
        n = capi.Normals(r, idx)
        if as_tensor:
            idx.zero_()                                      # the handle keeps its own copy
            torch.cuda.synchronize()
        n.update()
        results.append(sb.props.read(capi.tri_props_dtype))
        n.close(); r.close(); sb.close()
    assert_props(results[0], expected_props(capi, scene["props"], v, t), "numpy indices")
    assert_props(results[1], results[0], "device tensor indices")
    with pytest.raises(capi.GmuptError):
        capi.Normals(r, torch.from_numpy(t.astype(np.int64)).to("cuda:%d" % device.index))


def test_another_pose_and_back(pkg, device):
    capi, S = pkg.capi, pkg.scenes
    mesh = S.spheres_mesh(n_spheres=3, subdiv=2, floor_quads=2)
    t = np.ascontiguousarray(mesh["indices"], np.int32)
    poses = [S.wobble(mesh, p) for p in (0.3, 0.6, 0.3)]
    scene = tree_scene(capi, poses[0], t)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    r.bind_scene(sb)
    n = capi.Normals(r, t)
    got = []
    for v in poses:
        sb.verts.update(v)
        n.update()
        got.append(sb.props.read(capi.tri_props_dtype))
        assert_props(got[-1], expected_props(capi, scene["props"], v, t), "pose")
    assert got[0].tobytes() == got[2].tobytes() and got[0].tobytes() != got[1].tobytes()
    r.close(); sb.close()


def test_a_torch_pose_reaches_the_vertex_buffer(pkg, device, cornell_scene):
    """Buffer.update_from_device of a pose held by torch, update(), refit(): vertex, property and node buffers equal the host-upload path."""
    capi, S = pkg.capi, pkg.scenes
    scene = cornell_scene
    t = np.ascontiguousarray(S.cornell_mesh()["indices"], np.int32)
    w = S.wobble(scene, 0.3)
    out = []
    for from_device in (False, True):
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, 48, 27, pool_paths=2048)
        r.bind_scene(sb)
        n = capi.Normals(r, t)
        if from_device:
            sb.verts.update_from_device(torch.from_numpy(w).to("cuda:%d" % device.index))
        else:
            sb.verts.update(w)
        n.update()
        info = r.refit()
        assert info["rebuilt"] == 0
        out.append((sb.verts.read(np.float32).tobytes(), sb.props.read(capi.tri_props_dtype), sb.nodes.read(capi.bvh_node_dtype).tobytes()))
        if from_device:
            with pytest.raises(capi.GmuptError):
                sb.verts.update_from_device(torch.from_numpy(w))                      # host memory
            with pytest.raises(capi.GmuptError):
                sb.verts.update_from_device(torch.zeros(w.size + 3, device="cuda:%d" % device.index))   # too many bytes
            with pytest.raises(capi.GmuptError):
                sb.verts.update_from_device(torch.from_numpy(w).to("cuda:%d" % device.index).t())       # not contiguous
            assert sb.verts.read(np.float32).tobytes() == out[-1][0]
        r.close(); sb.close()
    assert out[0][0] == w.tobytes() and out[1][0] == out[0][0] and out[1][2] == out[0][2]
    assert_props(out[1][1], out[0][1], "device pose")
    assert_props(out[0][1], expected_props(capi, scene["props"], w, t), "host pose")


E2E_MESHES = {"cornell": lambda S: S.cornell_mesh(), "spheres3": lambda S: S.spheres_mesh(n_spheres=3, subdiv=2, floor_quads=2)}


@pytest.fixture(scope="module")
def e2e(pkg):
    """name -> (mesh, scene, moved vertices, the oracle's scene on the host rule's normals), built once."""
    S = pkg.scenes
    out = {}
    for name, make in E2E_MESHES.items():
        mesh = make(S)
        scene = S.build_scene(mesh)
        w = S.wobble(scene, 0.3)
        idx = np.ascontiguousarray(mesh["indices"], np.int32)
        out[name] = (idx, scene, w, S.refit_scene(scene, w, pkg.capi.vertex_normals_host(w, idx)))
    return out


@pytest.mark.parametrize("kernel", ["wide", "cast0"])
@pytest.mark.parametrize("name", sorted(E2E_MESHES))
def test_session_smooth_normals_equal_the_oracle(pkg, device, monkeypatch, e2e, kernel, name):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    capi = pkg.capi
    W, H, P, iters = 48, 27, 2048, 12
    idx, scene, w, moved = e2e[name]
    orc, hip, ocam, hcam, sb = PU.make_pair(pkg, device, scene, W, H, P)
    orc.close()
    orc = O.Renderer(moved, W, H, P, threads=8)
    sess = pkg.progressive.ProgressiveSession(hip, hcam, W, H, preview_every=0)
    info = sess.set_vertices(sb, w, normals="smooth", indices=idx)
    assert info["rebuilt"] == 0 and hcam.buffer.iterationCounter == -1
    ocam.buffer.iterationCounter = -1
    assert_props(sb.props.read(capi.tri_props_dtype), moved["props"], name)
    for it in range(iters):
        PU.step_both(orc, hip, ocam, hcam)
        if it < 2 or it == iters - 1:
            bad = PU.compare_state(orc, hip, P, P)
            assert not bad, "iteration %d: path state differs: %r" % (it, bad[:4])
            assert np.array_equal(orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32)), "iteration %d: framebuffer differs" % it
    assert int(hip.framebuffer()[..., 3].view(np.uint32).sum()) > 0
    assert bool(hip.stats().flags & capi.STAT_CAST_WIDE) == (kernel == "wide")
    # normals=None on the same session afterwards leaves the property buffer alone
    before = sb.props.read(capi.tri_props_dtype).tobytes()
    sess.set_vertices(sb, pkg.scenes.wobble(scene, 0.6))
    assert sb.props.read(capi.tri_props_dtype).tobytes() == before
    sess.close()
    assert sess.normals is None
    hip.close(); sb.close(); orc.close()


def test_session_smooth_normals_default_to_the_bound_records_and_take_a_torch_pose(pkg, device, cornell_scene):
    """Without `indices` and before any rebuild() the list is tris["v"] of the bound scene; the Cornell box has no split triangles, so the
    result is the mesh's.  The pose comes from a torch tensor."""
    capi = pkg.capi
    scene = cornell_scene
    w = pkg.scenes.wobble(scene, 0.3)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    r.bind_scene(sb)
    cam = capi.Camera(48, 27); cam.set_pose(*scene["camera"])
    sess = pkg.progressive.ProgressiveSession(r, cam, 48, 27, preview_every=0)
    sess.set_vertices(sb, torch.from_numpy(w).to("cuda:%d" % device.index), normals="smooth")
    assert sb.verts.read(np.float32).tobytes() == w.tobytes()
    assert_props(sb.props.read(capi.tri_props_dtype), expected_props(capi, scene["props"], w, scene["tris"]["v"]), "bound records")
    with pytest.raises(ValueError):
        sess.set_vertices(sb, w, normals="flat")
    sess.close(); cam.close(); r.close(); sb.close()


def test_rebuild_then_smooth_uses_the_new_index_list(pkg, device):
    capi, S = pkg.capi, pkg.scenes
    mesh = S.spheres_mesh(n_spheres=3, subdiv=2, floor_quads=2)
    scene = S.build_scene(mesh)
    idx = np.ascontiguousarray(mesh["indices"], np.int32)
    cut = np.ascontiguousarray(idx[np.arange(len(idx)) % 3 != 2])     # every third triangle dropped
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    r.bind_scene(sb)
    cam = capi.Camera(48, 27); cam.set_pose(*scene["camera"])
    sess = pkg.progressive.ProgressiveSession(r, cam, 48, 27, preview_every=0)
    w = S.wobble(scene, 0.3)
    sess.set_vertices(sb, w, normals="smooth", indices=idx)
    first = sess.normals
    assert_props(sb.props.read(capi.tri_props_dtype), expected_props(capi, scene["props"], w, idx), "full list")
    sess.rebuild(sb, indices=cut, vertex_material=mesh["vertex_material"])
    assert sess.normals is None and not first.h, "rebuild() drops the adjacency of the old list"
    w2 = S.wobble(scene, 0.6)
    sess.set_vertices(sb, w2, normals="smooth")
    want = expected_props(capi, scene["props"], w2, cut)
    assert_props(sb.props.read(capi.tri_props_dtype), want, "cut list")
    assert want.tobytes() != expected_props(capi, scene["props"], w2, idx).tobytes()
    sess.close(); cam.close(); r.close(); sb.close()


def test_errors_leave_the_buffers_unchanged(pkg, device, meshes):
    capi = pkg.capi
    v, t = meshes["strip257"]
    scene = tree_scene(capi, v, t)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    props0, verts0 = scene["props"].tobytes(), scene["verts"].tobytes()

    def unchanged():
        return sb.props.read(capi.tri_props_dtype).tobytes() == props0 and sb.verts.read(np.float32).tobytes() == verts0

    with pytest.raises(capi.GmuptError) as e:
        capi.Normals(r, t)                                   # nothing bound
    assert e.value.code == capi.ERR_NOT_BOUND and unchanged()
    r.bind_scene(sb)
    bad = t.copy(); bad[100, 2] = len(v)
    with pytest.raises(capi.GmuptError) as e:
        capi.Normals(r, bad)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and unchanged() and not r._normals
    n = capi.Normals(r, t)
    # a rebind to a scene with another vertex count
    v2, t2 = meshes["strip259"]
    scene2 = tree_scene(capi, v2, t2, 1)
    sb2 = capi.SceneBuffers(device, scene2)
    r.bind_scene(sb2)
    with pytest.raises(capi.GmuptError) as e:
        n.update()
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and unchanged()
    assert sb2.props.read(capi.tri_props_dtype).tobytes() == scene2["props"].tobytes()
    r.bind_scene(sb)                                         # back: the handle works on what is bound now
    n.update()
    assert_props(sb.props.read(capi.tri_props_dtype), expected_props(capi, scene["props"], scene["verts"], t), "after the rebind")
    r.close(); sb.close(); sb2.close()
    assert not n.h

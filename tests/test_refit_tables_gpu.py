"""GPU tests of the traversal tables a renderer holds (gmupt_debug_read_travtable), byte for byte:
  - after a bind: the host build of the same tree (capi.travtables with the renderer's switches) -- tables, scalars and refit maps;
  - after a refit: the rule of include/gmupt.h applied to the tables read after the bind (refit_tables_util.refit_tables, numpy only),
    with the node boxes of gmupt_bvh_refit_host.  Rays cannot see a box that is too large, a record no ray reaches or a clobbered kept
    word; this comparison does.  A fresh build of the refitted tree is not the expected value (test_refit_tables_cpu.py shows why).
Smallest shapes throughout: 48x27 renderers with a pool of 2048 paths.
"""
import ctypes as C

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import refit_tables_util as RT
from test_lbvh_gpu import DeviceBuiltScene

pytestmark = pytest.mark.gpu
W, H, P = 48, 27, 2048
FIXTURES = ("cornell", "soup", "spheres", "chain", "textured")
LBVH = [(1, 1), (2, 1), (3, 1), (255, 1), (256, 1), (257, 1), (258, 1), (257, 4)]     # (triangles, max_leaf_size): the record counts of the four kernels on either side of a 256-thread block; one and two leaves
REFIT_SCENES = FIXTURES + ("empty_leaf",) + tuple("lbvh%d_L%d" % nl for nl in LBVH)
KERNELS = ("wide", "cast0")


@pytest.fixture(scope="module")
def scenes(pkg, cornell_scene, soup_scene, spheres_small_scene):
    S = pkg.scenes
    out = {"cornell": cornell_scene, "soup": soup_scene, "spheres": spheres_small_scene,
           "chain": S.build_scene(S.deep_chain_mesh()), "textured": S.build_scene(S.textured_mesh()),
           "empty_leaf": RT.empty_leaf_scene(pkg)}
    for n, L in LBVH:
        out["lbvh%d_L%d" % (n, L)] = RT.lbvh_scene(pkg, n, 500 + n, L)
    return out


def bound(pkg, device, scene, sb=None):
    """(renderer, buffers) bound to `scene` (or to existing buffers)."""
    sb = sb or pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, W, H, pool_paths=P)
    r.bind_scene(sb)
    return r, sb


def host_tables(pkg, scene, kernel, nodes=None, verts=None, **switches):
    """What a bind of this tree uploads: the host build with the renderer's switches, the pairs dropped where there is no wide copy."""
    return RT.device_view(pkg.capi.travtables(scene["nodes"] if nodes is None else nodes, scene["tris"], scene["verts"] if verts is None else verts,
                                              want_wide=(kernel == "wide"), **switches))


def refit_and_check(pkg, r, sb, scene, verts, what, before=None):
    """Uploads `verts`, refits (no rebuild expected) and compares every table with the rule applied to the tables held before; returns
    (tables after, refitted nodes)."""
    capi = pkg.capi
    before = before or r.read_travtables()
    sb.verts.update(verts)
    info = r.refit()
    assert info["rebuilt"] == 0 and info["reason"] == 0, (what, info)
    nodes = capi.bvh_refit_host(scene["nodes"], scene["tris"], verts)
    assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == nodes.tobytes(), "%s: the node buffer differs from gmupt_bvh_refit_host" % what
    after = r.read_travtables()
    RT.assert_tables(after, RT.refit_tables(before, nodes, scene["tris"], verts), what)
    return after, nodes


# ---- a: the bind upload
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", FIXTURES + ("empty_leaf", "lbvh1_L1", "lbvh2_L1", "lbvh257_L4"))
def test_bind_uploads_the_host_built_tables(pkg, device, monkeypatch, scenes, name, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    r, sb = bound(pkg, device, scenes[name])
    got = r.read_travtables()
    assert sorted(got) == sorted(pkg.capi.TRAVTABLE_KINDS)
    RT.assert_tables(got, host_tables(pkg, scenes[name], kernel), "%s, %s" % (name, kernel))
    assert (len(got["wnode"]) > 0) == (kernel == "wide" and name != "lbvh1_L1") and len(got["rec64"]) == 0
    r.close(); sb.close()


@pytest.mark.parametrize("env,switches", [({"GMUPT_TOP_ORDER": "bfs"}, {"top_order_bfs": True}), ({"GMUPT_NODE_PAIRING": "0"}, {"node_pairing": False})])
def test_bind_uploads_the_host_built_tables_with_the_numbering_switches(pkg, device, monkeypatch, scenes, env, switches):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r, sb = bound(pkg, device, scenes["soup"])
    got = r.read_travtables()
    RT.assert_tables(got, host_tables(pkg, scenes["soup"], "wide", **switches), repr(env))
    assert RT.table_diffs(got, host_tables(pkg, scenes["soup"], "wide"), ("node_map",)), "the switch changed nothing"
    refit_and_check(pkg, r, sb, scenes["soup"], pkg.scenes.wobble(scenes["soup"], 0.3, 0.05), repr(env), before=got)
    r.close(); sb.close()


# ---- b: refit
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", REFIT_SCENES)
def test_refit_leaves_the_rule_applied_to_the_bind_tables(pkg, device, monkeypatch, scenes, name, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    scene = scenes[name]
    for phase in (0, 0.3):
        r, sb = bound(pkg, device, scene)
        before = r.read_travtables()
        after, _ = refit_and_check(pkg, r, sb, scene, pkg.scenes.wobble(scene, phase, 0.05), "%s, %s, phase %s" % (name, kernel, phase), before)
        if phase:
            assert RT.table_diffs(after, before, ("tri48", "scalars")), "the wobble moved nothing"
        r.close(); sb.close()


# ---- c: idempotence, and back to a pose
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_second_refit_and_a_return_to_a_pose_change_no_byte(pkg, device, monkeypatch, scenes, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    scene = scenes["soup"]
    r, sb = bound(pkg, device, scene)
    seen = {}
    for step, phase in enumerate((0.2, 0.45, 0.8, 0.2)):
        w = pkg.scenes.wobble(scene, phase, 0.05)
        after, _ = refit_and_check(pkg, r, sb, scene, w, "step %d, phase %s" % (step, phase))
        assert r.refit()["rebuilt"] == 0
        RT.assert_tables(r.read_travtables(), after, "a second refit on the vertices of phase %s" % phase)
        if phase in seen:
            RT.assert_tables(after, seen[phase], "back at phase %s" % phase)
        seen[phase] = after
    assert RT.table_diffs(seen[0.2], seen[0.8], ("tri48",))
    r.close(); sb.close()


# ---- d: a refused refit writes nothing
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_refused_refit_leaves_every_table_and_the_nodes_as_they_were(pkg, device, monkeypatch, scenes, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    capi = pkg.capi
    scene = scenes["cornell"]
    r, sb = bound(pkg, device, scene)
    refit_and_check(pkg, r, sb, scene, pkg.scenes.wobble(scene, 0.3, 0.05), "before the refusals")   # (the maps are on the device now)
    tables0, nodes0 = r.read_travtables(), sb.nodes.read(capi.bvh_node_dtype).tobytes()
    used = int(scene["tris"]["v"][len(scene["tris"]) // 2, 1])
    for bad in (np.nan, np.inf, -np.inf):
        v = pkg.scenes.wobble(scene, 0.45, 0.05)             # another pose: a write of any table would show
        v[used, 1] = bad
        sb.verts.update(v)
        with pytest.raises(capi.GmuptError) as e:
            r.refit()
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, e.value
        RT.assert_tables(r.read_travtables(), tables0, "refused refit (%s)" % bad)
        assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == nodes0, "a refused refit must not write the node buffer"
    r.close(); sb.close()


# ---- e: the fallbacks are a fresh bind
def snapped(scene):
    """The soup of test_flat_child_falls_back_to_the_host_pass: its lower half, by centroid, snapped onto the plane z = min z."""
    v = scene["verts"].copy()
    t = scene["tris"]["v"]
    cz = v[t][:, :, 2].mean(axis=1)
    v[np.unique(t[cz < np.median(cz)]), 2] = v[:, 2].min()
    return v


def fallback_check(pkg, dev, scene, variants):
    capi = pkg.capi
    r, sb = bound(pkg, dev, scene)
    before = r.read_travtables()
    v = snapped(scene)
    sb.verts.update(v)
    info = r.refit()
    assert info["rebuilt"] == 1 and info["reason"] & (capi.REFIT_VARIANTS_BUILD if variants else capi.REFIT_FLAT_CHILD), info
    nodes = capi.bvh_refit_host(scene["nodes"], scene["tris"], v)
    rebuilt = r.read_travtables()
    RT.assert_tables(rebuilt, host_tables(pkg, scene, "wide", nodes=nodes, verts=v), "tables of the rebuild")
    assert RT.table_diffs(rebuilt, before, ("node_map", "wide_map", "opened")), "the rebuild kept the maps of the first bind"
    assert (len(rebuilt["rec64"]) > 0) == variants
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    if not variants:
        # the refit kernels now work through the maps of the REBUILT tables: with the first bind's maps still on the device the
        # restatement through the rebuilt ones would not come out
        refit_and_check(pkg, r, sb, scene, w, "refit after the rebuild", before=rebuilt)
    else:
        sb.verts.update(w)
        assert r.refit()["rebuilt"] == 1
        RT.assert_tables(r.read_travtables(), host_tables(pkg, scene, "wide", nodes=capi.bvh_refit_host(scene["nodes"], scene["tris"], w), verts=w),
                         "second rebuild")
    r.close(); sb.close()


def test_flat_child_fallback_leaves_a_fresh_binds_tables_and_maps(pkg, device, monkeypatch, scenes):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    fallback_check(pkg, device, scenes["soup"], variants=False)


def test_variants_build_fallback_leaves_a_fresh_binds_tables_and_records(pkg, monkeypatch, scenes):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    with pkg.capi.use_build("variants"):
        dev = pkg.capi.Device(0)
        fallback_check(pkg, dev, scenes["soup"], variants=True)
        dev.close()


def test_refit_tables_in_the_tiny_stack_build(pkg, monkeypatch, scenes):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    with pkg.capi.use_build("wides8"):
        dev = pkg.capi.Device(0)
        r, sb = bound(pkg, dev, scenes["soup"])
        before = r.read_travtables()
        RT.assert_tables(before, host_tables(pkg, scenes["soup"], "wide"), "bind in the wides8 build")
        refit_and_check(pkg, r, sb, scenes["soup"], pkg.scenes.wobble(scenes["soup"], 0.3, 0.05), "wides8", before)
        r.close(); sb.close(); dev.close()


# ---- f: a tree built on the device
@pytest.mark.parametrize("kernel", KERNELS)
def test_bind_and_refit_of_a_device_built_tree(pkg, device, monkeypatch, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    builder = pkg.capi.Lbvh(device)
    d = DeviceBuiltScene(pkg, device, builder, pkg.scenes.random_triangles_mesh(300, seed=3))
    r, _ = bound(pkg, device, d.scene, sb=d.sb)
    before = r.read_travtables()
    RT.assert_tables(before, host_tables(pkg, d.scene, kernel), "bind of the device-built tree")
    for phase in (0, 0.3):
        before, _ = refit_and_check(pkg, r, d.sb, d.scene, pkg.scenes.wobble(d.scene, phase, 0.05), "device-built tree, phase %s" % phase, before)
    r.close(); d.close(); builder.close()


# ---- g: several renderers bound to the same buffers each call refit
def test_two_renderers_on_one_set_of_buffers_each_refit_their_own_tables(pkg, device, monkeypatch, scenes):
    capi = pkg.capi
    scene = scenes["spheres"]
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    rw, sb = bound(pkg, device, scene)
    monkeypatch.setenv("GMUPT_TRAVERSAL", "cast0")
    rc, _ = bound(pkg, device, scene, sb=sb)
    bw, bc = rw.read_travtables(), rc.read_travtables()
    assert len(bw["wnode"]) > 0 and len(bc["wnode"]) == 0
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    aw, nodes = refit_and_check(pkg, rw, sb, scene, w, "the wide renderer", bw)
    RT.assert_tables(rc.read_travtables(), bc, "the cast0 renderer before its own refit")
    ac, _ = refit_and_check(pkg, rc, sb, scene, w, "the cast0 renderer", bc)          # (the node buffer: the host refit's bytes after either call)
    RT.assert_tables(rw.read_travtables(), aw, "the wide renderer after the other's refit")
    RT.assert_tables(ac, RT.refit_tables(bc, nodes, scene["tris"], w), "the cast0 renderer holds its own tables")
    rw.close(); rc.close(); sb.close()


# ---- h: the reader's own contract
def test_reader_sizes_and_errors(pkg, device, monkeypatch, scenes):
    capi = pkg.capi
    read = capi.lib().gmupt_debug_read_travtable
    monkeypatch.setenv("GMUPT_TRAVERSAL", "cast0")
    n = C.c_size_t(77)
    assert read(None, 0, None, 0, C.byref(n)) == capi.ERR_INVALID_ARGUMENT
    r = capi.Renderer(device, W, H, pool_paths=P)
    assert read(r.h, 0, None, 0, C.byref(n)) == capi.ERR_NOT_BOUND and n.value == 0
    with pytest.raises(capi.GmuptError) as e:
        r.read_travtables()
    assert e.value.code == capi.ERR_NOT_BOUND
    sb = capi.SceneBuffers(device, scenes["cornell"])
    r.bind_scene(sb)
    assert read(r.h, 0, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    want = host_tables(pkg, scenes["cornell"], "cast0")
    for which, kind in enumerate(capi.TRAVTABLE_KINDS):
        n = C.c_size_t(77)
        assert read(r.h, which, None, 0, C.byref(n)) == 0 and n.value == len(want[kind]), kind          # the size query
        if not n.value:
            assert kind in ("tripair", "pair_ref", "wnode", "rec64", "wide_map", "opened"), kind        # absent without a wide copy: success, 0 bytes
            continue
        buf = np.full(n.value + 8, 0xAB, np.uint8)
        m = C.c_size_t(0)
        assert read(r.h, which, capi._ptr(buf), n.value - 1, C.byref(m)) == capi.ERR_INVALID_ARGUMENT and m.value == n.value
        assert (buf == 0xAB).all(), "%s: a buffer too small must stay unwritten" % kind
        assert read(r.h, which, None, n.value, C.byref(m)) == capi.ERR_INVALID_ARGUMENT
        assert read(r.h, which, capi._ptr(buf), buf.nbytes, C.byref(m)) == 0 and m.value == n.value
        assert buf[:n.value].tobytes() == want[kind].tobytes() and (buf[n.value:] == 0xAB).all(), kind
    for which in (-1, len(capi.TRAVTABLE_KINDS)):
        assert read(r.h, which, None, 0, C.byref(n)) == capi.ERR_INVALID_ARGUMENT and n.value == 0
    r.close(); sb.close()


def test_reading_the_tables_leaves_the_renderer_untouched(pkg, device, monkeypatch, scenes):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    scene = scenes["textured"]
    sb = pkg.capi.SceneBuffers(device, scene)
    runs = []
    for with_reads in (False, True):
        r, _ = bound(pkg, device, scene, sb=sb)
        cam = pkg.capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        for it in range(12):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            if with_reads and it % 3 == 1:
                r.read_travtables()
        r.synchronize()
        runs.append((r.framebuffer(), r.read_path_state(), r.read_queues(), r.counters(), r.stats().as_dict(), r.read_travtables()))
        r.close(); cam.close()
    sb.close()
    (fa, sa, qa, ca, ta, tta), (fb, sbb, qb, cb, tb, ttb) = runs
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(sa, sbb) and np.array_equal(qa, qb) and np.array_equal(ca, cb)
    assert ta == tb
    RT.assert_tables(ttb, tta, "tables after 12 iterations with reads in between")
    assert int(fa[..., 3].view(np.uint32).sum()) > 0

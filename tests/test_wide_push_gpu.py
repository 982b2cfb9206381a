"""GPU tests of the push sequence of the wide ray cast's node step (k_cast_w, csrc/pt_traverse_wide.hip).

A node step pushes its hit slots onto two stacks that share one LDS array per lane and grow towards each other -- inner nodes from the
bottom, leaves from the top -- and keeps one hit inner slot as the next node.  Which entry is kept and in which order the others are
pushed is free (the head of pt_traverse_wide.hip says why); that no push lands on a live entry of the other stack is not.  The shapes
here are the ones at which that can go wrong: stacks that meet all the time (the 8-word test build), nodes whose four slots are hit in
every split between inner and leaf slots, partial waves, exact ties, and the counted work.  Bar as everywhere: bit for bit against the
CPU oracle, through parity_util / trace_util.
"""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the query's rays and outputs are torch tensors)

import oracle_lib as O
import parity_util as PU
from test_parity_gpu import _assert_same
from trace_util import FLT_MAX, assert_matches_oracle, make_rays, oracle_truth

pytestmark = pytest.mark.gpu

WNODE = np.dtype([("p", "<f4", (6, 4)), ("link", "<i4", 4), ("aux", "<i4", 4)])
EMPTY_LINK = -0x80000000
CAST_FIELDS = ["surfacePoint", "baryCoord", "triangle", "isEmitter", "hitDistance", "inShadow"]


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


# ------------------------------------------------------------------------------------------------------------------ stack pressure
@pytest.mark.parametrize("scene_name", ["soup", "spheres"])
def test_push_with_meeting_stacks(pkg, monkeypatch, soup_scene, spheres_small_scene, scene_name):
    # the wides8 build gives a lane 8 LDS words for both stacks: a lane steps with pb - pa >= 3, so the free window between the stacks is
    # exactly four slots most of the time and every push lands next to a live entry of the other stack.  Every iteration is compared.
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    scene = {"soup": soup_scene, "spheres": spheres_small_scene}[scene_name]
    W, H, P = 32, 18, 1024
    with pkg.capi.use_build("wides8"):
        dev = pkg.capi.Device(0)
        orc, hip, ocam, hcam, sb = PU.make_pair(pkg, dev, scene, W, H, P, collect_stats=True)
        for it in range(8):
            PU.step_both(orc, hip, ocam, hcam)
            _assert_same(orc, hip, P, P, it)
        sh = hip.stats()
        assert sh.flags & pkg.capi.STAT_CAST_WIDE and not (sh.flags & (pkg.capi.STAT_STACK_OVERFLOW | pkg.capi.STAT_CAST_ABORTED))
        assert sh.cast_redo_rays > 0, "the full-stack parking path must be taken"
        hip.close(); sb.close(); orc.close(); dev.close()


# ------------------------------------------------------------------------------------------- every split of four hits at one node
def pierce_mesh(pkg, kinds, bundle, seed=3, **build):
    """Four objects in a row along x, 2 apart, each a `cluster` (a jittered 3 x 3 grid of quads, 18 triangles: an inner slot of the root
    WNode) or a `leaf` (`bundle` tilted triangles 0.02 apart: a leaf slot), of shrinking size and shifted centres, so that a ray along x
    through the middle pierces all four and rays off the middle pierce every subset."""
    rng = np.random.default_rng(seed)
    verts, idx = [], []
    for k, kind in enumerate(kinds):
        x, half = 2.0 * k, 1.0 - 0.15 * k
        cy, cz = ((0.0, 0.0), (0.35, -0.2), (-0.3, 0.3), (0.2, 0.35))[k]
        if kind == "leaf":
            for j in range(bundle):
                xx = x + 0.02 * j
                b = len(verts)
                verts += [[xx - 0.2, cy - 2 * half, cz - half], [xx + 0.1, cy + 2 * half, cz - half], [xx + 0.3, cy, cz + 3 * half]]
                idx.append([b, b + 1, b + 2])
        else:
            n = 3
            for a in range(n):
                for c in range(n):
                    y0, y1 = cy - half + 2 * half * a / n, cy - half + 2 * half * (a + 1) / n
                    z0, z1 = cz - half + 2 * half * c / n, cz - half + 2 * half * (c + 1) / n
                    xs = x + rng.uniform(-0.3, 0.3, 4)
                    b = len(verts)
                    verts += [[xs[0], y0, z0], [xs[1], y1, z0], [xs[2], y1, z1], [xs[3], y0, z1]]
                    idx += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    verts, idx = np.array(verts, np.float32), np.array(idx, np.int32)
    mesh = pkg.scenes.cornell_mesh()
    mesh.update({"verts": verts, "normals": np.tile(np.array([1.0, 0.0, 0.0], np.float32), (len(verts), 1)), "indices": idx,
                 "vertex_material": (np.arange(len(verts)) % 3).astype(np.uint32), "name": "pierce"})
    mesh.pop("uv", None)
    return pkg.scenes.build_scene(mesh, **build)


def pierce_rays(n, seed):
    """Ray 0 runs through the middle of all four objects; the others start on a 3.6 x 3.6 window in front of (or, every third one, behind)
    the row and are tilted a little: no zero component, every subset of the four objects."""
    rng = np.random.default_rng(seed)
    o = np.empty((n, 3), np.float32); d = np.empty((n, 3), np.float32)
    o[:, 0] = -2.0; o[:, 1:] = rng.uniform(-1.8, 1.8, (n, 2))
    d[:, 0] = 1.0; d[:, 1:] = rng.uniform(0.01, 0.12, (n, 2)) * rng.choice(np.array([-1.0, 1.0]), (n, 2))
    back = np.arange(n) % 3 == 2
    o[back, 0] = 9.0; d[back, 0] = -1.0
    o[0] = (-2.0, 0.05, 0.1); d[0] = (1.0, 0.004, 0.003)
    d[n // 2:] /= np.linalg.norm(d[n // 2:], axis=1, keepdims=True)
    return make_rays(o, d, FLT_MAX), make_rays(o, d, rng.uniform(1.0, 12.0, n).astype(np.float32))


def root_splits(pkg, scene, rays):
    """(link of the root WNode's four slots, the set of (inner hits, leaf hits) the rays make at the root): the slab test of ray_box
    recomputed with numpy in binary32 on the root record of the traversal tables."""
    w = pkg.capi.travtables(scene["nodes"], scene["tris"], scene["verts"])["wnode"].view(WNODE)[0]
    o, d = rays[:, 0:3].astype(np.float32), rays[:, 4:7].astype(np.float32)
    inv = (np.float32(1.0) / d).astype(np.float32)
    lo, hi = w["p"][0:3], w["p"][5:2:-1]                                   # rows 0..2 = min x, y, z; rows 5, 4, 3 = max x, y, z
    ta = ((lo[None, :, :] - o[:, :, None]) * inv[:, :, None]).astype(np.float32)
    tb = ((hi[None, :, :] - o[:, :, None]) * inv[:, :, None]).astype(np.float32)
    t0 = np.minimum(ta, tb).max(axis=1); t1 = np.maximum(ta, tb).min(axis=1)
    hit = (t1 >= t0) & (t1 > 0)
    inner = w["link"] >= 0
    return w["link"], set(zip((hit & inner).sum(axis=1).tolist(), (hit & ~inner).sum(axis=1).tolist()))


# kinds of the four objects, triangles per leaf object, builder options, (inner, leaf) slots of the root, splits that must occur
PIERCE_CASES = {
    "four_triangles": (["leaf"] * 4, 1, {"builder": "lbvh", "max_leaf_size": 1}, (0, 4), [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)]),
    "four_leaves": (["leaf"] * 4, 2, {}, (0, 4), [(0, 1), (0, 2), (0, 3), (0, 4)]),
    "four_clusters": (["cluster"] * 4, 2, {}, (4, 0), [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]),
    "three_one": (["cluster", "cluster", "cluster", "leaf"], 2, {}, (3, 1), [(3, 1), (3, 0), (2, 1), (1, 1), (0, 1)]),
    "two_two": (["cluster", "leaf", "cluster", "leaf"], 2, {}, (2, 2), [(2, 2), (2, 1), (1, 2), (0, 2), (1, 1)]),
    "one_three": (["leaf", "cluster", "leaf", "leaf"], 2, {}, (1, 3), [(1, 3), (1, 2), (0, 3), (1, 1), (1, 0)]),
}


@pytest.mark.parametrize("case", sorted(PIERCE_CASES))
def test_every_split_of_four_hits(pkg, device, wide, case):
    # one node whose four slots are hit in every split between inner and leaf slots: all pushes of a step meet between pa and pb.
    # four_triangles: four single-triangle leaves under the root (the LBVH host builder with one triangle per leaf; the SBVH puts four
    # triangles into two leaves); batches of 1, 63, 64, 65 and 129 rays: partial waves, one wave, the refill of a second and a third
    kinds, bundle, build, slots, splits = PIERCE_CASES[case]
    scene = pierce_mesh(pkg, kinds, bundle, **build)
    closest, any_rays = pierce_rays(129, seed=17)
    link, seen = root_splits(pkg, scene, closest)
    assert (int((link >= 0).sum()), int(((link < 0) & (link != EMPTY_LINK)).sum())) == slots, link
    assert all(s in seen for s in splits), (splits, sorted(seen))
    assert slots in root_splits(pkg, scene, closest[:1])[1], "the first ray pierces all four objects"
    truth = oracle_truth(scene, closest, any_rays, 0)
    sb = pkg.capi.SceneBuffers(device, scene)
    r = pkg.capi.Renderer(device, 32, 18, pool_paths=4096)
    r.bind_scene(sb)
    for n in (1, 63, 64, 65, 129):
        info = pkg.capi.TraceInfo()
        hits, occ = r.trace(torch.from_numpy(closest[:n].copy()).cuda(), torch.from_numpy(any_rays[:n].copy()).cuda(), info=info)
        assert info.flags & pkg.capi.STAT_CAST_WIDE
        h, oc = hits.cpu().numpy(), occ.cpu().numpy()
        assert_matches_oracle(scene, closest[:n], any_rays[:n], h, oc, 0, truth=truth)
        if n == 129:
            assert (h.view(np.int32)[:, 3] >= 0).sum() > 40 and oc.sum() > 20 and (oc == 0).sum() > 20
    r.close(); sb.close()


# ------------------------------------------------------------------------------------------- order freedom is not result freedom
def test_other_visit_order_same_ties(pkg, device, wide):
    # the adversarial grid mesh of test_wide_on_grid_meshes_with_exact_ties on a seed of its own: coplanar duplicates, shared edges, rays
    # along grid directions from grid points.  Which of two hits with equal t a walk meets first depends on the visit order; the result
    # does not: the tie is noticed and the ray walked again in the reference's order
    seed = 7
    rng = np.random.default_rng(seed)
    n_tris = int(rng.integers(20, 400)); grid = int(rng.choice([3, 5, 9])); nv = max(4, n_tris // 2)
    verts = (rng.integers(0, grid, (nv, 3)) * (8.0 / (grid - 1)) - 4.0).astype(np.float32)
    idx = rng.integers(0, nv, (n_tris, 3)).astype(np.int32)
    idx[: n_tris // 5] = idx[n_tris // 5: 2 * (n_tris // 5)][: n_tris // 5]
    mesh = pkg.scenes.cornell_mesh()
    mesh.update({"verts": verts, "normals": np.tile(np.array([0.0, 1.0, 0.0], np.float32), (nv, 1)), "indices": idx,
                 "vertex_material": rng.integers(0, 3, nv).astype(np.uint32), "name": "grid%d" % seed})
    mesh.pop("uv", None)
    scene = pkg.scenes.build_scene(mesh)
    P = 4096
    orc, hip, ocam, hcam, sb = PU.make_pair(pkg, device, scene, 32, 18, P, collect_stats=True)
    pts = (rng.integers(0, grid, (P, 3)) * (8.0 / (grid - 1)) - 4.0).astype(np.float32)
    dirs = rng.integers(-2, 3, (P, 3)).astype(np.float32); dirs[(dirs == 0).all(axis=1)] = (1.0, 0.0, 0.0)
    nz = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), (P, 3))
    third = np.arange(P) % 3 == 0
    dirs[third] = nz[third]
    dirs[: P // 2] /= np.linalg.norm(dirs[: P // 2], axis=1, keepdims=True)
    o = (pts - dirs * rng.integers(1, 4, (P, 1)).astype(np.float32)).astype(np.float32)
    st = orc.path_state()
    O.state_field(st, P, "rayOrigin").view(np.float32)[:] = o; O.state_field(st, P, "rayDirection").view(np.float32)[:] = dirs
    O.state_field(st, P, "shadowrayOrigin").view(np.float32)[:] = o; O.state_field(st, P, "shadowrayDirection").view(np.float32)[:] = dirs
    O.state_field(st, P, "lightDistance").view(np.float32)[:, 0] = rng.uniform(0.5, 12.0, P).astype(np.float32)
    orc.queues()[3][:] = np.arange(P, dtype=np.uint32); orc.queues()[4][:] = np.arange(P, dtype=np.uint32)[::-1]
    qc = orc.counters(); qc[:] = 0; qc[6] = P; qc[7] = P
    ocam.update(); hcam.update(0.0); orc.set_camera(ocam.buffer); hip.set_camera(hcam.buffer)
    frozen = (orc.path_state().copy(), orc.queues().copy(), orc.counters().copy())
    orc.stage("extension"); orc.stage("shadow")
    hip.write_path_state(frozen[0]); hip.write_queues(frozen[1]); hip.write_counters(frozen[2])
    hip.run_stage(pkg.capi.STAGE_RAYCASTS)
    bad = PU.compare_state(orc, hip, P, P, fields=CAST_FIELDS)
    assert not bad, bad[:3]
    sh = hip.stats()
    assert sh.flags & pkg.capi.STAT_CAST_WIDE
    assert sh.cast_redo_rays > 0, "exact ties must go to the exact walk"
    hip.close(); sb.close(); orc.close()


# ------------------------------------------------------------------------------------------------------- counted work is unchanged
@pytest.mark.parametrize("steps", ["6", "8"])
def test_counted_work_is_the_oracles(pkg, device, wide, monkeypatch, soup_scene, steps):
    # the leaves a ray reaches and the triangles it tests do not depend on the order of the pushes: rays, and -- over iterations in which no
    # ray was walked again (the exact walk counts its own visits) -- leaves and triangles of the extension rays equal the oracle's, for both
    # instantiations (six / eight steps between two looks at the queues); drained waves hand subtrees to their free lanes on the way
    monkeypatch.setenv("GMUPT_WIDE_STEPS", steps)
    W, H, P = 32, 18, 1024
    orc, hip, ocam, hcam, sb = PU.make_pair(pkg, device, soup_scene, W, H, P, collect_stats=True)
    prev = (0, 0, 0, 0, 0); clean = 0
    for it in range(8):
        PU.step_both(orc, hip, ocam, hcam)
        _assert_same(orc, hip, P, P, it)
        so, sh = orc.stats(), hip.stats()
        assert sh.flags & pkg.capi.STAT_CAST_WIDE
        assert (so.extRays, so.shRays) == (sh.ext_rays, sh.sh_rays), "iteration %d" % it
        now = (int(sh.cast_redo_rays), int(so.extLeaves), int(so.extTris), int(sh.ext_leaves), int(sh.ext_tris))
        if now[0] == prev[0]:
            clean += 1
            assert (now[1] - prev[1], now[2] - prev[2]) == (now[3] - prev[3], now[4] - prev[4]), "iteration %d: leaves, triangles" % it
        prev = now
    assert clean > 0, "no iteration without a ray walked again"
    assert sh.cast_helper_subtrees > 0 and sh.wide_iterations > 0
    hip.close(); sb.close(); orc.close()

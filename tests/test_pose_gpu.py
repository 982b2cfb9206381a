"""GPU tests of the pose stage (gmupt_pose_*): the bound vertex buffer after Pose.update() against gmupt_pose_host, bit for bit, over the
wave and block tails, both homes of the joint matrices and the skipped targets; the progressive front-end's set_pose against the CPU
oracle on scenes.refit_scene(scene, pose_host vertices, vertex_normals_host of them), bit for bit."""
import itertools

import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import oracle_lib as O
import parity_util as PU
import pose_util as PS

pytestmark = pytest.mark.gpu
LDS_JOINTS = 640          # the most joint matrices k_ps_pose keeps in LDS (include/gmupt.h "Pose"); 641 are read from global memory


def soup_scene(S, V):
    """A random triangle soup cut to exactly V vertices (the last triangle wraps round to the first vertices), as build_scene binds it."""
    m = dict(S.random_triangles_mesh((V + 2) // 3, seed=V))
    for k in ("verts", "normals", "vertex_material"):
        m[k] = m[k][:V].copy()
    m["indices"] = (m["indices"] % V).astype(np.int32)
    return S.build_scene(m)


def rig_for(V, K, J, T, seed=0):
    rig = PS.random_rig(V, K, J, T, seed)
    if J:
        rig["joints"][V // 2, 0] = J - 1; rig["weights"][V // 2, 0] = 0.5        # the last joint is used
    return rig


def make_pose(capi, r, rig, **kw):
    return capi.Pose(r, rig["rest"], rig["joints"], rig["weights"], rig["num_joints"], rig["deltas"] if len(rig["deltas"]) else None, **kw)


def cuda(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:%d" % device.index)


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_update_equals_the_host_rule(pkg, device, V):
    capi = pkg.capi
    sb = capi.SceneBuffers(device, soup_scene(pkg.scenes, V))
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    r.bind_scene(sb)
    for K, J, T in itertools.product((1, 4, 8), (1, LDS_JOINTS, LDS_JOINTS + 1), (0, 1, 3)):
        rig = rig_for(V, K, J, T)
        pose = make_pose(capi, r, rig)
        info = pose.update(rig["mats"], rig["target_weights"], info=True)
        want_active = int(np.count_nonzero(rig["target_weights"]))
        assert info["num_verts"] == V and info["active_targets"] == want_active == (T if T < 2 else T - 1) and info["ms"] > 0, (K, J, T, info)
        got = sb.verts.read(np.float32).reshape(-1, 3)
        n = PS.differing(got, PS.host(capi, rig))
        assert got.shape == (V, 3) and n == 0, "V %d K %d J %d T %d: %d vertices differ from gmupt_pose_host" % (V, K, J, T, n)
        pose.close()
    # morph only
    rig = rig_for(V, 0, 0, 3)
    pose = make_pose(capi, r, rig)
    assert pose.update(None, rig["target_weights"]) is None
    r.synchronize()
    assert PS.differing(sb.verts.read(np.float32), PS.host(capi, rig)) == 0
    r.close(); sb.close()
    assert not pose.h, "Renderer.close() closes the handle first"


def test_host_arrays_and_device_tensors_give_the_same_bytes(pkg, device):
    capi = pkg.capi
    V, K, J, T = 257, 4, 40, 3
    rig = rig_for(V, K, J, T, 1)
    want = PS.host(capi, rig).tobytes()
    sb = capi.SceneBuffers(device, soup_scene(pkg.scenes, V))
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    r.bind_scene(sb)
    poses = [make_pose(capi, r, rig),
             capi.Pose(r, cuda(device, rig["rest"]), cuda(device, rig["joints"].view(np.int16)), cuda(device, rig["weights"]), J, cuda(device, rig["deltas"]))]
    zero = np.zeros_like(rig["rest"])
    for pose in poses:
        for mats, tw in ((rig["mats"], rig["target_weights"]), (cuda(device, rig["mats"]), cuda(device, rig["target_weights"])),
                         (cuda(device, rig["mats"]), rig["target_weights"])):
            sb.verts.update(zero)
            pose.update(mats, tw)
            r.synchronize()
            assert sb.verts.read(np.float32).tobytes() == want
    with pytest.raises(capi.GmuptError):
        capi.Pose(r, cuda(device, rig["rest"].astype(np.float64)), rig["joints"], rig["weights"], J)
    with pytest.raises(capi.GmuptError):
        poses[0].update(rig["mats"][:-1], rig["target_weights"])
    r.close(); sb.close()


def test_another_pose_and_back(pkg, device):
    capi, S = pkg.capi, pkg.scenes
    scene = soup_scene(S, 257)
    rig = S.make_rig(scene, 5, 4, 3, seed=2)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    r.bind_scene(sb)
    pose = capi.Pose(r, rig["rest"], rig["joints"], rig["weights"], 5, rig["deltas"])
    got = []
    for phase in (0.3, 0.6, 0.3):
        mats, tw = S.rig_pose(rig, phase)
        pose.update(mats, tw)
        got.append(sb.verts.read(np.float32).tobytes())
        assert got[-1] == capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 5, mats, rig["deltas"], tw).tobytes()
    assert got[0] == got[2] and got[0] != got[1]
    r.close(); sb.close()


def test_a_nan_matrix_propagates_refit_refuses_and_a_finite_pose_recovers(pkg, device, cornell_scene):
    capi, S = pkg.capi, pkg.scenes
    scene = cornell_scene
    rig = S.make_rig(scene, 4, 4, 2, seed=0)
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, 48, 27, pool_paths=2048)
    r.bind_scene(sb)
    pose = capi.Pose(r, rig["rest"], rig["joints"], rig["weights"], 4, rig["deltas"])
    mats, tw = S.rig_pose(rig, 0.3)
    bad = mats.copy(); bad[1, 5] = np.nan
    pose.update(bad, tw)
    got = sb.verts.read(np.float32).reshape(-1, 3)
    want = capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 4, bad, rig["deltas"], tw)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() and not np.isnan(got).all()
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    with pytest.raises(capi.GmuptError) as e:
        r.refit()
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    pose.update(mats, tw)
    r.refit()
    moved = S.refit_scene(scene, capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 4, mats, rig["deltas"], tw))
    assert sb.verts.read(np.float32).tobytes() == moved["verts"].tobytes()
    assert sb.nodes.read(capi.bvh_node_dtype).tobytes() == moved["nodes"].tobytes()
    r.close(); sb.close()


def test_errors_create_no_handle_and_leave_the_buffer_unchanged(pkg, device):
    capi, S = pkg.capi, pkg.scenes
    V, K, J, T = 257, 4, 3, 1
    scene, scene2 = soup_scene(S, V), soup_scene(S, 65)
    rig = rig_for(V, K, J, T, 3)
    rig["weights"][rig["weights"] == 0] = 0.25
    rig["joints"][:] %= J
    sb, sb2 = capi.SceneBuffers(device, scene), capi.SceneBuffers(device, scene2)
    r = capi.Renderer(device, 16, 9, pool_paths=1024)
    verts0 = scene["verts"].tobytes()
    with pytest.raises(capi.GmuptError) as e:
        make_pose(capi, r, rig)                                                  # nothing bound
    assert e.value.code == capi.ERR_NOT_BOUND
    r.bind_scene(sb)
    bad = dict(rig, joints=rig["joints"].copy()); bad["joints"][100, 2] = J
    with pytest.raises(capi.GmuptError) as e:
        make_pose(capi, r, bad)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and not r._poses and sb.verts.read(np.float32).tobytes() == verts0
    ok = dict(bad, weights=rig["weights"].copy()); ok["weights"][100, 2] = -0.0      # the same joint number behind a weight of zero
    pose = make_pose(capi, r, ok)
    with pytest.raises(capi.GmuptError) as e:
        capi.Pose(r, rig["rest"], None, None, 0, None)                          # neither joints nor targets
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    # a rebind to a scene with another vertex count: update refuses and writes nothing
    r.bind_scene(sb2)
    for mats in (rig["mats"], cuda(device, rig["mats"])):
        with pytest.raises(capi.GmuptError) as e:
            pose.update(mats, rig["target_weights"])
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    r.synchronize()
    assert sb.verts.read(np.float32).tobytes() == verts0 and sb2.verts.read(np.float32).tobytes() == scene2["verts"].tobytes()
    r.bind_scene(sb)                                                             # back: the handle works on what is bound now
    pose.update(rig["mats"], rig["target_weights"])
    assert PS.differing(sb.verts.read(np.float32), PS.host(capi, ok)) == 0
    r.close(); sb.close(); sb2.close()
    assert not pose.h


@pytest.fixture(scope="module")
def e2e(pkg, cornell_scene):
    """The Cornell box with a make_rig rig and one pose of it: the index list, the rig, the pose, the oracle's scene on the host rule's
    vertices and normals, and the oracle's frame of the UNPOSED scene -- each built once."""
    S, capi = pkg.scenes, pkg.capi
    scene = cornell_scene
    idx = np.ascontiguousarray(S.cornell_mesh()["indices"], np.int32)
    rig = S.make_rig(scene, 4, 4, 2, seed=0)
    mats, tw = S.rig_pose(rig, 0.3)
    verts = capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 4, mats, rig["deltas"], tw)
    moved = S.refit_scene(scene, verts, capi.vertex_normals_host(verts, idx))
    W, H, P, iters = 48, 27, 2048, 12
    orc = O.Renderer(scene, W, H, P, threads=8)
    cam = O.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    for _ in range(iters):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    unposed = orc.framebuffer().copy()
    orc.close()
    return idx, rig, mats, tw, moved, unposed


@pytest.mark.parametrize("kernel", ["wide", "cast0"])
def test_session_set_pose_equals_the_oracle(pkg, device, monkeypatch, cornell_scene, e2e, kernel):
    monkeypatch.setenv("GMUPT_TRAVERSAL", kernel)
    capi = pkg.capi
    W, H, P, iters = 48, 27, 2048, 12
    idx, rig, mats, tw, moved, unposed = e2e
    orc, hip, ocam, hcam, sb = PU.make_pair(pkg, device, cornell_scene, W, H, P)
    orc.close()
    orc = O.Renderer(moved, W, H, P, threads=8)
    sess = pkg.progressive.ProgressiveSession(hip, hcam, W, H, preview_every=0)
    pose = capi.Pose(hip, rig["rest"], rig["joints"], rig["weights"], 4, rig["deltas"])
    info = sess.set_pose(sb, pose, mats, tw, normals="smooth", indices=idx)
    assert "rebuilt" in info and hcam.buffer.iterationCounter == -1
    ocam.buffer.iterationCounter = -1
    assert sb.verts.read(np.float32).tobytes() == moved["verts"].tobytes()
    assert sb.props.read(capi.tri_props_dtype).tobytes() == moved["props"].tobytes()
    for it in range(iters):
        PU.step_both(orc, hip, ocam, hcam)
        if it < 2 or it == iters - 1:
            bad = PU.compare_state(orc, hip, P, P)
            assert not bad, "iteration %d: path state differs: %r" % (it, bad[:4])
            assert np.array_equal(orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32)), "iteration %d: framebuffer differs" % it
    fb = hip.framebuffer()
    assert int(fb[..., 3].view(np.uint32).sum()) > 0
    assert not np.array_equal(fb.view(np.uint32), unposed.view(np.uint32)), "the posed frame equals the unposed one"
    assert bool(hip.stats().flags & capi.STAT_CAST_WIDE) == (kernel == "wide")
    sess.close()
    assert pose.h, "the session does not own the Pose"
    hip.close(); sb.close(); orc.close()
    assert not pose.h


def test_set_pose_rebuild_policy_returns_the_keys_of_set_vertices(pkg, device, cornell_scene):
    capi, S = pkg.capi, pkg.scenes
    scene = cornell_scene
    rig = S.make_rig(scene, 4, 4, 2, seed=0)
    mats, tw = S.rig_pose(rig, 0.3)
    verts = capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 4, mats, rig["deltas"], tw)
    infos = []
    for posed in (False, True):
        sb = capi.SceneBuffers(device, scene)
        r = capi.Renderer(device, 48, 27, pool_paths=2048)
        r.bind_scene(sb)
        cam = capi.Camera(48, 27); cam.set_pose(*scene["camera"])
        sess = pkg.progressive.ProgressiveSession(r, cam, 48, 27, preview_every=0)
        if posed:
            pose = capi.Pose(r, rig["rest"], rig["joints"], rig["weights"], 4, rig["deltas"])
            infos.append(sess.set_pose(sb, pose, cuda(device, mats), cuda(device, tw), rebuild_above=1.5))
            with pytest.raises(ValueError):
                sess.set_pose(sb, pose, mats, tw, normals="flat")
        else:
            infos.append(sess.set_vertices(sb, verts, rebuild_above=1.5))
        assert sb.verts.read(np.float32).tobytes() == verts.tobytes()
        sess.close(); cam.close(); r.close(); sb.close()
    assert sorted(infos[0]) == sorted(infos[1]) and {"cost", "baseline", "candidate_cost", "tree_rebuilt"} <= set(infos[1])
    for k in ("cost", "baseline", "candidate_cost", "tree_rebuilt", "rebuilt"):
        assert infos[0][k] == infos[1][k], k

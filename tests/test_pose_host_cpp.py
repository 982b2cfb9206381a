"""The C++ host path of the pose stage: Scene::loadRig + Renderer::poseScene through gmupt_render --rig FILE --pose FILE --smooth-normals,
against the CPU oracle on the Cornell box posed by gmupt_pose_host with the normals of gmupt_vertex_normals_host -- the frames are equal
bit for bit."""
import os
import subprocess

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "host")
EXE = os.path.join(HOST, "gmupt_render")


@pytest.fixture(scope="module")
def exe(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    return EXE


def test_help_lists_the_options(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--rig" in out and "--pose" in out


def test_pose_without_rig_is_refused(exe):
    r = subprocess.run([exe, "--scene", "cornell", "--pose", "pose.f32"], capture_output=True, text=True)          # refused before a device is opened
    assert r.returncode != 0 and "--rig" in r.stderr


def test_pose_with_vertices_is_refused(exe):
    r = subprocess.run([exe, "--scene", "cornell", "--rig", "rig.grig", "--pose", "pose.f32", "--vertices", "moved.f32"], capture_output=True, text=True)
    assert r.returncode != 0 and "--vertices" in r.stderr and "--pose" in r.stderr


@pytest.mark.gpu
def test_cpp_pose_equals_the_oracle(exe, pkg, oracle, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    S, capi = pkg.scenes, pkg.capi
    W, H, P, frames = 48, 27, 2048, 12
    scene = cornell_scene
    rig = S.make_rig(scene, 4, 4, 2, seed=0)
    mats, tw = S.rig_pose(rig, 0.3)
    S.save_grig(rig, str(tmp_path / "cornell.grig"))
    np.concatenate([mats.reshape(-1), tw]).astype("<f4").tofile(str(tmp_path / "pose.f32"))
    args = [exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P)]
    posed_args = args + ["--rig", str(tmp_path / "cornell.grig"), "--pose", str(tmp_path / "pose.f32"), "--smooth-normals"]
    subprocess.run(posed_args + ["--dump", str(tmp_path / "posed.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path))
    subprocess.run(args + ["--dump", str(tmp_path / "rest.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path))
    verts = capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 4, mats, rig["deltas"], tw)
    moved = S.refit_scene(scene, verts, capi.vertex_normals_host(verts, S.cornell_mesh()["indices"]))
    orc = oracle.Renderer(moved, W, H, P, live=P, threads=8)
    cam = oracle.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    cam.buffer.iterationCounter = -1
    for _ in range(frames):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    fb = orc.framebuffer().copy()
    orc.close()
    posed = np.fromfile(str(tmp_path / "posed.f32"), "<f4").reshape(H, W, 4)
    assert int(posed[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(posed.view(np.uint32), fb.view(np.uint32)), "the C++ path's frame differs from the oracle's on the host rule's pose"
    rest = np.fromfile(str(tmp_path / "rest.f32"), "<f4").reshape(H, W, 4)
    assert not np.array_equal(rest.view(np.uint32), posed.view(np.uint32)), "without --rig / --pose the loaded pose stays"
    # a pose file of the wrong length is refused
    np.zeros(5, "<f4").tofile(str(tmp_path / "short.f32"))
    r = subprocess.run(args + ["--rig", str(tmp_path / "cornell.grig"), "--pose", str(tmp_path / "short.f32")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "floats" in r.stderr

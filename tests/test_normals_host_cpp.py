"""The C++ host path of the smooth normals: Scene::setVertices + Renderer::refitScene(.., smoothNormals) through
gmupt_render --vertices FILE --smooth-normals, against the CPU oracle on the moved Cornell box with the normals of gmupt_vertex_normals_host
-- the frames are equal bit for bit."""
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


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--smooth-normals" in out


def test_smooth_normals_without_vertices_is_refused(exe):
    r = subprocess.run([exe, "--scene", "cornell", "--smooth-normals"], capture_output=True, text=True)    # refused before a device is opened
    assert r.returncode != 0 and "--vertices" in r.stderr


@pytest.mark.gpu
def test_cpp_smooth_normals_equal_the_oracle(exe, pkg, oracle, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    W, H, P, frames = 48, 27, 2048, 12
    scene = cornell_scene
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    w.astype("<f4").tofile(str(tmp_path / "moved.f32"))
    args = [exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
            "--vertices", str(tmp_path / "moved.f32")]
    subprocess.run(args + ["--smooth-normals", "--dump", str(tmp_path / "smooth.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path))
    subprocess.run(args + ["--dump", str(tmp_path / "stale.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path))
    indices = pkg.scenes.cornell_mesh()["indices"]
    moved = pkg.scenes.refit_scene(scene, w, pkg.capi.vertex_normals_host(w, indices))
    orc = oracle.Renderer(moved, W, H, P, live=P, threads=8)
    cam = oracle.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    cam.buffer.iterationCounter = -1
    for _ in range(frames):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    fb = orc.framebuffer().copy()
    orc.close()
    smooth = np.fromfile(str(tmp_path / "smooth.f32"), "<f4").reshape(H, W, 4)
    assert int(smooth[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(smooth.view(np.uint32), fb.view(np.uint32)), "the C++ path's frame differs from the oracle's on the host rule's normals"
    stale = np.fromfile(str(tmp_path / "stale.f32"), "<f4").reshape(H, W, 4)
    assert not np.array_equal(stale.view(np.uint32), smooth.view(np.uint32)), "without --smooth-normals the loader's normals stay"

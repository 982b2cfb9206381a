"""The C++ host path of the refit: Scene::setVertices + Renderer::refitScene through gmupt_render --vertices FILE, against the Python path
(capi: update the vertex buffer, refit) on the same moved Cornell box -- the frames are equal bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "host")
EXE = os.path.join(HOST, "gmupt_render")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    return EXE


def read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip(); w, h = map(int, f.readline().split()); scale = float(f.readline())
        assert kind == b"PF" and scale < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1]


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--vertices FILE" in out


@pytest.mark.gpu
def test_wrong_vertex_count_is_a_runtime_error(exe, tmp_path):
    np.zeros(9, "<f4").tofile(str(tmp_path / "few.f32"))
    r = subprocess.run([exe, "--scene", "cornell", "--size", "32x18", "--frames", "1", "--pool", "1024", "--live", "1024",
                        "--vertices", str(tmp_path / "few.f32")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "setVertices" in r.stderr


@pytest.mark.gpu
def test_cpp_set_vertices_and_refit_equal_the_python_path(exe, pkg, device, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    W, H, P, frames = 48, 27, 2048, 24
    scene = cornell_scene
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    w.astype("<f4").tofile(str(tmp_path / "moved.f32"))
    run = subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--vertices", str(tmp_path / "moved.f32"), "--pfm", str(tmp_path / "cpp.pfm"), "--dump", str(tmp_path / "cpp.f32")],
                         check=True, capture_output=True, text=True, cwd=str(tmp_path))
    info = json.loads([l for l in run.stdout.splitlines() if l.startswith('{"refit"')][0])["refit"]
    assert info["rebuilt"] == 0 and info["levels"] >= 1 and info["opened_nodes"] >= 1
    # the Python path: bound to the original scene, vertices updated, refitted
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
    r.bind_scene(sb)
    sb.verts.update(w)
    assert r.refit()["rebuilt"] == 0
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    cam.reset_accumulation()
    for _ in range(frames):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    fb = r.framebuffer()
    cpp = np.fromfile(str(tmp_path / "cpp.f32"), "<f4").reshape(H, W, 4)
    assert np.array_equal(cpp.view(np.uint32), fb.view(np.uint32)), "the C++ path's frame differs from the Python path's"
    assert np.array_equal(read_pfm(str(tmp_path / "cpp.pfm")).view(np.uint32), fb[..., :3].view(np.uint32))
    # and it is not the unmoved scene's frame
    still = subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                            "--dump", str(tmp_path / "still.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path))
    assert not np.array_equal(np.fromfile(str(tmp_path / "still.f32"), "<f4").view(np.uint32), cpp.reshape(-1).view(np.uint32))
    cam.close(); r.close(); sb.close()

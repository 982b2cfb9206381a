"""The C++ host path of the LBVH: BVHWrapper::buildLBVH through gmupt_render --build-only --builder lbvh against gmupt_lbvh_build_host (bit
for bit, no GPU), and Scene::rebuildOnDevice + Renderer::bindScene through gmupt_render --builder lbvh on a small generated glTF against
the oracle on the tree gmupt_lbvh_build_host gives for the loader's mesh."""
import json
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


@pytest.fixture()
def gltf(pkg, tmp_path):
    """(path, the mesh as saved, the mesh as the C++ loader reads it with the camera / lights of the saved one)."""
    path = str(tmp_path / "soup.gltf")
    mesh = pkg.scenes.save_gltf(pkg.scenes.random_triangles_mesh(700, seed=21), path)
    return path, mesh


def loaded_mesh(exe, pkg, path, mesh, tmp_path, extra=()):
    dump = str(tmp_path / "loaded.gmesh")
    out = json.loads(subprocess.run([exe, "--build-only", "--scene", path, "--dump-mesh", dump, *extra], check=True, capture_output=True, text=True).stdout)
    loaded = dict(pkg.scenes.load_gmesh(dump))
    for k in ("lights", "light_count", "camera", "name"):
        loaded[k] = mesh[k]
    return out, loaded


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--builder sbvh|lbvh" in out and "--leaf L" in out


def test_unknown_builder_is_a_usage_error(exe):
    r = subprocess.run([exe, "--builder", "kd"], capture_output=True, text=True)
    assert r.returncode == 2 and "sbvh or lbvh" in r.stderr


@pytest.mark.parametrize("L", [1, 4])
def test_build_lbvh_equals_the_host_reference(exe, pkg, gltf, tmp_path, L):
    path, mesh = gltf
    tree = str(tmp_path / "tree.bin")
    out, loaded = loaded_mesh(exe, pkg, path, mesh, tmp_path, ("--builder", "lbvh", "--leaf", str(L), "--dump-tree", tree))
    want = pkg.capi.lbvh_build_host(loaded["verts"], loaded["indices"], loaded["vertex_material"], L)
    assert out["nodes"] == len(want["nodes"]) and out["references"] == len(want["tris"]) == out["triangles"] == 700
    raw = open(tree, "rb").read()
    assert raw == want["nodes"].tobytes() + want["tris"].tobytes()
    # and the default stays the SBVH
    sbvh, _ = loaded_mesh(exe, pkg, path, mesh, tmp_path)
    ref = pkg.scenes.build_scene(loaded)
    assert sbvh["nodes"] == len(ref["nodes"]) and sbvh["references"] == len(ref["tris"]) and sbvh["sah"] > 0


@pytest.mark.parametrize("leaf", ["65", "0", "abc"])
def test_a_bad_leaf_size_is_a_usage_error(exe, leaf):
    r = subprocess.run([exe, "--build-only", "--scene", "cornell", "--builder", "lbvh", "--leaf", leaf], capture_output=True, text=True)
    assert r.returncode == 2 and "1..64" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("L", [4, 1])
def test_cpp_rebuild_on_device_equals_the_oracle(exe, pkg, oracle, gltf, tmp_path, monkeypatch, L):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    path, mesh = gltf
    W, H, P, frames = 48, 27, 2048, 16
    run = subprocess.run([exe, "--scene", path, "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--builder", "lbvh", "--leaf", str(L), "--dump", str(tmp_path / "cpp.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path))
    info = json.loads([l for l in run.stdout.splitlines() if l.startswith('{"lbvh"')][0])["lbvh"]
    _, loaded = loaded_mesh(exe, pkg, path, mesh, tmp_path)
    scene = pkg.scenes.build_scene(loaded, builder="lbvh", max_leaf_size=L)
    assert info["num_nodes"] == len(scene["nodes"]) and info["num_tris"] == 700 and info["depth"] == scene["depth"] and info["ms"] > 0
    orc = oracle.Renderer(scene, W, H, P, threads=8)
    cam = oracle.Camera(W, H); cam.set_pose(*scene["camera"])
    for _ in range(frames):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    fb = orc.framebuffer().copy()
    orc.close()
    cpp = np.fromfile(str(tmp_path / "cpp.f32"), "<f4").reshape(H, W, 4)
    assert int(cpp[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(cpp.view(np.uint32), fb.view(np.uint32)), "the C++ path's frame on the GPU-built tree differs from the oracle's on the host reference tree"

"""The C++ host path of the treelet optimiser: BVHWrapper with optimizePasses through gmupt_render --build-only --builder lbvh --optimize N
--dump-tree against gmupt_tree_optimize_host of the plain dump (byte for byte, no GPU), and Scene::rebuildOnDevice +
BVHWrapper::optimizeOnDevice through gmupt_render --builder lbvh --optimize N on a small generated glTF against the oracle on that tree."""
import json
import os
import subprocess

import numpy as np
import pytest

import treeopt_util as TO

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "host")
EXE = os.path.join(HOST, "gmupt_render")


@pytest.fixture(scope="module")
def exe(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    return EXE


@pytest.fixture()
def gltf(pkg, tmp_path):
    path = str(tmp_path / "soup.gltf")
    mesh = pkg.scenes.save_gltf(pkg.scenes.random_triangles_mesh(700, seed=21), path)
    return path, mesh


def build_only(exe, pkg, path, mesh, tmp_path, extra=()):
    dump = str(tmp_path / "loaded.gmesh")
    out = json.loads(subprocess.run([exe, "--build-only", "--scene", path, "--dump-mesh", dump, *extra], check=True, capture_output=True, text=True).stdout)
    loaded = dict(pkg.scenes.load_gmesh(dump))
    for k in ("lights", "light_count", "camera", "name"):
        loaded[k] = mesh[k]
    return out, loaded


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--optimize N" in out


@pytest.mark.parametrize("passes", ["9", "-1", "abc"])
def test_a_bad_pass_count_is_a_usage_error(exe, passes):
    r = subprocess.run([exe, "--build-only", "--scene", "cornell", "--builder", "lbvh", "--optimize", passes], capture_output=True, text=True)
    assert r.returncode == 2 and "0..8" in r.stderr


def test_optimize_needs_the_lbvh_builder(exe):
    for extra in (["--build-only"], ["--frames", "1"]):
        r = subprocess.run([exe, "--scene", "cornell", "--optimize", "3", *extra], capture_output=True, text=True)
        assert r.returncode != 0 and ("LBVH" in r.stderr or "lbvh" in r.stderr), r.stderr


@pytest.mark.parametrize("L", [1, 4])
def test_build_only_dump_equals_the_host_rule_on_the_plain_dump(exe, pkg, gltf, tmp_path, L):
    capi = pkg.capi
    path, mesh = gltf
    plain, opt = str(tmp_path / "plain.bin"), str(tmp_path / "opt.bin")
    out0, _ = build_only(exe, pkg, path, mesh, tmp_path, ("--builder", "lbvh", "--leaf", str(L), "--dump-tree", plain))
    out3, _ = build_only(exe, pkg, path, mesh, tmp_path, ("--builder", "lbvh", "--leaf", str(L), "--optimize", "3", "--dump-tree", opt))
    out00, _ = build_only(exe, pkg, path, mesh, tmp_path, ("--builder", "lbvh", "--leaf", str(L), "--optimize", "0", "--dump-tree", str(tmp_path / "zero.bin")))
    n = out0["nodes"]
    assert out3["nodes"] == n and out3["references"] == out0["references"] == 700
    raw0, raw3 = open(plain, "rb").read(), open(opt, "rb").read()
    assert open(str(tmp_path / "zero.bin"), "rb").read() == raw0, "--optimize 0 is no optimiser"
    nodes0 = np.frombuffer(raw0[:n * 48], capi.bvh_node_dtype)
    want, info = capi.tree_optimize_host(nodes0, 3)
    assert info["treelets_rewritten"] > 0
    assert raw3[:n * 48] == want.tobytes(), "the dumped nodes are gmupt_tree_optimize_host of the plain dump"
    assert raw3[n * 48:] == raw0[n * 48:], "the triangle records are those of the plain build"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [4, 1])
def test_cpp_rebuild_with_optimize_equals_the_oracle(exe, pkg, oracle, gltf, tmp_path, monkeypatch, L):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    path, mesh = gltf
    W, H, P, frames = 48, 27, 2048, 16
    run = subprocess.run([exe, "--scene", path, "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--builder", "lbvh", "--leaf", str(L), "--optimize", "3", "--dump", str(tmp_path / "cpp.f32")], check=True, capture_output=True, text=True,
                         cwd=str(tmp_path))
    lines = run.stdout.splitlines()
    info = json.loads([l for l in lines if l.startswith('{"lbvh"')][0])["lbvh"]
    oinfo = json.loads([l for l in lines if l.startswith('{"optimize"')][0])["optimize"]
    _, loaded = build_only(exe, pkg, path, mesh, tmp_path)
    scene = pkg.scenes.build_scene(loaded, builder="lbvh", max_leaf_size=L, optimize=3)
    assert info["num_nodes"] == len(scene["nodes"]) and info["num_tris"] == 700 and info["depth"] == scene["depth"]
    assert oinfo["passes"] == 3 and oinfo["ms"] > 0 and not TO.info_differs(oinfo, scene["optimize"]), (oinfo, scene["optimize"])
    orc = oracle.Renderer(scene, W, H, P, threads=8)
    cam = oracle.Camera(W, H); cam.set_pose(*scene["camera"])
    for _ in range(frames):
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    fb = orc.framebuffer().copy()
    orc.close()
    cpp = np.fromfile(str(tmp_path / "cpp.f32"), "<f4").reshape(H, W, 4)
    assert int(cpp[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(cpp.view(np.uint32), fb.view(np.uint32)), "the C++ path's frame on the GPU-optimised tree differs from the oracle's on the host rule's tree"

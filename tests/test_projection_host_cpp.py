"""The C++ host path of the camera projections: Renderer::setProjection through gmupt_render --projection, whose frame equals the
Python binding's with the same projection, and the refused flag combinations."""
import json
import math
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


@pytest.mark.parametrize("args, word", [
    (["--projection", "fisheye:180", "--aperture", "0.3", "--focus", "3"], "--projection and --aperture do not combine"),
    (["--projection", "equirect", "--temporal", "t"], "cannot be combined with --temporal"),
    (["--projection", "ortho:8", "--denoise", "d", "--infill"], "cannot be combined with --infill"),
    (["--projection", "equirect", "--ranks", "2", "--rank", "0", "--no-gather"], "--projection sets the camera of a single process"),
    (["--projection", "cube"], "--projection takes ortho:H, fisheye:DEG or equirect"), (["--projection"], "missing value for --projection"),
    (["--projection", "ortho:0"], "finite height H > 0"), (["--projection", "ortho:nan"], "finite height H > 0"), (["--projection", "ortho:"], "finite height H > 0"),
    (["--projection", "fisheye:0"], "(0, 360] degrees"), (["--projection", "fisheye:361"], "(0, 360] degrees"), (["--projection", "fisheye:wide"], "(0, 360] degrees")])
def test_refused_flag_combinations(exe, tmp_path, args, word):
    r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, cwd=str(tmp_path))   # refused before a device is opened
    assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--projection ortho:H | fisheye:DEG | equirect" in out


@pytest.mark.gpu
def test_cpp_projection_frame_equals_the_python_path(exe, pkg, device, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    capi = pkg.capi
    W, H, P, frames = 32, 16, 2048, 12
    proj = capi.projection.projection_params(capi.projection.FISHEYE, fov=float(np.float32(150.0) * np.float32(0.0174532925)))
    sb = capi.SceneBuffers(device, cornell_scene)
    r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*cornell_scene["camera"]); cam.buffer.lightCount = cornell_scene["light_count"]
    capi.projection.set_projection(r, proj)
    for _ in range(frames):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    fb = r.framebuffer()
    r.close(); sb.close(); cam.close()
    out = subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--dump", str(tmp_path / "fb.f32"), "--projection", "fisheye:150"], check=True, capture_output=True, text=True, cwd=str(tmp_path)).stdout
    lines = [l for l in out.splitlines() if l.startswith('{"projection"')]
    assert len(lines) == 1, out
    got = json.loads(lines[0])["projection"]
    cfb = np.fromfile(str(tmp_path / "fb.f32"), "<f4").reshape(H, W, 4)
    assert got["kind"] == capi.projection.FISHEYE and got["fov_bits"] == "%08x" % int(np.float32(proj.fov).view(np.uint32)) and abs(got["fov"] - math.radians(150)) < 1e-6
    assert int(fb[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(cfb.view(np.uint32), fb.view(np.uint32)), "the C++ frame is the binding's frame"

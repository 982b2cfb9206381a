"""The C++ host path of the guided infill: Renderer::preview through gmupt_render --infill, combined with --denoise and --temporal,
against the Python path (capi.Renderer.preview) on the same progressive start of the Cornell box -- bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_refit_host_cpp import read_pfm

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "host")
EXE = os.path.join(HOST, "gmupt_render")


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    return EXE


def test_help_lists_the_option_and_it_needs_a_preview(exe, tmp_path):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--infill" in out and "Renderer::preview" in out
    res = subprocess.run([exe, "--scene", "cornell", "--size", "16x9", "--frames", "1", "--infill"], capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode != 0 and "--denoise PREFIX or --temporal PREFIX" in res.stdout + res.stderr


@pytest.mark.gpu
def test_cpp_infilled_previews_equal_the_python_path(exe, pkg, device, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    W, H, P, frames = 48, 27, 256, 3                        # a progressive start: most pixels have no sample yet
    scene = cornell_scene
    subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                    "--denoise", str(tmp_path / "dn"), "--temporal", str(tmp_path / "tp"), "--infill"], check=True, capture_output=True, text=True,
                   cwd=str(tmp_path))
    cpp_dn, cpp_tp = read_pfm(str(tmp_path / "dn.pfm")), read_pfm(str(tmp_path / "tp.pfm"))
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    cam.reset_accumulation()
    for _ in range(frames):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    fb = r.framebuffer()
    assert (fb[..., 3].view(np.uint32) == 0).mean() > 0.25, "there are holes to fill"
    py_dn = r.preview(aov_samples=1, infill=True).cpu().numpy()
    py_tp = r.preview(t, motion=True, aov_samples=1, infill=True).cpu().numpy()
    plain = r.denoise(1).cpu().numpy()
    assert np.array_equal(cpp_dn.view(np.uint32), py_dn[..., :3].view(np.uint32)), "--denoise --infill differs from the Python path's"
    assert np.array_equal(cpp_tp.view(np.uint32), py_tp[..., :3].view(np.uint32)), "--temporal --infill differs from the Python path's"
    assert (plain[..., :3].max(-1) == 0).sum() > (py_dn[..., :3].max(-1) == 0).sum(), "the infill filled pixels the filter leaves black"
    cam.close(); r.close(); sb.close()

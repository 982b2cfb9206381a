"""The C++ host path of motion-aware temporal reuse: Renderer::refitScene(keepHistory) + Renderer::denoiseTemporalMotion through
gmupt_render --vertices FILE --temporal PREFIX, against the Python path (capi) on the same moved Cornell box -- bit for bit."""
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


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--temporal PREFIX" in out and "denoiseTemporalMotion" in out


@pytest.mark.gpu
def test_cpp_temporal_preview_across_a_refit_equals_the_python_path(exe, pkg, device, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    W, H, P, frames = 48, 27, 512, 6
    scene = cornell_scene
    w = pkg.scenes.wobble(scene, 0.05, 0.05)
    w.astype("<f4").tofile(str(tmp_path / "moved.f32"))
    subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                    "--vertices", str(tmp_path / "moved.f32"), "--temporal", str(tmp_path / "tp")], check=True, capture_output=True, text=True,
                   cwd=str(tmp_path))
    cpp = read_pfm(str(tmp_path / "tp.pfm"))
    capi = pkg.capi
    sb = capi.SceneBuffers(device, scene)
    r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
    r.bind_scene(sb)
    t = capi.Temporal(r)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    cam.reset_accumulation()

    def run():
        for _ in range(frames):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    run()
    r.denoise_temporal_motion(t, 1)
    sb.verts.update(w); r.refit(); cam.reset_accumulation()
    run()
    py = r.denoise_temporal_motion(t, 1).cpu().numpy()
    assert np.array_equal(cpp.view(np.uint32), py[..., :3].view(np.uint32)), "the C++ preview differs from the Python path's"
    assert not np.array_equal(py.view(np.uint32)[..., :3], r.denoise(1).cpu().numpy().view(np.uint32)[..., :3]), "the history was kept"
    cam.close(); r.close(); sb.close()

"""The C++ host path of the thin lens: Renderer::setLens / focusAt through gmupt_render --aperture R --focus D | --focus-at X,Y, whose
frame equals the Python binding's with the same lens, and the usage errors of the options."""
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


def test_help_lists_the_options(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    for opt in ("--aperture", "--focus D", "--focus-at X,Y", "pinhole centre ray"):
        assert opt in out, opt


@pytest.mark.parametrize("args, word", [
    (["--aperture", "0.3"], "exactly one of --focus D and --focus-at X,Y"), (["--focus", "3"], "which need it"), (["--focus-at", "1,1"], "which need it"),
    (["--aperture", "0.3", "--focus", "3", "--focus-at", "1,1"], "exactly one of"),
    (["--aperture", "0", "--focus", "3"], "--aperture takes a finite radius > 0"), (["--aperture", "nan", "--focus", "3"], "--aperture takes a finite radius > 0"),
    (["--aperture", "inf", "--focus", "3"], "--aperture takes a finite radius > 0"), (["--aperture", "-1", "--focus", "3"], "--aperture takes a finite radius > 0"),
    (["--aperture", "0.3", "--focus", "0"], "--focus takes a finite distance > 0"), (["--aperture", "0.3", "--focus", "far"], "--focus takes a finite distance > 0"),
    (["--aperture", "0.3", "--focus-at", "7"], "--focus-at takes a pixel X,Y"), (["--aperture"], "missing value for --aperture"),
    (["--aperture", "0.3", "--focus", "3", "--ranks", "2", "--rank", "0", "--no-gather"], "--aperture sets the lens of a single process")])
def test_usage_errors(exe, tmp_path, args, word):
    r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, cwd=str(tmp_path))   # refused before a device is opened
    assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


def run(exe, tmp_path, W, H, P, frames, extra):
    out = subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--dump", str(tmp_path / "fb.f32")] + extra, check=True, capture_output=True, text=True, cwd=str(tmp_path)).stdout
    lines = [l for l in out.splitlines() if l.startswith('{"lens"')]
    assert len(lines) == 1, out
    return json.loads(lines[0])["lens"], np.fromfile(str(tmp_path / "fb.f32"), "<f4").reshape(H, W, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["focus", "focus_at"])
def test_cpp_lens_frame_equals_the_python_path(exe, pkg, device, cornell_scene, tmp_path, monkeypatch, how):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    capi = pkg.capi
    W, H, P, frames, aperture = 32, 18, 2048, 12, 0.3
    sb = capi.SceneBuffers(device, cornell_scene)
    r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*cornell_scene["camera"]); cam.buffer.lightCount = cornell_scene["light_count"]
    if how == "focus":
        lens = capi.lens.lens_params(aperture_radius=aperture, focus_distance=11.5)
        extra = ["--aperture", repr(aperture), "--focus", "11.5"]
    else:   # the driver updates the camera once, focuses on the pixel, and restarts the accumulation
        cam.update(0.0); r.set_camera(cam.buffer)
        lens = capi.lens.focus_at(r, 18, 4, int(cam.buffer.lightCount), aperture_radius=aperture)
        cam.reset_accumulation()
        extra = ["--aperture", repr(aperture), "--focus-at", "18,4"]
    capi.lens.set_lens(r, lens)
    for _ in range(frames):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    fb = r.framebuffer()
    r.close(); sb.close(); cam.close()
    got, cfb = run(exe, tmp_path, W, H, P, frames, extra)
    print("C++ lens %r; Python lens (%r, %r)" % (got, lens.aperture_radius, lens.focus_distance))
    word = lambda x: "%08x" % int(np.float32(x).view(np.uint32))
    assert got["aperture_bits"] == word(lens.aperture_radius) and got["focus_bits"] == word(lens.focus_distance)
    assert int(fb[..., 3].view(np.uint32).sum()) > 0
    assert np.array_equal(cfb.view(np.uint32), fb.view(np.uint32)), "the C++ frame is the binding's frame"

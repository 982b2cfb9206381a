"""The C++ host path of the convergence monitor: Renderer::renderUntil through gmupt_render --until-error, whose JSON line and error map
equal gmupt_converge_host chained over the same checks of the same frames (rendered again through the Python binding), and the usage
errors of the options."""
import json
import os
import subprocess

import numpy as np
import pytest

import converge_util as CU

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "host")
EXE = os.path.join(HOST, "gmupt_render")


@pytest.fixture(scope="module")
def exe(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    return EXE


def test_help_lists_the_options(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    for opt in ("--until-error", "--check-every", "--allow-pixels", "--error-map"):
        assert opt in out, opt


@pytest.mark.parametrize("args, word", [
    (["--check-every", "4"], "they need --until-error T"), (["--allow-pixels", "3"], "they need --until-error T"), (["--error-map", "e.pfm"], "they need --until-error T"),
    (["--until-error", "0.1", "--check-every", "0"], "--check-every takes a number of frames >= 1"),
    (["--until-error", "0.1", "--check-every", "x"], "--check-every takes a number of frames >= 1"),
    (["--until-error", "nan"], "--until-error takes a threshold >= 0"), (["--until-error", "-1"], "--until-error takes a threshold >= 0"),
    (["--until-error", "abc"], "--until-error takes a threshold >= 0"),
    (["--until-error", "0.1", "--allow-pixels", "many"], "--allow-pixels takes a number of pixels"), (["--until-error"], "missing value for --until-error"),
    (["--until-error", "0.1", "--ranks", "2", "--rank", "0", "--no-gather"], "--until-error judges the frame of a single process")])
def test_usage_errors(exe, tmp_path, args, word):
    r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, cwd=str(tmp_path))   # refused before a device is opened
    assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
    assert not (tmp_path / "e.pfm").exists()


def read_pf(path, W, H):
    raw = open(path, "rb").read()
    head = b"Pf\n%d %d\n-1.0\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 4
    return np.frombuffer(raw[len(head):], "<f4").reshape(H, W)[::-1]


def run(exe, tmp_path, W, H, P, frames, extra):
    out = subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--error-map", str(tmp_path / "err.pfm"), "--dump", str(tmp_path / "fb.f32")] + extra,
                         check=True, capture_output=True, text=True, cwd=str(tmp_path)).stdout
    lines = [l for l in out.splitlines() if l.startswith('{"converge"')]
    assert len(lines) == 1, out
    return json.loads(lines[0])["converge"], read_pf(str(tmp_path / "err.pfm"), W, H), np.fromfile(str(tmp_path / "fb.f32"), "<f4").reshape(H, W, 4)


@pytest.mark.gpu
def test_cpp_render_until_equals_the_host_rule(exe, pkg, device, cornell_scene, tmp_path, monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    capi = pkg.capi
    W, H, P, every = 32, 18, 2048, 8
    # the same frames through the Python binding: the host rule chained over a check every 8 frames
    sb = capi.SceneBuffers(device, cornell_scene)
    r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*cornell_scene["camera"]); cam.buffer.lightCount = cornell_scene["light_count"]
    state = np.zeros((H, W), capi.converge_pixel_dtype)
    checks = []
    for _ in range(5):
        for _ in range(every):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        fb = r.framebuffer()
        info, err = capi.converge_host(state, fb, error=True, threshold=0.0)
        checks.append((fb, err, info, state.copy()))
    r.close(); sb.close(); cam.close()

    def same(got, plane, fb, k, prm):
        want_fb, _, _, _ = checks[k - 1]
        assert np.array_equal(fb.view(np.uint32), want_fb.view(np.uint32)), "the C++ frames are the binding's frames"
        st = checks[k - 2][3].copy() if k > 1 else np.zeros((H, W), capi.converge_pixel_dtype)
        info, err = capi.converge_host(st, want_fb, error=True, **prm)          # check k under the run's own parameters
        assert got["iterations"] == k * every and got["converged"] == int(info["converged"])
        for name in ("pixels", "unsampled", "known", "nonfinite", "below"):
            assert got[name] == info[name], name
        assert int(got["max_error"], 16) == int(CU.bits(np.float32(info["max_error"]))[0])
        assert int(got["sum_error"], 16) == int(CU.bits(np.float64(info["sum_error"]))[0]) and int(got["mean_error"], 16) == int(CU.bits(np.float64(info["mean_error"]))[0])
        assert got["ms"] > 0 and CU.fenced_equal(np.ascontiguousarray(plane), err, True)
        return info

    # threshold 0: runs out of frames at the third check
    got, plane, fb = run(exe, tmp_path, W, H, P, 24, ["--until-error", "0", "--check-every", str(every)])
    assert got["converged"] == 0
    same(got, plane, fb, 3, dict(threshold=0.0))
    # a threshold the fourth check meets and the third does not: stops there
    e3, e4 = checks[2][2]["max_error"], checks[3][2]["max_error"]
    assert e4 < e3, "the estimate falls between these checks"
    got, plane, fb = run(exe, tmp_path, W, H, P, 400, ["--until-error", repr(float(np.float32(e4))), "--check-every", str(every)])
    k = got["iterations"] // every
    assert 2 <= k <= 4 and got["converged"] == 1
    same(got, plane, fb, k, dict(threshold=float(np.float32(e4))))
    # allow_pixels: all but the worst pixels of the second check
    thr = float(np.median(checks[1][1]))
    allow = W * H - int(((checks[1][1] >= 0) & (checks[1][1] <= np.float32(thr))).sum())   # the worse half and the pixels still unknown then
    got, plane, fb = run(exe, tmp_path, W, H, P, 400, ["--until-error", repr(thr), "--check-every", str(every), "--allow-pixels", str(allow)])
    assert got["iterations"] == 2 * every and got["converged"] == 1 and got["pixels"] - got["below"] <= allow
    same(got, plane, fb, 2, dict(threshold=thr, allow_pixels=allow))
    # fewer frames than one check: every pixel unknown
    got, plane, _ = run(exe, tmp_path, W, H, P, 5, ["--until-error", "0.1"])
    assert got["iterations"] == 5 and got["pixels"] == 0 and (plane == -1.0).all()

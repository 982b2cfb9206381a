"""The C++ host path of adaptive sampling: Renderer::renderAdaptive through gmupt_render --until-error T --adaptive, whose JSON line and
frame equal the host rules (gmupt_converge_host, gmupt_adaptive_select_host) chained over the same checks of the same frames, rendered
again through the Python binding with the host's lists attached; and the usage errors of the options."""
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
    for opt in ("--adaptive", "--max-repeat", "--uniform-every", "paths_generated"):
        assert opt in out, opt


@pytest.mark.parametrize("args, word", [
    (["--adaptive"], "it needs --until-error T with a finite T > 0"), (["--until-error", "0", "--adaptive"], "it needs --until-error T with a finite T > 0"),
    (["--until-error", "inf", "--adaptive"], "it needs --until-error T with a finite T > 0"),
    (["--until-error", "0.1", "--max-repeat", "3"], "they need --adaptive"), (["--until-error", "0.1", "--uniform-every", "3"], "they need --adaptive"),
    (["--until-error", "0.1", "--adaptive", "--max-repeat", "0"], "--max-repeat takes a number in 1..64"),
    (["--until-error", "0.1", "--adaptive", "--max-repeat", "65"], "--max-repeat takes a number in 1..64"),
    (["--until-error", "0.1", "--adaptive", "--max-repeat", "x"], "--max-repeat takes a number in 1..64"),
    (["--until-error", "0.1", "--adaptive", "--uniform-every", "often"], "--uniform-every takes a number of paths"),
    (["--until-error", "0.1", "--adaptive", "--max-repeat"], "missing value for --max-repeat"),
    (["--until-error", "0.1", "--adaptive", "--ranks", "2", "--rank", "0", "--no-gather"], "--until-error judges the frame of a single process")])
def test_usage_errors(exe, tmp_path, args, word):
    r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, cwd=str(tmp_path))   # refused before a device is opened
    assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


def run(exe, tmp_path, W, H, P, frames, extra):
    out = subprocess.run([exe, "--scene", "cornell", "--size", "%dx%d" % (W, H), "--frames", str(frames), "--pool", str(P), "--live", str(P),
                          "--dump", str(tmp_path / "fb.f32")] + extra, check=True, capture_output=True, text=True, cwd=str(tmp_path)).stdout
    lines = [l for l in out.splitlines() if l.startswith('{"converge"')]
    assert len(lines) == 1, out
    return json.loads(lines[0])["converge"], np.fromfile(str(tmp_path / "fb.f32"), "<f4").reshape(H, W, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("uniform_every", [0, 5])
def test_cpp_render_adaptive_equals_the_host_rules(exe, pkg, device, cornell_scene, tmp_path, monkeypatch, uniform_every):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")
    capi = pkg.capi
    W, H, P, every, max_repeat, frames = 32, 18, 2048, 8, 8, 80

    def renderer():
        sb = capi.SceneBuffers(device, cornell_scene)
        r = capi.Renderer(device, W, H, pool_paths=P, live_paths=P)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*cornell_scene["camera"]); cam.buffer.lightCount = cornell_scene["light_count"]
        return r, sb, cam

    def step(r, cam):
        for _ in range(every):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()

    # the threshold: what a uniform run reaches at its fourth check; the pixels that never get a sample are allowed for
    r, sb, cam = renderer()
    state = np.zeros((H, W), capi.converge_pixel_dtype)
    for _ in range(4):
        step(r, cam)
        info = capi.converge_host(state, r.framebuffer())
    thr, allow = float(np.float32(info["max_error"])), info["pixels"] - info["known"]
    r.close(); sb.close(); cam.close()
    assert thr > 0
    # the loop through the binding, every decision taken by the host rules
    r, sb, cam = renderer()
    plan = capi.adaptive.Adaptive(r)
    state = np.zeros((H, W), capi.converge_pixel_dtype)
    ran, last_plan = 0, None
    while ran < frames:
        step(r, cam); ran += every
        fb = r.framebuffer()
        info, err = capi.converge_host(state, fb, error=True, threshold=thr, allow_pixels=allow)
        if info["converged"]:
            break
        lst, last_plan = capi.adaptive.adaptive_select_host(err, threshold=thr, max_repeat=max_repeat)
        plan.set_list(lst, W, H, uniform_every=uniform_every)
        capi.adaptive.set_adaptive(r, plan)
    r.synchronize()
    paths = r.stats().paths_generated
    r.close(); sb.close(); cam.close()
    assert last_plan is not None and last_plan["entries"] > 0, "at least one plan was made"
    got, cfb = run(exe, tmp_path, W, H, P, frames, ["--until-error", repr(thr), "--check-every", str(every), "--allow-pixels", str(allow), "--adaptive",
                                                   "--max-repeat", str(max_repeat), "--uniform-every", str(uniform_every)])
    print("C++: %r; host chain: %d frames, plan %r, %d paths" % (got, ran, last_plan, paths))
    assert np.array_equal(cfb.view(np.uint32), fb.view(np.uint32)), "the C++ frame is the frame of the host rules chained"
    assert got["iterations"] == ran and got["converged"] == int(info["converged"])
    for name in ("pixels", "unsampled", "known", "nonfinite", "below"):
        assert got[name] == info[name], name
    assert int(got["max_error"], 16) == int(CU.bits(np.float32(info["max_error"]))[0])
    assert int(got["sum_error"], 16) == int(CU.bits(np.float64(info["sum_error"]))[0])
    for name in ("active", "entries", "max_rep", "skipped_nonfinite"):
        assert got[name] == last_plan[name], name
    assert got["paths_generated"] == paths
    # without --adaptive the line is the one it was
    plain, _ = run(exe, tmp_path, W, H, P, 16, ["--until-error", repr(thr), "--check-every", str(every)])
    assert "active" not in plain and "paths_generated" not in plain

"""The C++ host path of the tree cost: Renderer::treeCost through gmupt_render --tree-cost, whose hex fields equal gmupt_tree_cost_host on the
same tree -- the Cornell box as loaded, and after --vertices FILE has been applied."""
import json
import os
import subprocess

import numpy as np
import pytest

import treecost_util as TU

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gmu-path-tracer_amd", "host")
EXE = os.path.join(HOST, "gmupt_render")


@pytest.fixture(scope="module")
def exe(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    return EXE


def test_help_lists_the_option(exe):
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--tree-cost" in out


def test_tree_cost_with_ranks_is_refused(exe):
    r = subprocess.run([exe, "--scene", "cornell", "--tree-cost", "--ranks", "2", "--rank", "0", "--no-gather"], capture_output=True, text=True)   # refused before a device is opened
    assert r.returncode != 0 and "--tree-cost" in r.stderr


def printed(stdout):
    """when -> the fields of the tree_cost lines, the hex strings as uint64 bit patterns."""
    out = {}
    for line in stdout.splitlines():
        if line.startswith("{\"tree_cost\""):
            rec = json.loads(line)["tree_cost"]
            out[rec["when"]] = {k: (int(v, 16) if k in TU.DOUBLE_FIELDS else v) for k, v in rec.items()}
    return out


def assert_fields(got, want, what):
    for k in TU.DOUBLE_FIELDS:
        assert got[k] == int(TU.bits(want[k])), (what, k, hex(got[k]), want[k])
    for k in TU.INT_FIELDS:
        assert got[k] == want[k], (what, k)
    assert got["ms"] > 0, what


@pytest.mark.gpu
def test_cpp_tree_cost_equals_the_host_rule(exe, pkg, cornell_scene, tmp_path):
    capi = pkg.capi
    scene = cornell_scene
    args = [exe, "--scene", "cornell", "--size", "48x27", "--frames", "2", "--pool", "2048", "--live", "2048", "--tree-cost"]
    plain = printed(subprocess.run(args, check=True, capture_output=True, text=True, cwd=str(tmp_path)).stdout)
    assert sorted(plain) == ["bind"]
    assert_fields(plain["bind"], capi.tree_cost_host(scene["nodes"]), "as loaded")
    w = pkg.scenes.wobble(scene, 0.3, 0.05)
    w.astype("<f4").tofile(str(tmp_path / "moved.f32"))
    moved = printed(subprocess.run(args + ["--vertices", str(tmp_path / "moved.f32")], check=True, capture_output=True, text=True, cwd=str(tmp_path)).stdout)
    assert sorted(moved) == ["bind", "vertices"]
    assert_fields(moved["bind"], capi.tree_cost_host(scene["nodes"]), "before --vertices")
    assert_fields(moved["vertices"], capi.tree_cost_host(capi.bvh_refit_host(scene["nodes"], scene["tris"], w)), "after --vertices")
    assert moved["vertices"]["sah"] != moved["bind"]["sah"]

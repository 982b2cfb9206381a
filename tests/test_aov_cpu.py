"""CPU tests of the AOV buffers (gmupt_render_aovs / gmupt_aov_ray): the record layout, exports, the rays of a pixel, argument checks
that need no device and the C++ driver's --aov option.  The buffers themselves are rendered on the GPU: tests/test_aov_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gmu-path-tracer_amd", "host")
FIELDS = ("albedo", "depth", "normal", "roughness", "position", "metallic", "triangle", "material", "light", "coverage")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gmupt.h"
#define OFF(f) printf(" %zu", offsetof(gmupt_aov, f))
int main(void) {
    printf("%zu", sizeof(gmupt_aov));
    OFF(albedo); OFF(depth); OFF(normal); OFF(roughness); OFF(position); OFF(metallic); OFF(triangle); OFF(material); OFF(light); OFF(coverage);
    printf("\n%d %u\n", GMUPT_AOV_MAX_SAMPLES, GMUPT_AOV_CHUNK_RAYS);
    return 0;
}
"""


def test_aov_record_layout_of_header_and_binding(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rec, consts = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    capi = pkg.capi
    assert rec == [64, 0, 12, 16, 28, 32, 44, 48, 52, 56, 60]
    assert rec == [C.sizeof(capi.Aov)] + [getattr(capi.Aov, n).offset for n in FIELDS]
    assert rec == [capi.aov_dtype.itemsize] + [capi.aov_dtype.fields[n][1] for n in FIELDS]
    assert consts == [capi.AOV_MAX_SAMPLES, capi.AOV_CHUNK_RAYS] == [8, 1 << 21]


def test_library_exports_the_aov_symbols(pkg):
    lib = pkg.capi.lib()
    for name in ("gmupt_render_aovs", "gmupt_aov_ray"):
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS


def offset(a, s):
    return np.float32(np.float32(2 * a + 1) / np.float32(s)) - np.float32(1.0)


@pytest.mark.parametrize("pose", [(0.0, 1.0, 3.5, 0.0, 0.0), (1.25, 2.0, -4.0, -0.3, 2.1)])
def test_aov_rays_are_pick_rays_through_the_stratified_points(pkg, pose):
    capi = pkg.capi
    cam = capi.Camera(96, 54)
    cam.set_pose(*pose); cam.update(0.0)
    cb = cam.buffer_copy()
    for x, y in [(0, 0), (95, 53), (48, 27), (7, 40)]:
        centre = bytes(capi.camera_pick_ray(cb, x, y))
        for s in range(1, 9):
            R = 1 if s == 1 else s * s + 1
            assert bytes(capi.aov_ray(cb, x, y, s, 0)) == centre
            for k in range(1, R):
                a, b = (k - 1) % s, (k - 1) // s
                px = np.float32(np.float32(x) + offset(a, s)); py = np.float32(np.float32(y) + offset(b, s))
                assert bytes(capi.aov_ray(cb, x, y, s, k)) == bytes(capi.camera_pick_ray(cb, float(px), float(py))), (x, y, s, k)
            with pytest.raises(capi.GmuptError) as e:
                capi.aov_ray(cb, x, y, s, R)
            assert e.value.code == capi.ERR_INVALID_ARGUMENT
    # the offsets of one axis are the cell centres of newPath's jitter range [-1, 1]: -(1 - 1/s) .. 1 - 1/s (to binary32 rounding)
    for s in range(2, 9):
        o = np.array([offset(a, s) for a in range(s)], np.float32)
        assert np.all(np.diff(o) > 0) and o[0] > -1 and o[-1] < 1 and np.allclose(o, -o[::-1], atol=1e-6)
    rays = capi.aov_rays(cb, [3, 9], [4, 1], 3)
    assert rays.shape == (2, 10, 8) and rays[1, 4].tobytes() == bytes(capi.aov_ray(cb, 9, 1, 3, 4))
    cam.close()


def test_arguments_are_refused_without_a_gpu(pkg):
    capi = pkg.capi
    lib = capi.lib()
    info = capi.TraceInfo()
    info.redo_rays = 77
    assert lib.gmupt_render_aovs(None, 1, None, 0, C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert info.redo_rays == 0, "info is cleared whatever happens"
    assert lib.gmupt_render_aovs(None, 1, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    ray = capi.Ray()
    cb = capi.CameraBuffer()
    assert lib.gmupt_aov_ray(None, 0, 0, 1, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_aov_ray(C.byref(cb), 0, 0, 1, 0, None) == capi.ERR_INVALID_ARGUMENT
    for s in (0, 9, 100):
        assert lib.gmupt_aov_ray(C.byref(cb), 0, 0, s, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT
    assert b"samples" in lib.gmupt_last_error()
    assert lib.gmupt_aov_ray(C.byref(cb), 0, 0, 1, 1, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT


def test_aov_fields_split_records(pkg):
    capi = pkg.capi
    rec = np.zeros((2, 3), capi.aov_dtype)
    rec["albedo"] = (0.25, 0.5, 0.75); rec["depth"] = 7.0; rec["triangle"] = -1; rec["light"] = 2; rec["coverage"] = 9
    rec[1, 2]["normal"] = (0.0, 1.0, 0.0); rec[1, 2]["triangle"] = 12345
    f = capi.aov_fields(rec.view(np.float32).reshape(2, 3, 16))
    assert f["albedo"].shape == (2, 3, 3) and f["depth"].shape == (2, 3) and f["triangle"].dtype == np.int32 and f["coverage"].dtype == np.uint32
    assert f["triangle"][1, 2] == 12345 and f["triangle"][0, 0] == -1 and (f["light"] == 2).all() and (f["coverage"] == 9).all()
    assert np.array_equal(f["normal"][1, 2], np.array([0, 1, 0], np.float32)) and (f["depth"] == 7.0).all()


def test_cpp_driver_lists_aov_and_refuses_ranks(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    exe = os.path.join(HOST, "gmupt_render")
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--aov PREFIX" in out and "--aov-samples S" in out
    r = subprocess.run([exe, "--aov", "/nonexistent/x", "--ranks", "2", "--rank", "0", "--no-gather"], capture_output=True, text=True)
    assert r.returncode != 0 and "--aov" in r.stderr and "--ranks" in r.stderr

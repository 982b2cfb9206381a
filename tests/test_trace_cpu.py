"""CPU tests of the ray-query API (gmupt_trace_rays / gmupt_camera_pick_ray / gmupt_pick): record layouts, exports, the pick ray's
arithmetic and the C++ driver's --pick option.  The queries themselves run on the GPU: tests/test_trace_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gmu-path-tracer_amd", "host")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gmupt.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(gmupt_ray), offsetof(gmupt_ray, origin), offsetof(gmupt_ray, tmax), offsetof(gmupt_ray, direction));
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(gmupt_hit), offsetof(gmupt_hit, t), offsetof(gmupt_hit, u), offsetof(gmupt_hit, v),
           offsetof(gmupt_hit, triangle), offsetof(gmupt_hit, light), offsetof(gmupt_hit, material));
    printf("%zu %zu %zu %zu\n", sizeof(gmupt_trace_info), offsetof(gmupt_trace_info, flags), offsetof(gmupt_trace_info, redo_rays), offsetof(gmupt_trace_info, ms));
    return 0;
}
"""


def test_record_layouts_of_header_and_binding(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    ray, hit, info = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    capi = pkg.capi
    assert ray == [32, 0, 12, 16] == [C.sizeof(capi.Ray), capi.Ray.origin.offset, capi.Ray.tmax.offset, capi.Ray.direction.offset]
    assert hit == [32, 0, 4, 8, 12, 16, 20] == [C.sizeof(capi.Hit)] + [getattr(capi.Hit, n).offset for n in ("t", "u", "v", "triangle", "light", "material")]
    assert info == [24, 0, 8, 16] == [C.sizeof(capi.TraceInfo), capi.TraceInfo.flags.offset, capi.TraceInfo.redo_rays.offset, capi.TraceInfo.ms.offset]
    assert capi.ray_dtype.itemsize == 32 and capi.hit_dtype.itemsize == 32 and capi.hit_dtype.fields["material"][1] == 20


def test_library_exports_the_query_symbols(pkg):
    lib = pkg.capi.lib()
    for name in ("gmupt_trace_rays", "gmupt_camera_pick_ray", "gmupt_pick"):
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.capi.lib()
    info = pkg.capi.TraceInfo()
    info.redo_rays = 77
    assert lib.gmupt_trace_rays(None, None, 0, None, None, 0, None, 0, C.byref(info)) == pkg.capi.ERR_INVALID_ARGUMENT
    assert info.redo_rays == 0, "info is cleared whatever happens"
    assert lib.gmupt_camera_pick_ray(None, 0.0, 0.0, None) == pkg.capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_pick(None, 0.0, 0.0, 0, None, None) == pkg.capi.ERR_INVALID_ARGUMENT


def pick_ray_numpy(cb, px, py):
    """newPath.hlsl:36-39 with zero jitter, in binary32 and in the shader's operation order."""
    f = np.float32
    u = f(f(px) + f(0.0)) * f(cb.pixelSize[0])
    v = f(f(py) + f(0.0)) * f(cb.pixelSize[1])
    ulc = np.array(cb.upperLeftCorner[:3], np.float32); hor = np.array(cb.horizontal[:3], np.float32); ver = np.array(cb.vertical[:3], np.float32)
    d = (ulc + hor * u) - ver * v
    dot = f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])
    inv = f(1.0) / np.sqrt(f(dot))
    return np.array(cb.position[:3], np.float32), (d * inv).astype(np.float32)


@pytest.mark.parametrize("pose", [(0.0, 1.0, 3.5, 0.0, 0.0), (1.25, 2.0, -4.0, -0.3, 2.1), (-3.0, 0.5, 1.0, 0.7, -1.2)])
def test_pick_ray_is_newpath_without_jitter(pkg, pose):
    capi = pkg.capi
    cam = capi.Camera(96, 54)
    cam.set_pose(*pose); cam.update(0.0)
    cb = cam.buffer_copy()
    rng = np.random.default_rng(3)
    pts = [(0, 0), (95, 53), (48, 27)] + [tuple(rng.integers(0, 96, 1).tolist() + rng.integers(0, 54, 1).tolist()) for _ in range(20)] + [(10.5, 7.25)]
    for px, py in pts:
        ray = capi.camera_pick_ray(cb, px, py)
        o, d = pick_ray_numpy(cb, px, py)
        assert np.array(ray.origin[:], np.float32).tobytes() == o.tobytes()
        assert np.array(ray.direction[:], np.float32).tobytes() == d.tobytes(), (px, py)
        assert ray.tmax == np.finfo(np.float32).max and ray.pad == 0
    cam.close()


def test_cpp_driver_lists_pick(pkg):
    pkg.capi.lib()
    subprocess.run(["make", "-C", HOST, "-s"], check=True)
    out = subprocess.run([os.path.join(HOST, "gmupt_render"), "--help"], check=True, capture_output=True, text=True).stdout
    assert "--pick X,Y" in out

"""Builds libgmupt.so (HIP kernels + C-ABI + host classes) for gfx950 with hipcc, in-tree.

The float flags are part of the numerical contract (see csrc/detmath.hpp and DESIGN.md):
no FMA contraction, correctly rounded fp32 divide/sqrt, fp32 denormals kept.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libgmupt.so")

DEVICE_SOURCES = ["csrc/pt_kernels.hip", "csrc/pt_traverse.hip", "csrc/pt_traverse_wide.hip", "csrc/pt_traverse_variants.hip", "csrc/pt_aov.hip", "csrc/pt_denoise.hip", "csrc/pt_infill.hip", "csrc/pt_temporal.hip", "csrc/pt_refit.hip", "csrc/pt_motion.hip", "csrc/pt_lbvh.hip", "csrc/pt_normals.hip", "csrc/pt_treecost.hip", "csrc/pt_treeopt.hip", "csrc/pt_pose.hip", "csrc/pt_converge.hip", "csrc/pt_adaptive.hip", "csrc/pt_lens.hip", "csrc/pt_lens_aov.hip", "csrc/pt_projection.hip", "csrc/pt_shutter.hip", "csrc/gmupt_capi.hip", "csrc/gmupt_capi_accel.hip", "csrc/gmupt_capi_query.hip", "csrc/gmupt_capi_denoise.hip", "csrc/gmupt_capi_infill.hip", "csrc/gmupt_capi_normals.hip", "csrc/gmupt_capi_treecost.hip", "csrc/gmupt_capi_treeopt.hip", "csrc/gmupt_capi_pose.hip", "csrc/gmupt_capi_converge.hip", "csrc/gmupt_capi_adaptive.hip", "csrc/gmupt_capi_lens.hip", "csrc/gmupt_capi_lens_aov.hip", "csrc/gmupt_capi_projection.hip", "csrc/gmupt_capi_shutter.hip"]   # pt_traverse_variants.hip is empty without -DGMUPT_VARIANTS
HOST_SOURCES = ["csrc/gmupt_capi_host.cpp", "csrc/pt_travtables.cpp", "csrc/pt_lbvh.cpp", "csrc/pt_normals.cpp", "csrc/pt_treecost.cpp", "csrc/pt_treeopt.cpp", "csrc/pt_pose.cpp", "csrc/pt_infill.cpp", "csrc/pt_converge.cpp", "csrc/pt_adaptive.cpp", "csrc/pt_lens.cpp", "csrc/pt_lens_aov.cpp", "csrc/pt_projection.cpp", "csrc/pt_shutter.cpp", "csrc/pt_denoise.cpp", "csrc/pt_temporal.cpp", "csrc/pt_motion.cpp", "csrc/pt_refit.cpp", "host/sbvh_builder.cpp", "host/Camera.cpp", "host/TextureLoader.cpp", "host/AvirResize.cpp"]
HEADERS = ["csrc/gmupt_internal.hpp", "csrc/gmupt_work.hpp", "csrc/pt_launch.hpp", "csrc/pt_scratch.hpp", "csrc/pt_levels.hpp", "csrc/pt_ordered_sum.hpp", "csrc/pt_traverse_common.hpp", "csrc/pt_shading.hpp", "csrc/pt_guides.hpp", "csrc/pt_bands.hpp", "csrc/pt_denoise.hpp", "csrc/pt_infill.hpp", "csrc/pt_temporal.hpp", "csrc/pt_refit.hpp", "csrc/pt_travtables.hpp", "csrc/pt_motion.hpp", "csrc/pt_lbvh.hpp", "csrc/pt_normals.hpp", "csrc/pt_treecost.hpp", "csrc/pt_treeopt.hpp", "csrc/pt_pose.hpp", "csrc/pt_converge.hpp", "csrc/pt_adaptive.hpp", "csrc/pt_camera_rays.hpp", "csrc/pt_lens.hpp", "csrc/pt_lens_aov.hpp", "csrc/pt_projection.hpp", "csrc/pt_shutter.hpp", "csrc/pt_traverse_deferred.hpp", "csrc/pt_cast_plumbing.hpp", "csrc/pt_kernel_util.hpp", "host/MeshData.hpp", "host/BVHWrapper.hpp", "csrc/pt_device.hpp", "csrc/detmath.hpp", "host/sbvh_builder.hpp", "host/Camera.hpp", "host/TextureLoader.hpp", "host/png_reader.hpp", "host/Constants.hpp", "../include/gmupt.h", "../include/gmupt_adaptive.h", "../include/gmupt_lens.h", "../include/gmupt_lens_aov.h", "../include/gmupt_projection.h", "../include/gmupt_shutter.h"]

FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero",
    "-fno-fast-math", "-Wall", "-Wno-unused-function",
]


# Test-only builds of the same sources (tests/test_parity_gpu.py): the traversal ladder kept for A/B timing, and a build whose
# two-level rank computation has one block per group (so that a small pool reaches the many-group paths of k_logic / k_material),
# and a build of the wide ray cast whose stacks overflow on ordinary scenes.
TEST_BUILDS = {"variants": ["-DGMUPT_VARIANTS"], "scan1": ["-DGMUPT_SCAN_GROUP=1"],
               "wides8": ["-DGMUPT_WIDE_STACK=8", "-DGMUPT_WIDE_TOP=64", "-DGMUPT_WIDE_PARK=4"]}   # wide ray cast with a tiny LDS share per lane: stacks run full, rays are parked for the exact walk all the time


def lib_path(name=None):
    return LIB if not name else os.path.join(HERE, "libgmupt_%s.so" % name)


def needs_build(name=None):
    lib = lib_path(name)
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = DEVICE_SOURCES + HOST_SOURCES + HEADERS + ["build.py"]
    return any(os.path.getmtime(os.path.join(HERE, d)) > t for d in deps if os.path.exists(os.path.join(HERE, d)))


def build(force=False, verbose=False, name=None):
    """Builds libgmupt.so (name=None) or one of TEST_BUILDS (libgmupt_<name>.so); returns the path."""
    lib = lib_path(name)
    if not force and not needs_build(name):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # GMUPT_EXTRA_FLAGS: extra compiler flags of a one-off build for A/B timing, e.g. GMUPT_EXTRA_FLAGS="-DGMUPT_WIDE_REPS=4"
    extra = os.environ.get("GMUPT_EXTRA_FLAGS", "").split() + (TEST_BUILDS[name] if name else [])
    cmd = [hipcc] + FLAGS + extra + ["-x", "hip"] + [os.path.join(HERE, s) for s in DEVICE_SOURCES + HOST_SOURCES] + ["-o", lib]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=HERE)
    return lib


def build_all(force=False, verbose=False):
    """The shipped library and the test builds, compiled concurrently."""
    from concurrent.futures import ThreadPoolExecutor
    names = [None] + sorted(TEST_BUILDS)
    with ThreadPoolExecutor(len(names)) as ex:
        return list(ex.map(lambda n: build(force=force, verbose=verbose, name=n), names))


if __name__ == "__main__":
    if "--all" in sys.argv:
        print("\n".join(build_all(force="--force" in sys.argv, verbose=True)))
    else:
        print(build(force="--force" in sys.argv, verbose=True))

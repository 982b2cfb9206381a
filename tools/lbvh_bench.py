"""A new tree for changed geometry: the host SBVH build (A) against the GPU LBVH build (B), and what the LBVH costs in tracing.

  A  capi.sbvh_build of the mesh (gmupt_sbvh_build + flatten) on the host: wall clock.  The upload and the bind come on top in both arms.
  B  capi.Lbvh.build on the device-resident vertices: wall clock around the call (it ends in a synchronise) and info.ms, the device time.
     The index list is on the device before the clock starts, as it is for a caller who keeps it there between frames.

Both arms run alternated in one process after one warm-up of each (the first B allocates the builder's scratch).  Quality: for the SBVH
tree and for the LBVH tree at every --leaf size, the renderer is bound to the tree and runs --warm iterations, then ms_extend of --steps
iterations (enable_timing(2), the extension ray cast alone) is recorded next to the tree's SAH cost (capi.tree_sah), depth and node count.
One JSON line; --out FILE also writes it there.  The run fails (exit status 1) unless B's wall clock is below A's in every repetition.

  python tools/lbvh_bench.py [--scene bench|config5] [--reps 10] [--leaf 1,2,4,8] [--out profiles/lbvh/bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmupt_pkg  # noqa: E402


def spread(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bench", choices=["bench", "config5"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leaf", default="1,2,4,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = gmupt_pkg.load()
    capi, S = pkg.capi, pkg.scenes
    mesh = S.spheres_mesh() if args.scene == "bench" else S.spheres_mesh(1953, 4, seed=1234)
    leaves = [int(x) for x in args.leaf.split(",")]
    scene = S.build_scene(mesh)                          # warm-up of A, and the SBVH tree of the quality table
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    idx = torch.from_numpy(np.ascontiguousarray(mesh["indices"], np.int32)).cuda()
    vm = torch.from_numpy(np.ascontiguousarray(mesh["vertex_material"]).astype(np.int32)).cuda()
    lb = capi.Lbvh(dev)

    def arm_a():
        t0 = time.perf_counter()
        capi.sbvh_build(mesh["verts"], mesh["indices"], mesh["vertex_material"])
        return (time.perf_counter() - t0) * 1e3

    def arm_b(L=4):
        t0 = time.perf_counter()
        nb, tb, info = lb.build(sb.verts, idx, vm, max_leaf_size=L)
        ms = (time.perf_counter() - t0) * 1e3
        nb.close(); tb.close()
        return ms, info

    first_b_ms, _ = arm_b()                              # allocates the scratch
    a_ms, b_ms, b_dev = [], [], []
    for _ in range(args.reps):
        a_ms.append(arm_a())
        ms, info = arm_b(); b_ms.append(ms); b_dev.append(info["ms"])

    # tree quality: steady-state extension ray cast on each tree
    r = capi.Renderer(dev, args.width, args.height)
    cam = capi.Camera(args.width, args.height); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]

    def trace_ms(bind_ms_out):
        t0 = time.perf_counter(); r.bind_scene(sb); bind_ms_out.append((time.perf_counter() - t0) * 1e3)
        cam.reset_accumulation()
        for _ in range(args.warm):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        r.synchronize(); r.reset_stats(); r.enable_timing(2)
        for _ in range(args.steps):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        st = r.stats()
        r.enable_timing(0)
        return st.ms_extend / max(st.timed_iterations, 1)

    quality = []
    bind = []
    ms = trace_ms(bind)
    quality.append({"tree": "sbvh", "ms_extend": ms, "sah": capi.tree_sah(scene["nodes"]), "depth": scene["depth"], "nodes": int(len(scene["nodes"])),
                    "references": int(len(scene["tris"])), "bind_ms": bind[-1]})
    sbvh_nodes, sbvh_tris = sb.nodes, sb.tris
    for L in leaves:
        sb.nodes, sb.tris, info = lb.build(sb.verts, idx, vm, max_leaf_size=L)
        ms = trace_ms(bind)
        nodes = sb.nodes.read(capi.bvh_node_dtype)
        quality.append({"tree": "lbvh", "max_leaf_size": L, "ms_extend": ms, "sah": capi.tree_sah(nodes), "depth": info["depth"], "nodes": info["num_nodes"],
                        "references": info["num_tris"], "bind_ms": bind[-1], "build_device_ms": info["ms"]})
        r.synchronize()
        sb.nodes.close(); sb.tris.close()
    sb.nodes, sb.tris = sbvh_nodes, sbvh_tris
    r.bind_scene(sb)

    out = {"scene": scene["name"], "triangles": scene["num_triangles"], "vertices": int(len(scene["verts"])), "width": args.width, "height": args.height,
           "A_host_sbvh_build_ms": spread(a_ms), "B_gpu_lbvh_build_ms": spread(b_ms), "B_device_ms": spread(b_dev), "B_first_build_ms": first_b_ms,
           "B_below_A_in_every_repetition": bool(max(b_ms) < min(a_ms)) and all(b < a for a, b in zip(a_ms, b_ms)),
           "ratio_A_over_B_median": float(np.median(a_ms) / np.median(b_ms)), "quality": quality}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    cam.close(); r.close(); lb.close(); sb.close(); dev.close()
    if not out["B_below_A_in_every_repetition"]:         # the condition of the feature: the result is written first, then the run fails
        sys.exit("lbvh_bench: the GPU build was not below the host build in every repetition (A %s, B %s)" % (a_ms, b_ms))


if __name__ == "__main__":
    main()

"""What the treelet optimiser buys: an LBVH at L = 4 as built (passes 0, the baseline) against the same tree after 1, 2 and 3 passes of
capi.TreeOptimizer, with the SBVH of the mesh as the yardstick.

Per tree: the build's and the optimiser's device time (info.ms), the wall clock of build + optimise (capi.Lbvh.build(optimize=N), which
ends in a synchronise), sah / depth / nodes, the wall clock of bind_scene, and the steady-state ms_extend by the procedure of
tools/lbvh_bench.py (--warm iterations, then enable_timing(2) over --steps).  Every tree is built, bound and timed --reps times, the
trees interleaved (sbvh, 0, 1, 2, 3, sbvh, 0, ...), and the spread over the repetitions is reported.  One JSON line; --out FILE also
writes it there.

  python tools/treeopt_bench.py [--scene bench|config5] [--reps 3] [--passes 0,1,2,3] [--out profiles/treeopt/bench.json]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--passes", default="0,1,2,3")
    ap.add_argument("--leaf", type=int, default=4)
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
    passes = [int(x) for x in args.passes.split(",")]
    scene = S.build_scene(mesh)
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    idx = torch.from_numpy(np.ascontiguousarray(mesh["indices"], np.int32)).cuda()
    vm = torch.from_numpy(np.ascontiguousarray(mesh["vertex_material"]).astype(np.int32)).cuda()
    lb = capi.Lbvh(dev)
    for p in (0, max(passes)):                            # warm-up: the scratch of the builder and of the optimiser
        nb, tb, _ = lb.build(sb.verts, idx, vm, max_leaf_size=args.leaf, optimize=p)
        nb.close(); tb.close()
    r = capi.Renderer(dev, args.width, args.height)
    cam = capi.Camera(args.width, args.height); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]

    def trace_ms():
        t0 = time.perf_counter(); r.bind_scene(sb); bind = (time.perf_counter() - t0) * 1e3
        cam.reset_accumulation()
        for _ in range(args.warm):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        r.synchronize(); r.reset_stats(); r.enable_timing(2)
        for _ in range(args.steps):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        st = r.stats()
        r.enable_timing(0)
        return bind, st.ms_extend / max(st.timed_iterations, 1)

    rows = {"sbvh": {"tree": "sbvh", "sah": capi.tree_cost_host(scene["nodes"])["sah"], "depth": scene["depth"], "nodes": int(len(scene["nodes"]))}}
    samples = {"sbvh": {"bind_ms": [], "ms_extend": []}}
    for p in passes:
        samples[p] = {"bind_ms": [], "ms_extend": [], "build_device_ms": [], "optimize_device_ms": [], "build_plus_optimize_wall_ms": []}
    sbvh_nodes, sbvh_tris = sb.nodes, sb.tris
    for _ in range(args.reps):
        sb.nodes, sb.tris = sbvh_nodes, sbvh_tris
        bind, ms = trace_ms()
        samples["sbvh"]["bind_ms"].append(bind); samples["sbvh"]["ms_extend"].append(ms)
        for p in passes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sb.nodes, sb.tris, info = lb.build(sb.verts, idx, vm, max_leaf_size=args.leaf, optimize=p)
            wall = (time.perf_counter() - t0) * 1e3
            bind, ms = trace_ms()
            s = samples[p]
            s["bind_ms"].append(bind); s["ms_extend"].append(ms); s["build_device_ms"].append(info["ms"]); s["build_plus_optimize_wall_ms"].append(wall)
            s["optimize_device_ms"].append(info["optimize"]["ms"] if p else 0.0)
            if p not in rows:
                nodes = sb.nodes.read(capi.bvh_node_dtype)
                rows[p] = {"tree": "lbvh", "max_leaf_size": args.leaf, "passes": p, "sah": capi.tree_cost_host(nodes)["sah"], "depth": info["depth"],
                           "nodes": info["num_nodes"], "treelets_rewritten": info["optimize"]["treelets_rewritten"] if p else 0}
            r.synchronize()
            sb.nodes.close(); sb.tris.close()
    sb.nodes, sb.tris = sbvh_nodes, sbvh_tris
    r.bind_scene(sb)
    for k, row in rows.items():
        row.update({name: spread(v) for name, v in samples[k].items()})

    # how much of the SBVH-to-LBVH gap each pass count closes, and after how many wavefront iterations the optimiser's time is earned back
    if 0 in rows:
        s, l = rows["sbvh"], rows[0]
        for p in passes:
            if not p:
                continue
            row = rows[p]
            row["sah_gap_closed"] = (l["sah"] - row["sah"]) / (l["sah"] - s["sah"]) if l["sah"] != s["sah"] else None
            gap = l["ms_extend"]["median"] - s["ms_extend"]["median"]
            gain = l["ms_extend"]["median"] - row["ms_extend"]["median"]
            row["ms_extend_gap_closed"] = gain / gap if gap else None
            extra = row["build_plus_optimize_wall_ms"]["median"] - l["build_plus_optimize_wall_ms"]["median"]
            row["iterations_to_earn_back"] = extra / gain if gain > 0 else None
    out = {"scene": scene["name"], "triangles": scene["num_triangles"], "width": args.width, "height": args.height, "reps": args.reps,
           "warm": args.warm, "steps": args.steps, "trees": [rows[k] for k in ["sbvh"] + passes]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    cam.close(); r.close(); lb.close(); sb.close(); dev.close()


if __name__ == "__main__":
    main()

"""The tree cost of the bound tree: the host route (A) against the device route (B), and what the number is worth for the choice between
refit and rebuild.

  A  Buffer.read of the node buffer + capi.tree_sah (numpy float64 over the host copy): wall clock.  The only route before
     gmupt_renderer_tree_cost existed.
  B  Renderer.tree_cost(): wall clock around the call (it ends in a synchronise) and info.ms, the device time of its launches.

Both routes run alternated in one process after one warm-up of each.  B's device time is set against the bound of the kernel, the node
bytes over the read-only streaming rate measured on this GPU (profiles/r02_micro/hbm_copy.txt: 5.0 TB/s); a node buffer that fits the
256 MiB Infinity Cache and was just written or read can come in below that bound, so the figure that counts is config5's.

--twist A0,A1,..: the mesh twisted about the vertical axis through its centre, by an angle that grows linearly with height up to A degrees
at the top.  For every angle: the scene is bound in its rest pose, the twisted vertices are uploaded and the tree refitted; recorded are the
sah ratio of the refitted tree to its bind-time value (Renderer.tree_cost), ms_extend of the refitted tree (enable_timing(2), --warm
iterations, then the mean over --steps, the protocol of tools/lbvh_bench.py), the same two figures for a refitted LBVH of the rest pose
(the tree a session holds after its first adoption), and sah and ms_extend of a fresh LBVH of that pose.  The table shows where refit
stops paying.

One JSON line; --out FILE also writes it there.  The run fails (exit status 1) unless B's wall clock is below A's in every repetition.

  python tools/treecost_bench.py [--scene bench|config5] [--reps 10] [--twist 0,15,30,60,90,135,180] [--out profiles/treecost/bench.json]
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

READ_RATE = 5.0e12   # bytes / s, read-only stream of 16-byte loads (profiles/r02_micro/hbm_copy.txt)


def spread(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def twisted(verts, degrees):
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    c = 0.5 * (lo + hi)
    a = np.radians(degrees) * (v[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-30)
    x, z = v[:, 0] - c[0], v[:, 2] - c[2]
    out = v.copy()
    out[:, 0] = c[0] + np.cos(a) * x - np.sin(a) * z
    out[:, 2] = c[2] + np.sin(a) * x + np.cos(a) * z
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bench", choices=["bench", "config5"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--twist", default="0,15,30,60,90,135,180")
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
    angles = [float(x) for x in args.twist.split(",") if x]
    scene = S.build_scene(mesh)
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, args.width, args.height)
    r.bind_scene(sb)
    node_bytes = int(len(scene["nodes"])) * 48

    def route_a():
        t0 = time.perf_counter()
        sah = capi.tree_sah(sb.nodes.read(capi.bvh_node_dtype))
        return (time.perf_counter() - t0) * 1e3, sah

    def route_b():
        t0 = time.perf_counter()
        info = r.tree_cost()
        return (time.perf_counter() - t0) * 1e3, info

    route_a(); first_b_ms, _ = route_b()                  # warm-up; the first B allocates the scratch
    a_ms, b_ms, b_dev = [], [], []
    for _ in range(args.reps):
        ms, sah_a = route_a(); a_ms.append(ms)
        ms, info = route_b(); b_ms.append(ms); b_dev.append(info["ms"])
    bound_ms = node_bytes / READ_RATE * 1e3
    out = {"scene": scene["name"], "triangles": scene["num_triangles"], "nodes": int(len(scene["nodes"])), "node_bytes": node_bytes,
           "A_read_plus_tree_sah_ms": spread(a_ms), "B_tree_cost_wall_ms": spread(b_ms), "B_device_ms": spread(b_dev), "B_first_call_ms": first_b_ms,
           "B_below_A_in_every_repetition": bool(max(b_ms) < min(a_ms)) and all(b < a for a, b in zip(a_ms, b_ms)),
           "ratio_A_over_B_median": float(np.median(a_ms) / np.median(b_ms)),
           "read_rate_bytes_per_s": READ_RATE, "bound_ms": bound_ms, "B_device_over_bound": float(np.median(b_dev) / bound_ms),
           "sah_A": sah_a, "sah_B": info["sah"], "sah_relative_difference": abs(sah_a - info["sah"]) / info["sah"]}

    # what the number is worth: refit against rebuild along a growing twist
    if angles:
        cam = capi.Camera(args.width, args.height); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
        idx = torch.from_numpy(np.ascontiguousarray(mesh["indices"], np.int32)).cuda()
        vm = torch.from_numpy(np.ascontiguousarray(mesh["vertex_material"]).astype(np.int32)).cuda()
        lb = capi.Lbvh(dev)

        def trace_ms():
            cam.reset_accumulation()
            for _ in range(args.warm):
                cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            r.synchronize(); r.reset_stats(); r.enable_timing(2)
            for _ in range(args.steps):
                cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
            st = r.stats()
            r.enable_timing(0)
            return st.ms_extend / max(st.timed_iterations, 1)

        table = []
        sbvh_nodes, sbvh_tris = sb.nodes, sb.tris
        for angle in angles:
            w = twisted(scene["verts"], angle)
            sb.nodes.update(scene["nodes"]); sb.verts.update(scene["verts"])      # the rest pose, bound as a user's session has it
            r.bind_scene(sb)
            base = r.tree_cost()["sah"]
            sb.verts.update(w)
            refit = r.refit()
            cost = r.tree_cost()
            row = {"angle": angle, "sah_bind": base, "sah_refitted": cost["sah"], "ratio": cost["sah"] / base, "tree_cost_ms": cost["ms"],
                   "refit_ms": refit["ms"], "refit_rebuilt": int(refit["rebuilt"]), "ms_extend_refitted": trace_ms()}
            r.synchronize()
            # the same for an LBVH of the rest pose, the tree a session holds after its first adoption: no spatial splits, so a refit
            # costs it nothing at angle 0
            sb.verts.update(scene["verts"])
            sb.nodes, sb.tris, _ = lb.build(sb.verts, idx, vm)
            r.bind_scene(sb)
            base_l = r.tree_cost()["sah"]
            sb.verts.update(w)
            r.refit()
            row.update({"sah_lbvh_rest": base_l, "sah_lbvh_refitted": r.tree_cost()["sah"], "ms_extend_lbvh_refitted": trace_ms()})
            row["ratio_lbvh"] = row["sah_lbvh_refitted"] / base_l
            r.synchronize()
            sb.nodes.close(); sb.tris.close()
            sb.nodes, sb.tris, info = lb.build(sb.verts, idx, vm)
            row["sah_lbvh"] = r.tree_cost(nodes=sb.nodes)["sah"]
            row["lbvh_build_ms"] = info["ms"]
            r.bind_scene(sb)
            row["ms_extend_lbvh"] = trace_ms()
            r.synchronize()
            sb.nodes.close(); sb.tris.close()
            sb.nodes, sb.tris = sbvh_nodes, sbvh_tris
            table.append(row)
            print("twist %g: refitted SBVH x%.4f %.4f ms, refitted rest-pose LBVH x%.4f %.4f ms, fresh LBVH %.4f ms (sah %.2f)" % (
                angle, row["ratio"], row["ms_extend_refitted"], row["ratio_lbvh"], row["ms_extend_lbvh_refitted"], row["ms_extend_lbvh"], row["sah_lbvh"]),
                  file=sys.stderr, flush=True)
        sb.nodes.update(scene["nodes"]); sb.verts.update(scene["verts"])
        r.bind_scene(sb)
        out.update({"width": args.width, "height": args.height, "warm": args.warm, "steps": args.steps, "twist": table})
        cam.close(); lb.close()

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    r.close(); sb.close(); dev.close()
    if not out["B_below_A_in_every_repetition"]:          # the condition of the feature: the result is written first, then the run fails
        sys.exit("treecost_bench: the device route was not below the host route in every repetition (A %s, B %s)" % (a_ms, b_ms))


if __name__ == "__main__":
    main()

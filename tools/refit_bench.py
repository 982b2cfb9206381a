"""Moved vertices on screen: what a vertex edit costs with a rebind (A) and with a refit (B).

  A  verts.update(w) + Renderer.bind_scene on the same (stale) tree -- the only way before gmupt_renderer_refit.  Reported next to it, not
     summed: the host SBVH build of the moved mesh (what a user who wants fitted boxes pays on top).
  B  verts.update(w) + Renderer.refit(): wall clock and info.ms (device time of the kernels).

Both arms run alternated in one process on the same renderer and buffers, after one warm-up of each; the host clock is read around calls
that end in a synchronise (bind_scene and refit both do).  One JSON line; --out FILE also writes it there.

  python tools/refit_bench.py [--scene bench|config5] [--reps 10] [--amplitude 0.01] [--out profiles/refit/bench.json]
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
    ap.add_argument("--amplitude", type=float, default=0.01)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = gmupt_pkg.load()
    capi, S = pkg.capi, pkg.scenes
    mesh = S.spheres_mesh() if args.scene == "bench" else S.spheres_mesh(1953, 4, seed=1234)
    t0 = time.perf_counter(); scene = S.build_scene(mesh); build_s = time.perf_counter() - t0
    poses = [S.wobble(scene, 0.1 + 0.8 * k / max(args.reps, 1), args.amplitude) for k in range(args.reps + 1)]
    moved_mesh = dict(mesh); moved_mesh["verts"] = poses[0]
    t0 = time.perf_counter(); capi.sbvh_build(moved_mesh["verts"], mesh["indices"], mesh["vertex_material"]); rebuild_s = time.perf_counter() - t0
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, 64, 36, pool_paths=4096)
    t0 = time.perf_counter(); r.bind_scene(sb); first_bind_ms = (time.perf_counter() - t0) * 1e3
    nodes0 = np.ascontiguousarray(scene["nodes"])

    def arm_a(w):
        sb.nodes.update(nodes0)                    # outside the clock: A binds the stale tree as the builder left it
        t0 = time.perf_counter()
        sb.verts.update(w); r.bind_scene(sb)
        return (time.perf_counter() - t0) * 1e3

    def arm_b(w):
        t0 = time.perf_counter()
        sb.verts.update(w); info = r.refit()
        return (time.perf_counter() - t0) * 1e3, info

    arm_a(poses[-1]); arm_b(poses[-1])             # warm-up of both (the first refit after a bind uploads its maps)
    a_ms, b_ms, b_dev, b_first, rebuilt = [], [], [], [], 0
    for k in range(args.reps):
        a_ms.append(arm_a(poses[k]))
        ms, info = arm_b(poses[k]); b_first.append(ms)     # the first refit after a bind: with the upload of the maps
        ms, info = arm_b(poses[k + 1]); b_ms.append(ms); b_dev.append(info["ms"]); rebuilt += info["rebuilt"]
    out = {"scene": scene["name"], "triangles": scene["num_triangles"], "nodes": int(len(scene["nodes"])), "references": int(len(scene["tris"])),
           "vertices": int(len(scene["verts"])), "depth": scene["depth"], "amplitude": args.amplitude, "levels": info["levels"],
           "opened_nodes": info["opened_nodes"], "rebuilt": rebuilt,
           "A_update_bind_ms": spread(a_ms), "B_update_refit_ms": spread(b_ms), "B_first_refit_after_bind_ms": spread(b_first),
           "B_device_ms": spread(b_dev), "first_bind_ms": first_bind_ms, "host_sbvh_build_s": build_s, "host_sbvh_build_moved_s": rebuild_s,
           "B_below_A_in_every_repetition": bool(max(b_ms) < min(a_ms)) and all(b < a for a, b in zip(a_ms, b_ms)),
           "ratio_A_over_B_median": float(np.median(a_ms) / np.median(b_ms))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    r.close(); sb.close(); dev.close()


if __name__ == "__main__":
    main()

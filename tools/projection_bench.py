"""What a camera projection costs (csrc/pt_projection.hip) on the benchmark's scene: 1920x1080, 202 spheres at subdivision 3, pool 2^21.

    python tools/projection_bench.py [--out FILE.json]
        one process, one renderer: rounds of ITERATIONS iterations, alternating no projection / orthographic / fisheye / equirect, each
        round timed by a host clock around work that ends in a synchronise, after WARMUP rounds of each kind.  Prints the median ms per
        iteration of each kind, its difference to "none" and the spread (max - min) of the rounds of a kind.  A projection changes
        the picture and with it the paths (an equirect camera sees the whole room), so a difference here is the extra launch plus the
        other workload; the launch alone is k_lens_retarget's twin (tools/lens_bench.py).  The renderer is the same object, so "none"
        here is this tree; the parent commit is compared through bench.py (which binds no projection), alternated by the caller.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch   # first: torch's HIP runtime is the one libgmupt binds to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H, POOL, ITERATIONS, ROUNDS, WARMUP = 1920, 1080, 1 << 21, 40, 7, 1


def iterate(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    r.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    P = capi.projection
    torch.zeros(1, device="cuda")
    dev = capi.Device(0)
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, W, H, pool_paths=POOL)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    kinds = {"none": None, "orthographic": P.orthographic(12.0), "fisheye": P.fisheye(180.0), "equirect": P.equirect()}
    ms = {k: [] for k in kinds}
    iterate(r, cam, ITERATIONS)                       # fills the pool
    for rnd in range(WARMUP + ROUNDS):
        for kind, proj in kinds.items():
            P.set_projection(r, proj)
            iterate(r, cam, ITERATIONS)               # the paths of the previous kind drain: the timed span is this kind's steady state
            t0 = time.perf_counter()
            iterate(r, cam, ITERATIONS)
            dt = (time.perf_counter() - t0) * 1000.0 / ITERATIONS
            if rnd >= WARMUP:
                ms[kind].append(dt)
    out = {"width": W, "height": H, "pool": POOL, "iterations_per_round": ITERATIONS, "rounds": ROUNDS,
           "ms_per_iteration": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in ms.items()}}
    out["minus_none_ms"] = {k: round(out["ms_per_iteration"][k]["median"] - out["ms_per_iteration"]["none"]["median"], 4) for k in kinds if k != "none"}
    out["spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 4)
    line = json.dumps({"projection_end_to_end": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    r.close(); sb.close(); cam.close(); dev.close()


if __name__ == "__main__":
    main()

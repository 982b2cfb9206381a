"""What the thin lens costs (csrc/pt_lens.hip) on the benchmark's scene: 1920x1080, 202 spheres at subdivision 3, pool 2^21.

    python tools/lens_bench.py [--out FILE.json]
        one process, one renderer: rounds of ITERATIONS iterations, alternating no lens / lens attached, each round timed by a host
        clock around work that ends in a synchronise, after WARMUP rounds of each kind.  Prints the median ms per iteration of each
        kind, the differences of the medians and the spread (max - min) of the rounds of a kind.  The renderer is the same object, so
        "no lens" here is this tree; the parent commit is compared through bench.py (which binds no lens), alternated by the caller.
    rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o lens -- python tools/lens_bench.py --trace-job
    python tools/lens_bench.py --parse-trace DIR/prof [--out FILE.json]
        the job: 12 iterations with a lens and the identity sampling plan attached, so that k_ad_retarget and k_lens_retarget run side
        by side on the same queues.  --parse-trace gives the median of the last 7 launches of each.  Modelled bytes per fresh path:
        k_lens_retarget reads 4 (queue entry) + 8 (screen coordinate) and writes 24; k_ad_retarget reads 8 and writes 20.  The fresh
        paths per iteration are read from the renderer's statistics, not assumed.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch   # first: torch's HIP runtime is the one libgmupt binds to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H, POOL, ITERATIONS, ROUNDS, WARMUP = 1920, 1080, 1 << 21, 40, 7, 1
APERTURE, FOCUS = 0.3, 20.0
LENS_BYTES, RETARGET_BYTES = 36, 28


def setup():
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    torch.zeros(1, device="cuda")
    dev = capi.Device(0)
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, W, H, pool_paths=POOL)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    return capi, dev, sb, r, cam


def iterate(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    r.synchronize()


def parse_trace(args):
    files = sorted(glob.glob(os.path.join(args.parse_trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % args.parse_trace)
    rows = []
    for fn in files:
        with open(fn, newline="") as f:
            for rec in csv.DictReader(f):
                rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), rec["Kernel_Name"]))
    rows.sort()
    fresh = None
    side = os.path.join(args.parse_trace, "..", "lens_trace_job.json")
    if os.path.exists(side):
        fresh = json.load(open(side))["fresh_per_iteration"]
    out = {"width": W, "height": H, "pool": POOL, "fresh_per_iteration": fresh, "kernels": []}
    for name, nbytes in (("k_lens_retarget", LENS_BYTES), ("k_ad_retarget", RETARGET_BYTES), ("k_material", None)):
        us = [(e - s) / 1000.0 for s, e, k in rows if name in k]
        if not us:
            continue
        rec = {"kernel": name, "launches": len(us), "median_us": round(statistics.median(us[-7:]), 2)}
        if nbytes and fresh:
            rec["bytes_per_fresh_path"] = nbytes
            rec["gb_per_s"] = round(fresh * nbytes / (rec["median_us"] * 1e-6) / 1e9, 1)
            rec["fresh_paths_per_us"] = round(fresh / rec["median_us"], 1)
        out["kernels"].append(rec)
    line = json.dumps({"lens_kernels": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def trace_job(args):
    capi, dev, sb, r, cam = setup()
    plan = capi.adaptive.Adaptive(r)
    plan.set_list(np.arange(W * H, dtype=np.uint32), W, H)
    capi.adaptive.set_adaptive(r, plan)
    capi.lens.set_lens(r, capi.lens.lens_params(aperture_radius=APERTURE, focus_distance=FOCUS))
    iterate(r, cam, 5)
    before = r.stats().paths_generated
    iterate(r, cam, 7)
    fresh = (r.stats().paths_generated - before) / 7.0
    line = json.dumps({"fresh_per_iteration": fresh})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    r.close(); sb.close(); cam.close(); dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parse-trace")
    ap.add_argument("--trace-job", action="store_true")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args)
    if args.trace_job:
        return trace_job(args)
    capi, dev, sb, r, cam = setup()
    lens = capi.lens.lens_params(aperture_radius=APERTURE, focus_distance=FOCUS)
    ms = {"none": [], "lens": []}
    iterate(r, cam, ITERATIONS)                       # fills the pool: the steady state of the alternation below
    for rnd in range(WARMUP + ROUNDS):
        for kind in ("none", "lens"):
            capi.lens.set_lens(r, lens if kind == "lens" else None)
            t0 = time.perf_counter()
            iterate(r, cam, ITERATIONS)
            dt = (time.perf_counter() - t0) * 1000.0 / ITERATIONS
            if rnd >= WARMUP:
                ms[kind].append(dt)
    out = {"width": W, "height": H, "pool": POOL, "iterations_per_round": ITERATIONS, "rounds": ROUNDS,
           "ms_per_iteration": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in ms.items()}}
    out["lens_minus_none_ms"] = round(out["ms_per_iteration"]["lens"]["median"] - out["ms_per_iteration"]["none"]["median"], 4)
    out["spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 4)
    line = json.dumps({"lens_end_to_end": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    r.close(); sb.close(); cam.close(); dev.close()


if __name__ == "__main__":
    main()

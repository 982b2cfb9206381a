"""What the shutter costs (csrc/pt_shutter.hip) on the benchmark's scene: 1920x1080, 202 spheres at subdivision 3, pool 2^21.

    python tools/shutter_bench.py [--out FILE.json]
        one process, one renderer: rounds of ITERATIONS iterations, alternating no shutter / shutter attached (the pinhole rule), each
        round timed by a host clock around work that ends in a synchronise, after WARMUP rounds of each kind.  Prints the median ms per
        iteration of each kind, the difference of the medians and the spread (max - min) of the rounds of a kind.  The renderer is the
        same object, so "no shutter" here is this tree; the parent commit is compared through bench.py (which binds no shutter),
        alternated by the caller.
    rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o shutter -- python tools/shutter_bench.py --trace-job
    python tools/shutter_bench.py --parse-trace DIR/prof [--out FILE.json]
        the job, one process: PHASE iterations each with a lens alone (k_lens_retarget), the lens under a shutter
        (k_shutter_retarget_lens), the shutter alone (k_shutter_retarget_pinhole) and a fisheye under the shutter
        (k_shutter_retarget_proj), so that every launch is measured on the same renderer in the same run.  --parse-trace gives the median
        of the last 7 launches of each.  Modelled bytes per fresh path: each of these kernels reads 4 (queue entry) + 8 (screen coordinate)
        and writes 24.  The fresh paths per iteration are read from the renderer's statistics, not assumed.
"""
import argparse
import csv
import glob
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

W, H, POOL, ITERATIONS, ROUNDS, WARMUP, PHASE = 1920, 1080, 1 << 21, 40, 7, 1, 12
APERTURE, FOCUS = 0.3, 20.0
CLOSE_OFFSET = (0.5, 0.1, -0.2, 1.0, 3.0)      # the close pose: the scene's camera moved and turned by this much (x, y, z, pitch, yaw)
RETARGET_BYTES = 36
KERNELS = ("k_lens_retarget", "k_shutter_retarget_lens", "k_shutter_retarget_pinhole", "k_shutter_retarget_proj", "k_material")


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
    close = capi.Camera(W, H); close.set_pose(*[a + b for a, b in zip(scene["camera"], CLOSE_OFFSET)]); close.update(0.0)
    shutter = capi.shutter.from_camera(close.buffer_copy())
    close.close()
    return capi, dev, sb, r, cam, shutter


def iterate(r, cam, n):
    for _ in range(n):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    r.synchronize()


def write(line, path):
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


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
    side = os.path.join(args.parse_trace, "..", "shutter_trace_job.json")
    if os.path.exists(side):
        fresh = json.load(open(side))["fresh_per_iteration"]
    out = {"width": W, "height": H, "pool": POOL, "fresh_per_iteration": fresh, "kernels": []}
    for name in KERNELS:
        us = [(e - s) / 1000.0 for s, e, k in rows if name in k]
        if not us:
            continue
        rec = {"kernel": name, "launches": len(us), "median_us": round(statistics.median(us[-7:]), 2)}
        if name != "k_material" and fresh:
            rec["bytes_per_fresh_path"] = RETARGET_BYTES
            rec["gb_per_s"] = round(fresh * RETARGET_BYTES / (rec["median_us"] * 1e-6) / 1e9, 1)
            rec["fresh_paths_per_us"] = round(fresh / rec["median_us"], 1)
        out["kernels"].append(rec)
    write(json.dumps({"shutter_kernels": out}), args.out)


def trace_job(args):
    capi, dev, sb, r, cam, shutter = setup()
    lens = capi.lens.lens_params(aperture_radius=APERTURE, focus_distance=FOCUS)
    capi.lens.set_lens(r, lens)
    iterate(r, cam, PHASE)                            # k_lens_retarget
    capi.shutter.set_shutter(r, shutter)
    iterate(r, cam, PHASE)                            # k_shutter_retarget_lens
    capi.lens.set_lens(r, None)
    iterate(r, cam, PHASE - 7)                        # k_shutter_retarget_pinhole
    before = r.stats().paths_generated
    iterate(r, cam, 7)
    fresh = (r.stats().paths_generated - before) / 7.0
    capi.projection.set_projection(r, capi.projection.fisheye(180.0))
    iterate(r, cam, PHASE)                            # k_shutter_retarget_proj
    write(json.dumps({"fresh_per_iteration": fresh}), args.out)
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
    capi, dev, sb, r, cam, shutter = setup()
    ms = {"none": [], "shutter": []}
    iterate(r, cam, ITERATIONS)                       # fills the pool: the steady state of the alternation below
    for rnd in range(WARMUP + ROUNDS):
        for kind in ("none", "shutter"):
            capi.shutter.set_shutter(r, shutter if kind == "shutter" else None)
            t0 = time.perf_counter()
            iterate(r, cam, ITERATIONS)
            dt = (time.perf_counter() - t0) * 1000.0 / ITERATIONS
            if rnd >= WARMUP:
                ms[kind].append(dt)
    out = {"width": W, "height": H, "pool": POOL, "iterations_per_round": ITERATIONS, "rounds": ROUNDS,
           "ms_per_iteration": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in ms.items()}}
    out["shutter_minus_none_ms"] = round(out["ms_per_iteration"]["shutter"]["median"] - out["ms_per_iteration"]["none"]["median"], 4)
    out["spread_ms"] = round(max(max(v) - min(v) for v in ms.values()), 4)
    write(json.dumps({"shutter_end_to_end": out}), args.out)
    r.close(); sb.close(); cam.close(); dev.close()


if __name__ == "__main__":
    main()

"""Kernel times of adaptive sampling (csrc/pt_adaptive.hip) at 1920x1080 next to k_cv_update from the same job.

    rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o ad -- python tools/adaptive_bench.py
    python tools/adaptive_bench.py --parse-trace DIR/prof [--out FILE.json]

The job: 9 monitor updates with the error plane on synthetic frames in which every pixel has a new batch (k_cv_update, 92 modelled
bytes per pixel, as tools/converge_bench.py); 9 selections (k_ad_count, k_ad_scan twice -- 8 100 run totals, then 32 --, k_ad_emit) on a
synthetic error plane of which half the pixels lie at or below the threshold and the rest spread up to the cap, max_repeat 8; and 12
Cornell iterations with that plan attached, pool 2^20 (k_ad_retarget).  --parse-trace gives the median of the last 7 launches of each
kernel and the bandwidth of the modelled bytes: k_ad_count reads 4 bytes per pixel, k_ad_emit reads 4 and writes 4 per entry, the three
select kernels together move 8 + 4 * entries / pixels; k_ad_retarget reads 8 bytes (queue entry, list entry) and writes 20 per fresh path.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch   # first: torch's HIP runtime is the one libgmupt binds to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H, REPS, T, MAX_REPEAT, POOL, ITERATIONS = 1920, 1080, 9, 0.01, 8, 1 << 20, 12


def error_plane():
    rng = np.random.default_rng(3)
    e = (rng.random((H, W), dtype=np.float32) * np.float32(T)).astype(np.float32)          # at or below T
    hot = rng.random((H, W)) < 0.5
    e[hot] = (np.float32(T) * (1 + rng.random(int(hot.sum()), dtype=np.float32) * np.float32(2.2))).astype(np.float32)   # (err/T)^2 up to 10: past the cap of 8
    return e


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
    from gmupt_pkg import load
    lst, info = load().capi.adaptive.adaptive_select_host(error_plane(), threshold=T, max_repeat=MAX_REPEAT)
    n, entries = W * H, info["entries"]

    def med(name, pick=lambda us: us):
        us = pick([(e - s) / 1000.0 for s, e, k in rows if name in k])
        return statistics.median(us[-7:]), len(us)

    out = {"width": W, "height": H, "max_repeat": MAX_REPEAT, "entries": entries, "active": info["active"], "kernels": []}

    def row(name, us, launches, nbytes, per):
        out["kernels"].append({"kernel": name, "launches": launches, "median_us": round(us, 2), "bytes": nbytes, "per": per,
                               "tb_per_s": round(nbytes / (us * 1e-6) / 1e12, 3)})
        return us

    cv = row("k_cv_update", *med("k_cv_update"), n * 92, "92 per pixel")
    c = row("k_ad_count", *med("k_ad_count"), n * 4, "4 per pixel")
    s0 = row("k_ad_scan level 0", *med("k_ad_scan", lambda us: us[0::2]), ((n + 255) // 256) * 20, "16 read + 4 written per run total")
    s1 = row("k_ad_scan level 1", *med("k_ad_scan", lambda us: us[1::2]), 32 * 20, "16 read + 4 written per total")
    e = row("k_ad_emit", *med("k_ad_emit"), n * 4 + entries * 4, "4 per pixel + 4 per entry")
    us, launches = med("k_ad_retarget")
    out["kernels"].append({"kernel": "k_ad_retarget", "launches": launches, "median_us": round(us, 2), "per": "grid = the pool (2^20 slots); 28 bytes per fresh path"})
    sel = c + s0 + s1 + e
    out["select_us"] = round(sel, 2)
    out["select_bytes"] = n * 8 + entries * 4
    out["select_tb_per_s"] = round(out["select_bytes"] / (sel * 1e-6) / 1e12, 3)
    out["k_cv_update_tb_per_s"] = round(n * 92 / (cv * 1e-6) / 1e12, 3)
    out["select_over_k_cv_update"] = round(out["select_tb_per_s"] / out["k_cv_update_tb_per_s"], 3)
    line = json.dumps({"adaptive_kernels": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parse-trace")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args)
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    torch.zeros(1, device="cuda")
    dev = capi.Device(0)
    scene = pkg.scenes.build_scene(pkg.scenes.cornell_mesh())
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, W, H, pool_paths=POOL)
    r.bind_scene(sb)
    rng = np.random.default_rng(1)
    frame = rng.random((H, W, 4), dtype=np.float32)
    counts = np.zeros((H, W), np.uint32)
    c = capi.Converge(r)
    for _ in range(REPS):
        counts += 8
        frame[..., 3] = counts.view(np.float32)
        frame[..., :3] += np.float32(0.001)
        r.write_framebuffer(frame)
        c.update(error=True)
    plan = capi.adaptive.Adaptive(r)
    err = torch.from_numpy(error_plane()).cuda()
    ms = []
    for _ in range(REPS):
        ms.append(plan.select(err, threshold=T, max_repeat=MAX_REPEAT)["ms"])
    info = plan.select(err, threshold=T, max_repeat=MAX_REPEAT)
    capi.adaptive.set_adaptive(r, plan)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    for _ in range(ITERATIONS):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    r.synchronize()
    print(json.dumps({"adaptive_select": {"width": W, "height": H, "entries": info["entries"], "active": info["active"], "ms_median": statistics.median(ms[2:]), "ms": ms[2:]}}))
    r.close(); sb.close(); cam.close(); dev.close()


if __name__ == "__main__":
    main()

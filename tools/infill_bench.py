#!/usr/bin/env python3
"""Cost of the guided infill (gmupt_infill_image: k_if_prepare + one k_if_pass per pass) on the bench scene's AOVs (config 3, the seeded
~260k-triangle sphere room) at 1920x1080 and 3840x2160, against the a-trous denoiser on the same images, and the parameter sweep behind
the defaults.

  python tools/infill_bench.py [--reps 9] [--out DIR]              timing: device events per call (ms), median; DIR/infill_bench.json
  rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o if -- python tools/infill_bench.py --reps 5 --no-json
  python tools/infill_bench.py --parse-trace DIR/prof [--out DIR]  per-kernel medians of that run, per size, hole fraction and pass;
                                                                   DIR/infill_kernels.json
  python tools/infill_bench.py --sweep [--out DIR]                 quality sweep on progressive starts; DIR/quality_sweep.txt

Frames: the AOVs of the scene's camera at s = 1, beauty images made from their albedo plus seeded noise with 1..2 samples per pixel, of
which a fraction (HOLES) is set to no sample at random.  Per size and fraction the tool runs one warm call and `reps` timed calls of
gmupt_infill_image (default parameters, six passes) and then `reps` calls of gmupt_denoise_image on the filled image: the yardstick is
one k_dn_atrous pass of that same job.  --parse-trace relies on this order: a k_if_prepare that follows a k_dn_atrous starts the next
(size, fraction) pair.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = [(1920, 1080), (3840, 2160)]
HOLES = [0.0, 0.5, 0.9, 0.99]


def timing(args):
    import numpy as np
    import torch
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    os.environ.setdefault("GMUPT_TRAVERSAL", "wide")
    dev = capi.Device(0)
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    sb = capi.SceneBuffers(dev, scene)
    results = []
    for (W, H) in SIZES:
        r = capi.Renderer(dev, W, H, pool_paths=1 << 16)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
        r.set_camera(cam.buffer)
        aov = r.aovs(1)
        alb = aov.cpu().numpy()[..., 0:3]
        rng = np.random.default_rng(1)
        rgb = np.clip(alb * 0.6 + rng.normal(0, 0.15, alb.shape), 0, 1).astype(np.float32)
        count = rng.integers(1, 3, (H, W)).astype(np.uint32)
        pick = rng.random((H, W))
        for frac in HOLES:
            b = np.empty((H, W, 4), np.float32)
            hole = pick < frac
            b[..., :3] = np.where(hole[..., None], 0.0, rgb)
            b[..., 3] = np.where(hole, 0, count).astype(np.uint32).view(np.float32)
            bt = torch.from_numpy(b).cuda()
            filled, info = capi.infill_image(r, bt, aov, info=True)       # warm: grows the scratch
            ms_if, ms_dn = [], []
            for _ in range(args.reps):
                ms_if.append(capi.infill_image(r, bt, aov, info=True)[1]["ms"])
            for _ in range(args.reps):
                capi.denoise_image(r, filled, aov, ms=ms_dn)
            row = {"size": [W, H], "hole_fraction": frac, "reps": args.reps, "sources": info["sources"], "holes": info["holes"],
                   "filled": info["filled"], "open_left": info["open_left"], "ms_infill_image": statistics.median(ms_if),
                   "ms_denoise_image": statistics.median(ms_dn), "ms_all_infill_calls": ms_if}
            print(json.dumps(row), flush=True)
            results.append(row)
        r.close(); cam.close()
    sb.close(); dev.close()
    if not args.no_json:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "infill_bench.json"), "w") as f:
            json.dump({"scene": scene["name"], "results": results}, f, indent=1)


def parse_trace(args):
    """Per-kernel medians (microseconds) of a rocprofv3 --kernel-trace run of the timing mode, per (size, fraction) pair and pass."""
    files = sorted(glob.glob(os.path.join(args.parse_trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % args.parse_trace)
    rows = []
    for fn in files:
        with open(fn, newline="") as f:
            for rec in csv.DictReader(f):
                rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), rec["Kernel_Name"]))
    rows.sort()
    pairs = [(s, h) for s in SIZES for h in HOLES]
    segs, seg, last, k = [], None, None, 0
    for start, end, name in rows:
        short = next((n for n in ("k_if_prepare", "k_if_pass", "k_dn_prepare", "k_dn_variance", "k_dn_atrous") if n in name), None)
        if short is None:
            continue
        if short == "k_if_prepare":
            if last in (None, "k_dn_atrous"):
                seg = {}; segs.append(seg)
            k = 0
        key = short
        if short == "k_if_pass":
            key = "k_if_pass[%d]" % k; k += 1
        seg.setdefault(key, []).append((end - start) / 1000.0)
        last = short
    out = []
    for (size, frac), seg in zip(pairs, segs):
        row = {"size": list(size), "hole_fraction": frac, "median_us": {key: round(statistics.median(v), 2) for key, v in sorted(seg.items())},
               "launches": {key: len(v) for key, v in sorted(seg.items())}}
        row["median_us"]["k_if_pass (sum of passes)"] = round(sum(v for key, v in row["median_us"].items() if key.startswith("k_if_pass[")), 2)
        print(json.dumps(row))
        out.append(row)
    if len(segs) != len(pairs):
        print("warning: %d segments for %d (size, fraction) pairs" % (len(segs), len(pairs)), file=sys.stderr)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "infill_kernels.json"), "w") as f:
        json.dump({"unit": "microseconds, median per launch", "results": out}, f, indent=1)


def sweep(args):
    import numpy as np
    import torch
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    os.environ.setdefault("GMUPT_TRAVERSAL", "wide")
    dev = capi.Device(0)
    W, H = 96, 54
    lines = ["infill quality sweep: progressive start (pool 512, 3 iterations, yaw +2), %dx%d, MSE over surface pixels vs 1024 spp; infill + default denoise" % (W, H)]
    for name, mesh in (("cornell", pkg.scenes.cornell_mesh()), ("textured", pkg.scenes.textured_mesh())):
        scene = pkg.scenes.build_scene(mesh)
        sb = capi.SceneBuffers(dev, scene)
        x, y, z, pitch, yaw = scene["camera"]
        pose = (x, y, z, pitch, yaw + 2.0)
        r = capi.Renderer(dev, W, H, pool_paths=1 << 16, path_budget=W * H * 1024); r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*pose); cam.buffer.lightCount = scene["light_count"]
        r.render_budget(cam, 1 << 20); ref = r.framebuffer(); r.close(); cam.close()
        rp = capi.Renderer(dev, W, H, pool_paths=512); rp.bind_scene(sb)
        cp = capi.Camera(W, H); cp.set_pose(*pose); cp.buffer.lightCount = scene["light_count"]; cp.update(0.0)
        for _ in range(3):
            cp.update(0.0); rp.set_camera(cp.buffer); rp.iterate()
        fp = torch.from_numpy(rp.framebuffer()).cuda(); aov = rp.aovs(2)
        f = aov.cpu().numpy().view(np.uint32); surf = (f[..., 12].view(np.int32) != -1) & (f[..., 14] == 0)
        mse = lambda a: float(((a.cpu().numpy()[..., :3].astype(np.float64) - ref[..., :3]) ** 2)[surf].mean())
        base = mse(capi.denoise_image(rp, fp, aov))
        lines.append("%s: surface pixels %d, denoise alone MSE %.6f" % (name, surf.sum(), base))
        lines.append("  passes sigma_n sigma_x sigma_a   holes filled open_left   MSE      gain")
        for passes in (4, 6, 8):
            for sn in (128.0, 32.0, 8.0, 2.0):
                for sx in (0.02, 0.1):
                    for sa in (0.1, 0.5):
                        filled, info = capi.infill_image(rp, fp, aov, info=True, passes=passes, sigma_normal=sn, sigma_plane=sx, sigma_albedo=sa)
                        m = mse(capi.denoise_image(rp, filled, aov))
                        lines.append("  %6d %7g %7g %7g %7d %6d %9d   %.6f %6.2f" % (passes, sn, sx, sa, info["holes"], info["filled"], info["open_left"], m, base / m))
                        print(lines[-1], flush=True)
        rp.close(); cp.close(); sb.close()
    dev.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "quality_sweep.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="profiles/infill")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--parse-trace", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.parse_trace:
        parse_trace(a)
    elif a.sweep:
        sweep(a)
    else:
        timing(a)

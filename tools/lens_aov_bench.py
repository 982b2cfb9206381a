#!/usr/bin/env python3
"""Cost of the lens-filtered AOV planes (gmupt_render_aovs_lens) on the bench scene (config 3: the seeded ~260k-triangle sphere room) at
1920x1080, next to gmupt_render_aovs at the same sample count in the same process -- unchanged code, so it stands for the parent.

  python tools/lens_aov_bench.py [--samples 1 2 4] [--reps 7] [--out DIR]                 timing: device time per call (info.ms), median
  rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o laov -- python tools/lens_aov_bench.py --profile-pass --prof DIR/prof [--reps 3]
  python tools/lens_aov_bench.py --split DIR/prof [--out DIR]                             raygen / walk / resolve per call from the trace

The timing pass prints one JSON line per (sample count, kind) -- kind = "pinhole" (gmupt_render_aovs, s*s + 1 rays per pixel, 1 at s = 1),
"lens0" (aperture 0) and "lens" (aperture APERTURE, focused at FOCUS) -- and writes DIR/lens_aov_bench.json: ms per call, rays per call and
G rays/s of the whole call.  The profile pass makes the pinhole and the open-lens calls in a fixed order (one warm-up call, then --reps,
per sample count and kind) and writes the order to DIR/prof/order.json; --split assigns the traced dispatches of k_(l)aov_raygen,
k_cast_w<..QueryIO> and k_(l)aov_resolve to the calls in that order and writes DIR/lens_aov_split.json: medians over the calls, summed
over the chunks of a call, the walk's own G rays/s for lens rays next to pinhole rays, and raygen + resolve as a share of the call.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H = 1920, 1080
CHUNK = 1 << 21
APERTURE, FOCUS = 0.3, 11.0   # 3 % of the room's width, focused at the depth of the camera's distance to the room's centre


def rays_per_pixel(s, kind):
    return s * s if kind != "pinhole" else 1 if s == 1 else s * s + 1


def chunks(s, kind):
    rows = CHUNK // (W * rays_per_pixel(s, kind))
    return (H + rows - 1) // rows


def setup():
    import torch  # noqa: F401  (first: torch's HIP runtime is the one libgmupt binds to)
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, W, H, pool_paths=1 << 21)          # the bench pool, as tools/aov_bench.py
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    r.set_camera(cam.buffer)
    lenses = {"lens0": capi.lens.lens_params(aperture_radius=0.0, focus_distance=FOCUS), "lens": capi.lens.lens_params(aperture_radius=APERTURE, focus_distance=FOCUS)}

    def call(kind, s, info=None):
        return r.aovs(s, info=info) if kind == "pinhole" else capi.lens_aov.aovs(r, s, lenses[kind], info=info)
    return capi, r, call, (cam, sb, dev)


def timing(args):
    import numpy as np
    capi, r, call, keep = setup()
    out = []
    for s in args.samples:
        for kind in ("pinhole", "lens0", "lens"):
            info = capi.TraceInfo()
            call(kind, s, info)                               # warm-up (the first call allocates the chunk scratch)
            ms = []
            for _ in range(args.reps):
                call(kind, s, info)
                ms.append(info.ms)
            n = W * H * rays_per_pixel(s, kind)
            med = float(np.median(ms))
            d = {"samples": s, "kind": kind, "rays": n, "chunks": chunks(s, kind), "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                 "grays_s": round(n / med / 1e6, 3), "redo_rays": int(info.redo_rays)}
            print(json.dumps(d), flush=True)
            out.append(d)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "lens_aov_bench.json"), "w") as f:
        json.dump({"scene": "spheres_mesh(202, 3, seed=1234)", "size": [W, H], "reps": args.reps, "aperture": APERTURE, "focus": FOCUS, "calls": out}, f, indent=1)
    r.close()


def profile_pass(args):
    capi, r, call, keep = setup()
    order = []
    for s in args.samples:
        for kind in ("pinhole", "lens"):
            for _ in range(1 + args.reps):
                call(kind, s)
            order.append({"samples": s, "kind": kind, "calls": 1 + args.reps, "warmup": 1, "chunks": chunks(s, kind), "rays": W * H * rays_per_pixel(s, kind)})
    os.makedirs(args.prof, exist_ok=True)
    with open(os.path.join(args.prof, "order.json"), "w") as f:
        json.dump(order, f)
    r.close()


def split(args):
    import numpy as np
    order = json.load(open(os.path.join(args.split, "order.json")))
    files = glob.glob(os.path.join(args.split, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    kind = lambda n: "raygen" if "aov_raygen" in n else "resolve" if "aov_resolve" in n else "walk" if ("k_cast_w" in n and "QueryIO" in n) else None
    disp = sorted([(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), kind(x["Kernel_Name"])) for x in rows if kind(x["Kernel_Name"])])
    pos = 0
    out = []
    for o in order:
        per_call = []
        for c in range(o["calls"]):
            seq = disp[pos:pos + 3 * o["chunks"]]
            pos += 3 * o["chunks"]
            assert [k for _, _, k in seq] == ["raygen", "walk", "resolve"] * o["chunks"], "unexpected dispatch order"
            if c < o["warmup"]:
                continue
            t = {k: sum(e - b for b, e, kk in seq if kk == k) / 1e6 for k in ("raygen", "walk", "resolve")}
            per_call.append(t)
        med = {k: float(np.median([t[k] for t in per_call])) for k in ("raygen", "walk", "resolve")}
        busy = med["raygen"] + med["walk"] + med["resolve"]
        d = {"samples": o["samples"], "kind": o["kind"], "chunks": o["chunks"], "calls": len(per_call), "ms": {k: round(v, 4) for k, v in med.items()},
             "walk_grays_s": round(o["rays"] / med["walk"] / 1e6, 3), "raygen_plus_resolve_share": round((med["raygen"] + med["resolve"]) / busy, 4)}
        print(json.dumps(d), flush=True)
        out.append(d)
    assert pos == len(disp), "dispatches left over: %d of %d" % (len(disp) - pos, len(disp))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "lens_aov_split.json"), "w") as f:
        json.dump({"trace": "rocprofv3 --kernel-trace --stats", "size": [W, H], "aperture": APERTURE, "focus": FOCUS, "calls": out}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/lens_aov")
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--prof", default=None, help="--profile-pass: where order.json goes (the rocprofv3 -d directory)")
    ap.add_argument("--split", default=None, help="rocprofv3 output directory of a --profile-pass run")
    args = ap.parse_args()
    if args.split:
        split(args)
    elif args.profile_pass:
        if not args.prof:
            ap.error("--profile-pass needs --prof DIR (the rocprofv3 output directory)")
        profile_pass(args)
    else:
        timing(args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the a-trous denoiser (gmupt_denoise_image, 5 passes) on a frame of the bench scene (config 3: the seeded ~260k-triangle sphere
room: its AOVs at s = 1 and a noisy beauty image made from their albedo), at 1920x1080 and 3840x2160, with gmupt_denoise_host on 16 threads as the CPU figure.

  python tools/denoise_bench.py [--reps 9] [--out DIR]                                       timing: device events per call (ms), median
  rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o dn -- python tools/denoise_bench.py --profile-pass --prof DIR/prof [--reps 5]
  python tools/denoise_bench.py --split DIR/prof [--out DIR]                                 per kernel and per pass from the trace

The gathered bytes of a pass are counted from the layout of csrc/pt_guides.hpp over the frame's actual valid pixels: per valid pixel the
centre (col 16 + nw 16 + xa 16 + ag 8 + z 4 B), the variance words of its in-image 3x3 neighbours (4 B each), 16 B of col per in-image tap and
40 B more (nw, xa, ag) per valid one, and the 16 B store; an invalid pixel reads 16 B and writes 16 B.  The timing pass writes
DIR/denoise_bench.json; --split writes DIR/denoise_split.json (medians over the calls).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = [(1920, 1080), (3840, 2160)]
PASSES = 5
TAP_COL, TAP_GUIDE, CENTRE, STORE, VAR_WORD = 16, 40, 60, 16, 4


def frame(pkg, dev, sb, scene, W, H):
    """The bench scene's AOVs at W x H (s = 1) and a beauty image made from them (albedo * 0.6 + seeded noise, one sample per pixel):
    (beauty, aov) torch tensors on the GPU, and the renderer.  The filter's work depends on which pixels are valid, which the AOVs decide."""
    import numpy as np
    import torch
    capi = pkg.capi
    r = capi.Renderer(dev, W, H, pool_paths=1 << 16)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
    r.set_camera(cam.buffer)
    aov = r.aovs(1)
    alb = aov.cpu().numpy()[..., 0:3]
    b = np.empty(alb.shape[:2] + (4,), np.float32)
    b[..., :3] = np.clip(alb * 0.6 + np.random.default_rng(1).normal(0, 0.15, alb.shape), 0, 1)
    b[..., 3] = np.uint32(1).view(np.float32)
    return r, cam, torch.from_numpy(b).cuda(), aov


def gathered_bytes(beauty, aov, passes=PASSES):
    """Bytes each pass reads + writes by the layout of pt_guides.hpp, over this frame's valid pixels (see the module text)."""
    import numpy as np
    b = beauty.cpu().numpy(); a = aov.cpu().numpy()
    u = a.view(np.uint32)
    n = a[..., 4:7].astype(np.float64)
    valid = (b[..., 3].view(np.uint32) > 0) & (u[..., 12].view(np.int32) != -1) & (u[..., 14] == 0) & ((n * n).sum(-1) > 0)
    H, W = valid.shape

    def count(dy, dx):   # per pixel: is p + (dx, dy) inside the image, and is it valid
        ins = np.zeros((H, W), bool); ok = np.zeros((H, W), bool)
        if abs(dy) < H and abs(dx) < W:
            dst = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            src = (slice(max(0, dy), H + min(0, dy)), slice(max(0, dx), W + min(0, dx)))
            ins[dst] = True; ok[dst] = valid[src]
        return ins, ok

    gauss = sum(count(dy, dx)[0].astype(np.int64) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    out = []
    for k in range(passes):
        s = 1 << k
        tap_col = np.zeros((H, W), np.int64); tap_guide = np.zeros((H, W), np.int64)
        for j in range(-2, 3):
            for i in range(-2, 3):
                ins, ok = count(s * j, s * i)
                tap_col += ins; tap_guide += ok
        per_valid = CENTRE + VAR_WORD * gauss + TAP_COL * tap_col + TAP_GUIDE * tap_guide + STORE
        total = int(per_valid[valid].sum()) + int((~valid).sum()) * (16 + STORE)
        out.append({"pass": k, "step": s, "bytes": total, "taps_per_valid_pixel": round(float(tap_guide[valid].mean()), 3)})
    return out, float(valid.mean())


def setup():
    import torch  # noqa: F401  (first: torch's HIP runtime is the one libgmupt binds to)
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    return pkg, capi, scene, dev, sb


def timing(args):
    import numpy as np
    pkg, capi, scene, dev, sb = setup()
    out = []
    for (W, H) in SIZES:
        r, cam, beauty, aov = frame(pkg, dev, sb, scene, W, H)
        capi.denoise_image(r, beauty, aov)                            # warm-up (first call allocates the scratch)
        ms = []
        for _ in range(args.reps):
            capi.denoise_image(r, beauty, aov, ms=ms)
        host = []
        b_np, a_np = beauty.cpu().numpy(), aov.cpu().numpy()
        for _ in range(3):
            t0 = time.perf_counter(); capi.denoise_host(b_np, a_np, threads=16); host.append((time.perf_counter() - t0) * 1e3)
        per_pass, valid = gathered_bytes(beauty, aov)
        med = float(np.median(ms))
        d = {"size": [W, H], "passes": PASSES, "valid_fraction": round(valid, 4), "ms": round(med, 4), "ms_min": round(min(ms), 4),
             "ms_max": round(max(ms), 4), "reps": args.reps, "host_ms_16_threads": round(float(np.median(host)), 1),
             "bytes_per_pass": per_pass, "scratch_bytes": W * H * 76}
        print(json.dumps(d), flush=True)
        out.append(d)
        r.close(); cam.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "denoise_bench.json"), "w") as f:
        json.dump({"scene": "spheres_mesh(202, 3, seed=1234): AOVs s = 1, beauty = albedo * 0.6 + N(0, 0.15), 1 sample", "calls": out}, f, indent=1)


def profile_pass(args):
    pkg, capi, scene, dev, sb = setup()
    order = []
    for (W, H) in SIZES:
        r, cam, beauty, aov = frame(pkg, dev, sb, scene, W, H)
        for _ in range(1 + args.reps):
            capi.denoise_image(r, beauty, aov)
        order.append({"size": [W, H], "calls": 1 + args.reps, "warmup": 1})
        r.close(); cam.close()
    os.makedirs(args.prof, exist_ok=True)
    with open(os.path.join(args.prof, "order.json"), "w") as f:
        json.dump(order, f)


def split(args):
    import numpy as np
    order = json.load(open(os.path.join(args.split, "order.json")))
    files = glob.glob(os.path.join(args.split, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    kind = lambda n: "prepare" if "k_dn_prepare" in n else "variance" if "k_dn_variance" in n else "atrous" if "k_dn_atrous" in n else None
    disp = sorted([(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), kind(x["Kernel_Name"])) for x in rows if kind(x["Kernel_Name"])])
    per_call = 2 + PASSES
    names = ["prepare", "variance"] + ["pass%d" % k for k in range(PASSES)]
    pos = 0
    out = []
    for o in order:
        calls = []
        for c in range(o["calls"]):
            seq = disp[pos:pos + per_call]
            pos += per_call
            assert [k for _, _, k in seq] == ["prepare", "variance"] + ["atrous"] * PASSES, "unexpected dispatch order"
            if c >= o["warmup"]:
                t = {n: (e - b) / 1e6 for n, (b, e, _) in zip(names, seq)}
                t["span"] = (seq[-1][1] - seq[0][0]) / 1e6
                calls.append(t)
        med = {k: round(float(np.median([t[k] for t in calls])), 4) for k in names + ["span"]}
        d = {"size": o["size"], "calls": len(calls), "ms": med}
        print(json.dumps(d), flush=True)
        out.append(d)
    assert pos == len(disp), "dispatches left over: %d of %d" % (len(disp) - pos, len(disp))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "denoise_split.json"), "w") as f:
        json.dump({"trace": "rocprofv3 --kernel-trace --stats", "calls": out}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", default=None, help="WxH: only this size (e.g. for a rocprofv3 --pmc pass of its own)")
    ap.add_argument("--out", default="profiles/r06_denoise")
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--prof", default=None, help="--profile-pass: where order.json goes (the rocprofv3 -d directory)")
    ap.add_argument("--split", default=None, help="rocprofv3 output directory of a --profile-pass run")
    args = ap.parse_args()
    if args.size:
        SIZES[:] = [tuple(int(v) for v in args.size.split("x"))]
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

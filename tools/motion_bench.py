#!/usr/bin/env python3
"""Cost of motion-aware temporal reuse on the bench scene (config 3, the seeded ~260k-triangle sphere room) at 1920x1080 and 3840x2160:
k_mv_resolve (gmupt_render_aovs_motion against gmupt_render_aovs), k_tp_integrate_mv (gmupt_temporal_denoise_image_motion against
gmupt_temporal_denoise_image), the whole call gmupt_render_denoised_temporal_motion after a refit against gmupt_render_denoised_temporal
on the same frame, and the pose snapshot.

  python tools/motion_bench.py [--reps 9] [--size WxH] [--out DIR] [--label NAME]     device events per call (ms), medians; DIR/motion_bench_NAME.json
  python tools/motion_bench.py --tree PARENT_CHECKOUT --label parent ...              the same script on another (built) checkout: the arms it has
  python tools/motion_bench.py --scene config5 [--reps 5]                             whole call and snapshot at 64x36 on the 10 M-triangle scene
  rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o NAME -- python tools/motion_bench.py --reps 5 --size 1920x1080 --no-json
  python tools/motion_bench.py --summarise DIR/prof --out DIR                         DIR/kernel_stats.txt from the *_kernel_stats.csv files

A checkout without the motion entry points (the parent commit) runs the plain arms only, so one job can alternate the two trees.

Frames: pose 0 is the scene as built, pose k = scenes.wobble(phase 0.1 + 0.05 k, amplitude 0.01), uploaded and refitted.
  aovs / aovs_motion: TraceInfo.ms of the call (device events around all chunks) at pose 1, the motion plane against pose 0.
  image calls: beauty images made from the albedo plus seeded noise with 0..2 samples per pixel (as tools/temporal_bench.py); call 1
    integrates pose 0, the timed calls integrate pose 1 against those records (new_accumulation = 0), with and without the motion plane.
  whole call: per repetition a new pose, refit, restart, two iterations, then the first call (it folds; with the motion entry it takes the
    snapshot) and a second call on the same frame (no fold, no snapshot): TraceInfo.ms (AOVs + integration + filter, device) and wall clock.
    The plain entry runs on the same frames through a handle of its own.
  snapshot: wall(first) - wall(second) of the motion entry, and a device-to-device copy of the vertex buffer's size timed with events.
Bytes per pixel by layout: k_mv_resolve 32 (hit) + 16 (triangle record) + 72 (six vertices) + 16 (position) + 16 (store) = 152 on a surface
pixel, 48 elsewhere; k_tp_integrate_mv adds 16 to the 336 of k_tp_integrate on a surface pixel with taps.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1920, 1080), (3840, 2160)]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)} if xs else None


def beauty_from(aov, rng):
    import numpy as np
    import torch
    alb = aov.cpu().numpy()[..., 0:3]
    b = np.empty(alb.shape[:2] + (4,), np.float32)
    b[..., :3] = np.clip(alb * 0.6 + rng.normal(0, 0.15, alb.shape), 0, 1)
    b[..., 3] = rng.integers(0, 3, alb.shape[:2]).astype(np.uint32).view(np.float32)
    return torch.from_numpy(b).cuda()


def d2d_copy_ms(nbytes, reps):
    import torch
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda"); b = torch.empty_like(a)
    b.copy_(a); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def whole_call(pkg, r, sb, scene, cam, reps, amplitude, has_motion):
    """Per repetition: a new pose, refit, restart, two iterations, first and second call of each entry on that frame."""
    capi = pkg.capi
    arms = {"plain": (capi.Temporal(r), r.denoise_temporal)}
    if has_motion:
        arms["motion"] = (capi.Temporal(r), r.denoise_temporal_motion)
    res = {k: {"first_device_ms": [], "first_wall_ms": [], "second_device_ms": [], "second_wall_ms": []} for k in arms}

    def frames(n):
        for _ in range(n):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        r.synchronize()

    cam.reset_accumulation(); frames(2)
    for t, call in arms.values():
        call(t, 1)
    for k in range(reps + 1):                         # repetition 0 warms up (scratch growth, the first refit's upload)
        sb.verts.update(pkg.scenes.wobble(scene, 0.1 + 0.05 * k, amplitude)); r.refit()
        cam.reset_accumulation(); frames(2)
        order = list(arms) if k % 2 == 0 else list(arms)[::-1]
        for name in order:
            t, call = arms[name]
            for which in ("first", "second"):
                info = capi.TraceInfo()
                t0 = time.perf_counter(); call(t, 1, info=info); wall = (time.perf_counter() - t0) * 1e3
                if k:
                    res[name][which + "_device_ms"].append(info.ms); res[name][which + "_wall_ms"].append(wall)
    for t, _ in arms.values():
        t.close()
    return {k: {m: med(v) for m, v in d.items()} for k, d in res.items()}


def timing(args, pkg):
    import numpy as np
    import torch
    capi = pkg.capi
    has_motion = hasattr(capi.Renderer, "aovs_motion")
    os.environ.setdefault("GMUPT_TRAVERSAL", "wide")
    dev = capi.Device(0)
    S = pkg.scenes
    config5 = args.scene == "config5"
    scene = S.build_scene(S.spheres_mesh(1953, 4, seed=1234) if config5 else S.spheres_mesh(202, 3, seed=1234))
    nv = int(len(scene["verts"]))
    sizes = [(64, 36)] if config5 else ([tuple(map(int, args.size.split("x")))] if args.size else SIZES)
    results = []
    for (W, H) in sizes:
        sb = capi.SceneBuffers(dev, scene)
        r = capi.Renderer(dev, W, H, pool_paths=1 << 16)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
        r.set_camera(cam.buffer)
        row = {"size": [W, H], "reps": args.reps, "vertices": nv, "snapshot_bytes": nv * 12}
        rng = np.random.default_rng(1)
        if not config5:
            prev = scene["verts"]
            aov0 = r.aovs(1); b0 = beauty_from(aov0, rng); cam0 = cam.buffer_copy()
            sb.verts.update(S.wobble(scene, 0.1, args.amplitude)); r.refit()
            pv = torch.from_numpy(prev).cuda()
            aov1 = r.aovs(1); b1 = beauty_from(aov1, rng)
            mv = r.aovs_motion(pv, 1)[1] if has_motion else None
            t_a, t_m = [], []
            for _ in range(args.reps):
                i = capi.TraceInfo(); r.aovs(1, info=i); t_a.append(i.ms)
                if has_motion:
                    i = capi.TraceInfo(); r.aovs_motion(pv, 1, info=i); t_m.append(i.ms)
            row["ms_aovs"] = med(t_a); row["ms_aovs_motion"] = med(t_m)
            t = capi.Temporal(r)
            capi.temporal_denoise_image(t, b0, aov0, cam0, True)
            capi.temporal_denoise_image(t, b1, aov1, cam0, True)      # warm: folds pose 0 into the history
            t_p, t_v = [], []
            for _ in range(args.reps):
                capi.temporal_denoise_image(t, b1, aov1, cam0, False, ms=t_p)
                if has_motion:
                    capi.temporal_denoise_image(t, b1, aov1, cam0, False, ms=t_v, motion=mv)
            row["ms_temporal_image"] = med(t_p); row["ms_temporal_image_motion"] = med(t_v)
            if has_motion:
                f = capi.motion_fields(mv)
                row["surface_pixels"] = int((f["flags"] == 1).sum())
                row["moved_pixels"] = int((f["prev_position"] != aov1.cpu().numpy()[..., 8:11]).any(-1).sum())
            t.close()
        row["whole_call"] = whole_call(pkg, r, sb, scene, cam, args.reps, args.amplitude, has_motion)
        row["ms_d2d_copy_of_snapshot_size"] = med(d2d_copy_ms(nv * 12, args.reps))
        if has_motion:
            w = row["whole_call"]["motion"]
            row["ms_snapshot_wall_first_minus_second"] = w["first_wall_ms"]["median"] - w["second_wall_ms"]["median"]
        print(json.dumps(row), flush=True)
        results.append(row)
        r.close(); sb.close(); cam.close()
    dev.close()
    if not args.no_json:
        os.makedirs(args.out, exist_ok=True)
        name = "motion_bench_%s%s.json" % (args.label, "_config5" if config5 else "")
        with open(os.path.join(args.out, name), "w") as f:
            json.dump({"scene": scene["name"], "triangles": scene["num_triangles"], "tree": args.label, "has_motion_entry_points": has_motion,
                       "results": results}, f, indent=1)


def summarise(args):
    """One line per kernel of every *_kernel_stats.csv under the directory: calls, total / average / min / max in microseconds."""
    lines = []
    for path in sorted(glob.glob(os.path.join(args.summarise, "**", "*kernel_stats.csv"), recursive=True)):
        lines.append("== " + os.path.relpath(path, args.summarise))
        with open(path) as f:
            for row in csv.DictReader(f):
                ns = lambda k: float(row.get(k) or 0) / 1e3
                lines.append("%-60s calls %6s  total %12.1f us  avg %10.2f us  min %10.2f  max %10.2f  %5.1f %%" % (
                    str(row.get("Name")).split("(")[0][:60], row.get("Calls"), ns("TotalDurationNs"), ns("AverageNs"), ns("MinNs"), ns("MaxNs"), float(row.get("Percentage") or 0)))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "kernel_stats.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", default="")
    ap.add_argument("--scene", default="bench", choices=["bench", "config5"])
    ap.add_argument("--amplitude", type=float, default=0.01)
    ap.add_argument("--tree", default=HERE_ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default="profiles/motion")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--summarise", default="")
    a = ap.parse_args()
    if a.summarise:
        summarise(a)
    else:
        root = os.path.abspath(a.tree)
        for _p in (root, os.path.join(root, "tests")):
            sys.path.insert(0, _p)
        import gmupt_pkg
        timing(a, gmupt_pkg.load())

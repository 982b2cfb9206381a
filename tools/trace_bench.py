#!/usr/bin/env python3
"""Throughput of the ray-query API (gmupt_trace_rays) on the bench scene (config 3: the seeded ~260k-triangle sphere room).

  python tools/trace_bench.py [--prewarm 400] [--iters 20] [--reps 5] [--out DIR]

Three cases, each as one gmupt_trace_rays call (device time of the launch, median of --reps calls):
  (a) pipeline  the extension + shadow rays of one steady-state iteration (pool 2^21, 1920x1080), read from the path state after the
                shading stage and traced in one call; next to it ms_extend of the renderer's own fused ray cast (gmupt_enable_timing(r, 2),
                mean over --iters iterations just before)
  (b) primary   1920x1080 closest-hit rays through the pixel corners of the camera (gmupt_camera_pick_ray's formula, vectorised): coherent
  (c) random    2^21 uniformly random rays (origins in the scene's box, isotropic directions): incoherent; closest hit and any hit
Prints one JSON line and writes it to DIR/trace_bench.json.
"""
import argparse
import json
import os
import sys
import time

import torch   # first: torch's HIP runtime is the one libgmupt binds to

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FLT_MAX = np.finfo(np.float32).max


def pick_rays(cb, w, h):
    """gmupt_camera_pick_ray for every pixel of a w x h frame (newPath.hlsl:36-39, jitter 0), in binary32."""
    f = np.float32
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs.ravel().astype(f) * f(cb.pixelSize[0]))[:, None]
    v = (ys.ravel().astype(f) * f(cb.pixelSize[1]))[:, None]
    ulc = np.array(cb.upperLeftCorner[:3], f); hor = np.array(cb.horizontal[:3], f); ver = np.array(cb.vertical[:3], f)
    d = ((ulc + hor * u) - ver * v).astype(f)
    dot = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d = d * (f(1.0) / np.sqrt(dot))[:, None]
    r = np.zeros((w * h, 8), f)
    r[:, 0:3] = np.array(cb.position[:3], f); r[:, 3] = FLT_MAX; r[:, 4:7] = d
    return r


def timed(r, capi, closest, any_rays, reps, light_count):
    ms = []
    info = capi.TraceInfo()
    for _ in range(reps):
        r.trace(closest, any_rays, light_count=light_count, info=info)
        ms.append(info.ms)
    return float(np.median(ms)), int(info.redo_rays)


def case(name, n, ms, redo, **extra):
    d = {"case": name, "rays": n, "ms": round(ms, 4), "grays_s": round(n / ms / 1e6, 3), "redo_rays": redo}
    d.update(extra)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prewarm", type=int, default=400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/r04_trace")
    args = ap.parse_args()
    import gmupt_pkg
    import oracle_lib as O    # (the reference path-state layout of the debug readers only)
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    W, H, P = 1920, 1080, 1 << 21
    scene = pkg.scenes.build_scene(pkg.scenes.spheres_mesh(202, 3, seed=1234))
    lc = scene["light_count"]
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, W, H, pool_paths=P)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = lc

    def step(n):
        for _ in range(n):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()

    step(args.prewarm); r.synchronize()
    r.reset_stats(); r.enable_timing(2)
    step(args.iters)
    st = r.stats()
    ms_extend = st.ms_extend / max(st.timed_iterations, 1)
    r.enable_timing(0)
    # (a) one iteration's rays: shade, read them, trace them in one call
    cam.update(0.0); r.set_camera(cam.buffer)
    r.run_stage(capi.STAGE_SHADE)
    state, q, qc = r.read_path_state(), r.read_queues(), r.counters()
    ext = q[3][: qc[7]]; ext = ext[ext != 0xFFFFFFFF]
    sh = q[4][: qc[6]]
    f32 = lambda name: O.state_field(state, P, name).view(np.float32)
    closest = np.zeros((len(ext), 8), np.float32); closest[:, 0:3] = f32("rayOrigin")[ext]; closest[:, 3] = FLT_MAX; closest[:, 4:7] = f32("rayDirection")[ext]
    anyr = np.zeros((len(sh), 8), np.float32); anyr[:, 0:3] = f32("shadowrayOrigin")[sh]; anyr[:, 3] = f32("lightDistance")[sh, 0]; anyr[:, 4:7] = f32("shadowrayDirection")[sh]
    c, a = torch.from_numpy(closest).cuda(), torch.from_numpy(anyr).cuda()
    ms_a, redo_a = timed(r, capi, c, a, args.reps, lc)
    res = [case("pipeline", len(ext) + len(sh), ms_a, redo_a, closest=len(ext), any=len(sh), ms_extend=round(ms_extend, 4),
                ratio_to_ms_extend=round(ms_a / ms_extend, 4) if ms_extend > 0 else None)]
    del c, a
    # (b) primary rays of the whole frame
    prim = torch.from_numpy(pick_rays(cam.buffer_copy(), W, H)).cuda()
    ms_b, redo_b = timed(r, capi, prim, None, args.reps, lc)
    res.append(case("primary", W * H, ms_b, redo_b))
    del prim
    # (c) random rays
    rng = np.random.default_rng(7)
    v = scene["verts"].reshape(-1, 3); lo, hi = v.min(axis=0), v.max(axis=0)
    n = 1 << 21
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32); rays[:, 0:3] = o; rays[:, 3] = FLT_MAX; rays[:, 4:7] = d
    rc = torch.from_numpy(rays).cuda()
    ms_c, redo_c = timed(r, capi, rc, None, args.reps, lc)
    res.append(case("random_closest", n, ms_c, redo_c))
    rays[:, 3] = np.float32(np.linalg.norm(hi - lo) * 0.25)
    ra = torch.from_numpy(rays).cuda()
    ms_d, redo_d = timed(r, capi, None, ra, args.reps, lc)
    res.append(case("random_any", n, ms_d, redo_d, tmax=float(rays[0, 3])))
    out = {"metric": "gmupt_trace_rays throughput", "scene": "config3: %d-tri seeded sphere room" % scene["num_triangles"],
           "gpu": torch.cuda.get_device_name(0), "prewarm": args.prewarm, "reps": args.reps, "cases": res,
           "time": time.strftime("%Y-%m-%d %H:%M:%S")}
    line = json.dumps(out)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "trace_bench.json"), "w") as fh:
        fh.write(line + "\n")
    r.close(); sb.close(); cam.close(); dev.close()


if __name__ == "__main__":
    main()

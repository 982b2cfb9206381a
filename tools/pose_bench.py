"""The pose stage: k_ps_pose against a memory floor, and the whole set_pose step against the route a caller had before it.

  1  kernel   capi.Pose.update(info=True) -- info.ms, the device time of the two small copies and the two launches -- for K = 4 influences,
              J = 64 joints and T = 0 targets / T = 4 with 2 active, at the vertex count of --scene and at --big vertices (10 M).  The
              floor: a device-to-device copy (torch copy_ of a contiguous byte tensor: hipMemcpyAsync) that moves the same number of
              bytes -- it copies HALF the bytes the launch reads and writes by the handle's layout (per vertex 12 of rest position, 6 per
              influence, 12 per ACTIVE target, 12 stored), so that its reads plus its writes are that count -- timed with events in the
              same process, alternated with the update.  ratio = update / copy: the fixed part of the update (two copies of a few
              kilobytes, the one-block launch) is inside it and weighs most at small vertex counts.
              The big case binds a scene of a few triangles whose vertex buffer is padded to --big vertices (a vertex no triangle uses
              may hold anything), with a rig drawn on the device.
  2  step     A: gmupt_pose_host on 16 threads, then ProgressiveSession.set_vertices(host array, normals="smooth") -- pose on the CPU,
              whole-mesh upload.  B: ProgressiveSession.set_pose(normals="smooth").  Wall clock around each (both end in the refit's
              synchronise), alternated in one process, --reps times after one warm-up of each, the phase changing every repetition.
One JSON line; --out FILE also writes it there.

  python tools/pose_bench.py [--scene bench|config5] [--big 10000000] [--reps 10] [--out profiles/pose/bench.json]
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

K, J = 4, 64


def spread(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def layout_bytes(V, active):
    return V * (12 + 6 * K + 12 * active + 12)


def kernel_case(torch, capi, r, V, T, active, reps):
    """Pose.update(info=True) on a device-drawn rig of V vertices against a copy that moves the same bytes, alternated."""
    g = torch.Generator(device="cuda"); g.manual_seed(V + T)
    rest = torch.rand((V, 3), generator=g, device="cuda") * 8 - 4
    joints = torch.randint(0, J, (V, K), generator=g, device="cuda").to(torch.int16)
    weights = torch.rand((V, K), generator=g, device="cuda") + 0.05
    weights = weights / weights.sum(dim=1, keepdim=True)
    deltas = (torch.rand((T, V, 3), generator=g, device="cuda") - 0.5) if T else None
    torch.cuda.synchronize()
    pose = capi.Pose(r, rest, joints, weights, J, deltas)
    del rest, joints, weights, deltas
    mats = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (J, 1)) + np.random.default_rng(1).normal(0, 0.05, (J, 12)).astype(np.float32)
    tw = np.zeros(T, np.float32); tw[:active] = 0.5
    nbytes = layout_bytes(V, active)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").random_(0, 255, generator=g); dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy_ms():
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    pose.update(mats, tw, info=True); copy_ms()           # warm-up of each
    k_ms, c_ms = [], []
    for _ in range(reps):
        info = pose.update(mats, tw, info=True); k_ms.append(info["ms"])
        c_ms.append(copy_ms())
    assert info["active_targets"] == active and info["num_verts"] == V
    pose.close()
    km, cm = float(np.median(k_ms)), float(np.median(c_ms))
    return {"vertices": V, "influences": K, "joints": J, "targets": T, "active_targets": active, "bytes_by_layout": nbytes,
            "pose_update_info_ms_copies_and_both_launches": spread(k_ms), "copy_of_half_those_bytes_ms": spread(c_ms), "ratio_update_over_copy": km / cm,
            "update_bytes_per_second": nbytes / (km * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bench", choices=["bench", "config5"])
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = gmupt_pkg.load()
    capi, S = pkg.capi, pkg.scenes
    mesh = S.spheres_mesh() if args.scene == "bench" else S.spheres_mesh(1953, 4, seed=1234)
    scene = S.build_scene(mesh, builder="lbvh")          # the tree's quality plays no part here; the host LBVH is the quickest to get
    idx_host = np.ascontiguousarray(mesh["indices"], np.int32)
    V = int(len(scene["verts"]))
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, 64, 36, pool_paths=4096)
    r.bind_scene(sb)
    cam = capi.Camera(64, 36); cam.set_pose(*scene["camera"])

    # ---- 1: the kernel against the copy, at the scene's vertex count ...
    kernel = [kernel_case(torch, capi, r, V, T, active, args.reps) for T, active in ((0, 0), (4, 2))]
    sb.verts.update(scene["verts"])

    # ---- 2: the whole step, on the scene's own synthetic rig
    rig = S.make_rig(scene, J, K, 4, seed=0)
    pose = capi.Pose(r, rig["rest"], rig["joints"], rig["weights"], J, rig["deltas"])
    sess = pkg.progressive.ProgressiveSession(r, cam, 64, 36, preview_every=0)

    def arm_a(mats, tw):
        t0 = time.perf_counter()
        verts = capi.pose_host(rig["rest"], rig["joints"], rig["weights"], J, mats, rig["deltas"], tw, threads=16)
        sess.set_vertices(sb, verts, normals="smooth", indices=None)
        return (time.perf_counter() - t0) * 1e3, verts

    def arm_b(mats, tw):
        t0 = time.perf_counter()
        sess.set_pose(sb, pose, mats, tw, normals="smooth")
        return (time.perf_counter() - t0) * 1e3

    def pose_of(k):
        mats, tw = S.rig_pose(rig, 0.02 + 0.013 * k)
        tw[2:] = 0.0                                     # 2 of the 4 targets active
        return mats, tw

    sess.set_vertices(sb, scene["verts"], normals="smooth", indices=idx_host)      # creates the session's Normals before the clock starts
    mats, tw = pose_of(0)
    arm_a(mats, tw); arm_b(mats, tw)                     # warm-up of each
    a_ms, b_ms = [], []
    for k in range(args.reps):
        mats, tw = pose_of(k + 1)
        ms, verts = arm_a(mats, tw); a_ms.append(ms)
        b_ms.append(arm_b(mats, tw))
    same = bool(sb.verts.read(np.float32).tobytes() == verts.tobytes())      # B's bytes are A's
    step = {"scene": scene["name"], "vertices": V, "triangles": int(len(idx_host)), "influences": K, "joints": J, "targets": 4, "active_targets": 2,
            "A_pose_host_16_threads_then_set_vertices_ms": spread(a_ms), "B_set_pose_ms": spread(b_ms),
            "ratio_A_over_B_median": float(np.median(a_ms) / np.median(b_ms)), "B_below_A_in_every_repetition": all(b < a for a, b in zip(a_ms, b_ms)),
            "B_equals_A": same}
    sess.close(); pose.close(); cam.close(); r.close(); sb.close()

    # ---- 1, continued: ... and at --big vertices, on a scene of a few triangles with a padded vertex buffer
    if args.big:
        small = S.random_triangles_mesh(64, seed=3)
        pad = dict(small)
        n0 = len(small["verts"])
        for k, width in (("verts", 3), ("normals", 3)):
            pad[k] = np.zeros((args.big, width), np.float32); pad[k][:n0] = small[k]
        pad["vertex_material"] = np.zeros(args.big, np.uint32); pad["vertex_material"][:n0] = small["vertex_material"]
        big_scene = S.build_scene(pad, builder="lbvh")
        sb = capi.SceneBuffers(dev, big_scene)
        r = capi.Renderer(dev, 64, 36, pool_paths=4096)
        r.bind_scene(sb)
        kernel += [kernel_case(torch, capi, r, args.big, T, active, args.reps) for T, active in ((0, 0), (4, 2))]
        r.close(); sb.close()
    dev.close()

    out = {"kernel": kernel, "step": step}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

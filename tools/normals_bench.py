"""Shading normals after a deformation: what a caller did before gmupt_normals_update against the call itself.

  A   scenes.vertex_normals (float64 numpy, np.add.at) on the host, the property buffer read back, the `normal` column patched, the buffer
      uploaded again: the path of ProgressiveSession.set_vertices(normals=<array>).
  A'  the same with gmupt_vertex_normals_host at 16 threads in place of numpy, so that B is not compared with a slow helper only.
  B   capi.Normals.update(info=True): two launches on the renderer's stream; wall clock around the call (it ends in a synchronise) and
      info.ms, the device time.

The arms run alternated in one process, --reps times, after one warm-up of each, on a pose wobbled by --amplitude (1 %) whose phase
changes every repetition.  Also reported: the one-time cost of Normals() (the index list on the device before the clock starts; first and
second create), the bytes the two launches move by the algorithm's count (per triangle: 12 of indices, 36 of vertices, 16 of face vector
stored; per corner: 4 of corner number, 16 of face vector; per vertex: 8 of offsets and the 12 bytes of the normal) and that count over
info.ms as a share of the 6.29 TB/s copy rate DESIGN.md quotes.  One JSON line; --out FILE also writes it there.

  python tools/normals_bench.py [--scene bench|config5] [--reps 10] [--out profiles/normals/bench.json]
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

COPY_RATE = 6.29e12


def spread(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bench", choices=["bench", "config5"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--amplitude", type=float, default=0.01)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    pkg = gmupt_pkg.load()
    capi, S = pkg.capi, pkg.scenes
    mesh = S.spheres_mesh() if args.scene == "bench" else S.spheres_mesh(1953, 4, seed=1234)
    scene = S.build_scene(mesh, builder="lbvh")          # the tree plays no part here; the host LBVH is the quickest to get
    idx_host = np.ascontiguousarray(mesh["indices"], np.int32)
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, 64, 36, pool_paths=4096)
    r.bind_scene(sb)
    idx = torch.from_numpy(idx_host).cuda()
    torch.cuda.synchronize()

    create_ms = []
    normals = None
    for _ in range(2):
        if normals is not None:
            normals.close()
        t0 = time.perf_counter()
        normals = capi.Normals(r, idx)
        create_ms.append((time.perf_counter() - t0) * 1e3)

    def arm_host(compute):
        def run(w):
            t0 = time.perf_counter()
            n = compute(w)
            props = sb.props.read(capi.tri_props_dtype)
            props["normal"] = n
            sb.props.update(props)
            return (time.perf_counter() - t0) * 1e3
        return run

    arm_a = arm_host(lambda w: S.vertex_normals(w, idx_host))
    arm_a1 = arm_host(lambda w: capi.vertex_normals_host(w, idx_host, threads=16))

    def arm_b(w):
        t0 = time.perf_counter()
        info = normals.update(info=True)
        return (time.perf_counter() - t0) * 1e3, info

    def pose(k):
        w = S.wobble(scene, 0.1 + 0.07 * k, args.amplitude)
        sb.verts.update(w)
        return w

    w = pose(0)
    arm_a(w); arm_a1(w); arm_b(w)                       # warm-up of each
    a_ms, a1_ms, b_ms, b_dev = [], [], [], []
    info = None
    for k in range(args.reps):
        w = pose(k + 1)
        a_ms.append(arm_a(w))
        a1_ms.append(arm_a1(w))
        ms, info = arm_b(w); b_ms.append(ms); b_dev.append(info["ms"])
    # the three arms leave the same normals up to the float64 helper's rounding: B's bytes are A''s
    got = sb.props.read(capi.tri_props_dtype)["normal"]
    same = bool(np.array_equal(got.view(np.uint32), capi.vertex_normals_host(w, idx_host).view(np.uint32)))

    T, V = int(len(idx_host)), int(len(scene["verts"]))
    moved = T * (12 + 36 + 16) + 3 * T * (4 + 16) + V * (8 + 12)
    dev_med = float(np.median(b_dev))
    out = {"scene": scene["name"], "triangles": T, "vertices": V, "max_valence": info["max_valence"], "amplitude": args.amplitude,
           "A_numpy_readback_patch_upload_ms": spread(a_ms), "A1_host_rule_16_threads_readback_patch_upload_ms": spread(a1_ms),
           "B_normals_update_ms": spread(b_ms), "B_device_ms": spread(b_dev), "create_ms_first_second": create_ms,
           "B_bytes_moved": moved, "B_share_of_copy_rate": moved / (dev_med * 1e-3) / COPY_RATE if dev_med > 0 else None,
           "B_below_A1_in_every_repetition": all(b < a for a, b in zip(a1_ms, b_ms)), "B_equals_host_rule": same,
           "ratio_A_over_B_median": float(np.median(a_ms) / np.median(b_ms)), "ratio_A1_over_B_median": float(np.median(a1_ms) / np.median(b_ms))}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    normals.close(); r.close(); sb.close(); dev.close()


if __name__ == "__main__":
    main()

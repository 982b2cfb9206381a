"""The convergence estimate against reality: on the bench scene (the seeded sphere room of bench.py) at 160x90, the ratio of the
estimated standard error (gmupt_converge_update, a check every 4 iterations from the start of the accumulation) to the actual RMS
deviation of the frame's luminance from the 4 096-spp frame of the same accumulation, taken when the mean sample count passes 16, 64
and 256.  Both sides are root mean squares over the pixels whose error is known and finite; the actual deviation is divided by
sqrt(1 - n / N) per pixel, because the reference holds the frame's own samples.  Prints one JSON line.

    python tools/converge_truth.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch   # first: torch's HIP runtime is the one libgmupt binds to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F = np.float32


def luminance(fb):
    return (F(0.2126) * fb[..., 0] + F(0.7152) * fb[..., 1]) + F(0.0722) * fb[..., 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reference-spp", type=int, default=4096)
    args = ap.parse_args()
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi, scenes = pkg.capi, pkg.scenes
    torch.zeros(1, device="cuda")
    dev = capi.Device(0)
    scene = scenes.build_scene(scenes.spheres_mesh(202, 3, seed=1234))
    W, H, P, every = 160, 90, 1 << 16, 4
    sb = capi.SceneBuffers(dev, scene)
    r = capi.Renderer(dev, W, H, pool_paths=P)
    r.bind_scene(sb)
    cam = capi.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = scene["light_count"]
    c = capi.Converge(r)
    marks, taken, it = [16, 64, 256], [], 0
    while True:
        for _ in range(every):
            cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
        it += every
        need_plane = bool(marks)
        out = c.update(error=need_plane)
        fb = r.framebuffer()
        mean_spp = float(fb[..., 3].view(np.uint32).mean())
        if marks and mean_spp >= marks[0]:
            taken.append({"mark": marks.pop(0), "iterations": it, "mean_spp": mean_spp, "info": out[0], "err": out[1].cpu().numpy(), "y": luminance(fb),
                          "n": fb[..., 3].view(np.uint32).copy()})
        if mean_spp >= args.reference_spp:
            break
        if not marks:
            every = 64                                   # only the reference is still to come
    ref_y, ref_n = luminance(fb).astype(np.float64), fb[..., 3].view(np.uint32).astype(np.float64)
    rows = []
    for t in taken:
        ok = (t["err"] >= 0) & np.isfinite(t["err"]) & (t["n"] > 0) & (t["n"] < ref_n)
        est = np.sqrt(np.mean(t["err"][ok].astype(np.float64) ** 2))
        dev2 = (t["y"][ok].astype(np.float64) - ref_y[ok]) ** 2 / (1.0 - t["n"][ok] / ref_n[ok])
        actual = np.sqrt(np.mean(dev2))
        per_pixel = t["err"][ok].astype(np.float64) / np.sqrt(np.maximum(dev2, 1e-300))
        rows.append({"spp_mark": t["mark"], "iterations": t["iterations"], "mean_spp": round(t["mean_spp"], 2), "pixels_used": int(ok.sum()),
                     "batches": t["iterations"] // 4, "estimated_rms": est, "actual_rms": actual, "ratio": est / actual,
                     "median_pixel_ratio": float(np.median(per_pixel)), "max_error": t["info"]["max_error"], "mean_error": t["info"]["mean_error"]})
    line = json.dumps({"converge_truth": {"scene": scene["name"], "width": W, "height": H, "pool": P, "reference_mean_spp": float(ref_n.mean()),
                                          "reference_iterations": it, "rows": rows}})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    c.close(); r.close(); sb.close(); cam.close(); dev.close()


if __name__ == "__main__":
    main()

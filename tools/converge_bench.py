"""Cost of a convergence update (gmupt_converge_update, csrc/pt_converge.hip): info.ms -- the device time of k_cv_update and the
k_cv_reduce levels -- at 1920x1080 and 3840x2160, with and without the error plane, as the median of 7 updates in which every pixel
has a new batch (the state of every pixel is read and written: the expensive case).  Next to it the modelled bytes per pixel -- 16 of
the pixel, 36 of state read, 36 written, 4 of the error plane -- and the bandwidth they amount to.  Prints one JSON line.

    python tools/converge_bench.py [--out FILE.json]
    rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o cv -- python tools/converge_bench.py --stream
    python tools/converge_bench.py --parse-trace DIR/prof [--out FILE.json]

--stream also runs the project's other per-pixel streaming kernels on the same box, at the same sizes, on a synthetic all-surface
frame: k_dn_prepare (gmupt_denoise_image: 80 bytes read, 60 written per pixel) and k_tp_integrate (gmupt_temporal_denoise_image: 80
read and 64 written, and from the second call on the pixel's own 48-byte history record once more), so that a kernel trace of the
run holds all of them; --parse-trace turns that trace into medians per kernel and size with the modelled bandwidth next to them.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch   # first: torch's HIP runtime is the one libgmupt binds to (the error plane is a torch tensor)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


SIZES = ((1920, 1080), (3840, 2160))
REPS = 9                                             # two to warm up, seven that count
MODEL_BYTES = {"k_cv_update": 88, "k_dn_prepare": 140, "k_tp_integrate": 192}   # per pixel; k_cv_update 92 with the error plane


def stream_arm(capi, r, W, H):
    """REPS calls each of the denoiser and the temporal chain on an all-surface synthetic frame of the renderer's size."""
    rng = np.random.default_rng(2)
    beauty = rng.random((H, W, 4), dtype=np.float32)
    beauty[..., 3] = np.full((H, W), 4, np.uint32).view(np.float32)
    aov = np.zeros((H, W), capi.aov_dtype)
    aov["albedo"] = 0.5; aov["depth"] = 5.0; aov["normal"] = (0.0, 0.0, 1.0); aov["roughness"] = 0.5; aov["coverage"] = 1
    aov["position"][..., 0] = np.linspace(-1, 1, W, dtype=np.float32)[None, :]; aov["position"][..., 1] = np.linspace(-1, 1, H, dtype=np.float32)[:, None]
    aov["position"][..., 2] = -5.0
    b = torch.from_numpy(beauty).cuda()
    a = torch.from_numpy(aov.view(np.float32).reshape(H, W, 16)).cuda()
    cam = capi.Camera(W, H)
    cam.update(0.0)
    t = capi.Temporal(r)
    for u in range(REPS):
        capi.denoise_image(r, b, a)
        capi.temporal_denoise_image(t, b, a, cam.buffer_copy(), u == 0)
    r.synchronize()
    t.close(); cam.close()


def parse_trace(args):
    """Medians per kernel and size of a rocprofv3 --kernel-trace run of --stream: the launches of a kernel come in two equal halves, the
    sizes in ascending order; of each half the first launches are warm-up (for k_cv_update a half is two monitors, without and with the
    error plane)."""
    files = sorted(glob.glob(os.path.join(args.parse_trace, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % args.parse_trace)
    rows = []
    for fn in files:
        with open(fn, newline="") as f:
            for rec in csv.DictReader(f):
                rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]), rec["Kernel_Name"]))
    rows.sort()
    out = []
    for name in ("k_cv_update", "k_cv_reduce", "k_dn_prepare", "k_tp_integrate"):
        us = [(e - s0) / 1000.0 for s0, e, n in rows if name in n and (name + "_mv") not in n]
        half = len(us) // 2
        for k, (W, H) in enumerate(SIZES):
            part = us[k * half:(k + 1) * half]
            groups = [part] if name != "k_cv_update" else [part[:len(part) // 2], part[len(part) // 2:]]
            for g, grp in enumerate(groups):
                timed = grp[2 * (len(grp) // REPS):] if len(grp) >= REPS else grp
                med = statistics.median(timed)
                row = {"kernel": name, "width": W, "height": H, "launches": len(grp), "median_us": round(med, 2)}
                if name == "k_cv_update":
                    row["error_plane"] = bool(g)
                if name in MODEL_BYTES:
                    bpp = MODEL_BYTES[name] + (4 if name == "k_cv_update" and g else 0)
                    row["bytes_per_pixel"] = bpp; row["tb_per_s"] = round(W * H * bpp / (med * 1e-6) / 1e12, 3)
                out.append(row)
    line = json.dumps({"converge_kernels": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--parse-trace")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args)
    import gmupt_pkg
    capi = gmupt_pkg.load().capi
    torch.zeros(1, device="cuda")                   # torch initialises the device before the library does
    dev = capi.Device(0)
    rng = np.random.default_rng(1)
    rows = []
    for W, H in SIZES:
        r = capi.Renderer(dev, W, H, pool_paths=1024)
        frame = rng.random((H, W, 4), dtype=np.float32)
        counts = np.zeros((H, W), np.uint32)
        for error in (False, True):
            c = capi.Converge(r)
            ms = []
            for u in range(REPS):
                counts += 8
                frame[..., 3] = counts.view(np.float32)
                frame[..., :3] += np.float32(0.001)
                r.write_framebuffer(frame)
                out = c.update(error=error)
                info = out[0] if error else out
                assert info["pixels"] == W * H and info["known"] == (W * H if u else 0)
                ms.append(info["ms"])
            c.close()
            med = statistics.median(ms[2:])
            bpp = 16 + 36 + 36 + (4 if error else 0)
            rows.append({"width": W, "height": H, "error_plane": error, "ms_median": med, "ms": ms[2:], "bytes_per_pixel": bpp,
                         "tb_per_s": W * H * bpp / (med * 1e-3) / 1e12})
        if args.stream:
            stream_arm(capi, r, W, H)
        r.close()
    dev.close()
    line = json.dumps({"converge_update": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

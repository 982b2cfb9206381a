#!/usr/bin/env python3
"""Cost of temporal reuse (gmupt_temporal_denoise_image: k_tp_integrate + the 5-pass denoiser) on the bench scene (config 3, the seeded
~260k-triangle sphere room) after a camera move, at 1920x1080 and 3840x2160, and the parameter sweep behind the defaults.

  python tools/temporal_bench.py [--reps 9] [--out DIR]            timing: device events per call (ms), median; DIR/temporal_bench.json
  rocprofv3 --kernel-trace --stats -f csv -d DIR/prof -o tp -- python tools/temporal_bench.py --reps 5 --no-json
  python tools/temporal_bench.py --sweep [--out DIR]                Cornell 96x54 quality sweep; DIR/quality_sweep.txt

Frames: the AOVs of pose A (the scene's camera) and pose B (yaw + 2 degrees) at s = 1, beauty images made from their albedo plus seeded
noise with 0..2 samples per pixel.  Call 1 integrates A (no history), the timed calls integrate B against A's records
(new_accumulation = 0, so the history stays A's).  Next to the whole call, gmupt_denoise_image on the same integrated image is timed; the
two differ by less than their run-to-run spread, so the time of k_tp_integrate itself comes from the rocprofv3 run.  Bytes per pixel are modelled from the layout of csrc/pt_temporal.hpp: the beauty
texel and the AOV record (16 + 64 B), three float4 per tap record for the four taps of a surface pixel whose taps fall in the previous
rectangle (192 B), and the integrated texel plus the new record (16 + 48 B).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = [(1920, 1080), (3840, 2160)]


def frames(pkg, dev, sb, scene, W, H):
    import numpy as np
    import torch
    capi = pkg.capi
    r = capi.Renderer(dev, W, H, pool_paths=1 << 16)
    r.bind_scene(sb)
    rng = np.random.default_rng(1)
    out = []
    x, y, z, pitch, yaw = scene["camera"]
    for pose in [(x, y, z, pitch, yaw), (x, y, z, pitch, yaw + 2.0)]:
        cam = capi.Camera(W, H); cam.set_pose(*pose); cam.buffer.lightCount = scene["light_count"]; cam.update(0.0)
        r.set_camera(cam.buffer)
        aov = r.aovs(1)
        alb = aov.cpu().numpy()[..., 0:3]
        b = np.empty((H, W, 4), np.float32)
        b[..., :3] = np.clip(alb * 0.6 + rng.normal(0, 0.15, alb.shape), 0, 1)
        b[..., 3] = rng.integers(0, 3, (H, W)).astype(np.uint32).view(np.float32)
        out.append((torch.from_numpy(b).cuda(), aov, cam.buffer_copy()))
        cam.close()
    return r, out


def modelled_bytes(pkg, A, B):
    """Bytes k_tp_integrate moves for B given A's records, from the layout (see the module text)."""
    import numpy as np
    capi = pkg.capi
    (bA, aA, cA), (bB, aB, cB) = A, B
    _, hist = capi.temporal_integrate_host(bA.cpu().numpy(), aA.cpu().numpy())
    integ, _ = capi.temporal_integrate_host(bB.cpu().numpy(), aB.cpu().numpy(), hist, cA)
    a = aB.cpu().numpy()
    u = a.view(np.uint32)
    surface = (u[..., 12].view(np.int32) != -1) & (u[..., 14] == 0) & (a[..., 4:7] != 0).any(-1)
    npix = surface.size
    # a surface pixel whose projection lands in the previous rectangle loads its four taps; approximated by "all surface pixels"
    # (the bench pose pair keeps almost every surface point in view)
    total = npix * (16 + 64 + 16 + 48) + int(surface.sum()) * 4 * 48
    took = surface & (integ[..., 3].view(np.uint32) != bB.cpu().numpy()[..., 3].view(np.uint32))
    return total, int(surface.sum()), int(took.sum())


def timing(args):
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
        r, (A, B) = frames(pkg, dev, sb, scene, W, H)
        t = capi.Temporal(r)
        capi.temporal_denoise_image(t, A[0], A[1], A[2], True)
        capi.temporal_denoise_image(t, B[0], B[1], B[2], True)        # warm: folds A into the history
        whole, spatial = [], []
        for _ in range(args.reps):
            capi.temporal_denoise_image(t, B[0], B[1], B[2], False, ms=whole)
        integ, _ = capi.temporal_integrate_host(B[0].cpu().numpy(), B[1].cpu().numpy(), *_history(capi, A))
        it = torch.from_numpy(integ).cuda()
        for _ in range(args.reps):
            capi.denoise_image(r, it, B[1], ms=spatial)
        tw, ts = statistics.median(whole), statistics.median(spatial)
        total, surf, took = modelled_bytes(pkg, A, B)
        row = {"size": [W, H], "reps": args.reps, "ms_temporal_call": tw, "ms_denoise_image": ts,
               "modelled_integrate_bytes": total, "modelled_bytes_per_pixel": total / (W * H), "surface_pixels": surf,
               "pixels_using_history": took, "ms_all_calls": whole}
        print(json.dumps(row))
        results.append(row)
        t.close(); r.close()
    sb.close(); dev.close()
    if not args.no_json:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "temporal_bench.json"), "w") as f:
            json.dump({"scene": scene["name"], "results": results}, f, indent=1)


def _history(capi, A):
    _, hist = capi.temporal_integrate_host(A[0].cpu().numpy(), A[1].cpu().numpy())
    return hist, A[2]


def sweep(args):
    import numpy as np
    import torch
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    os.environ.setdefault("GMUPT_TRAVERSAL", "wide")
    dev = capi.Device(0)
    scene = pkg.scenes.build_scene(pkg.scenes.cornell_mesh())
    sb = capi.SceneBuffers(dev, scene)
    W, H = 96, 54
    x, y, z, pitch, yaw = scene["camera"]
    poseB = (x, y, z, pitch, yaw + 2.0)

    def render(spp, pose):
        r = capi.Renderer(dev, W, H, pool_paths=min(1 << 16, W * H * spp // 2), path_budget=W * H * spp)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*pose); cam.buffer.lightCount = scene["light_count"]
        r.render_budget(cam, 1 << 20)
        return r, cam, r.framebuffer()

    rr, cr, ref = render(1024, poseB); rr.close(); cr.close()
    ra, ca, fa = render(64, scene["camera"]); aovA, camA = ra.aovs(2), ca.buffer_copy(); ra.close(); ca.close()
    rb, cb, fb = render(2, poseB); aovB, camB = rb.aovs(2), cb.buffer_copy()
    mse = lambda a: float(((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean())
    lines = ["cornell %dx%d, history A at 64 spp, B = yaw + 2 at 2 spp, reference B at 1024 spp, AOVs s = 2" % (W, H),
             "noisy mse %.6f" % mse(fb), "spatial mse %.6f" % mse(capi.denoise_image(rb, torch.from_numpy(fb).cuda(), aovB).cpu().numpy())]
    t = capi.Temporal(rb)
    for cap in (4.0, 8.0, 16.0, 32.0, 64.0):
        for cosn in (0.8, 0.9, 0.95):
            for pd in (0.01, 0.02, 0.05):
                t.reset()
                kw = {"history_cap": cap, "min_normal_cos": cosn, "plane_dist": pd}
                capi.temporal_denoise_image(t, torch.from_numpy(fa).cuda(), aovA, camA, True, **kw)
                out = capi.temporal_denoise_image(t, torch.from_numpy(fb).cuda(), aovB, camB, True, **kw).cpu().numpy()
                lines.append("cap %g cos %g plane %g temporal mse %.6f" % (cap, cosn, pd, mse(out)))
                print(lines[-1], flush=True)
    t.close(); rb.close(); cb.close(); sb.close(); dev.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "quality_sweep.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="profiles/r07_temporal")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    sweep(a) if a.sweep else timing(a)

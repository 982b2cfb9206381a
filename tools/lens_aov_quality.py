#!/usr/bin/env python3
"""What lens-filtered guide records do to the denoised image of a frame with depth of field (DESIGN.md "Lens AOVs").

  python tools/lens_aov_quality.py [--spp 4] [--ref-spp 4096] [--out profiles/lens_aov/quality.txt]

The view of the lens image test (tests/test_lens_gpu.py): Cornell 64x36, the camera outside the opening, the lens focused on the back wall
through focus_at on the centre pixel, aperture 0.5.  Reference: the lens beauty at --ref-spp, rendered twice with different seeds (pool
sizes), so that the reference's own error is known.  Inputs: the lens beauty at --spp for four seeds, denoised with default parameters
(a) by gmupt_render_denoised, pinhole records, and (b) by gmupt_render_denoised_lens, lens records, both at 4 samples per axis.  Region:
the pixels with 0 < coverage < 16 in the lens record together with H, the pixels that are surface pixels of the lens record but not
of the pinhole record.  Reported: the MSE over rgb (values clamped at 4.0, as the lens image test does) of (a), (b) and the undenoised
input against the reference, over the region and over the whole frame, per seed, and the spread (max - min) of (a) over the seeds.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W, H, APERTURE, S = 64, 36, 0.5, 4
DOF_POSE = (-3.5, 8.0, 7.0, 0.0, 270.0)
SEED_POOLS = (4096, 3072, 2048, 1536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default="profiles/lens_aov/quality.txt")
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import gmupt_pkg
    pkg = gmupt_pkg.load()
    capi = pkg.capi
    scene = pkg.scenes.build_scene(pkg.scenes.cornell_mesh())
    dev = capi.Device(0)
    sb = capi.SceneBuffers(dev, scene)

    def frame(spp, pool):
        r = capi.Renderer(dev, W, H, pool_paths=pool, path_budget=W * H * spp)
        r.bind_scene(sb)
        cam = capi.Camera(W, H); cam.set_pose(*DOF_POSE); cam.buffer.lightCount = scene["light_count"]
        cam.update(0.0); r.set_camera(cam.buffer)
        lens = capi.lens.focus_at(r, W / 2, H / 2, 0, aperture_radius=APERTURE)
        cam.reset_accumulation()
        capi.lens.set_lens(r, lens)
        r.render_budget(cam, 1 << 20)
        assert np.all(r.framebuffer()[..., 3].view(np.uint32) == spp)
        cam.update(0.0); r.set_camera(cam.buffer)
        return r, cam

    clamp = lambda x: np.minimum(np.asarray(x)[..., :3].astype(np.float64), 4.0)
    refs = []
    for pool in (8192, 6144):
        r, cam = frame(args.ref_spp, pool)
        refs.append(clamp(r.framebuffer()))
        r.close(); cam.close()
    ref = refs[0]
    lines = ["Cornell %dx%d, pose %r, aperture %.2f focused on the back wall, guides at s = %d, default denoiser parameters" % (W, H, DOF_POSE, APERTURE, S),
             "reference %d spp; input %d spp; MSE over rgb, values clamped at 4.0" % (args.ref_spp, args.spp)]
    surface = lambda f: (f["triangle"] >= 0) & (f["light"] == 0) & (np.abs(f["normal"]).sum(axis=-1) > 0)
    rows = []
    for pool in SEED_POOLS:
        r, cam = frame(args.spp, pool)
        raw = clamp(r.framebuffer())
        pin = surface(capi.aov_fields(r.aovs(S)))
        lf = capi.aov_fields(capi.lens_aov.aovs(r, S))
        region = ((lf["coverage"] > 0) & (lf["coverage"] < S * S)) | (~pin & surface(lf))
        a = clamp(r.denoise(S).cpu().numpy())
        b = clamp(capi.lens_aov.denoise(r, S).cpu().numpy())
        mse = lambda x, m=None: float(((x - ref) ** 2)[m].mean()) if m is not None else float(((x - ref) ** 2).mean())
        rows.append({"pool": pool, "region_pixels": int(region.sum()), "H_pixels": int((~pin & surface(lf)).sum()),
                     "region": {"raw": mse(raw, region), "pinhole": mse(a, region), "lens": mse(b, region)},
                     "frame": {"raw": mse(raw), "pinhole": mse(a), "lens": mse(b)}})
        r.close(); cam.close()
    region = rows[0]["region_pixels"]
    ref_mse_frame = float(((refs[0] - refs[1]) ** 2).mean())
    lines.append("two references (other seeds) differ by MSE %.6g over the frame; the %d spp input's MSE is %.6g (seed %d)" % (ref_mse_frame, args.spp, rows[0]["frame"]["raw"], SEED_POOLS[0]))
    for w in ("region", "frame"):
        for row in rows:
            lines.append("%-6s seed(pool %4d)%s: raw %.6g  (a) pinhole guides %.6g  (b) lens guides %.6g" % (
                w, row["pool"], " %d pixels, %d in H" % (row["region_pixels"], row["H_pixels"]) if w == "region" else "", row[w]["raw"], row[w]["pinhole"], row[w]["lens"]))
        av = [row[w]["pinhole"] for row in rows]; bv = [row[w]["lens"] for row in rows]
        lines.append("%-6s (a) mean %.6g spread (max - min) %.6g; (b) mean %.6g; (a) - (b) mean %.6g, smallest %.6g" % (
            w, np.mean(av), max(av) - min(av), np.mean(bv), np.mean(av) - np.mean(bv), min(x - y for x, y in zip(av, bv))))
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"ref_vs_ref_mse": ref_mse_frame, "rows": rows}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    sb.close(); dev.close()
    assert region > 0


if __name__ == "__main__":
    main()

"""CPU half of the extreme-lens tests (include/gmupt_lens.h, "Extreme lenses"): the lenses of lens_extremes_util.LENS_CLASSES through the
host rule, the numpy restatements and the oracle alone.  No device.

The census below is the precondition of tests/test_lens_extremes_gpu.py: every class must contain the rays it is named for, counted here
from gmupt_lens_ray_host alone (q = 0 .. 4095 over the pixels of the 32 x 18 frame, the default Cornell camera and one off-axis pose).
What it found on the host CPU, both poses alike (the draws r1, r2 do not depend on the pose), ordinary / zero / NaN directions of 4096:
    0.3, 13 (the lens of the older tests)   4096 / 0 / 0        0.3, 1e-45 and 0.3, 1e-30    4090 / 0 / 6   (r1 = 0: Pf == origin)
    1e-45, 13 and 1e-38, 13                  4096 / 0 / 0        0.3, 1e19                    4096 / 0 / 0
    1e18, 13 and 1.5e19, 13                  4096 / 0 / 0        0.3, 1e30                    0 / 4096 / 0
    3e19, 13 (a mixed wave, by the draw r1) 1491 / 2605 / 0     0.3, 1.5e19 (a mixed wave, by the pixel)   2474 / 1622 / 0
    1e30, 13 and FLT_MAX, 13                 6 / 4090 / 0        0.3, 3e38                    0 / 1534 / 2562 (off axis 1528 / 2568)
                                                                 0.3, FLT_MAX and 1e-45, 1e-45   0 / 0 / 4096
(the off-axis pose has another seed: 10 draws with r1 = 0 where the default camera has 6).  No class has a non-finite origin, and no
direction is anything but a unit vector, (0, 0, 0) or a NaN.  With 3e19 and with 0.3, 1.5e19 every one of the 64 aligned runs of 64 q
holds both ordinary and zero-direction rays.  The second mixed class is not in the issue's table: the ordinary rays of the first start
1e19 units from the room and see no surface, so the lens AOV test, which needs partly covered pixels, could not use it.
Through the oracle (Cornell, its two light spheres): every zero-direction and every NaN-direction ray gets the miss record.  The ordinary
rays of the 1e18 aperture, whose origins lie about 1e18 from the room, are recorded, not judged: of 4096, 13 hit a triangle, 2722 "hit" a
light sphere and 1361 miss (1e18: 1.5e19 gives figures of the same kind).  From that far the sphere test's d2 = dot(p, p) - tca * tca
cancels to 0 or below whatever the direction, so most rays see a light and their paths end on an emitter; the renderer must give
exactly these answers, and tests/test_lens_extremes_gpu.py compares whole iterations of that lens with the oracle.  The ordinary rays of
a tiny focus leave the lens sideways, in its plane; the default camera stands outside the room's opening, so all of them miss.
"""
import os
import re

import numpy as np
import pytest

import lens_aov_util as LA
import lens_extremes_util as X
import lens_util as LU
import trace_util as T

F = LU.F
POSES = {"default": (LU.POSES[0], 1), "off_axis": (X.OFF_AXIS_POSE, 2)}      # pose, camera updates (another randomSeed)


@pytest.fixture(scope="module")
def cameras(pkg):
    return {k: X.camera_buffer(pkg.capi, pose, updates) for k, (pose, updates) in POSES.items()}


@pytest.fixture(scope="module")
def censuses(pkg, cameras):
    """{(class, pose): (counts, masks, rays)} from the host rule, computed once."""
    return {(name, p): X.census(pkg.capi, cb, name) for name in X.LENS_CLASSES for p, cb in cameras.items()}


def test_every_class_holds_what_it_is_named_for(censuses, cameras):
    for (name, p), (counts, masks, rays) in censuses.items():
        kind = X.LENS_CLASSES[name][2]
        print("%-22s %-8s ordinary %4d  zero %4d  nan %4d  other %d  bad origin %d  mixed runs %d" % (
            name, p, counts["ordinary"], counts["zero"], counts["nan"], counts["other"], counts["bad_origin"], len(X.mixed_runs(masks))))
        assert X.census_holds(kind, counts, masks, rays, cameras[p]) is None, (name, p, X.census_holds(kind, counts, masks, rays, cameras[p]))
        assert counts["ordinary"] + counts["zero"] + counts["nan"] == X.N and counts["bad_origin"] == 0
        assert np.all(rays[:, 3] == np.finfo(F).max) and not LU.bits(rays[:, 7]).any()
        if kind in X.NO_NAN_KINDS:
            assert X.nan_words(rays) == 0, (name, p)
        else:
            assert X.nan_words(rays[:, 0:3]) == 0 and X.nan_words(rays) > 0, (name, p)
        if kind == "mixed":     # a wave of k_lens_retarget is 64 consecutive q: at least one holds both kinds
            assert len(X.mixed_runs(masks)) >= 1
    # the far-away ordinary classes really are far away
    for name in ("aperture_1e18", "aperture_1p5e19"):
        rays = censuses[(name, "default")][2]
        assert np.median(np.abs(rays[:, 0:3]).max(axis=1)) > 1e17


def test_same_words_is_a_cap_not_a_tolerance():
    nan_pos, nan_neg = np.array([0x7FC00000], np.uint32).view(F), np.array([0xFFC00000], np.uint32).view(F)
    payload = np.array([0x7F800001], np.uint32).view(F)
    want = np.array([1.0, np.nan, 0.0, np.inf], F)
    want[1] = nan_neg[0]
    for other in (nan_pos, nan_neg, payload):
        got = want.copy(); got[1] = other[0]
        assert X.same_words(got, want)
    assert X.nan_words(want) == 1
    for k, v in ((0, np.nextafter(F(1.0), F(2.0))), (2, F(-0.0)), (3, F(-np.inf)), (3, nan_pos[0]), (0, nan_pos[0]), (1, F(np.inf)), (1, F(0.0))):
        got = want.copy(); got[k] = v
        assert not X.same_words(got, want), (k, v)        # a NaN where the reference has a number, and a number where it has a NaN, both fail
    assert not X.same_words(want[:3], want)
    assert X.same_words(np.zeros((2, 3), F), np.zeros((2, 3), F)) and X.nan_words(np.zeros(4, F)) == 0


def test_a_denormal_aperture_moves_the_origin_only_of_a_camera_at_the_origin(pkg, oracle, censuses, cameras):
    """pos + right*lx with |lx| <= 1e-38 is pos for every camera that stands anywhere: the stage test of the GPU file could not tell a
    kept denormal offset from a flushed one there.  At ORIGIN_POSE the offset IS the origin."""
    at_origin = X.camera_buffer(pkg.capi, X.ORIGIN_POSE)
    assert list(at_origin.position)[:3] == [0.0, 0.0, 0.0]
    for name in X.DENORMAL_APERTURES:
        for p, cb in cameras.items():
            rays = censuses[(name, p)][2]
            assert (rays[:, 0:3] == np.array(list(cb.position)[:3], F)).all(), "absorbed by the position"
        counts, masks, rays = X.census(pkg.capi, at_origin, name)
        assert counts["ordinary"] == X.N, counts
        o = rays[:, 0:3]
        moved = (o != 0).any(axis=1)
        print("%s at the origin: %d of %d origins are a denormal offset, largest %.3g" % (name, moved.sum(), X.N, np.abs(o).max()))
        assert moved.sum() > X.N // 2 and np.abs(o).max() < T.FLT_MIN and np.abs(o[o != 0]).min() >= F(1e-45)
        with np.errstate(all="ignore"):
            want = LU.rule(oracle, at_origin, X.LENS_CLASSES[name][0], X.LENS_CLASSES[name][1], *X.census_inputs())
        assert X.nan_words(want["origin"]) == 0 and np.array_equal(LU.bits(o), LU.bits(want["origin"]))


def test_host_rules_equal_the_restatements_on_every_class(pkg, oracle, censuses, cameras):
    """gmupt_lens_ray_host against lens_util.rule, and gmupt_aov_lens_ray against lens_aov_util.rule (s = 1, 2, 3; every pixel of the
    frame), with same_words and the number of excepted words counted from the restatement."""
    ys, xs = np.mgrid[0:X.H, 0:X.W]
    xs, ys = xs.ravel().astype(np.uint32), ys.ravel().astype(np.uint32)
    q, cx, cy = X.census_inputs()
    for name, (a, f, kind) in X.LENS_CLASSES.items():
        for p, cb in cameras.items():
            with np.errstate(all="ignore"):
                want = LU.rule(oracle, cb, a, f, q, cx, cy)
            rays = censuses[(name, p)][2]
            excepted = X.nan_words(want["origin"]) + X.nan_words(want["direction"])
            assert X.same_words(rays[:, 0:3], want["origin"]) and X.same_words(rays[:, 4:7], want["direction"]), (name, p)
            assert X.nan_words(want["origin"]) == 0 and (excepted == 0 if kind in X.NO_NAN_KINDS else excepted > 0), (name, p, excepted)
            lens = X.lens_of(pkg.capi, name)
            for s in (1, 2, 3):
                got = pkg.capi.lens_aov.aov_lens_rays(cb, lens, xs.tolist(), ys.tolist(), s)
                with np.errstate(all="ignore"):
                    exp = LA.rays_of(LA.rule(oracle, cb, a, f, xs, ys, s))
                n = X.nan_words(exp)
                assert X.same_words(got, exp), (name, p, s)
                assert X.nan_words(exp[..., 0:4]) == 0 and (n == 0 if kind in X.NO_NAN_KINDS else True), (name, p, s, n)
                if kind in ("nan", "zero_nan"):
                    assert n > 0, (name, p, s)


def test_the_oracle_alone_on_the_lens_rays(pkg, oracle, cornell_scene, censuses):
    """The lens rays of every class as extension rays and as shadow rays (light distance FLT_MAX) through the oracle's two stages, as
    test_degenerate_rays_cpu.py takes its classes: it returns, reports no NaN distance, and every zero-direction and NaN-direction ray
    gets the miss record of include/gmupt.h ("Degenerate rays"): no triangle, no light, t = FLT_MAX, not occluded."""
    lc = cornell_scene["light_count"]
    for name, (a, f, kind) in X.LENS_CLASSES.items():
        counts, masks, rays = censuses[(name, "default")]
        truth = T.oracle_truth(cornell_scene, rays, rays, lc)
        n = len(rays)
        assert not np.isnan(truth["hitDistance"][:n, 0].view(F)).any(), name
        miss = T.is_miss_record(truth, n) & (truth["isEmitter"][:n, 0] == 0)
        degenerate = masks["zero"] | masks["nan"]
        hits = int((truth["triangle"][:n, 0] != T.NO_TRI).sum())
        print("%-22s %4d triangle hits, %4d lights, %4d occluded, %4d miss records (%d degenerate rays)" % (
            name, hits, int((truth["isEmitter"][:n, 0] > 0).sum()), int(truth["inShadow"][:n, 0].sum()), int(miss.sum()), int(degenerate.sum())))
        assert miss[degenerate].all(), name
        if name in ("tested_today", "aperture_min_denormal", "aperture_denormal"):
            assert hits == n, "every pixel of the default camera sees a wall"
        if name in ("aperture_1e18", "aperture_1p5e19"):      # recorded in the module docstring, not judged; what must hold is finiteness
            assert counts["ordinary"] == n and np.isfinite(truth["hitDistance"][:n, 0].view(F)).all(), name
        if kind == "mixed":
            assert miss[masks["zero"]].all()


def test_every_sentence_of_the_headers_names_a_test_that_exists():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    defined = {}
    for f in ("test_lens_extremes_cpu.py", "test_lens_extremes_gpu.py"):
        defined[f] = set(re.findall(r"^def (test_\w+)\(", open(os.path.join(root, "tests", f)).read(), re.M))
    for header, least in (("gmupt_lens.h", 6), ("gmupt_lens_aov.h", 3)):
        text = open(os.path.join(root, "include", header)).read()
        assert "Extreme lenses" in text
        para = text[text.index("Extreme lenses"):]
        named = re.findall(r"\b(test_[a-z_0-9]+)\b(?!\.py)", para)
        assert len(set(named)) >= least, named
        for name in named:
            assert any(name in tests for tests in defined.values()), (header, name)
    assert "lens_extremes_util.py" in open(os.path.join(root, "include", "gmupt_lens.h")).read()
    run_sh = open(os.path.join(root, "tools", "sanitize", "run.sh")).read()
    assert "lens_main.cpp" in run_sh and "pt_lens.cpp" in run_sh
    assert "Extreme lenses" in open(os.path.join(root, "DESIGN.md")).read()

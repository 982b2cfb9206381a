"""GPU tests of the lens stages on extreme lenses (include/gmupt_lens.h, "Extreme lenses"): k_lens_retarget, the path-state ray casts
behind it, k_laov_raygen / k_laov_resolve and the denoiser on their records, with the lenses of lens_extremes_util.LENS_CLASSES --
lenses that gmupt_renderer_set_lens admits and whose rays have a zero or a NaN direction, or an origin 1e18 units away.  Truth is the
host rule for the stage and the CPU oracle for everything after it; the census of what each class contains is
tests/test_lens_extremes_cpu.py's.  Every comparison is on bits, or lens_extremes_util.same_words (a NaN of the reference matches any
NaN) with the number of such words counted from the reference; shade_util.compare is the same rule for whole renderer states.

Why every class terminates (read before the first run: k_lens_retarget, then the path-state instantiation StateIO of k_cast_w with its
exact walk, and k_cast_f, which take the rays out of the path state; test_degenerate_rays_gpu.py states the same for caller rays):
  - k_lens_retarget has no loop: one thread per queue entry, straight-line arithmetic, two guarded stores.  Its guards (queueIndex < nNew,
    index < L, the budget) are compared BEFORE the rule runs and depend on counters and the queue only, never on the lens;
  - a ray enters a walk through ray_box(root) > 0, t1 >= t0 and t1 > 0 inside it, and every later slab test is the same two
    comparisons (slab_hit_pk / slab_hit_ordered, inner_compute_flat).  A comparison with a NaN is false: a NaN direction gives NaN
    products, the root test fails and the ray never walks.  A zero direction gives 1 / d = +-inf: (plane - o) * inf is +-inf or, where
    the origin lies in a plane, NaN, which v_min / v_max drop -- the wave takes the general slab form (byte 3 of RayPk's sg is set for
    an infinite or NaN 1 / d), and the outcome is only WHICH boxes pass;
  - the walks follow child links of a finite tree and never revisit a node: a step descends into children whose test passed or pops.
    The wide step pushes at most four entries and checks the room for them before it steps (pb - pa >= 3; a full stack parks the ray
    for the exact walk, whose overflow stack is bounds-checked and flags GMUPT_STAT_STACK_OVERFLOW instead of writing); k_cast_f's
    DefStack is sized by the tree depth on the host.  So trip counts are bounded by the tree, whatever the ray's bits;
  - the triangles of a leaf run from its first record to the one that carries `last`: the table's count.  With d = 0 the determinant is
    0 and the |det| < 1e-8 rejection holds; with a NaN every acceptance comparison (u < 0, u + v > 1 are false, but t >= 0 and
    t < distance are false too) leaves the hit as it was; nothing iterates "until t exceeds something";
  - finish_extension_ray reads p.scene.tris[hitRef] only under distance < FLT_MAX, which only an accepted triangle (hitRef >= 0) or a
    helper's report with refT >= 0 can bring about; the light-sphere loop runs lightCount times;
  - the drain pairs lanes by ballots of haveRay / cur / stack pointers; a lane gives at most twelve subtrees per ray and only entries
    that its own walk pushed: a ray that never walks never gives;
  - the queues are consumed through counters; a path whose ray missed ends in the next shading stage (hitDistance == FLT_MAX), which
    reads neither its origin nor its direction, and is regenerated: a degenerate ray lives for one iteration;
  - k_laov_resolve loops k < R over records it reads by index; a NaN or zero direction only enters o + d * t of a SURFACE sample, which
    such a ray never is;
  - the watchdog (castLoopCap iterations per wave) backstops the persistent loops: it would set GMUPT_STAT_CAST_ABORTED, which every
    test here that casts asserts absent, with GMUPT_STAT_STACK_OVERFLOW.
Nothing in that reading has a trip count that depends on the ray.

Measured on the MI355X: all 73 cases pass, each in well under a second; the stage test's docstring has the NaN figures.  Whole iterations,
lens AOV records and the denoiser met the oracle without any use of the NaN exception outside the fields named in NAN_FIELDS.
"""
import numpy as np
import pytest
import torch   # first: torch's HIP runtime is the one libgmupt binds to

import adaptive_util as AU
import lens_extremes_util as X
import lens_util as LU
import oracle_lib as O
import shade_util as SU
from test_aov_gpu import ENV, compare_records, make_camera, pixels, renderer
from test_lens_aov_gpu import expected, surface_pixels
from test_lens_gpu import RECT, close, host_rays, make, snapshot

pytestmark = pytest.mark.gpu

F = LU.F
W, H, POOL = X.W, X.H, X.N
FAULTS = lambda capi: capi.STAT_STACK_OVERFLOW | capi.STAT_CAST_ABORTED


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


def ray_words(raw, pool, slots):
    """The six ray words of `slots` of a read_path_state() array, (n, 6) float32."""
    o, d = LU.state_rays(raw, pool)
    return np.concatenate([o[slots], d[slots]], axis=1)


def nan_report(tag, got, want):
    """Prints how the device's NaN words differ from the reference's: the figure the header's sentence on NaN sign and payload rests on."""
    g, w = LU.bits(np.asarray(got, F)), LU.bits(np.asarray(want, F))
    m = X.is_nan_words(w)
    if m.any():
        print("%s: %d NaN words in the reference (bits %s), on the device bits %s, %d differ" % (
            tag, int(m.sum()), sorted({hex(int(v)) for v in np.unique(w[m])}), sorted({hex(int(v)) for v in np.unique(g[m])}), int((g[m] != w[m]).sum())))


# ---------------------------------------------------------------------------------------------------------------- a. the stage
STAGE_SHAPES = {"first_stage_16_blocks": dict(), "live_3000_of_4096": dict(live=3000)}     # test_lens_gpu.STAGE_CASES
STAGE_POSES = {"default": None, "off_axis": X.OFF_AXIS_POSE}


def stage_scene(scene, name, pose):
    """The scene with the camera the case asks for: a denormal aperture stands at the origin, where its offsets survive (the census)."""
    if name in X.DENORMAL_APERTURES:
        return dict(scene, camera=X.ORIGIN_POSE)
    return scene if STAGE_POSES[pose] is None else dict(scene, camera=STAGE_POSES[pose])


@pytest.fixture(scope="module")
def plain_stage(pkg, device, cornell_scene):
    """{(shape, camera pose): the snapshot after STAGE_SHADE of a renderer without a lens}: the same for every lens, made once."""
    cache = {}

    def get(shape, scene):
        key = (shape, scene["camera"])
        if key not in cache:
            r, sb, cam = make(pkg, device, scene, **STAGE_SHAPES[shape])
            cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(pkg.capi.STAGE_SHADE)
            cache[key] = snapshot(r) + (cam.buffer_copy(),)
            close(r, sb, cam)
        return cache[key]
    return get


@pytest.mark.parametrize("shape, pose", [("first_stage_16_blocks", "default"), ("live_3000_of_4096", "default"), ("first_stage_16_blocks", "off_axis")])
@pytest.mark.parametrize("name", list(X.LENS_CLASSES))
def test_stage_holds_the_host_rays(pkg, device, wide, cornell_scene, plain_stage, name, shape, pose):
    """test_lens_gpu.test_stage_equals_the_host_rule on every lens class: the fresh slots hold gmupt_lens_ray_host under same_words,
    every other word of state, queues, counters and frame is the run without a lens.  One traversal setting: the stage does not cast.

    Measured on the MI355X: all 48 cases equal word for word with no use of the exception -- the device's generated NaNs were
    0xffc00000 like the host's in every class that has any (18 words of 24 576 with a tiny focus, 7 686 with focus 3e38, all 12 288
    direction words with focus FLT_MAX and with both at 1e-45); nan_report prints the two sets of bit patterns."""
    kind = X.LENS_CLASSES[name][2]
    scene = stage_scene(cornell_scene, name, pose)
    kw = STAGE_SHAPES[shape]
    live = kw.get("live", 0) or POOL
    plain = plain_stage(shape, scene)
    r, sb, cam = make(pkg, device, scene, **kw)
    lens = X.lens_of(pkg.capi, name)
    pkg.capi.lens.set_lens(r, lens)
    cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(pkg.capi.STAGE_SHADE)
    lensed = snapshot(r) + (cam.buffer_copy(),)
    close(r, sb, cam)
    assert bytes(plain[4]) == bytes(lensed[4]), "the same camera stream"
    q, slots = LU.fresh(lensed[3], lensed[2], live)
    assert q.size == live and (live == POOL or live % 256)
    assert np.array_equal(LU.bits(plain[0]), LU.bits(lensed[0])) and np.array_equal(plain[2], lensed[2]) and np.array_equal(plain[3], lensed[3])
    rays = host_rays(pkg, lensed[4], lens, plain[1], POOL, q, slots)
    want = rays[:, [0, 1, 2, 4, 5, 6]]
    got = ray_words(lensed[1], POOL, slots)
    excepted = X.nan_words(want)
    nan_report("%s %s %s" % (name, shape, pose), got, want)
    assert excepted == 0 if kind in X.NO_NAN_KINDS else excepted > 0, (name, excepted)
    assert X.same_words(got, want), "fresh slots hold the host rule's ray"
    # every other word: the run without a lens (the fresh ray words, compared above, are taken out of the comparison)
    rest = LU.patch_rays(lensed[1], POOL, slots, np.zeros((q.size, 8), F))
    assert np.array_equal(rest, LU.patch_rays(plain[1], POOL, slots, np.zeros((q.size, 8), F)))
    # the census of the class holds for the rays the device made, classified from the DEVICE's words
    dev = np.zeros((q.size, 8), F); dev[:, 0:3] = got[:, 0:3]; dev[:, 4:7] = got[:, 3:6]
    m_dev, m_host = X.classify(dev), X.classify(rays)
    assert all(np.array_equal(m_dev[k], m_host[k]) for k in m_dev)
    if name in X.DENORMAL_APERTURES:
        pos = np.array(list(lensed[4].position)[:3], F)
        assert not pos.any()
        moved = (got[:, 0:3] != pos).any(axis=1)
        assert moved.sum() > live // 2 and np.abs(got[:, 0:3]).max() < np.finfo(F).tiny, "a denormal lens offset kept, not flushed"


# ---------------------------------------------------------------------------------------------------------------- b. whole iterations
ITER_CLASSES = ["aperture_1e18", "aperture_mixed_wave", "focus_mixed_wave", "focus_1e30", "focus_flt_max", "focus_1e_30"]
# Where the oracle's state may hold a NaN word at all, per class, and so where shade_util.compare may match a NaN by kind.  rayDirection:
# the lens rule's own NaNs (the census).  directLight: not the lens's -- the few ordinary rays from 1e18 away that reach a triangle get a
# surface point o + d * t that is off by t * 2^-24 ~ 1e11 units, and the next-event estimate from there divides inf by inf.  The oracle
# run on the CPU found 6 such words after iteration 2 and 24 (aperture 1e18) / 12 (3e19) after iteration 8; asserted: no other field.
NAN_FIELDS = {"aperture_1e18": {"directLight"}, "aperture_mixed_wave": {"directLight"}, "focus_mixed_wave": set(), "focus_1e30": set(),
              "focus_flt_max": {"rayDirection"}, "focus_1e_30": {"rayDirection"}}
ALL_MISS = ("focus_1e30", "focus_flt_max", "focus_1e_30")       # test_lens_extremes_cpu.py: every ray of these gets the miss record from the default camera
CHECK_AT = (1, 2, 8)


class Snap:
    """What shade_util.compare reads of an oracle, frozen after an iteration."""

    def __init__(self, orc):
        self.pool = orc.pool
        self._s, self._q, self._c, self._f = orc.path_state().copy(), orc.queues().copy(), orc.counters().copy(), orc.framebuffer().copy()

    def path_state(self):
        return self._s

    def queues(self):
        return self._q

    def counters(self):
        return self._c

    def framebuffer(self):
        return self._f


def oracle_iterations(pkg, scene, name):
    """The oracle WITHOUT a lens, the host rule's rays written into the fresh slots between its shading stages and its extension stage,
    for max(CHECK_AT) iterations.  Returns (the camera buffers of the iterations, {iteration: Snap}, fresh paths patched in all)."""
    capi = pkg.capi
    lens = X.lens_of(capi, name)
    orc = O.Renderer(scene, W, H, POOL, threads=8)
    ocam = O.Camera(W, H); ocam.set_pose(*scene["camera"]); ocam.buffer.lightCount = scene["light_count"]
    hcam = capi.Camera(W, H); hcam.set_pose(*scene["camera"]); hcam.buffer.lightCount = scene["light_count"]
    for i, v in enumerate(ENV):
        ocam.buffer.envColor[i] = v; hcam.buffer.envColor[i] = v
    cams, snaps, moved = [], {}, 0
    for it in range(1, max(CHECK_AT) + 1):
        ocam.update(); hcam.update(0.0)
        assert bytes(ocam.buffer) == bytes(hcam.buffer), "host camera streams diverged"
        cb = hcam.buffer_copy()
        cams.append(cb)
        orc.set_camera(ocam.buffer)
        for stage in ("logic", "new_path", "material_ue4", "material_glass"):
            orc.stage(stage)
        q, slots = LU.fresh(orc.counters(), orc.queues(), POOL)
        if q.size:
            st = orc.path_state()
            xy = O.state_field(st, POOL, "screenCoord")[slots]
            rays = capi.lens.lens_rays_host(cb, lens, q, xy[:, 0], xy[:, 1])
            O.state_field(st, POOL, "rayOrigin").view(F)[slots] = rays[:, 0:3]
            O.state_field(st, POOL, "rayDirection").view(F)[slots] = rays[:, 4:7]
            moved += q.size
        orc.stage("extension"); orc.stage("shadow")
        if it in CHECK_AT:
            snaps[it] = Snap(orc)
    assert tuple(cb.envColor)[:3] == tuple(F(v) for v in ENV)
    orc.close(); hcam.close()
    return cams, snaps, moved


@pytest.fixture(scope="module")
def oracle_runs(pkg, cornell_scene):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_iterations(pkg, cornell_scene, name)
        return cache[name]
    return get


def nan_fields(snap):
    """{field: NaN words} of the float fields of an oracle state."""
    out = {}
    for field, (_, _, _, kind) in O.STATE_FIELDS.items():
        if kind == "f":
            n = int(X.is_nan_words(O.state_field(snap.path_state(), snap.pool, field)).sum())
            if n:
                out[field] = n
    return out


@pytest.mark.parametrize("traversal", ["wide", "cast0"])
@pytest.mark.parametrize("name", ITER_CLASSES)
def test_whole_iterations_equal_the_oracle(pkg, device, monkeypatch, cornell_scene, oracle_runs, name, traversal):
    """A: the renderer with the lens attached, gmupt_iterate, through the shipped kernel `traversal`.  B: the oracle without a lens, the
    host rule patched into its fresh slots before its extension stage.  All 21 state fields, the queues, the counters and the frame
    after iterations 1, 2 and 8 (shade_util.compare: bits; a NaN word only where the oracle has one, and the oracle only in the fields
    of NAN_FIELDS -- the miss record writes hitDistance and isEmitter, and the next shading stage reads no direction of a path that
    missed, so a NaN direction stays where it is).  The frame is finite in every class, as the oracle's is."""
    monkeypatch.setenv("GMUPT_TRAVERSAL", traversal)
    capi = pkg.capi
    kind = X.LENS_CLASSES[name][2]
    cams, snaps, moved = oracle_runs(name)
    assert moved > POOL, "fresh paths in more than the first iteration"
    r, sb, cam = make(pkg, device, cornell_scene)
    capi.lens.set_lens(r, X.lens_of(capi, name))
    names = np.full(POOL, "lens")
    for it, cb in enumerate(cams, start=1):
        r.set_camera(cb); r.iterate()
        if it not in CHECK_AT:
            continue
        r.synchronize()
        snap = snaps[it]
        nf = nan_fields(snap)
        print("%s %s iteration %d: NaN words of the oracle's state %r" % (name, traversal, it, nf))
        assert set(nf) <= NAN_FIELDS[name] and (kind in X.NO_NAN_KINDS or nf.get("rayDirection", 0) > 0), (name, it, nf)
        SU.compare(snap, r, POOL, POOL, names, nan_classes=("lens",) if NAN_FIELDS[name] else (), nan_pixels=np.zeros((H, W), bool),
                   where="%s %s iteration %d: " % (name, traversal, it))
        ofb = snap.framebuffer()
        assert np.isfinite(ofb[..., :3]).all() and np.isfinite(r.framebuffer()[..., :3]).all(), "a finite frame"
    flags = r.stats(check=False).flags
    assert not (flags & FAULTS(capi)), "flags %#x" % flags
    assert flags & (capi.STAT_CAST_WIDE if traversal == "wide" else capi.STAT_CAST_FETCH), "flags %#x" % flags
    fb = r.framebuffer()
    counts = fb[..., 3].view(np.uint32)
    assert int(counts.sum()) > 0
    if name in ALL_MISS:       # every path ends in the iteration after it began, as a miss with throughput 1: the frame is the environment
        assert int(counts.sum()) == (max(CHECK_AT) - 1) * POOL, "the first shading stage clears and starts 4096 paths; each later one ends all 4096 and starts them again"
        want = X.env_frame(O, ENV, counts)
        assert np.array_equal(LU.bits(fb[..., :3]), LU.bits(want)), "every finished sample is the environment colour"
    close(r, sb, cam)


# ---------------------------------------------------------------------------------------------------------------- c. lens AOV records
AOV_CLASSES = ["focus_mixed_wave", "aperture_mixed_wave", "focus_1e30", "focus_flt_max", "focus_1e_30"]
AOV_W, AOV_H = 40, 24


def compare_records_capped(scene, got, exp, rec, names):
    """test_aov_gpu.compare_records with same_words on the float words: a word that is a NaN in the expected record may be any NaN on the
    device.  Returns the number of such words (from the expected records alone)."""
    g = np.ascontiguousarray(got, dtype=F).reshape(-1, 16).view(np.uint32).copy()
    excepted = X.is_nan_words(exp[:, :12])
    assert X.is_nan_words(g[:, :12][excepted]).all(), "a number where the reference has a NaN"
    g[:, :12][excepted] = exp[:, :12][excepted]
    compare_records(scene, g.view(F), exp, rec, names)
    return int(excepted.sum())


@pytest.fixture(scope="module")
def aov_truth(pkg, cornell_scene):
    """{(class, s): expected() of the whole 40 x 24 frame}: the oracle's answer, made once."""
    cache = {}

    def get(name, s):
        if (name, s) not in cache:
            cam = make_camera(pkg, cornell_scene, AOV_W, AOV_H)
            cache[(name, s)] = expected(pkg, cornell_scene, cam.buffer_copy(), X.lens_of(pkg.capi, name), *pixels(AOV_W, AOV_H), s)
            cam.close()
        return cache[(name, s)]
    return get


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("name", AOV_CLASSES)
def test_lens_aov_records_equal_the_oracle(pkg, device, wide, cornell_scene, aov_truth, name, s):
    capi = pkg.capi
    kind = X.LENS_CLASSES[name][2]
    lens = X.lens_of(capi, name)
    exp, rec, names, v, truth = aov_truth(name, s)
    R = s * s
    cov = v["surface"].reshape(-1, R).sum(axis=1)
    cam = make_camera(pkg, cornell_scene, AOV_W, AOV_H)
    rays = capi.lens_aov.aov_lens_rays(cam.buffer, lens, *pixels(AOV_W, AOV_H), s)
    m = X.classify(rays.reshape(-1, 8))
    degenerate = (m["zero"] | m["nan"]).reshape(-1, R)
    print("%s s = %d: coverage 0 in %d pixels, partial in %d, full in %d; %d zero-direction, %d NaN-direction rays of %d" % (
        name, s, int((cov == 0).sum()), int(((cov > 0) & (cov < R)).sum()), int((cov == R).sum()), int(m["zero"].sum()), int(m["nan"].sum()), rays.shape[0] * R))
    # preconditions, from the oracle's per-ray values and the host rule
    assert not v["surface"].reshape(-1, R)[degenerate].any() and not v["hit_tri"].reshape(-1, R)[degenerate].any() and not v["light"].reshape(-1, R)[degenerate].any()
    if name == "focus_mixed_wave":
        surface = v["surface"].reshape(-1, R)
        assert m["zero"].sum() > 100 and (cov == 0).sum() > 100 and (cov == R).sum() > 100, "zero-direction pixels at the corners, the room in the middle"
        if s > 1:      # the ring between them: pixels with 0 < coverage < s*s whose uncovered samples are all zero-direction rays
            ring = (cov > 0) & (cov < R) & (~surface == degenerate).all(axis=1)
            assert ring.sum() >= 16, int(ring.sum())
    if name == "aperture_mixed_wave" and s > 1:      # half the strata ordinary but 1.5e19 away, where every ray "sees" a light sphere (the CPU file)
        assert degenerate.sum(axis=1).min() > 0 and (~degenerate).sum(axis=1).min() > 0 and not cov.any() and (exp.view(np.uint32)[:, 14] > 0).all()
    if name in ALL_MISS or (name == "aperture_mixed_wave" and s == 1):      # (one stratum at s = 1: its radius 3e19 * sqrt(0.5) is beyond the overflow)
        e = exp.view(np.uint32)
        assert not cov.any() and not exp[:, 8:11].view(F).any(), "coverage 0 everywhere, position (0, 0, 0)"
        assert (e[:, 13] == 0).all() and (e[:, 14] == 0).all() and not names.any() and (exp[:, 3].view(F) == np.finfo(F).max).all(), "the k = 0 miss record"
    r, sb = renderer(pkg, device, cornell_scene, AOV_W, AOV_H)
    r.set_camera(cam.buffer)
    info = capi.TraceInfo()
    got = capi.lens_aov.aovs(r, s, lens, info=info).cpu().numpy()
    assert info.flags & capi.STAT_CAST_WIDE and not (info.flags & FAULTS(capi)), "flags %#x" % info.flags
    excepted = compare_records_capped(cornell_scene, got, exp, rec, names)
    print("%s s = %d: %d NaN words in the expected records" % (name, s, excepted))
    assert excepted == 0, "no record of these classes holds a NaN: a degenerate ray is never a surface sample, and a miss has position 0"
    f = capi.aov_fields(got)
    assert np.array_equal(f["coverage"].ravel(), cov)
    if name in ALL_MISS:
        assert (f["triangle"] == -1).all() and not f["light"].any() and not f["material"].any() and not f["position"].any()
    r.close(); sb.close(); cam.close()


# ---------------------------------------------------------------------------------------------------------------- d. the denoiser on them
def beauty_frame(pkg, device, scene, iterations=6):
    """A renderer that holds a few pinhole iterations of the default camera (the beauty the lens records are to guide)."""
    r, sb, cam = make(pkg, device, scene)
    for _ in range(iterations):
        cam.update(0.0); r.set_camera(cam.buffer); r.iterate()
    r.synchronize()
    return r, sb, cam


def test_denoiser_copies_a_frame_without_a_surface_pixel(pkg, device, wide, cornell_scene):
    """focus 1e30: every lens ray has a zero direction, every record has coverage 0, no pixel is a surface pixel (gd_prepare): the
    filter has nothing to do and gmupt_render_denoised_lens returns the beauty bit for bit."""
    capi = pkg.capi
    r, sb, cam = beauty_frame(pkg, device, cornell_scene)
    beauty = r.framebuffer().view(np.uint32)
    assert int(beauty[..., 3].sum()) > 0 and beauty[..., :3].any()
    for name in ("focus_1e30", "focus_flt_max"):
        lens = X.lens_of(capi, name)
        for s in (1, 2):
            f = capi.aov_fields(capi.lens_aov.aovs(r, s, lens))
            assert not f["coverage"].any() and not surface_pixels(f).any(), (name, s)
            info = capi.TraceInfo()
            out = capi.lens_aov.denoise(r, s, lens, info=info).cpu().numpy().view(np.uint32)
            assert not (info.flags & FAULTS(capi))
            assert np.array_equal(out, beauty), (name, s)
    assert np.array_equal(r.framebuffer().view(np.uint32), beauty)
    close(r, sb, cam)


def test_denoiser_on_the_mixed_records(pkg, device, wide, cornell_scene):
    """The mixed-wave focus (0.3, 1.5e19) at s = 2: records whose samples are part ordinary, part zero-direction.  The output is finite wherever
    the beauty is, and every pixel that is no surface pixel of the lens record is the beauty's."""
    capi = pkg.capi
    r, sb, cam = beauty_frame(pkg, device, cornell_scene)
    beauty = r.framebuffer()
    lens = X.lens_of(capi, "focus_mixed_wave")
    f = capi.aov_fields(capi.lens_aov.aovs(r, 2, lens))
    surf = surface_pixels(f)
    assert 100 < surf.sum() < surf.size - 100 and ((f["coverage"] > 0) & (f["coverage"] < 4)).sum() >= 16
    print("mixed records: %d surface pixels of %d, coverage histogram %r" % (int(surf.sum()), surf.size, np.bincount(f["coverage"].ravel(), minlength=5).tolist()))
    out = capi.lens_aov.denoise(r, 2, lens).cpu().numpy()
    finite = np.isfinite(beauty[..., :3]).all(axis=-1)
    assert finite.all() and np.isfinite(out[..., :3][finite]).all()
    assert np.array_equal(out.view(np.uint32)[~surf], beauty.view(np.uint32)[~surf])
    assert np.array_equal(out[..., 3].view(np.uint32), beauty[..., 3].view(np.uint32))
    close(r, sb, cam)


# ---------------------------------------------------------------------------------------------------------------- e. the guards together
def test_tile_budget_and_plan_together(pkg, device, wide, cornell_scene):
    """One renderer with a tile origin, a path budget below the pool and a sampling plan at once, the ordinary lens (0.3, 13): after
    STAGE_SHADE the fresh slots that pass k_lens_retarget's guards hold the host rule's ray for the pixel in their state -- the tile
    origin and the plan's pixel are in it -- and the retired slots and every other word are the same renderer's without a lens."""
    capi = pkg.capi
    tile, pool, budget = (4, 3, 20, 12), 1024, 700          # test_adaptive_gpu.test_rectangle_plan_on_a_tile_renderer's tile; RECT lies inside it
    x0, y0, w, h = RECT
    lens = LU.lens_struct(capi, 0.3, 13.0)
    runs = []
    for with_lens in (False, True):
        r, sb, cam = make(pkg, device, cornell_scene, tile=tile, pool=pool, budget=budget)
        plan = capi.adaptive.Adaptive(r)
        plan.set_list(AU.rect_list(tile[2], x0 - tile[0], y0 - tile[1], w, h), tile[2], tile[3])
        capi.adaptive.set_adaptive(r, plan)
        if with_lens:
            capi.lens.set_lens(r, lens)
        cam.update(0.0); r.set_camera(cam.buffer); r.run_stage(capi.STAGE_SHADE)
        runs.append(snapshot(r) + (cam.buffer_copy(),))
        close(r, sb, cam)
    plain, lensed = runs
    qc = lensed[3]
    n_new = min(int(qc[0]), pool)
    q, slots = LU.fresh(qc, lensed[2], pool, budget)
    retired = np.setdiff1d(lensed[2][0][:n_new].astype(np.int64), slots)
    print("guards together: new-path count %d, lastPathCnt %d, fresh after the guards %d, retired %d" % (n_new, int(qc[1]), q.size, retired.size))
    assert n_new == pool and q.size == budget - int(qc[1]) and 0 < q.size < n_new and retired.size == n_new - q.size, "the budget retired part of the queue"
    xy = LU.state_screen(lensed[1], pool)[slots]
    assert ((xy[:, 0] >= x0) & (xy[:, 0] < x0 + w) & (xy[:, 1] >= y0) & (xy[:, 1] < y0 + h)).all(), "the plan's pixels, in frame coordinates"
    k = (int(qc[1]) + q).astype(np.int64) % (tile[2] * tile[3])
    unplanned = np.stack([tile[0] + k % tile[2], tile[1] + k // tile[2]], axis=1)
    assert (xy != unplanned).any(axis=1).sum() > q.size // 2, "the plan moved pixels away from where newPath.hlsl:33-34 puts them"
    assert np.array_equal(LU.bits(plain[0]), LU.bits(lensed[0])) and np.array_equal(plain[2], lensed[2]) and np.array_equal(plain[3], lensed[3])
    rays = host_rays(pkg, lensed[4], lens, plain[1], pool, q, slots)
    assert X.nan_words(rays) == 0
    want = LU.patch_rays(plain[1], pool, slots, rays)
    assert np.array_equal(want, lensed[1]), "fresh slots hold the host rule's ray for their pixel; retired slots and every other word are the run without a lens"
    o, _ = LU.state_rays(lensed[1], pool)
    pos = np.array(list(lensed[4].position)[:3], F)
    assert ((o[slots] != pos).any(axis=1)).mean() > 0.95 and (o[retired] == LU.state_rays(plain[1], pool)[0][retired]).all()

"""The census of the crafted shading states (shade_util.py) on the CPU oracle alone: every class reaches the queue and the branch it
claims to reach, before any GPU time is spent on it (tests/test_shade_edges_gpu.py runs the same states through k_logic + k_material).

Census findings that differ from what one might expect (also in shade_util.py and DESIGN.md, "Non-finite path state"):
  - a throughput of (-0.0, -0.0, -0.0) ends the path at logic.hlsl:237, a NaN throughput does not; saturate(NaN) = 0, so a NaN radiance
    accumulates as 0 and no ended path leaves a NaN in the target unless the pixel already held one or its count wraps;
  - a zero interpolated normal is stored as 0, not NaN (no normalize at logic.hlsl:94); the NaN appears one step later, in the tangent frame
    (normalize of a zero cross product): the normal-mapped variant stores a NaN normal, the plain one a NaN ray direction.  Glass with a
    zero normal stays finite: refract's k < 0 guard and cos2t < 0 send it to reflect(rayDir, 0) = rayDir;
  - the zero-radius light gives directLight = NaN (lightPdf = d^2 / 0 = inf, powerHeuristic inf / inf) whenever the BSDF evaluates to
    something non-zero, and the light is drawn by the slot's own RNG: such slots are the "+radius0" pseudo class; the zero-falloff light
    gives saturate(1 - inf) = 0, i.e. directLight = 0 * finite = 0;
  - roulette with pr = +-0 (rr_201_pr_zero, rr_201_pr_negzero) ends the path: a throughput whose maximum is +-0 fails :237 already, and
    1 / pr = +-inf is dropped.  Past :237 with pr = +-0 needs a NaN component beside the zeros, and then the path ends unless rand is
    exactly 0; that hangs on a single draw and is not crafted;
  - hmax(0, -0.0) = -0.0 and hmax(x, NaN) = x are not observable through these stages: the only consumer of a signed-zero maximum is the
    roulette's 1 / pr, and a path with pr = +-0 ends.  fmaxf has the same NaN rule as o_max, so an oracle built with it gives the same
    census; a NaN-propagating maximum (a + b when either is a NaN) fails the warm-up check of shaded(), test_branch_evidence and
    test_block_layouts_and_accumulation.
"""
import numpy as np
import pytest

import oracle_lib as O
import shade_util as S

P, L, W, H = S.P_POOL, S.L_LIVE, S.WIDTH, S.HEIGHT
STAGES = ("logic", "new_path", "material_ue4", "material_glass")


@pytest.fixture(scope="module")
def scene(pkg):
    return S.edge_scene(pkg)


def shaded(scene, layout, seed=3, max_depth=0, tile=None):
    """(oracle after the shade group on the crafted state, slot class names, the crafted state before the stages)"""
    w, h = (16, 8) if tile else (W, H)
    orc = O.Renderer(scene, w, h, P, live=L, tile=tile, max_depth=max_depth, threads=8)
    cam = O.Camera(W, H); cam.set_pose(*scene["camera"]); cam.buffer.lightCount = S.WARMUP_LIGHTS
    for _ in range(6):                      # ordinary iterations with the two ordinary lights: the state under the crafted one is NaN-free
        cam.update(); orc.set_camera(cam.buffer); orc.iterate()
    assert not nan_slots(orc).any()
    cam.buffer.lightCount = scene["light_count"]
    names = S.craft(orc, scene, layout, seed, origin=tile or (0, 0), size=(w, h))
    S.craft_framebuffer(orc.framebuffer())
    before = (orc.path_state().copy(), orc.framebuffer().copy())
    cam.update(); orc.set_camera(cam.buffer)
    for s in STAGES:
        orc.stage(s)
    return orc, S.with_light_suffix(orc, names), before


@pytest.fixture(scope="module")
def families(scene):
    out = {fam: shaded(scene, S.family_layout(fam)) for fam in S.FAMILIES}
    yield out
    for orc, _, _ in out.values():
        orc.close()


def queue_of(orc):
    qc, q = orc.counters(), orc.queues()
    where = np.full(L, "none", "U5")
    for qi, n, tag in ((0, qc[0], "ended"), (1, qc[2], "ue4"), (2, qc[3], "glass")):
        where[q[qi][:n]] = tag
    shadow = np.zeros(L, bool); shadow[q[4][:qc[6]]] = True
    return where, shadow


def nan_slots(orc, skip=()):
    st = orc.path_state()
    out = np.zeros(L, bool)
    for name, (_, _, _, t) in O.STATE_FIELDS.items():
        if t == "f" and name not in skip:
            out |= S._is_nan_bits(O.state_field(st, P, name, L)).any(axis=1)
    return out


def base(names):
    return np.array([n.split("+")[0] for n in names])


def f32(orc, name):
    return O.state_field(orc.path_state(), P, name, L).view(np.float32)


def test_every_class_ends_in_its_queue(families):
    # the census table; NaN = slots with a NaN word that the zero-radius light does not explain, dl = slots whose directLight is NaN through it
    print("\n%-28s %5s %-6s %6s %4s %3s" % ("class", "slots", "queue", "shadow", "NaN", "dl"))
    for fam, (orc, names, _) in families.items():
        where, shadow = queue_of(orc)
        r0 = np.char.endswith(names, "+radius0")
        nans = np.where(r0, nan_slots(orc, skip=("directLight",)), nan_slots(orc))
        dl = r0 & nan_slots(orc) & ~nans
        b = base(names)
        for cn in [n for n, c in S.CLASSES.items() if c["family"] == fam]:
            sl = b == cn
            got = sorted(set(where[sl].tolist()))
            print("%-28s %5d %-6s %6d %4d %3d" % (cn, sl.sum(), ",".join(got), shadow[sl].sum(), nans[sl].sum(), dl[sl].sum()))
            assert bool(nans[sl].any()) == (cn in S.NAN_CLASSES), cn
            assert sl.sum() >= 30 and got == [S.CLASSES[cn]["kind"]], (cn, got)
        qc = orc.counters()
        assert qc[0] + qc[2] + qc[3] == L and qc[4] == qc[0] and qc[5] == qc[0] + qc[2]


def test_nan_classes_are_the_literal_list(families):
    # a class is a NaN class if any of its slots holds a NaN word that the zero-radius light does not explain: any NaN in a slot without
    # the "+radius0" suffix, and any NaN outside directLight in a slot with it
    found, n_lit = set(), 0
    for fam, (orc, names, _) in families.items():
        b = base(names)
        unexplained = np.where(np.char.endswith(names, "+radius0"), nan_slots(orc, skip=("directLight",)), nan_slots(orc))
        found |= set(b[unexplained].tolist())
        lit = np.char.endswith(names, "+radius0") & ~np.isin(b, list(S.NAN_CLASSES))
        assert not nan_slots(orc, skip=("directLight",))[lit].any(), "directLight is the only NaN of a zero-radius-light slot"
        n_lit += int(lit.sum())
    assert n_lit > 500
    assert found == set(S.NAN_CLASSES), (sorted(found - set(S.NAN_CLASSES)), sorted(set(S.NAN_CLASSES) - found))
    every = [n for n, c in S.CLASSES.items() if c["family"] in S.FAMILIES]
    outside = [n for n in every if n not in S.NAN_CLASSES]
    assert len(outside) >= len(every) // 4, "a test made mostly of NaNs pins little"
    assert not [n for n, c in S.CLASSES.items() if c["layout"] and n in S.NAN_CLASSES]     # (the slots: test_block_layouts_and_accumulation)


def test_branch_evidence(scene, families):
    orc, names, before = families["ue4"]
    b = base(names)
    d, n, mr = f32(orc, "rayDirection"), f32(orc, "normal"), f32(orc, "matMR")
    q1 = orc.queues()[1][:orc.counters()[2]]
    assert np.array_equal(q1, np.arange(L)), "an all-UE4 pool: queue index = slot, so equal slots would give equal seeds"
    # the cosine lobe stays in the normal's hemisphere by construction (dz >= 0); the branch itself: test_diffuse_and_specular_branch_for_equal_seeds
    dn = (d.astype(np.float64) * n).sum(axis=1)
    assert (dn[b == "diffuse_only"] >= -1e-6).all()
    assert (mr[b == "rough_nan", 1] == np.float32(0.014)).all() and (mr[b == "rough_0", 1] == np.float32(0.014)).all()
    assert (mr[b == "rough_1", 1] == 1.0).all() and (mr[b == "metallic_2", 0] == 2.0).all()
    assert not n[b == "zero_normal"].any() and np.isnan(d[b == "zero_normal"]).all()
    assert np.isnan(n[b == "zero_normal_mapped"]).all()
    for cn in S.NORMAL_EDGES:                      # both sides of the 0.999 switch give a finite, orthonormal tangent frame: unit directions
        assert np.allclose(np.linalg.norm(d[b == cn].astype(np.float64), axis=1), 1.0, atol=1e-4), cn
        length = np.linalg.norm(d[b == cn + "_mapped"].astype(np.float64), axis=1)   # the mapped normal is not renormalised (logic.hlsl:123)
        assert np.isfinite(length).all() and (length > 0.5).all() and (length < 1.5).all(), cn
    assert (f32(orc, "lightThroughput")[b == "ray_along_plus_n"] == 0).all(), "back face: NdotV < 0 evaluates to 0"

    orc, names, before = families["glass"]
    b = base(names)
    d = f32(orc, "rayDirection").astype(np.float64)
    for cn in ("glass_tir", "glass_tir_other_side"):   # total internal reflection: the path stays on the side it came from (+z, inside)
        incoming = np.asarray(S.CLASSES[cn]["dir"], np.float64)
        assert incoming[2] > 0 and (d[b == cn][:, 2] < 0).all() and np.allclose(d[b == cn][:, :2], incoming[:2], atol=1e-6), cn
    assert (d[b == "glass_leaving_normal"][:, 2] != 0).all() and np.isfinite(d).all()
    assert (np.abs(d[b == "glass_normal_incidence"][:, 2]) == 1).all()
    assert np.array_equal(f32(orc, "lightThroughput")[b == "glass_tilted"], np.tile(np.float32((0.9, 0.95, 1.0)), ((b == "glass_tilted").sum(), 1)))

    orc, names, before = families["texture"]
    b = base(names)
    col, n = f32(orc, "matColor"), f32(orc, "normal")
    size = scene["tex_diffuse"].shape[1]
    texel0 = orc.sample(0, 0.5 / size, 0.5 / size, 0)[:3]          # the guard zeroes x = u * size - 0.5, i.e. texel 0 at weight 1
    assert np.array_equal(texel0, scene["tex_diffuse"][0, 0, 0, :3].astype(np.float32) / np.float32(255))
    assert (col[b == "uv_beyond_guard"] == texel0).all()
    assert (col[b == "uv_guard_u_only"] == orc.sample(0, 0.5 / size, 0.3, 0)[:3]).all()
    assert (col[b == "uv_neg_half"] == orc.sample(0, 0.5, 0.5, 0)[:3]).all() and (col[b == "uv_neg_1"] == orc.sample(0, 0.0, 0.0, 0)[:3]).all()
    assert (col[b == "uv_1"] == col[b == "uv_0"][0]).all() and (col[b == "uv_tiled"] == orc.sample(0, 0.25, 0.25, 0)[:3]).all()
    assert (col[b == "uv_0"] == orc.sample(0, 0.0, 0.0, 0)[:3]).all(), "u = 0 blends the last and the first texel"
    assert not np.array_equal(orc.sample(0, 0.0, 0.0, 0), orc.sample(0, 0.5 / size, 0.5 / size, 0))
    assert np.isnan(n[b == "bary_nan"]).all() and (col[b == "bary_nan"] == texel0).all()

    orc, names, before = families["nee"]
    b = base(names)
    where, shadow = queue_of(orc)
    assert shadow[b == "nee_all_lights_above"].all() and not shadow[b == "nee_no_light_above"].any()
    for cn in ("nee_grazing_light1", "nee_grazing_radius0"):
        assert 0 < shadow[b == cn].sum() < (b == cn).sum(), cn
    li = O.state_field(orc.path_state(), P, "lightIndex", L)[:, 0]
    dl = f32(orc, "directLight")
    far = (b == "nee_all_lights_above")
    assert ((li[far] == S.RADIUS0_LIGHT).sum() > 10) and ((li[far] == S.FALLOFF0_LIGHT).sum() > 10), "both edge lights are sampled"
    assert np.isnan(dl[far & (li == S.RADIUS0_LIGHT)]).all(), "zero radius: inf / inf in the power heuristic"
    assert not dl[far & (li == S.FALLOFF0_LIGHT)].any(), "zero falloff: saturate(1 - inf) = 0"
    close = (b == "nee_close") & (li == S.RADIUS0_LIGHT)
    assert close.sum() > 10 and np.isnan(dl[close]).all()
    ordinary = (b == "nee_close") & (li < 2)
    assert np.isfinite(dl[ordinary]).all() and dl[ordinary].any()

    orc, names, before = families["logic"]
    b = base(names)
    where, _ = queue_of(orc)
    thr = f32(orc, "throughput")
    assert (where[b == "thr_negzero"] == "ended").all() and (where[b == "thr_nan"] == "ue4").all() and (where[b == "thr_nan_x"] == "ue4").all()
    assert np.isnan(thr[b == "thr_nan"]).all() and np.isnan(thr[b == "thr_inf_lthr_zero"]).all()
    c = S.CLASSES["rr_201_survives"]
    t0 = np.asarray(c["thr"], np.float32) * np.asarray(c["lthr"], np.float32)
    assert (thr[b == "rr_201_survives"] == t0 * (np.float32(1.0) / t0.max())).all(), "throughput * (1 / pr)"
    got = thr[b == "rr_201_pr_inf"]
    assert np.isnan(got[:, 0]).all() and not got[:, 1:].any(), "inf * (1 / inf) = NaN, finite * 0 = 0"
    assert np.isnan(thr[b == "rr_201_pr_nan"]).all()
    assert (where[np.isin(b, ["rr_201_pr_zero", "rr_201_pr_negzero"])] == "ended").all(), "1 / pr with pr = +-0 is computed and dropped"
    assert (O.state_field(orc.path_state(), P, "pathLength", L)[b == "rr_200", 0] == 201).all()
    # ended paths were regenerated by newPath: throughput 1, pathLength 0 -- and none of them left a NaN in the target
    assert (thr[where == "ended"] == 1).all()
    assert np.array_equal(np.isnan(orc.framebuffer()[..., :3]), np.isnan(before[1][..., :3])), "saturate(NaN) = 0: a NaN radiance accumulates as 0"
    assert (where[np.isin(b, ["miss_rad_nan", "miss_thr_nan", "emit_above_light_count"])] == "ended").all()


def test_diffuse_and_specular_branch_for_equal_seeds(scene):
    # materialUE4 seeds its RNG by queue index; in an all-UE4 pool that is the slot.  The same slots crafted once as diffuse_only (metallic 0:
    # `rand < diffuseRatio` always) and once as specular_only (metallic 1: never) draw the same numbers and must leave in different directions.
    out = {}
    for cn in ("diffuse_only", "specular_only"):
        orc, names, _ = shaded(scene, np.full(L, cn))
        assert np.array_equal(orc.queues()[1][:orc.counters()[2]], np.arange(L)), "queue index = slot"
        out[cn] = f32(orc, "rayDirection").astype(np.float64)
        orc.close()
    a, s = out["diffuse_only"], out["specular_only"]
    assert np.isfinite(a).all() and np.isfinite(s).all() and (np.abs(a - s).max(axis=1) > 1e-3).all()
    mirror = S.GEN_DIR.astype(np.float64) - 2.0 * np.dot(S.GEN_DIR, S.N_GEN) * S.N_GEN.astype(np.float64)
    assert np.median(s @ mirror) > 0.9 > np.median(a @ mirror), "roughness 0.3: the specular lobe hugs the mirror direction, the cosine lobe does not"


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_block_layouts_and_accumulation(scene, variant):
    layout = S.block_layout(variant)
    orc, names, before = shaded(scene, layout, seed=3)
    where, shadow = queue_of(orc)
    want = np.array([{"E": "ended", "S": "ue4", "N": "ue4", "G": "glass"}[k] for k in layout])
    assert np.array_equal(where, want)
    assert np.array_equal(shadow, layout == "S"), "shadow-queue membership follows the layout"
    qc = orc.counters()
    assert (qc[0], qc[2], qc[3], qc[6]) == tuple(int((layout == k).sum()) if k != "U" else int(((layout == "S") | (layout == "N")).sum()) for k in ("E", "U", "G", "S"))
    if variant == 0:
        assert shadow[256:512].all() and not shadow[512:768].any() and (where[0:256] == "ended").all() and (where[768:1024] == "glass").all()
        blk = lambda b: [int(((where[b * 256:(b + 1) * 256]) == k).sum()) for k in ("ue4", "glass", "ended")]
        assert blk(4) == [63, 64, 129] and blk(6) == [1, 0, 255] and blk(7) == [64, 79, 65] and where[1791] == "ue4"
    # layout and accumulation classes stay finite, slot by slot: the only NaN is the directLight of a slot that drew the zero-radius light
    assert not nan_slots(orc, skip=("directLight",)).any()
    dl_nan = nan_slots(orc) 
    assert dl_nan.any() and np.char.endswith(names[dl_nan], "+radius0").all() and (layout[dl_nan] == "S").all()
    assert S.plan_is_complete(names)
    fb0, fb = before[1].view(np.uint32), orc.framebuffer().view(np.uint32)
    for name, (dx, dy), count, colour, paths in S.ACCUMULATION_PLAN:
        if count is not None:
            assert fb[dy, dx, 3] == (count + paths) & 0xFFFFFFFF, name
    assert fb[1, 5, 3] == 255 and np.isnan(orc.framebuffer()[1, 5, :3]).all(), "count 0xFFFFFFFF wraps: division by (float)0, then NaN * 0"
    nanpix = np.isnan(orc.framebuffer()[..., :3]).any(axis=2)
    assert np.array_equal(nanpix, S.nan_pixel_mask((H, W)) & nanpix) and nanpix[1, 5] and nanpix[1, 11] and not nanpix[1, 10]
    assert np.isinf(orc.framebuffer()[1, 10, :2]).all()
    # the paths aimed outside the target change no pixel: the counts of the whole target grow by exactly the in-target enders
    out_paths = sum(e[4] for e in S.ACCUMULATION_PLAN if e[2] is None)
    grown = (fb[..., 3].astype(np.int64) - fb0[..., 3].astype(np.int64)) % (1 << 32)
    assert int(grown.sum()) == int(qc[0]) - out_paths
    orc.close()


def test_tile_and_depth_legs(scene):
    # tile (8, 4) of a 32 x 18 frame, 16 x 8 pixels: the plan's outside coordinates are now inside the frame but outside the tile
    orc, names, before = shaded(scene, S.block_layout(0), tile=(8, 4))
    fb0, fb = before[1].view(np.uint32), orc.framebuffer().view(np.uint32)
    assert fb.shape == (8, 16, 4) and fb[1, 4, 3] == 7 + 256 and fb[1, 5, 3] == 255
    grown = (fb[..., 3].astype(np.int64) - fb0[..., 3].astype(np.int64)) % (1 << 32)
    assert int(grown.sum()) == int(orc.counters()[0]) - sum(e[4] for e in S.ACCUMULATION_PLAN if e[2] is None)
    orc.close()
    orc, names, _ = shaded(scene, S.family_layout("depth"), max_depth=S.DEPTH)
    where, _ = queue_of(orc)
    b = base(names)
    for cn in ("depth_below", "depth_at", "depth_above", "depth_roulette_survivor"):
        assert (where[b == cn] == S.CLASSES[cn]["kind"]).all(), cn
    orc.close()


def test_crafting_is_deterministic(scene):
    a = shaded(scene, S.block_layout(2), seed=9)
    b = shaded(scene, S.block_layout(2), seed=9)
    c = shaded(scene, S.block_layout(2), seed=10)
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1].view(np.uint32), b[2][1].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[2][0], c[2][0])
    for x in (a, b, c):
        x[0].close()

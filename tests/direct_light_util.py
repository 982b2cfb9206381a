"""Set-ups and checks for the direct-light triple (directLight, F_DL_R), shared by test_direct_light_cpu.py (the slot-class preconditions on
the oracle alone) and test_direct_light_gpu.py (k_logic + k_material against the oracle).  Needs no device unless one is passed in.

k_logic evaluates materialUE4.hlsl:184-188 for the slots it gives the shadow bit and stores directLight; k_material only pushes those slots
to the shadow queue.  What that split can break, and what is checked here:
  - WHO writes: directLight of every slot is pre-filled with its own bit pattern (signalling and quiet NaNs among them); after the shade
    group the slots of the shadow queue, and no others, hold something else;
  - WHICH operands: the stored light distance (distance - epsilon, not distance), the incoming ray direction, the stored normal and
    material values, the clamped light record.

Built on shade_util (scene, craft, compare) and parity_util without changing them; what shade_util.craft cannot place (a surface point
thousands of units away, the light count) is patched onto the crafted state afterwards.
"""
import numpy as np

import oracle_lib as O
import shade_util as S

STAGES = ("logic", "new_path", "material_ue4", "material_glass")
P, L, W, H = S.P_POOL, S.L_LIVE, S.WIDTH, S.HEIGHT                 # 2048 slots, 2000 live: 8 blocks of 256, the last one cut by L
MAX_LIGHTS = 128                                                    # rows of the light table: the largest light count it allows

# ---- the mid-flight pool with retired slots: every path ends at depth 3, and the budget lets only MIDFLIGHT_REFILL of the L slots start a
# second path; the others have retired when the crafted state arrives (a retired slot stays retired whatever its state holds)
MIDFLIGHT_DEPTH, MIDFLIGHT_REFILL = S.DEPTH, 600


def sentinels(pool):
    """(pool, 3) uint32, all distinct: negative finite values around -1.1e-16 (slot % 4 in 0, 2), signalling NaNs (1), quiet negative NaNs with a
    payload (3).  No direct light the shading arithmetic stores has one of these patterns: a generated NaN has no payload."""
    k = np.arange(pool * 3, dtype=np.uint32).reshape(pool, 3)
    slot = np.arange(pool)[:, None]
    w = np.uint32(0xA5000000) + k
    w = np.where(slot % 4 == 1, np.uint32(0x7F800001) + k, w)
    w = np.where(slot % 4 == 3, np.uint32(0xFFC00001) + k, w)
    return w.astype(np.uint32)


def prefill(orc, hip=None):
    """directLight of the whole pool := sentinels, in the oracle and (hip given) on the device; returns the sentinels"""
    s = sentinels(orc.pool)
    O.state_field(orc.path_state(), orc.pool, "directLight")[:] = s
    if hip is not None:
        hip.write_path_state(orc.path_state())
    return s


def census(orc, live):
    """Per live slot what the shade group made of it, from the oracle's queues: E ended (new path or retired now), S UE4 with a shadow ray,
    N UE4 without, G glass, R retired earlier (in no queue)."""
    qc, q = orc.counters(), orc.queues()
    kind = np.full(live, "R", "U1")
    kind[q[0][:min(int(qc[0]), live)]] = "E"
    kind[q[1][:qc[2]]] = "N"
    kind[q[2][:qc[3]]] = "G"
    shadow = q[4][:qc[6]]
    assert (kind[shadow] == "N").all(), "a shadow ray from a slot that is not in the UE4 queue"
    kind[shadow] = "S"
    return kind


def _is_nan(u):
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


def check_direct_light(orc, hip, live, sent, kind, strict=False, where=""):
    """directLight on bits, whole pool.  The one exception is shade_util.compare's: where the arithmetic GENERATED a NaN (zero-radius light:
    inf / inf) host and device may differ in its sign, so in a rewritten word a NaN matches a NaN; strict=True allows not even that."""
    pool = orc.pool
    a = O.state_field(orc.path_state(), pool, "directLight")
    b = O.state_field(hip.read_path_state(), pool, "directLight")
    pushed = np.zeros(pool, bool); pushed[:live] = kind == "S"
    generated = _is_nan(a) & _is_nan(b) & pushed[:, None] & (a != sent) & (b != sent) & (not strict)
    diff = (a != b) & ~generated
    assert not diff.any(), "%sdirectLight differs in %d words, first slot %d (%s): oracle %#x device %#x" % (
        where, diff.sum(), np.argwhere(diff)[0][0], kind[np.argwhere(diff)[0][0]] if np.argwhere(diff)[0][0] < live else "dead",
        a[tuple(np.argwhere(diff)[0])], b[tuple(np.argwhere(diff)[0])])
    # glass, UE4 without the shadow bit, ended, retired and dead slots keep their pattern
    kept = ~pushed
    assert np.array_equal(b[kept], sent[kept]), "%sa slot that pushes no shadow ray had its directLight written: slot %d" % (
        where, np.nonzero(kept)[0][(b[kept] != sent[kept]).any(axis=1)][0])
    # the rewritten slots are the shadow queue, and QC_SHADOWRAY counts them
    rewritten = np.nonzero((b != sent).any(axis=1))[0]
    qc = hip.counters()
    assert len(rewritten) == int(qc[6]), "%s%d slots rewritten, QC_SHADOWRAY = %d" % (where, len(rewritten), int(qc[6]))
    assert sorted(hip.read_queues()[4][:qc[6]].tolist()) == rewritten.tolist(), "%sthe shadow queue is not the set of rewritten slots" % where
    assert np.array_equal(orc.counters()[:7], qc[:7])


# ---------------------------------------------------------------------------------------------------------------- crafted pools
# operand identity: one class per operand the direct light takes (shade_util.CLASSES), cycled over the live slots at their own surface points
OPERAND_CLASSES = ("diffuse_only", "rough_0", "specular_only", "rough_clamp", "metallic_2", "colour_big", "ray_along_plus_n", "ray_perpendicular",
                   "ray_along_minus_n", "ray_unnormalised", "thr_nan", "thr_inf", "bary_nan", "bary_inf", "zero_normal", "nee_close",
                   "nee_grazing_light1", "nee_all_lights_above", "nee_no_light_above", "tex_normal", "glass_tilted", "acc_miss")
FAR = 12000.0            # light distances in [8192, 16384): one ulp is 2^-10 there, so distance - 1e-3 is the binary32 just below distance
FAR_FALLOFF = 1.0e5      # light 0 reaches that far (operand_scene), so the falloff term does not zero the product


def operand_layout():
    return np.array([OPERAND_CLASSES[i % len(OPERAND_CLASSES)] for i in range(L)])


def operand_scene(pkg):
    scene = dict(S.edge_scene(pkg))
    scene["lights"] = scene["lights"].copy()
    scene["lights"][0]["falloff"] = FAR_FALLOFF
    return scene


def far_slots(names):
    """every other slot of class "diffuse_only": moved FAR units below its triangle by place_far"""
    idx = np.nonzero(names == "diffuse_only")[0]
    return idx[::2]


def place_far(orc, scene, names):
    recs = scene["tris"].view(np.uint32).reshape(-1, 4)
    corner = scene["verts"].reshape(-1, 3)[recs[scene["edge_rows"]["diffuse_only"]][0]].astype(np.float64)
    sp = (corner - FAR * S.N_GEN.astype(np.float64)).astype(np.float32)
    O.state_field(orc.path_state(), orc.pool, "surfacePoint").view(np.float32)[far_slots(names)] = sp


class Crafted:
    """The oracle (and, with a device, the HIP renderer in lock step) after 6 ordinary iterations, then the crafted state with directLight
    pre-filled, `light_count` lights, and the shade group run once -- test_shade_edges_gpu.Pair with the two patches of this file."""

    def __init__(self, pkg, scene, layout, dev=None, light_count=None, far=False, seed=3, path_budget=0, max_depth=0):
        self.pkg, self.scene = pkg, scene
        self.orc = orc = O.Renderer(scene, W, H, P, live=L, path_budget=path_budget, max_depth=max_depth, threads=8)
        self.ocam = O.Camera(W, H); self.ocam.set_pose(*scene["camera"])
        self.hip = self.sb = self.hcam = None
        if dev is not None:
            self.sb = pkg.capi.SceneBuffers(dev, scene)
            self.hip = pkg.capi.Renderer(dev, W, H, pool_paths=P, live_paths=L, path_budget=path_budget, max_depth=max_depth)
            self.hip.bind_scene(self.sb)
            self.hcam = pkg.capi.Camera(W, H); self.hcam.set_pose(*scene["camera"])
        self._lights(S.WARMUP_LIGHTS)
        for _ in range(6):
            self.step()
        names = S.craft(orc, scene, layout, seed)
        if far:
            place_far(orc, scene, names)
        S.craft_framebuffer(orc.framebuffer())
        self.sent = prefill(orc)
        hip = self.hip
        if hip is not None:
            hip.write_path_state(orc.path_state()); hip.write_queues(orc.queues()); hip.write_counters(orc.counters())
            hip.write_framebuffer(orc.framebuffer())
        self._lights(scene["light_count"] if light_count is None else light_count)
        self._cameras()
        for s in STAGES:
            orc.stage(s)
        if hip is not None:
            hip.run_stage(pkg.capi.STAGE_SHADE)
        self.names = S.with_light_suffix(orc, names)
        self.kind = census(orc, L)

    def _lights(self, n):
        self.ocam.buffer.lightCount = n
        if self.hcam is not None:
            self.hcam.buffer.lightCount = n

    def _cameras(self):
        self.ocam.update(); self.orc.set_camera(self.ocam.buffer)
        if self.hip is not None:
            self.hcam.update(0.0)
            assert bytes(self.ocam.buffer) == bytes(self.hcam.buffer), "host camera streams diverged"
            self.hip.set_camera(self.hcam.buffer)

    def step(self):
        self._cameras()
        self.orc.iterate()
        if self.hip is not None:
            self.hip.iterate()

    def casts(self):
        self.orc.stage("extension"); self.orc.stage("shadow")
        if self.hip is not None:
            self.hip.run_stage(self.pkg.capi.STAGE_RAYCASTS)

    def compare(self, where=""):
        """the full state, queues, counters and framebuffer as shade_util.compare compares them.  The sentinels put NaNs into the radiance of
        slots of any class (logic.hlsl:230 adds directLight), so the class fence is off; "the same words hold a NaN on both sides" stays."""
        S.compare(self.orc, self.hip, P, L, self.names, class_fence=False, where=where)

    def field(self, name):
        return O.state_field(self.orc.path_state(), P, name, L)

    def close(self):
        flags = 0
        if self.hip is not None:
            flags = self.hip.stats().flags
            self.hip.close(); self.sb.close()
        self.orc.close()
        if self.hip is not None:
            assert not (flags & (self.pkg.capi.STAT_STACK_OVERFLOW | self.pkg.capi.STAT_CAST_ABORTED)), "flags %#x" % flags


def layout_preconditions(kind, variant):
    """what the block layouts of shade_util.block_layout are run for, read off the oracle's census"""
    blocks = [kind[b:b + 256] for b in range(0, L, 256)]
    assert len(blocks[-1]) < 256, "no tail block"
    for k in "ESNG":
        assert (kind == k).any(), "no slot of kind %s" % k
    if variant < 2:                                                     # the shuffle has no homogeneous block
        assert any(not (b == "S").any() for b in blocks[:-1]), "no full block without a shadow-pushing slot"
    if variant == 0:
        assert (blocks[1] == "S").all(), "block 1 is not all shadow-pushing"
        assert (blocks[6] == "S").nonzero()[0].tolist() == [255], "block 6 does not hold its one shadow-pushing slot in the last lane"


def operand_preconditions(c, light_count):
    """every operand case of the direct light is present among the slots that push a shadow ray (or, where the case means that none is
    pushed, among those that do not)"""
    kind, names = c.kind, np.char.partition(c.names, "+")[:, 0]
    pushed = kind == "S"
    dl = c.field("directLight").view(np.float32)
    dist = c.field("lightDistance").view(np.float32)[:, 0]
    li = c.field("lightIndex")[:, 0]
    lights = c.scene["lights"]
    with np.errstate(all="ignore"):
        lit = pushed & np.isfinite(dl).all(axis=1) & (dl != 0).any(axis=1)
        row = lights[np.minimum(li, MAX_LIGHTS - 1)]
        real = row["radius"] > 0                                        # rows beyond the scene's lights are zero; light 2 has radius 0
        assert (li[pushed] < light_count).all() and (li[kind != "E"] == light_count - 1).any(), "the last light was not sampled"
        if light_count == 1:
            # distance - epsilon one ulp below distance, in a product that is not zero (light 0 reaches that far)
            far = np.zeros(L, bool); far[far_slots(names)] = True
            assert (far & lit & (dist >= 8192.0) & (dist < 16384.0)).any(), "no lit slot at a distance where epsilon is one ulp"
        else:
            # falloff smaller than the distance (light 3: falloff 0): lightFalloff is exactly 0 and so is the product
            short = pushed & real & (row["falloff"] < dist)
            assert short.any() and (dl[short] == 0).all(), "falloff < distance does not give a zero direct light"
            assert (pushed & ~real).any(), "no slot sampled a zero row of the light table"
        for name in ("rough_0", "specular_only", "metallic_2", "colour_big", "tex_normal", "thr_nan", "thr_inf", "ray_unnormalised"):
            assert (pushed & (names == name)).any(), "no shadow-pushing slot of class %s" % name
        for name in ("ray_along_plus_n", "ray_perpendicular"):          # NdotV <= 0: ue4Evaluate returns 0
            sel = pushed & real & (names == name)
            assert sel.any() and (dl[sel] == 0).all(), name
        assert ((names == "bary_nan") & (kind == "N")).any(), "a NaN normal must not push a shadow ray"
        assert (kind == "G").any() and (kind == "E").any() and (kind == "N").any()

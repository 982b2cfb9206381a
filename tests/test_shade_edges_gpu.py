"""GPU tests of the shading stages (k_logic + k_material: logic, newPath, materialUE4, materialGlass) on crafted edge states, bit for bit
against the CPU oracle: non-finite and signed-zero path state, BSDF / NEE / texture-addressing edges, homogeneous and boundary class
layouts of k_material's LDS regroup, and the accumulation edges of accumulate_pixel.  The states come from shade_util.py; what each class
reaches is established on the oracle alone by tests/test_shade_edges_cpu.py.

Why every test terminates (read before the first run):
  - k_logic and k_material have no data-dependent loop except accumulate_pixel.  Everything a crafted value can change there is WHICH branch
    a lane takes and what it stores: a NaN fails every comparison, float -> int conversions are of RNG values (index-derived, in [0, 1)) and of
    texture coordinates behind the |x| < 1e9 guard, table indices are clamped (material, light) or copied from real rows of the scene
    (triangle), and pixel_index() bounds every screen coordinate before it is used;
  - accumulate_pixel's outer loop runs once per list entry and its inner loop walks the list: the lists are built by atomicExch in k_logic
    (each slot is pushed at most once, so they are acyclic) and the longest one here has 256 entries -- 256^2 dependent loads in one lane,
    milliseconds;
  - the scans' loops run over groups and waves (counts of the launch, not of the data);
  - the ray casts that follow in some tests take NaN / zero / unnormalised rays written by stage_ue4 and stage_glass: covered by the
    argument at the top of test_degenerate_rays_gpu.py plus the watchdog, whose flag every test here asserts absent.
"""
import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
import shade_util as S

pytestmark = pytest.mark.gpu
P, L, W, H = S.P_POOL, S.L_LIVE, S.WIDTH, S.HEIGHT
STAGES = ("logic", "new_path", "material_ue4", "material_glass")
CAST_FIELDS = ["surfacePoint", "baryCoord", "triangle", "isEmitter", "hitDistance", "inShadow"]


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def scene(pkg):
    return S.edge_scene(pkg)


class Pair:
    """The oracle and the HIP renderer after 6 lock-step ordinary iterations, then the crafted state on both and the shade group run."""

    def __init__(self, pkg, dev, scene, layout, seed=3, tile=None, max_depth=0):
        self.pkg, self.tile = pkg, tile
        w, h = (16, 8) if tile else (W, H)
        self.orc, self.hip, self.ocam, self.hcam, self.sb = PU.make_pair(pkg, dev, scene, w, h, P, live=L, tile=tile, max_depth=max_depth,
                                                                         full=(W, H) if tile else None)
        orc, hip = self.orc, self.hip
        self.ocam.buffer.lightCount = self.hcam.buffer.lightCount = S.WARMUP_LIGHTS
        for _ in range(6):
            PU.step_both(orc, hip, self.ocam, self.hcam)
        self.names = np.full(L, "generic", "U48")
        self.compare(nan_classes=(), where="after 6 ordinary iterations: ")          # strict: no NaN anywhere yet
        self.ocam.buffer.lightCount = self.hcam.buffer.lightCount = scene["light_count"]
        names = S.craft(orc, scene, layout, seed, origin=tile or (0, 0), size=(w, h))
        S.craft_framebuffer(orc.framebuffer())
        hip.write_path_state(orc.path_state()); hip.write_queues(orc.queues()); hip.write_counters(orc.counters())
        hip.write_framebuffer(orc.framebuffer())
        self.ocam.update(); self.hcam.update(0.0)
        assert bytes(self.ocam.buffer) == bytes(self.hcam.buffer)
        orc.set_camera(self.ocam.buffer); hip.set_camera(self.hcam.buffer)
        for s in STAGES:
            orc.stage(s)
        hip.run_stage(pkg.capi.STAGE_SHADE)
        self.names = S.with_light_suffix(orc, names)
        self.compare(where="shade group: ")

    def compare(self, **kw):
        kw.setdefault("nan_pixels", S.nan_pixel_mask(self.orc.framebuffer().shape[:2]))
        S.compare(self.orc, self.hip, P, L, self.names, **kw)

    def casts(self):
        self.orc.stage("extension"); self.orc.stage("shadow")
        self.hip.run_stage(self.pkg.capi.STAGE_RAYCASTS)
        self.compare(fields=CAST_FIELDS, queues=False, where="ray casts: ")

    def close(self):
        flags = self.hip.stats().flags
        self.hip.close(); self.sb.close(); self.orc.close()
        assert not (flags & (self.pkg.capi.STAT_STACK_OVERFLOW | self.pkg.capi.STAT_CAST_ABORTED)), "flags %#x" % flags


@pytest.mark.parametrize("variant", [0, 1, 2], ids=["fixed", "mirror", "shuffle"])
def test_block_layouts(pkg, device, scene, variant):
    # all-ended, all-UE4 (with / without the shadow bit), all-glass blocks, class counts 63 / 64 / 65 across wave boundaries, a lone item in
    # lane 255 / lane 0, a block cut by L: s_item / s_srank packing, nBlk offsets, the early return and the s_pre[3] + s_srank shadow rank
    p = Pair(pkg, device, scene, S.block_layout(variant))
    qc = p.hip.counters()
    layout = S.block_layout(variant)
    assert (int(qc[0]), int(qc[3]), int(qc[6])) == (int((layout == "E").sum()), int((layout == "G").sum()), int((layout == "S").sum()))
    p.casts()                                  # the rays that stage_ue4 / stage_glass wrote then go through the shipped cast
    p.close()


def test_block_layouts_with_one_block_per_group(pkg, scene):
    # the scan1 build has one block per group: 8 groups, every block adds up the group totals before its own
    with pkg.capi.use_build("scan1"):
        dev = pkg.capi.Device(0)
        for variant in (0, 1, 2):
            p = Pair(pkg, dev, scene, S.block_layout(variant))
            p.casts()
            p.close()
        dev.close()


@pytest.mark.parametrize("family", S.FAMILIES)
def test_value_classes(pkg, device, scene, family):
    p = Pair(pkg, device, scene, S.family_layout(family))
    p.casts()
    p.close()


def test_accumulation_edges(pkg, device, scene):
    # 1 / 2 / 64 / 256 paths ending on one pixel, sample counts 0, 2^24 - 1, 2^24, 2^24 + 1 and 0xFFFFFFFF, inf and NaN colours, screen
    # coordinates outside the target (Pair compares the whole framebuffer); then the same with a tile, where "outside" lies inside the frame
    p = Pair(pkg, device, scene, S.block_layout(0), seed=4)
    fb = p.hip.framebuffer().view(np.uint32)
    for name, (dx, dy), count, colour, paths in S.ACCUMULATION_PLAN:
        if count is not None:
            assert fb[dy, dx, 3] == (count + paths) & 0xFFFFFFFF, name
    p.close()
    p = Pair(pkg, device, scene, S.block_layout(2), seed=4, tile=(8, 4))
    fb = p.hip.framebuffer().view(np.uint32)
    assert fb.shape == (8, 16, 4) and fb[1, 4, 3] == 7 + 256 and fb[1, 5, 3] == 255
    p.close()
    p = Pair(pkg, device, scene, S.family_layout("depth"), max_depth=S.DEPTH)
    qc = p.hip.counters()
    assert qc[0] == sum(S.CLASSES[str(n).split("+")[0]]["kind"] == "ended" for n in p.names)
    p.close()


def test_two_more_iterations_stay_identical(pkg, device, scene):
    # whatever the edge values left behind is consumed identically: an infinite throughput meeting envColor or a zero lightThroughput, NaN
    # rays that miss, NaN radiance that ends.  A slot's class no longer describes its content after further iterations (inf * 0 makes new
    # NaNs in finite classes), so compare() runs with class_fence=False; "the same words hold a NaN on both sides" still holds.
    p = Pair(pkg, device, scene, S.family_layout("logic"))
    p.casts()
    for it in range(2):
        PU.step_both(p.orc, p.hip, p.ocam, p.hcam)
        p.compare(class_fence=False, where="iteration %d after: " % (it + 1))
    p.close()

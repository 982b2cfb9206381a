"""Crafted edge states for the shading stages (logic + newPath + materialUE4 + materialGlass), shared by test_shade_edges_cpu.py (the
census on the oracle alone) and test_shade_edges_gpu.py (k_logic + k_material against the oracle).  Needs no device.

  edge_scene(pkg)          the textured Cornell room plus a panel of small triangles whose vertex normals, uvs and materials are edge values,
                           and two more lights (radius 0, falloff 0)
  craft(orc, ...)          patches the oracle's path state in place, slot by slot, from the table of value CLASSES; a LAYOUT decides
                           which slot gets which kind (ended / UE4 with shadow ray / UE4 without / glass), so the regroup of k_material
                           can be driven block by block
  craft_framebuffer(fb)    edge sample counts and colours on the pixels that craft() aims ended paths at
  compare(orc, hip, ...)   all 21 state fields, the queues up to their counters, counters 0-6 and the framebuffer, on bits -- with one
                           fenced exception for generated NaNs (see compare)

What the census (test_shade_edges_cpu.py) found, kept here because it shapes the table:
  - the RNG draws of a slot depend on its index, not on the crafted values: which LIGHT a slot samples cannot be chosen.  The zero-radius
    and zero-falloff lights are therefore reached by count (four lights, hundreds of UE4 slots), and the census asserts that they were;
  - a slot cannot be retired from outside (retirement is the path budget's doing), so the fourth quarter of block 4 is ended paths;
  - the guard of sample_bilinear acts on x = u * size - 0.5, not on u: a coordinate beyond 1e9 samples texel 0 at weight 1, which is
    sample(u = 0.5 / size), not sample(u = 0);
  - with pathLength > 200, `1 / pr` with pr == +-0 is computed and dropped: a throughput whose maximum is +-0 has ended at :237 already.
    Only a NaN component beside the zeros gets past :237 with pr == +-0, and then the path ends unless rand is exactly 0 -- an outcome that
    hangs on one draw of one slot, so it is not crafted (thr_nan_rest_nonpositive has those values below the roulette threshold).
    pr = NaN survives (rand > NaN is false) and pr = +inf survives with inf * (1 / inf) = NaN.
"""
import numpy as np

import oracle_lib as O

FLT_MAX = np.float32(3.4028234663852886e38)
F = np.float32
NAN, INF = F(np.nan), F(np.inf)
P_POOL, L_LIVE, WIDTH, HEIGHT = 2048, 2000, 32, 18

Z999 = F(0.999)
Z999_BELOW, Z999_ABOVE = np.nextafter(Z999, F(0)), np.nextafter(Z999, F(1))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


N_GEN = _unit((0.3, 0.2, 0.93))
GEN_DIR = _unit((0.2, -0.3, -0.9))        # front-facing for N_GEN and for (0, 0, 1)


def _nz(z):
    """a unit-length normal (to binary32 rounding) whose z component is exactly z"""
    z = F(z)
    return np.array([np.sqrt(max(0.0, 1.0 - float(z) ** 2)), 0.0, z], np.float32)


# ---------------------------------------------------------------------------------------------------------------- the scene
# materials appended to the three textured ones of textured_mesh(): (colour, metallic, roughness, type, textureIndices)
M_DIFFUSE, M_SPECULAR, M_MET_NEG, M_MET_2, M_ROUGH_0, M_ROUGH_CLAMP, M_ROUGH_1, M_ROUGH_NAN, M_COL_BIG, M_COL_NEG, M_GLASS, M_GENERIC, \
    M_TEX_COLOUR, M_TEX_MR, M_TEX_NORMAL = range(3, 18)
_MATERIALS = [
    ((0.7, 0.6, 0.5), 0.0, 1.0, 0, (-1, -1, -1)), ((0.7, 0.6, 0.5), 1.0, 0.3, 0, (-1, -1, -1)), ((0.7, 0.6, 0.5), -0.5, 0.5, 0, (-1, -1, -1)),
    ((0.7, 0.6, 0.5), 2.0, 0.5, 0, (-1, -1, -1)), ((0.7, 0.6, 0.5), 0.5, 0.0, 0, (-1, -1, -1)), ((0.7, 0.6, 0.5), 0.5, 0.014, 0, (-1, -1, -1)),
    ((0.7, 0.6, 0.5), 0.5, 1.0, 0, (-1, -1, -1)), ((0.7, 0.6, 0.5), 0.5, np.nan, 0, (-1, -1, -1)), ((2.5, 1.5, 3.0), 0.5, 0.5, 0, (-1, -1, -1)),
    ((-0.5, 0.3, -1.0), 0.5, 0.5, 0, (-1, -1, -1)), ((0.9, 0.95, 1.0), 0.0, 0.1, 1, (-1, -1, -1)), ((0.6, 0.6, 0.6), 0.5, 0.4, 0, (-1, -1, -1)),
    ((0.5, 0.5, 0.5), 0.3, 0.6, 0, (2, -1, -1)), ((0.5, 0.5, 0.5), 0.3, 0.6, 0, (-1, 1, -1)), ((0.5, 0.5, 0.5), 0.3, 0.6, 0, (-1, -1, 0)),
]
UV_EDGES = {"uv_0": (0.0, 0.0), "uv_1": (1.0, 1.0), "uv_neg_half": (-0.5, -0.5), "uv_neg_1": (-1.0, -1.0), "uv_tiled": (7.25, 7.25),
            "uv_beyond_guard": (2e9, 2e9), "uv_0_1": (0.0, 1.0), "uv_neg_tiled": (-0.5, 7.25), "uv_guard_u_only": (2e9, 0.3)}
NORMAL_EDGES = {"nz_plus": (0.0, 0.0, 1.0), "nz_minus": (0.0, 0.0, -1.0), "nz_below_999": _nz(Z999_BELOW), "nz_at_999": _nz(Z999),
                "nz_above_999": _nz(Z999_ABOVE), "nz_below_m999": _nz(-Z999_BELOW), "nz_at_m999": _nz(-Z999), "nz_above_m999": _nz(-Z999_ABOVE)}
_CANCEL = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]      # zero at bary (0.5, 0.5, 0)


def edge_triangles():
    """{name: (three vertex normals, three vertex uvs, material index)}"""
    t = {}
    flat = lambda n, uv, m: ([n] * 3, [uv] * 3, m)
    for m, name in ((M_DIFFUSE, "diffuse_only"), (M_SPECULAR, "specular_only"), (M_MET_NEG, "metallic_neg"), (M_MET_2, "metallic_2"),
                    (M_ROUGH_0, "rough_0"), (M_ROUGH_CLAMP, "rough_clamp"), (M_ROUGH_1, "rough_1"), (M_ROUGH_NAN, "rough_nan"),
                    (M_COL_BIG, "colour_big"), (M_COL_NEG, "colour_neg"), (M_GENERIC, "generic"), (M_TEX_COLOUR, "tex_colour"), (M_TEX_MR, "tex_mr"),
                    (M_TEX_NORMAL, "tex_normal"), (1, "tex_colour_room"), (2, "tex_mr_normal_room")):
        t[name] = flat(N_GEN, (7.25, 3.5), m)
    for name, n in NORMAL_EDGES.items():
        t[name] = flat(n, (0.3, 0.6), M_GENERIC)
        t[name + "_mapped"] = flat(n, (0.3, 0.6), M_TEX_NORMAL)
    t["zero_normal"] = (_CANCEL, [(0.3, 0.6)] * 3, M_GENERIC)
    t["zero_normal_mapped"] = (_CANCEL, [(0.3, 0.6)] * 3, M_TEX_NORMAL)
    t["glass"] = flat((0.0, 0.0, 1.0), (0.3, 0.6), M_GLASS)
    t["glass_tilted"] = flat(N_GEN, (0.3, 0.6), M_GLASS)
    t["glass_zero_normal"] = (_CANCEL, [(0.3, 0.6)] * 3, M_GLASS)
    for name, uv in UV_EDGES.items():
        t[name] = flat(N_GEN, uv, 0)                               # material 0: all three texture kinds
    t["nee_up"] = flat((0.0, 0.0, 1.0), (0.3, 0.6), M_GENERIC)
    return t


def edge_scene(pkg):
    capi = pkg.capi
    mesh = pkg.scenes.textured_mesh()
    tris = edge_triangles()
    mats = np.zeros(len(_MATERIALS), dtype=capi.material_dtype)
    for k, (col, met, rough, mtype, tex) in enumerate(_MATERIALS):
        mats[k]["color"] = (*col, 1.0); mats[k]["metallic"], mats[k]["roughness"] = met, rough
        mats[k]["refractIndex"], mats[k]["transmittance"] = 1.458, 0.0
        mats[k]["textureIndices"] = tex; mats[k]["materialType"] = mtype
    nv0 = mesh["verts"].shape[0]
    v, n, uv, vm, idx, first = [], [], [], [], [], {}
    for k, (name, (normals, uvs, m)) in enumerate(tris.items()):
        x, y, z = -4.4 + 0.7 * (k % 12), 1.0 + 0.9 * (k // 12), -4.8
        first[name] = nv0 + 3 * k
        v += [(x, y, z), (x + 0.5, y, z), (x, y + 0.5, z)]; n += list(normals); uv += list(uvs); vm += [m] * 3
        idx.append((nv0 + 3 * k, nv0 + 3 * k + 1, nv0 + 3 * k + 2))
    lights = mesh["lights"].copy()
    lights[2]["position"] = (-2.0, 8.0, 1.0); lights[2]["falloff"] = 100.0; lights[2]["emission"] = (60.0, 30.0, 90.0); lights[2]["radius"] = 0.0
    lights[3]["position"] = (3.0, 7.0, -1.0); lights[3]["falloff"] = 0.0; lights[3]["emission"] = (50.0, 90.0, 20.0); lights[3]["radius"] = 0.5
    mesh.update({"verts": np.concatenate([mesh["verts"], np.asarray(v, np.float32)]),
                 "normals": np.concatenate([mesh["normals"], np.asarray(n, np.float32)]),
                 "uv": np.concatenate([mesh["uv"], np.asarray(uv, np.float32)]),
                 "vertex_material": np.concatenate([mesh["vertex_material"], np.asarray(vm, np.uint32)]),
                 "indices": np.concatenate([mesh["indices"], np.asarray(idx, np.int32)]),
                 "materials": np.concatenate([mesh["materials"], mats]), "lights": lights, "light_count": 4, "name": "shade_edges"})
    scene = pkg.scenes.build_scene(mesh)
    recs = scene["tris"].view(np.uint32).reshape(-1, 4)
    rows = {}
    for name, f in first.items():
        hit = np.nonzero((recs[:, 0] == f) & (recs[:, 1] == f + 1) & (recs[:, 2] == f + 2))[0]
        assert len(hit), "edge triangle %s has no reference in the flattened tree" % name
        assert recs[hit[0], 3] == tris[name][2]
        rows[name] = int(hit[0])
    scene["edge_rows"] = rows                                      # name -> a real row of scene["tris"]
    scene["edge_triangles"] = tris
    return scene


# ---------------------------------------------------------------------------------------------------------------- value classes
# kind: the queue the class is MEANT for ("ue4", "glass", "ended"); the census checks it.  sp: "on" the triangle, or "below" / "above" =
# 1000 units along -normal / +normal (every light then lies in the normal's hemisphere / outside it), or an explicit point.
_DEF = dict(tri="generic", bary=(1.0, 0.0, 0.0), dir=GEN_DIR, sp="on", thr=(0.8, 0.7, 0.6), lthr=(0.9, 0.9, 0.9), rad=(0.1, 0.2, 0.05),
            dl=(0.3, 0.2, 0.1), insh=0, pl=2, emit=0, hit=2.5, layout=False)


def _classes():
    c = {}

    def add(family, name, kind, **kw):
        assert name not in c
        c[name] = dict(_DEF, family=family, kind=kind, **kw)

    # ---- logic: non-finite, negative and signed-zero state at logic.hlsl:237, :248-255 and the tonemap
    add("logic", "thr_nan", "ue4", thr=(NAN, NAN, NAN))
    add("logic", "thr_nan_x", "ue4", thr=(NAN, 0.5, 0.5))
    add("logic", "thr_nan_rest_nonpositive", "ue4", thr=(NAN, -0.0, 0.0))
    add("logic", "thr_inf", "ue4", thr=(INF, INF, INF))
    add("logic", "thr_neg", "ended", thr=(-0.5, -0.5, -0.5))
    add("logic", "thr_negzero", "ended", thr=(-0.0, -0.0, -0.0))
    add("logic", "thr_one_negative", "ue4", thr=(-1.0, 0.5, 0.2))
    add("logic", "lthr_zero", "ended", lthr=(0.0, 0.0, 0.0))
    add("logic", "lthr_negzero", "ended", lthr=(-0.0, -0.0, -0.0))
    add("logic", "thr_neg_lthr_neg", "ue4", thr=(-1.0, -1.0, -1.0), lthr=(-1.0, -1.0, -1.0))
    add("logic", "thr_inf_lthr_zero", "ue4", thr=(INF, INF, INF), lthr=(0.0, 0.0, 0.0))        # inf * 0 = NaN survives :237
    add("logic", "dl_nan_lit", "ue4", dl=(NAN, 1.0, INF))
    add("logic", "dl_nan_in_shadow", "ue4", dl=(NAN, 1.0, INF), insh=1)
    add("logic", "insh_large", "ue4", insh=0xFFFFFFFF, dl=(5.0, 5.0, 5.0))
    add("logic", "miss_rad_nan", "ended", rad=(NAN, NAN, NAN), hit=FLT_MAX)
    add("logic", "miss_rad_inf", "ended", rad=(INF, -INF, INF), hit=FLT_MAX)
    add("logic", "miss_rad_neg", "ended", rad=(-3.0, -0.0, -1e-30), thr=(0.0, 0.0, 0.0), hit=FLT_MAX)
    add("logic", "miss_thr_inf", "ended", thr=(INF, INF, INF), hit=FLT_MAX)                    # inf * envColor
    add("logic", "miss_thr_nan", "ended", thr=(NAN, 1.0, 1.0), hit=FLT_MAX)
    add("logic", "hit_inf", "ue4", hit=INF)                                                    # only == FLT_MAX is a miss
    add("logic", "hit_nan", "ue4", hit=NAN)
    add("logic", "emit_1", "ended", emit=1)
    add("logic", "emit_radius0_light", "ended", emit=3, thr=(INF, 0.5, NAN))
    add("logic", "emit_last_light", "ended", emit=4)
    add("logic", "emit_above_light_count", "ended", emit=5)                                    # a zero row of the table: 0 / 0
    add("logic", "emit_table_end", "ended", emit=128)
    add("logic", "emit_beyond_table", "ended", emit=200)
    add("logic", "emit_all_ones", "ended", emit=0xFFFFFFFF)
    add("logic", "rr_200", "ue4", pl=200, thr=(1e-3, 1e-3, 1e-3))                              # not yet roulette
    add("logic", "rr_201_survives", "ue4", pl=201, thr=(300.0, 100.0, 50.0), lthr=(1.0, 1.0, 1.0))   # pr * 0.004 > 1 > rand
    add("logic", "rr_202_survives", "ue4", pl=202, thr=(600.0, 900.0, 50.0), lthr=(1.0, 1.0, 1.0))
    add("logic", "rr_201_pr_tiny", "ended", pl=201, thr=(1e-30, 1e-30, 1e-30))
    add("logic", "rr_201_pr_zero", "ended", pl=201, thr=(0.0, -0.0, 0.0))                      # pr = hmax(0, hmax(-0.0, 0)) = +0: 1 / pr = inf, dropped
    add("logic", "rr_201_pr_negzero", "ended", pl=201, thr=(0.0, 0.0, -0.0))                   # pr = hmax(0, hmax(0, -0.0)) = -0.0: 1 / pr = -inf, dropped
    add("logic", "rr_201_pr_nan", "ue4", pl=201, thr=(NAN, NAN, NAN))
    add("logic", "rr_201_pr_inf", "ue4", pl=201, thr=(INF, 0.5, 0.25), lthr=(1.0, 1.0, 1.0))
    add("logic", "rr_201_pr_negative_nan", "ended", pl=202, thr=(NAN, -1.0, -2.0))
    # ---- UE4: materials, tangent frames, ray directions
    for name in ("diffuse_only", "specular_only", "metallic_neg", "metallic_2", "rough_0", "rough_clamp", "rough_1", "rough_nan", "colour_big", "colour_neg"):
        add("ue4", name, "ue4", tri=name, layout=True)
    for name in NORMAL_EDGES:
        add("ue4", name, "ue4", tri=name, layout=True)
        add("ue4", name + "_mapped", "ue4", tri=name + "_mapped")
    add("ue4", "zero_normal", "ue4", tri="zero_normal", bary=(0.5, 0.5, 0.0))
    add("ue4", "zero_normal_mapped", "ue4", tri="zero_normal_mapped", bary=(0.5, 0.5, 0.0))
    add("ue4", "ray_along_plus_n", "ue4", tri="nee_up", dir=(0.0, 0.0, 1.0))                    # back face, NdotV = -1
    add("ue4", "ray_along_minus_n", "ue4", tri="nee_up", dir=(0.0, 0.0, -1.0))
    add("ue4", "ray_perpendicular", "ue4", tri="nee_up", dir=(1.0, 0.0, 0.0))                   # NdotV = 0
    add("ue4", "ray_perpendicular_specular", "ue4", tri="specular_only", dir=_unit((N_GEN[1], -N_GEN[0], 0.0)))
    add("ue4", "ray_zero", "ue4", tri="generic", dir=(0.0, 0.0, 0.0))
    add("ue4", "ray_unnormalised", "ue4", tri="generic", dir=(2.0, -3.0, -9.0))
    # ---- glass
    add("glass", "glass_normal_incidence", "glass", tri="glass", dir=(0.0, 0.0, -1.0), layout=True)
    add("glass", "glass_grazing", "glass", tri="glass", dir=_unit((1.0, 0.0, -1e-4)), layout=True)
    add("glass", "glass_perpendicular", "glass", tri="glass", dir=(1.0, 0.0, 0.0), layout=True)
    add("glass", "glass_tir", "glass", tri="glass", dir=_unit((0.9, 0.0, 0.435)), layout=True)   # leaving the medium beyond the critical angle
    add("glass", "glass_tir_other_side", "glass", tri="glass", dir=_unit((0.0, -0.95, 0.31)), layout=True)
    add("glass", "glass_leaving_normal", "glass", tri="glass", dir=(0.0, 0.0, 1.0), layout=True)
    add("glass", "glass_leaving_at_critical", "glass", tri="glass", dir=_unit((0.6858711, 0.0, 0.7277228)), layout=True)  # sin = 1 / 1.458
    add("glass", "glass_tilted", "glass", tri="glass_tilted", layout=True)
    add("glass", "glass_zero_normal", "glass", tri="glass_zero_normal", bary=(0.5, 0.5, 0.0))
    add("glass", "glass_thr_inf", "glass", tri="glass", dir=(0.0, 0.0, -1.0), thr=(INF, 1.0, 1.0))
    # ---- next-event estimation
    add("nee", "nee_all_lights_above", "ue4", tri="nee_up", sp="below")
    add("nee", "nee_no_light_above", "ue4", tri="nee_up", sp="above")
    add("nee", "nee_grazing_light1", "ue4", tri="nee_up", sp=(5.0, 4.5, 2.0))                   # light 1 at z = 2.0 with radius 0.5: dot of either sign
    add("nee", "nee_grazing_radius0", "ue4", tri="nee_up", sp=(2.0, 8.0, 1.0 - 1e-3))           # the zero-radius light at exactly z = 1.0
    add("nee", "nee_on_radius0_light", "ue4", tri="nee_up", sp=(-2.0, 8.0, 1.0 - 1e-3))         # light direction 0 / 0 for that light
    add("nee", "nee_close", "ue4", tri="specular_only", sp="on")
    add("nee", "nee_glass_far", "glass", tri="glass", dir=(0.0, 0.0, -1.0), sp="below")
    # ---- texture addressing
    for name in UV_EDGES:
        add("texture", name, "ue4", tri=name)
    for name in ("tex_colour", "tex_mr", "tex_normal", "tex_colour_room", "tex_mr_normal_room"):
        add("texture", name, "ue4", tri=name, layout=name in ("tex_colour", "tex_mr", "tex_colour_room"))
    add("texture", "uv_interpolated", "ue4", tri="uv_neg_tiled", bary=(0.25, 0.5, 0.25))
    add("texture", "bary_nan", "ue4", tri="uv_tiled", bary=(NAN, 0.3, 0.3))
    add("texture", "bary_inf", "ue4", tri="uv_tiled", bary=(INF, 0.3, 0.3))
    add("texture", "bary_huge", "ue4", tri="uv_1", bary=(3e9, 0.0, 0.0))
    # ---- depth limit (only with max_depth = DEPTH)
    add("depth", "depth_below", "ue4", pl=DEPTH - 1)
    add("depth", "depth_at", "ended", pl=DEPTH)
    add("depth", "depth_above", "ended", pl=DEPTH + 1)
    add("depth", "depth_roulette_survivor", "ended", pl=201, thr=(300.0, 100.0, 50.0), lthr=(1.0, 1.0, 1.0))
    # ---- accumulation: paths ended by a miss, aimed at the pixels of ACCUMULATION_PLAN
    add("accumulation", "acc_miss", "ended", hit=FLT_MAX, layout=True)
    add("accumulation", "acc_zero_throughput", "ended", lthr=(0.0, 0.0, 0.0), layout=True)
    add("accumulation", "acc_emitter", "ended", emit=2, layout=True)
    return c


DEPTH = 3
CLASSES = _classes()
FAMILIES = ("logic", "ue4", "glass", "nee", "texture")

# The classes whose oracle output holds a NaN word in any state field after the shade group (census: test_shade_edges_cpu.py compares this
# literal with what the oracle produces).  Only in slots of these classes may compare() match a NaN by kind instead of by bits.
# A slot that sampled the zero-radius light in materialUE4 carries the suffix "+radius0" (with_light_suffix) whatever its class: it may hold
# a NaN in directLight, and nowhere else unless its class is listed here.
NAN_CLASSES = (
    "bary_huge", "bary_inf", "bary_nan", "dl_nan_lit", "hit_nan", "nee_on_radius0_light", "rr_201_pr_inf", "rr_201_pr_nan", "thr_inf_lthr_zero", "thr_nan",
    "thr_nan_rest_nonpositive", "thr_nan_x", "zero_normal", "zero_normal_mapped",
)

# pixel (dx, dy) relative to the target's origin -> (sample-count bits, colour or None to keep, paths ending there)
ACCUMULATION_PLAN = [
    ("one", (1, 1), 5, None, 1), ("two", (2, 1), 5, None, 2), ("sixty_four", (3, 1), 5, None, 64), ("cap", (4, 1), 7, None, 256),
    ("count_wraps", (5, 1), 0xFFFFFFFF, (0.25, 0.5, 0.75), 256), ("count_0", (6, 1), 0, (0.25, 0.5, 0.75), 1),
    ("count_2p24_minus_1", (7, 1), (1 << 24) - 1, (0.25, 0.5, 0.75), 2), ("count_2p24", (8, 1), 1 << 24, (0.25, 0.5, 0.75), 2),
    ("count_2p24_plus_1", (9, 1), (1 << 24) + 1, (0.25, 0.5, 0.75), 2), ("colour_inf", (10, 1), 9, (np.inf, -np.inf, 0.5), 1),
    ("colour_nan", (11, 1), 9, (np.nan, 0.5, np.nan), 1),
    # outside the target: no pixel may change
    ("left_of_target", (-1, 1), None, None, 2), ("right_of_target", ("W", 0), None, None, 2), ("below_target", (1, "H"), None, None, 2),
    ("all_ones", (0xFFFFFFFF, 0xFFFFFFFF), None, None, 2), ("x_all_ones", (0xFFFFFFFF, 3), None, None, 2),
]
# pixels of the plan whose colour is NaN after the shade group (census): the oracle's (x * 2^32 + r) / (float)0 and NaN colours
NAN_PIXELS = ("count_wraps", "colour_inf", "colour_nan")


def plan_coord(entry, origin, size):
    (dx, dy) = entry[1]
    x = origin[0] + size[0] if dx == "W" else dx if dx == 0xFFFFFFFF else (origin[0] + dx) & 0xFFFFFFFF
    y = origin[1] + size[1] if dy == "H" else dy if dy == 0xFFFFFFFF else (origin[1] + dy) & 0xFFFFFFFF
    return x, y


def craft_framebuffer(fb):
    """Edge sample counts and colours on the plan's pixels of the (H, W, 4) float32 target `fb` (a tile's own target included), in place."""
    bits = fb.view(np.uint32)
    for name, (dx, dy), count, colour, _ in ACCUMULATION_PLAN:
        if count is None:
            continue
        if colour is not None:
            fb[dy, dx, :3] = np.asarray(colour, np.float32)
        bits[dy, dx, 3] = count
    return fb


# ---------------------------------------------------------------------------------------------------------------- layouts
# kinds: E ended, S UE4 that pushes a shadow ray, N UE4 that does not, G glass
def block_layout(variant=0, P=P_POOL, L=L_LIVE):
    """Per-slot kinds of the fixed layout (8 blocks of 256, the last one cut by L); variant 1 mirrors the classes (what was UE4 becomes
    glass, glass ended, ended UE4) and puts the lone slot of block 6 in lane 0; variant >= 2 is a seeded shuffle of variant 0's multiset."""
    assert P == 2048
    k = np.empty(P, "U1")
    k[0:256] = "E"
    k[256:512] = "S"
    k[512:768] = "N"
    k[768:1024] = "G"
    b = 1024
    k[b:b + 63] = "S"; k[b + 63:b + 127] = "G"; k[b + 127:b + 192] = "E"; k[b + 192:b + 256] = "E"
    k[1280:1536] = np.array(["S", "G", "E", "N"])[np.arange(256) % 4]
    k[1536:1792] = "E"; k[1791] = "S"
    b = 1792
    k[b:b + 65] = "E"; k[b + 65:b + 129] = "N"; k[b + 129:b + 192] = "G"; k[b + 192:b + 256] = "G"
    if variant == 1:
        k = np.array([{"S": "G", "N": "G", "G": "E", "E": "S"}[x] for x in k], "U1")
        k[0:256] = "E"                       # block 0 stays all ended
        k[1536:1792] = "E"; k[1536] = "N"    # lone UE4 slot in lane 0, without the shadow bit
        k[1280:1536] = np.array(["E", "N", "G", "S", "G"])[np.arange(256) % 5]
    elif variant >= 2:
        live = k[:L].copy()
        np.random.default_rng([7, variant]).shuffle(live)
        k[:L] = live
    return k[:L]


def family_layout(family, L=L_LIVE):
    """None-kind layout: slot i carries class i mod n of the family, each with its own surface point"""
    names = [n for n, c in CLASSES.items() if c["family"] == family]
    return np.array([names[i % len(names)] for i in range(L)])


def _class_normal(scene, c):
    normals = np.asarray(scene["edge_triangles"][c["tri"]][0], np.float64)
    return normals.T @ np.asarray(c["bary"], np.float64)


def craft(orc, scene, layout, seed, origin=(0, 0), size=(WIDTH, HEIGHT)):
    """Patches the oracle's path state in place.  `layout`: per live slot either a kind (block_layout) or a class name (family_layout).
    Returns the per-slot array of class names.  Ended slots are aimed at the pixels of ACCUMULATION_PLAN (in the order of a seeded
    permutation of the ended slots, so that one pixel's list spans blocks) while the plan lasts; every other slot meant to end is aimed
    below the plan's rows, so that the plan's pixels receive exactly the plan's paths."""
    P = orc.pool
    L = len(layout)
    rng = np.random.default_rng(seed)
    pools = {"S": [n for n, c in CLASSES.items() if c["layout"] and c["kind"] == "ue4"], "G": [n for n, c in CLASSES.items() if c["layout"] and c["kind"] == "glass"],
             "E": [n for n, c in CLASSES.items() if c["layout"] and c["kind"] == "ended"]}
    pools["N"] = pools["S"]
    start = {k: int(rng.integers(0, len(v))) for k, v in pools.items()}
    seen = {k: 0 for k in pools}
    names = np.empty(L, "U40")
    sp_override = [None] * L
    for i, tag in enumerate(layout):
        tag = str(tag)
        if tag in pools:
            names[i] = pools[tag][(start[tag] + seen[tag]) % len(pools[tag])]; seen[tag] += 1
            sp_override[i] = {"S": "below", "N": "above"}.get(tag)
        else:
            names[i] = tag
    st = orc.path_state()
    fu = lambda name: O.state_field(st, P, name)
    ff = lambda name: O.state_field(st, P, name).view(np.float32)
    recs = scene["tris"].view(np.uint32).reshape(-1, 4)
    verts = scene["verts"].reshape(-1, 3)
    with np.errstate(all="ignore"):
        for i in range(L):
            c = CLASSES[names[i]]
            row = recs[scene["edge_rows"][c["tri"]]]
            fu("triangle")[i] = row
            ff("baryCoord")[i] = np.asarray(c["bary"], np.float32)
            ff("rayDirection")[i] = np.asarray(c["dir"], np.float32)
            sp = sp_override[i] or c["sp"]
            corner = verts[row[0]].astype(np.float64)
            if isinstance(sp, str):
                n = _class_normal(scene, c)
                sp = corner if sp == "on" else corner - 1000.0 * n if sp == "below" else corner + 1000.0 * n
            ff("surfacePoint")[i] = np.asarray(sp, np.float32)
            ff("throughput")[i] = np.asarray(c["thr"], np.float32); ff("lightThroughput")[i] = np.asarray(c["lthr"], np.float32)
            ff("radiance")[i] = np.asarray(c["rad"], np.float32); ff("directLight")[i] = np.asarray(c["dl"], np.float32)
            fu("inShadow")[i, 0] = c["insh"]; fu("pathLength")[i, 0] = c["pl"]; fu("isEmitter")[i, 0] = c["emit"]
            ff("hitDistance")[i, 0] = np.float32(c["hit"])
    ended = np.array([i for i in range(L) if CLASSES[names[i]]["family"] == "accumulation"], np.int64)
    order = ended[rng.permutation(len(ended))] if len(ended) else ended
    k = 0
    for entry in ACCUMULATION_PLAN:
        take = order[k:k + entry[4]]; k += entry[4]
        if len(take) < entry[4]:
            break
        fu("screenCoord")[take] = np.asarray(plan_coord(entry, origin, size), np.uint32)
    planned = set(order[:k].tolist())
    for i in range(L):
        if CLASSES[names[i]]["kind"] == "ended" and i not in planned:
            fu("screenCoord")[i] = (origin[0] + i % size[0], origin[1] + 3 + (i // size[0]) % (size[1] - 3))
    return names


RADIUS0_LIGHT, FALLOFF0_LIGHT = 2, 3
WARMUP_LIGHTS = 2          # light count of the ordinary iterations before crafting: the two edge lights join with the crafted state


def with_light_suffix(orc, names):
    """The class names with "+radius0" appended for the slots that went through materialUE4 with the zero-radius light sampled (the light
    is drawn by the slot's RNG, so this is known only from the oracle's output): lightPdf is infinite there and the power heuristic inf / inf."""
    P, L = orc.pool, len(names)
    qc, q = orc.counters(), orc.queues()
    li = O.state_field(orc.path_state(), P, "lightIndex", L)[:, 0]
    out = names.astype("U48")
    for s in q[1][:qc[2]]:
        if li[s] == RADIUS0_LIGHT:
            out[s] = names[s] + "+radius0"
    return out


def plan_is_complete(names):
    return int(sum(CLASSES[str(n).split("+")[0]]["family"] == "accumulation" for n in names)) >= sum(e[4] for e in ACCUMULATION_PLAN)


# ---------------------------------------------------------------------------------------------------------------- comparison
def _is_nan_bits(u):
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


def compare(orc, hip, P, L, names, fields=None, nan_classes=NAN_CLASSES, nan_pixels=None, queues=True, framebuffer=True, class_fence=True, where=""):
    """Asserts that the HIP renderer holds what the oracle holds: the state fields of the live slots, counters 0-6, the four queues up to
    their counters (the shadow queue as a set, as test_parity_gpu._assert_same compares it) and the framebuffer.

    Equality is on bits, with one exception: a float word that is a NaN in the oracle matches ANY NaN on the device (the host CPU and the GPU
    may give a generated NaN different sign and payload bits).  The exception is fenced: per field the set of words holding a NaN must be
    identical on both sides, a NaN is accepted only in a slot whose class is in `nan_classes` -- or, in directLight alone, in a slot with
    the "+radius0" suffix -- (a framebuffer NaN only in a pixel of `nan_pixels`, an (H, W) mask), and every other word is compared as
    parity_util.compare_state compares it.  class_fence=False drops the class and pixel condition, not the others: for state that has
    gone through further iterations, where a slot's class no longer says what it holds."""
    a, b = orc.path_state(), hip.read_path_state()
    names = np.asarray(names).astype("U48")
    in_class = np.isin(np.char.partition(names, "+")[:, 0], list(nan_classes))
    radius0 = np.char.endswith(names, "+radius0")
    for name in (fields or O.STATE_FIELDS.keys()):
        fa, fb = O.state_field(a, P, name, L), O.state_field(b, P, name, L)
        if O.STATE_FIELDS[name][3] == "f":
            na, nb = _is_nan_bits(fa), _is_nan_bits(fb)
            if not np.array_equal(na, nb):
                idx = np.argwhere(na != nb)[0]
                raise AssertionError("%s%s: NaN in slot %d (%s) comp %d on one side only: oracle %#x device %#x" % (where, name, idx[0], names[idx[0]], idx[1], fa[tuple(idx)], fb[tuple(idx)]))
            stray = na.any(axis=1) & ~(in_class[:L] | (radius0[:L] if name == "directLight" else False)) & class_fence
            assert not stray.any(), "%s%s: NaN in slot %d of class %s, which is not a NaN class" % (where, name, np.nonzero(stray)[0][0], names[np.nonzero(stray)[0][0]])
            diff = (fa != fb) & ~na
        else:
            diff = fa != fb
        if diff.any():
            idx = np.argwhere(diff)
            raise AssertionError("%s%s differs in %d words, first slot %d (%s) comp %d: oracle %#x device %#x" % (where, name, len(idx), idx[0][0], names[idx[0][0]], idx[0][1], fa[tuple(idx[0])], fb[tuple(idx[0])]))
    qa, qb = orc.counters(), hip.counters()
    assert np.array_equal(qa[:7], qb[:7]), "%scounters %r vs %r" % (where, qa.tolist(), qb.tolist())
    if queues:
        oq, hq = orc.queues(), hip.read_queues()
        n_ext = min(int(qa[0]), L) + int(qa[2]) + int(qa[3])
        for q, n in ((0, min(int(qa[0]), L)), (1, int(qa[2])), (2, int(qa[3])), (3, n_ext)):
            assert np.array_equal(oq[q][:n], hq[q][:n]), "%squeue %d" % (where, q)
        assert sorted(oq[4][:qa[6]].tolist()) == sorted(hq[4][:qb[6]].tolist()), "%sshadow queue" % where
    if framebuffer:
        fa, fb = orc.framebuffer().view(np.uint32), hip.framebuffer().view(np.uint32)
        na, nb = _is_nan_bits(fa), _is_nan_bits(fb)
        na[..., 3] = False; nb[..., 3] = False                      # the sample count is an integer
        assert np.array_equal(na, nb), "%sframebuffer: NaN pixels differ" % where
        if na.any() and class_fence:
            assert nan_pixels is not None and not (na.any(axis=2) & ~nan_pixels).any(), "%sframebuffer: NaN outside the plan's NaN pixels" % where
        assert np.array_equal(fa[~na], fb[~na]), "%sframebuffer differs" % where


def nan_pixel_mask(shape):
    m = np.zeros(shape, bool)
    for name, (dx, dy), count, _, _ in ACCUMULATION_PLAN:
        if name in NAN_PIXELS:
            m[dy, dx] = True
    return m

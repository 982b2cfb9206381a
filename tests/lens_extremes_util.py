"""What the extreme-lens tests share (test_lens_extremes_cpu.py, test_lens_extremes_gpu.py): the table of lenses that
gmupt_renderer_set_lens admits and that make the rule of include/gmupt_lens.h overflow, underflow or cancel, the census of the rays they
produce, and the one comparison those tests use.  Needs no device.

The rule has no guard: `focus / dot3(d, fn)`, `pos + d*t` and `normalize3(Pf - origin)` are computed as written.  Three things happen:
  - a lens offset or a focal distance beyond about 1.84e19 makes dot3(v, v) inside normalize3 overflow: the length is +inf, 1 / inf = 0
    and every component times 0 is a ZERO direction;
  - a component that is itself infinite (d * t with t beyond FLT_MAX, or an origin minus it) meets that 0: inf * 0 = NaN; and a focal
    point that rounds onto the origin (a tiny focus with the draw r1 = 0, or a tiny focus with a tiny aperture) is the zero vector
    times 1 / 0: NaN again;
  - a denormal aperture gives denormal lens offsets, which only a camera at the origin keeps (pos + 1e-45 is pos anywhere else).
The origin stays finite throughout: an aperture is finite and sqrt(r1), |cos|, |sin| <= 1.

The comparison.  Host CPU and GPU may give a GENERATED NaN different sign and payload bits (x86's default NaN has the sign bit set).
same_words() is therefore equality of the 32-bit words except that a word that is a NaN in the REFERENCE may be any NaN in what is
compared with it.  It is a cap on one case, not a tolerance: every other word is compared on bits, a NaN where the reference has a
number fails, and every test that uses it states the number of excepted words from the reference alone (nan_words), 0 wherever the
census says a class generates no NaN.
"""
import numpy as np

import lens_util as LU

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
W, H, N = 32, 18, 4096
ORIGIN_POSE = (0.0, 0.0, 0.0, 0.0, 270.0)     # the default camera's orientation at the origin: the only place a denormal offset survives `pos + offset`
OFF_AXIS_POSE = LU.POSES[1]

# name: (aperture_radius, focus_distance, kind).  kind says what the census must find (census_holds):
#   ordinary   every direction a finite unit vector
#   zero       every direction (0, 0, 0) but those of the draws with a zero lens offset (r1 = 0), which stay ordinary
#   zero_all   every direction (0, 0, 0)
#   mixed      ordinary and zero directions, and at least one 64-aligned run of q with both.  Two of them: the aperture splits a wave by
#              the draw r1 (lens offsets around the 1.84e19 of the overflow; the ordinary rays start 1e19 from the scene), the focus by
#              the pixel (t = focus / dot3(d, fn) crosses 1.84e19 between the centre and the corners of the frame; the ordinary rays
#              start on a 0.3 lens and see the room)
#   tiny_focus every direction ordinary but those of the draws with a zero lens offset, which are NaN (Pf == origin)
#   zero_nan   zero and NaN directions, nothing ordinary
#   nan        every direction NaN
LENS_CLASSES = {
    "tested_today": (0.3, 13.0, "ordinary"),
    "aperture_min_denormal": (1e-45, 13.0, "ordinary"),
    "aperture_denormal": (1e-38, 13.0, "ordinary"),
    "aperture_1e18": (1e18, 13.0, "ordinary"),
    "aperture_1p5e19": (1.5e19, 13.0, "ordinary"),
    "aperture_mixed_wave": (3e19, 13.0, "mixed"),
    "aperture_1e30": (1e30, 13.0, "zero"),
    "aperture_flt_max": (FLT_MAX, 13.0, "zero"),
    "focus_min_denormal": (0.3, 1e-45, "tiny_focus"),
    "focus_1e_30": (0.3, 1e-30, "tiny_focus"),
    "focus_1e19": (0.3, 1e19, "ordinary"),
    "focus_mixed_wave": (0.3, 1.5e19, "mixed"),
    "focus_1e30": (0.3, 1e30, "zero_all"),
    "focus_3e38": (0.3, 3e38, "zero_nan"),
    "focus_flt_max": (0.3, FLT_MAX, "nan"),
    "both_min_denormal": (1e-45, 1e-45, "nan"),
}
DENORMAL_APERTURES = ("aperture_min_denormal", "aperture_denormal")
NO_NAN_KINDS = ("ordinary", "zero", "zero_all", "mixed")          # the classes whose reference may hold no NaN word at all


def lens_of(capi, name):
    a, f, _ = LENS_CLASSES[name]
    return LU.lens_struct(capi, a, f)


def census_inputs(n=N):
    """The inputs of the census: q = 0 .. n - 1 over the pixels of the 32 x 18 frame in scan order."""
    q = np.arange(n, dtype=np.uint32)
    return q, (q % W).astype(np.uint32), ((q // W) % H).astype(np.uint32)


def camera_buffer(capi, pose, updates=1):
    cam = LU.camera(capi, W, H, pose, updates=updates)
    cb = cam.buffer_copy()
    cam.close()
    return cb


def is_nan_words(u):
    u = np.asarray(u, np.uint32)
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


def nan_words(want):
    """How many 32-bit words of the reference are NaNs: the words same_words() compares by kind and not by bits."""
    return int(is_nan_words(LU.bits(np.asarray(want, F))).sum())


def same_words(got, want):
    """True when got equals want word for word, a word that is a NaN in `want` being allowed to be any NaN in `got`."""
    g, w = LU.bits(np.asarray(got, F)), LU.bits(np.asarray(want, F))
    if g.shape != w.shape:
        return False
    excepted = is_nan_words(w)
    return bool(np.array_equal(g[~excepted], w[~excepted]) and is_nan_words(g[excepted]).all())


def classify(rays):
    """Per ray of an (n, 8) array of gmupt_ray records: dict of masks -- ordinary (a finite direction of length 1 within 1e-3), zero (all
    three components +-0), nan (any component NaN), other (anything else: an infinite or a non-unit direction), bad_origin (a non-finite
    origin component)."""
    d = rays[:, 4:7].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(d).any(axis=1)
        zero = (d == 0).all(axis=1)
        unit = np.isfinite(d).all(axis=1) & (np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0) < 1e-3)
    return dict(ordinary=unit & ~nan, zero=zero, nan=nan, other=~(unit | zero | nan), bad_origin=~np.isfinite(rays[:, 0:3]).all(axis=1))


def census(capi, cb, name, n=N):
    """(counts, masks, rays) of class `name` under camera buffer `cb` from the host rule alone."""
    q, cx, cy = census_inputs(n)
    rays = capi.lens.lens_rays_host(cb, lens_of(capi, name), q, cx, cy)
    m = classify(rays)
    return {k: int(v.sum()) for k, v in m.items()}, m, rays


def mixed_runs(masks):
    """The 64-aligned runs of q that hold both an ordinary and a zero-direction ray."""
    o, z = masks["ordinary"].reshape(-1, 64).any(axis=1), masks["zero"].reshape(-1, 64).any(axis=1)
    return np.nonzero(o & z)[0]


def census_holds(kind, counts, masks, rays, cb):
    """The sentence of `kind` (see LENS_CLASSES) on a census; returns a string that says what failed, or None."""
    n = len(rays)
    if counts["bad_origin"] or counts["other"]:
        return "a non-finite origin or a direction that is neither ordinary, zero nor NaN: %r" % (counts,)
    pos = np.array(list(cb.position)[:3], F)
    centre = (rays[:, 0:3] == pos).all(axis=1)            # the draws whose lens offset is zero (r1 = 0), or was absorbed by pos
    if kind == "ordinary":
        ok = counts["ordinary"] == n
    elif kind == "zero":
        ok = counts["zero"] >= n - 16 and counts["nan"] == 0 and np.array_equal(masks["ordinary"], centre)
    elif kind == "zero_all":
        ok = counts["zero"] == n
    elif kind == "mixed":
        ok = counts["nan"] == 0 and counts["ordinary"] >= 64 and counts["zero"] >= 64 and len(mixed_runs(masks)) >= 1
    elif kind == "tiny_focus":
        ok = counts["zero"] == 0 and counts["ordinary"] >= n - 16 and 0 < counts["nan"] and np.array_equal(masks["nan"], centre)
    elif kind == "zero_nan":
        ok = counts["ordinary"] == 0 and counts["zero"] > 0 and counts["nan"] > 0
    elif kind == "nan":
        ok = counts["nan"] == n
    else:
        raise KeyError(kind)
    return None if ok else "%s does not hold: %r" % (kind, counts)


def env_frame(O, env, counts):
    """The frame of a renderer whose every finished sample was a miss with throughput 1: logic.hlsl:49-53 on the environment colour (saturate,
    x / (x + 1), pow 1 / 2.2 -- the oracle's pow), then the running mean of :73 replayed in binary32 for every pixel's sample count.
    counts: (H, W) uint32.  Returns (H, W, 3) float32."""
    e = np.clip(np.asarray(env, F), F(0.0), F(1.0))
    v = O.detmath(4, (e / (e + F(1.0))).astype(F), np.full(3, F(1.0) / F(2.2), F))
    out = np.zeros(counts.shape + (3,), F)
    for k in range(int(counts.max())):
        step = (((out * F(k)).astype(F) + v).astype(F) / F(k + 1)).astype(F)
        out = np.where((counts > k)[..., None], step, out)
    return out

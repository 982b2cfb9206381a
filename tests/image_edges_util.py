"""Crafted frames for the image stages (denoiser, temporal integration, motion plane) on non-finite and extreme pixels, and the rule that
compares device and host output on them (include/gmupt.h, "Non-finite and extreme input"; DESIGN.md "The image stages on non-finite and
extreme pixels").

A frame is a clean synthetic frame in which single VALID pixels are overwritten with one poison each, one poison per cell of a fixed
grid; its plan lists (y, x, class), so a failure can name the class.  Two layouts: ISOLATED (cells of 24 x 24, for passes <= 2, whose
reach 2 * (2^2 - 1) = 6 keeps the footprints apart) and DENSE (cells of 8 x 8, for passes 1..5, where they merge)."""
import numpy as np

from test_denoise_cpu import beauty_of, random_inputs, records, shifted

f32 = np.float32
W0, H0 = 96, 48
ISOLATED, DENSE = 24, 8
CUT_SHAPES = [(1, 1), (7, 3), (193, 5)]          # (W, H) of the existing synthetic tests: edges everywhere, the 64-pixel block border
PSETS = [{}, {"sigma_color": 1.5, "sigma_normal": 16.0, "sigma_plane": 0.5, "sigma_albedo": 0.8}]
NAN_A, NAN_B = 0x7FC00001, 0xFFC00000
FLT_MAX = np.finfo(f32).max


def word(bits):
    """The float32 with these bits (numpy scalar; assigning it into a float32 array keeps the bits)."""
    return np.array([bits], np.uint32).view(f32)[0]


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def is_nan_bits(u):
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


# ---------------------------------------------------------------------------------------------------- poison classes
def _rgb(ch, bits_):
    def put(b, a, y, x):
        b.view(np.uint32)[y, x, ch] = bits_
    return put


def _fw(v):
    return int(np.array([v], f32).view(np.uint32)[0])


def _normal(fn):
    def put(b, a, y, x):
        a[y, x, 4:7] = fn(a[y, x, 4:7].copy())
    return put


def _set(lo, hi, value):
    def put(b, a, y, x):
        a[y, x, lo:hi] = value
    return put


def _comp(i, value):
    def put(b, a, y, x):
        a[y, x, i] = value
    return put


def _count(bits_):
    def put(b, a, y, x):
        b.view(np.uint32)[y, x, 3] = bits_
    return put


def _nan_first(n):
    n[0] = np.nan
    return n


def _inf_first(n):
    n[0] = np.inf
    return n


def _inf_by_invalid(b, a, y, x):
    b[y, x, 0] = np.inf
    if x + 1 < b.shape[1]:
        a.view(np.uint32)[y, x + 1, 12] = 0xFFFFFFFF          # the right neighbour is a miss


# every infinity sits in the red channel: the poison of an infinite colour floods one channel of a small frame at five passes (reach 62),
# and at least half of the colour words must stay comparable on bits
CLASSES = {
    "rgb_pinf": _rgb(0, 0x7F800000), "rgb_ninf": _rgb(0, 0xFF800000), "rgb_nan_a": _rgb(2, NAN_A), "rgb_nan_b": _rgb(0, NAN_B),
    "rgb_3e38": _rgb(1, _fw(3e38)), "rgb_denormal": _rgb(2, _fw(1e-40)), "rgb_negative": _rgb(0, _fw(-0.25)), "rgb_negzero": _rgb(1, 0x80000000),
    "n_nan": _normal(_nan_first), "n_inf": _normal(_inf_first), "n_1e30": _normal(lambda n: n * f32(1e30)),
    "n_1em20": _normal(lambda n: n * f32(1e-20)), "n_1em30": _normal(lambda n: n * f32(1e-30)),
    "z_zero": _comp(3, 0.0), "z_neg": _comp(3, -1.0), "z_inf": _comp(3, np.inf), "z_nan": _comp(3, np.nan), "z_denormal": _comp(3, 1e-40),
    "z_fltmax": _comp(3, FLT_MAX),
    "x_nan": _comp(9, np.nan), "x_inf": _comp(8, np.inf), "x_1e38": _set(8, 11, 1e38),
    "a_nan": _comp(1, np.nan), "a_pinf": _comp(0, np.inf), "a_ninf": _comp(2, -np.inf),
    "cnt_snan": _count(0x7F800001), "cnt_qnan": _count(NAN_B), "cnt_signbit": _count(0x80000000), "cnt_ones": _count(0xFFFFFFFF),
    "pinf_by_invalid": _inf_by_invalid,
}
NAMES = list(CLASSES)
# classes whose outcome hangs on a binary32 overflow or underflow that float64 does not have: the float64 comparison leaves out the
# pixels within their reach; the exact expectations and device == host hold them
F32_ONLY = {"rgb_3e38": "l * l overflows binary32", "n_1e30": "dot3(n, n) overflows, n becomes 0", "n_1em20": "dot3(n, n) is a denormal with 16 bits",
            "n_1em30": "dot3(n, n) underflows to 0: the pixel is invalid", "x_1e38": "position differences overflow",
            "lambda_denormal": "d / lambda overflows"}


def make_valid(b, a, y, x):
    """Pixel (y, x) becomes a valid surface pixel whatever the clean frame had there; its colour, depth, position and albedo stay."""
    u, bu = a.view(np.uint32), b.view(np.uint32)
    if u[y, x, 12] == 0xFFFFFFFF:
        u[y, x, 12] = 7
    u[y, x, 14] = 0
    if bu[y, x, 3] == 0:
        bu[y, x, 3] = 2
    if not a[y, x, 4:7].any():
        a[y, x, 4:7] = (0.0, 0.0, 1.0)


def _axis(n, cell, edge):
    m = (n + cell - 1) // cell
    pos = [min(i * cell + cell // 2, n - 1) for i in range(m)]
    if edge:
        pos[-1] = n - 1
        pos[0] = 0
    return pos


def plan(W, H, cell, variant=0, edge=False):
    """[(y, x, class)]: one poison per cell, at the cell's centre (edge: the outer cells put theirs in the first / last row and column);
    `variant` rotates the class list, so that some number of variants puts every class somewhere.  The dense layout of a frame wider
    than a block adds poisons on both sides of the 64-pixel block border."""
    ys, xs = _axis(H, cell, edge), _axis(W, cell, edge)
    spots = [(y, x) for y in ys for x in xs]
    if cell == DENSE and W > 66:
        spots += [(H // 2, 63), (H // 2, 64)]
    return [(y, x, NAMES[(variant * len(spots) + k) % len(NAMES)]) for k, (y, x) in enumerate(spots)]


def variants_for(W, H, cell):
    spots = len(plan(W, H, cell))
    return min(-(-len(NAMES) // spots), 6)


def poison(beauty, aov, pl):
    b, a = beauty.copy(), aov.copy()
    for (y, x, name) in pl:
        make_valid(b, a, y, x)
    for (y, x, name) in pl:
        CLASSES[name](b, a, y, x)
    return b, a


def frame(W, H, cell, variant=0, edge=False, seed=None):
    """(beauty, aov, plan) of the crafted frame."""
    beauty, aov = random_inputs(W, H, 100 + variant if seed is None else seed)
    pl = plan(W, H, cell, variant, edge)
    b, a = poison(beauty, aov, pl)
    return b, a, pl


def denoise_cases():
    """Every (name, beauty, aov, plan, pass counts) the device denoiser is compared on: both layouts on the full frame (centre and edge
    placement, every class somewhere) and cut to the small shapes."""
    out = []
    for (W, H) in [(W0, H0)] + CUT_SHAPES:
        for cell, passes in ((ISOLATED, (1, 2)), (DENSE, (1, 2, 3, 4, 5))):
            for v in range(variants_for(W, H, cell)):
                for edge in ((False, True) if (W, H) == (W0, H0) or v == 0 else (bool(v & 1),)):
                    b, a, pl = frame(W, H, cell, v, edge)
                    out.append(("%dx%d/%s/v%d%s" % (W, H, "isolated" if cell == ISOLATED else "dense", v, "e" if edge else ""), b, a, pl, passes))
    return out


def denormal_plane(W=40, H=12):
    """A flat valid plane whose colours are all of order 1e-40: the output must consist of non-zero denormals."""
    rng = np.random.default_rng(77)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    rgb = (rng.uniform(0.5, 4.0, (H, W, 3)) * 1e-40).astype(f32)
    aov = records(np.full((H, W, 3), 0.5, f32), np.full((H, W), 3.0, f32), np.tile(f32([0, 0, 1]), (H, W, 1)),
                  np.stack([xs * 0.02, ys * 0.02, np.full_like(xs, 3.0)], -1), np.zeros((H, W), np.int32), np.zeros((H, W), np.uint32))
    return beauty_of(rgb, np.full((H, W), 3, np.uint32)), aov


def valid_mask32(beauty, aov):
    """The denoiser's validity test in binary32, as include/gmupt.h states it."""
    n = aov[..., 4:7]
    with np.errstate(all="ignore"):
        d = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        length = np.sqrt(d)
    u = aov.view(np.uint32)
    return (beauty[..., 3].view(np.uint32) > 0) & (u[..., 12] != 0xFFFFFFFF) & (u[..., 14] == 0) & (length > 0)


def dilate(valid, source, passes, first=0):
    """The pixels that have, after passes first .. passes-1, a chain of taps back to `source`: per pass the 5x5 pattern at step 1 << k,
    over valid pixels, skipping invalid and outside taps.  `source` is included."""
    m = source & valid
    for k in range(first, passes):
        s = 1 << k
        new = m.copy()
        for j in range(-2, 3):
            for i in range(-2, 3):
                q, inside = shifted(m, s * j, s * i)
                new |= q & inside
        m = new & valid
    return m


def reach(passes):
    return 2 * ((1 << passes) - 1)


def near(shape, pl, names, r):
    """Mask of the pixels within r (per axis) of a poison whose class is in `names`."""
    H, W = shape
    m = np.zeros((H, W), bool)
    for (y, x, name) in pl:
        if name in names:
            m[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return m


# ---------------------------------------------------------------------------------------------------- the comparison rule
def same_or_nan(got, exp, what, plan_=None, alpha=True):
    """Device against host, (..., 4) RGBA or any (..., k) float32 words.  Words are equal on bits, except that a word that is a NaN on
    the host matches any NaN on the device (the two give a GENERATED NaN different sign and payload bits).  The exception is fenced: the
    same words are NaN on both sides.  Infinities compare on bits, sign included.  With alpha, word 3 of every texel is opaque bits and
    always compares on bits, NaN patterns too.  Returns the mask of the words excused as NaN."""
    g, e = bits(got), bits(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    ng, ne = is_nan_bits(g), is_nan_bits(e)
    if alpha:
        ng[..., 3] = False; ne[..., 3] = False

    def where(bad):
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        near_ = ""
        if plan_ is not None and len(idx) >= 3:
            y, x = idx[-3], idx[-2]
            d, cls = min((max(abs(y - py), abs(x - px)), name) for (py, px, name) in plan_)
            near_ = ", nearest poison %s at distance %d" % (cls, d)
        return "%s: %d words, first %r: device %#x host %#x%s" % (what, int(bad.sum()), idx, g[idx], e[idx], near_)
    assert np.array_equal(ng, ne), "NaN on one side only, " + where(ng != ne)
    diff = (g != e) & ~ne
    assert not diff.any(), "differs, " + where(diff)
    return ne


def comparable_share(out, valid):
    """Share of the valid pixels' colour words that are not NaN, i.e. compared on bits by same_or_nan."""
    if not valid.any():
        return 1.0
    return float((~is_nan_bits(bits(out)[..., :3][valid])).mean())


# ---------------------------------------------------------------------------------------------------- temporal sequences
def crafted_camera(pkg, W, H, kind="plain"):
    """An axis-aligned camera at the origin looking down -z with exact power-of-two products: u = (X.x / -X.z + 1) / 2 * W,
    v = (0.5 - X.y / -X.z) * H for W, H powers of two.  kind: "plain", "zero_f" (F = U + Hv / 2 - V / 2 = 0) or "zero_ps" (pixelSize = 0)."""
    cam = pkg.capi.Camera(W, H)
    cam.set_pose(0.0, 0.0, 0.0, 0.0, 0.0)
    cam.update(0.0)
    buf = cam.buffer_copy()
    cam.close()

    def put(field, v):
        for i in range(3):
            field[i] = v[i]
    put(buf.position, (0.0, 0.0, 0.0)); put(buf.horizontal, (2.0, 0.0, 0.0)); put(buf.vertical, (0.0, 1.0, 0.0))
    put(buf.upperLeftCorner, (-1.0, 0.5, 0.0 if kind == "zero_f" else -1.0))
    buf.pixelSize[0], buf.pixelSize[1] = (0.0, 0.0) if kind == "zero_ps" else (1.0 / W, 1.0 / H)
    return buf


def plane_point(W, H, u, v):
    """The point of the plane z = -1 that the plain crafted camera projects to (u, v)."""
    return (2.0 * u / W - 1.0, 0.5 - v / H, -1.0)


PW, PH = 64, 32
# class -> the AOV position of the second call (None: the shifted plane point)
PROJECTION = {
    "lambda_zero": (0.0, 0.0, 0.0), "lambda_denormal": (1.0, 0.0, -1e-40), "lambda_nan": (0.5, np.nan, -1.0), "behind": (0.0, 0.0, 1.0),
    "u_p2e31": (2.0 ** 26, 0.0, -1.0), "u_m2e31": (-2.0 ** 26, 0.0, -1.0), "v_p2e31": (0.0, -2.0 ** 26, -1.0), "v_m2e31": (0.0, 2.0 ** 26, -1.0),
    "u_p1e30": (1e30, 0.0, -1.0), "u_m1e30": (-1e30, 0.0, -1.0), "v_p1e30": (0.0, -1e30, -1.0),
    "x_pinf": (np.inf, 0.0, -1.0), "x_ninf": (-np.inf, 0.0, -1.0), "z_ninf": (0.0, 0.0, -np.inf), "all_nan": (np.nan, np.nan, np.nan),
    "fu_m1": plane_point(PW, PH, -1.0, 5.0), "fu_m05": plane_point(PW, PH, -0.5, 5.25), "fu_wm1": plane_point(PW, PH, PW - 1.0, 7.0),
    "fu_wm05": plane_point(PW, PH, PW - 0.5, 7.5), "fu_w": plane_point(PW, PH, float(PW), 7.0), "fv_m1": plane_point(PW, PH, 9.0, -1.0),
    "fv_hm1": plane_point(PW, PH, 9.5, PH - 1.0), "fv_h": plane_point(PW, PH, 9.0, float(PH)), "fu_m1_fv_m1": plane_point(PW, PH, -1.0, -1.0),
    "corner": plane_point(PW, PH, PW - 1.0, PH - 1.0), "just_out": plane_point(PW, PH, -1.0 - 2.0 ** -18, 3.0),
}
# exact expectation of the plain camera: these give N_h = 0 (outside the guard, not in front, or NaN): the beauty texel, count = nf
NO_HISTORY = ("lambda_zero", "lambda_denormal", "lambda_nan", "behind", "u_p2e31", "u_m2e31", "v_p2e31", "v_m2e31", "u_p1e30", "u_m1e30",
              "v_p1e30", "x_pinf", "x_ninf", "z_ninf", "all_nan", "fu_w", "fv_h", "just_out")


def projection_sequence():
    """(first, second, plan) on the crafted plane z = -1, PW x PH: first = (beauty, aov) whose records become the history, second =
    (beauty, aov) seen 0.3 px right and 0.6 px down, with the PROJECTION positions in single pixels (plan: (y, x, class)) and the count
    words 0 and 0xFFFFFFFF in others."""
    rng = np.random.default_rng(5)
    H, W = PH, PW
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

    def aov_at(du, dv):
        pos = np.stack([2.0 * (xs + du) / W - 1.0, 0.5 - (ys + dv) / H, np.full_like(xs, -1.0)], -1)
        a = records(np.full((H, W, 3), 0.5, f32), np.full((H, W), 1.0, f32), np.tile(f32([0, 0, 1]), (H, W, 1)), pos,
                    np.arange(H * W, dtype=np.int32).reshape(H, W), np.zeros((H, W), np.uint32))
        a.view(np.uint32)[..., 13] = 3
        return a
    first = (beauty_of(rng.uniform(0.1, 0.9, (H, W, 3)).astype(f32), rng.integers(1, 5, (H, W)).astype(np.uint32)), aov_at(0.0, 0.0))
    b2 = beauty_of(rng.uniform(0.1, 0.9, (H, W, 3)).astype(f32), rng.integers(0, 4, (H, W)).astype(np.uint32))
    a2 = aov_at(0.3, 0.6)
    pl = []
    for k, (name, pos) in enumerate(PROJECTION.items()):
        y, x = 2 + 5 * (k // 10), 3 + 6 * (k % 10)
        a2[y, x, 8:11] = pos
        b2.view(np.uint32)[y, x, 3] = k % 3                      # with and without samples of its own
        pl.append((y, x, name))
    for k, w_ in enumerate((0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0x7F800001, 0x80000000)):
        y, x = 20 + 2 * (k // 3), 5 + 9 * (k % 3)
        b2.view(np.uint32)[y, x, 3] = w_
        pl.append((y, x, "n_%08x" % w_))
    return first, (b2, a2), pl


def motion_plane_for(aov, pl_seed=9):
    """gmupt_motion records for an AOV image: flags 1 with prev_position = the position nudged by a millimetre; single records with a NaN
    or infinite prev_position under flags 1, and flags 2 (not 1: the record is ignored)."""
    H, W = aov.shape[:2]
    rng = np.random.default_rng(pl_seed)
    m = np.zeros((H, W, 4), f32)
    m[..., :3] = aov[..., 8:11] + rng.normal(0, 1e-3, (H, W, 3)).astype(f32)
    mu = m.view(np.uint32)
    mu[..., 3] = 1
    pl = []
    kinds = [("mv_nan", (np.nan, 0.0, 0.0), 1), ("mv_pinf", (np.inf, 0.0, 0.0), 1), ("mv_ninf", (0.0, -np.inf, 0.0), 1), ("mv_all_nan", (np.nan,) * 3, 1),
             ("mv_flags2", None, 2), ("mv_flags2_nan", (np.nan,) * 3, 2), ("mv_flags0", None, 0)]
    for k in range(min(4 * len(kinds), (H * W) // 7)):
        name, pos, flags = kinds[k % len(kinds)]
        y, x = (7 * k + 3) // W % H, (7 * k + 3) % W
        y = (y * 5 + k) % H
        if pos is not None:
            m[y, x, :3] = pos
        mu[y, x, 3] = flags
        pl.append((y, x, name))
    return m, pl


# ---------------------------------------------------------------------------------------------------- the host chain and its cases
SPATIAL = ("passes", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo")


class Chain:
    """The temporal handle's semantics on the host (HostChain of test_temporal_gpu), with an optional motion plane and an optional infill
    between the integration and the filter."""

    def __init__(self, capi):
        self.capi, self.frozen, self.last, self.integrated = capi, None, None, None

    def call(self, beauty, aov, cam, origin, new_accumulation, motion=None, infill=None, **params):
        if new_accumulation:
            self.frozen, self.last = self.last, self.frozen
        prev = self.frozen or (None, None, (0, 0))
        integrated, hist = self.capi.temporal_integrate_motion_host(beauty, aov, motion, *prev, **params)
        self.last = (hist, cam, origin)
        self.integrated = integrated
        if infill is not None:
            integrated = self.capi.infill_host(integrated, aov, **infill)[0]
        return self.capi.denoise_host(integrated, aov, **{k: v for k, v in params.items() if k in SPATIAL})


def room_sequence(pkg):
    """The poisoned first call (dense layout, every class) and a second call from a moved pose with poisons of its own."""
    from test_temporal_cpu import BASE, camera, noisy_beauty, room_aov
    W, H = W0, H0
    cam0, cam1 = camera(pkg, W, H, BASE), camera(pkg, W, H, (0.6, 1.5, 1.0, -5.0, 198.0))
    pl0 = plan(W, H, DENSE, 0, True)
    b0, a0 = poison(noisy_beauty(W, H, 31, zero_frac=0.1), room_aov(cam0, W, H, seed=30), pl0)
    pl1 = plan(W, H, DENSE, 1, False)
    b1, a1 = poison(noisy_beauty(W, H, 33), room_aov(cam1, W, H, seed=32), pl1)
    for k, w_ in enumerate((0, 0xFFFFFFFF, 0, 0xFFFFFFFF)):
        b1.view(np.uint32)[9 + 8 * k, 7 + 16 * k, 3] = w_
    return (b0, a0, cam0, pl0), (b1, a1, cam1, pl1)


def temporal_cases(pkg):
    """[(name, calls)] of every sequence the device handle is compared on; a call is (beauty, aov, camera, origin, new_accumulation,
    keywords).  The filter runs two passes (reach 6) on the poisoned room: a history of infinite colours floods a 96 x 48 frame at five."""
    (b0, a0, cam0, pl0), (b1, a1, cam1, pl1) = room_sequence(pkg)
    mv, _ = motion_plane_for(a1)
    first = (b0, a0, cam0, (0, 0), 1, {"passes": 2})
    out = [("fold", [first, (b1, a1, cam1, (0, 0), 1, {"passes": 2})]),
           ("no fold, then fold", [first, (b1, a1, cam1, (0, 0), 0, {"passes": 1}), (b1, a1, cam1, (0, 0), 1, {"history_cap": 65536.0, "passes": 2})]),
           ("cap 0", [first, (b1, a1, cam1, (0, 0), 1, {"history_cap": 0.0, "passes": 3})]),
           ("motion", [first, (b1, a1, cam1, (0, 0), 1, {"motion": mv, "passes": 2})]),
           ("infill", [first, (b1, a1, cam1, (0, 0), 1, {"infill": {}, "passes": 2})])]
    x0, y0, w, h = 13, 9, 50, 30               # a sub-rectangle of the second frame, with its origin, against the whole first frame
    sub = (np.ascontiguousarray(b1[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(a1[y0:y0 + h, x0:x0 + w]))
    out.append(("sub-rectangle", [first, (sub[0], sub[1], cam1, (x0, y0), 1, {"passes": 2}), (b1, a1, cam1, (0, 0), 1, {"passes": 1})]))
    p1, p2, _ = projection_sequence()
    for kind in ("plain", "zero_f", "zero_ps"):
        cam = crafted_camera(pkg, PW, PH, kind)
        for origin in ((0, 0), (5, 3)):                            # the first call's origin shifts every projection
            out.append(("projection/%s/%d" % (kind, origin[0]), [(p1[0], p1[1], cam, origin, 1, {}), (p2[0], p2[1], cam, (0, 0), 1, {"passes": 2})]))
    # colours of order 1e-40 in the history and in the frame: the blend's products and sums are denormals, a flush would zero them
    tiny = lambda b: np.concatenate([(b[..., :3].astype(np.float64) * 1e-40).astype(f32), b[..., 3:]], -1)
    cam = crafted_camera(pkg, PW, PH)
    out.append(("denormal history", [(tiny(p1[0]), p1[1], cam, (0, 0), 1, {"passes": 1}), (tiny(p2[0]), p2[1], cam, (0, 0), 1, {"passes": 1})]))
    return out


def surface_mask32(aov):
    """The integration's surface test in binary32: the denoiser's validity test without the sample count."""
    return valid_mask32(np.ones(aov.shape[:2] + (4,), f32), aov)

"""CPU tests of the image stages on non-finite and extreme pixels (include/gmupt.h, "Non-finite and extreme input"): the host filter
gmupt_denoise_host and the host integration gmupt_temporal_integrate_host on the crafted frames of image_edges_util, against the float64
restatements of test_denoise_cpu / test_temporal_cpu and against exact expectations derived from the stated rule; the share of words
that same_or_nan compares on bits, for every frame tests/test_image_edges_gpu.py compares; thread-count independence.

Every bit-level read of a float in the four shared headers, and why a GENERATED NaN (whose sign and payload differ between x86 and
gfx950) or an out-of-range value cannot reach it:

  pt_denoise.hpp   dn_prepare: f2u(beauty.w), and gd_prepare (pt_guides.hpp, which it calls): f2u(a3.x), f2u(a3.z) -- the sample count,
                   triangle and light words.  Caller words, read as
                   integers and never the result of arithmetic: a NaN pattern in them is an input, the same bits on both sides
                   (cnt_* classes; test_count_words_come_through_on_bits).
  pt_temporal.hpp  tp_pixel_t: f2u(a3.x / a3.y / a3.z), f2u(m.w), f2u(b.w) -- caller words as above (mv_flags*, n_* classes).
                   f2u(q2.w), f2u(q1.w) -- the valid and material words of a history record: written by u2f(integer), never by arithmetic.
                   (int)fu, (int)fv -- behind the guard -1 <= fu <= W - 1 (and fv), which is false for NaN and +-inf, so the conversion sees
                   integers of the previous rectangle only (PROJECTION classes; test_projection_edges_take_no_history).
                   (uint32_t)ceilf(N_h) -- N_h = hmin(cap, Sn / Sw): hmin drops a NaN second operand and cap is finite, in [0, 65536];
                   Sn / Sw is not negative (counted taps have count > 0 and weights >= 0), so N_h is in [0, 65536] and, where this is
                   evaluated, not 0 (test_crafted_history_records: count +inf, NaN, denormal, negative).
                   (float)n, n + (uint32_t)..: integer arithmetic on a caller word; wraps modulo 2^32 for n = 0xFFFFFFFF on both sides.
  pt_motion.hpp    none (u2f(1u) only).  pt_motion.hip reads f2u(h0.w), f2u(h1.x): the hit's triangle and light words, integers.
  detmath.hpp      dlog2: f2u(x), exponent and mantissa bits -- reached through dpow alone, which returns 0 for x <= 0; in gd_wn (pt_guides.hpp) x is
                   hmax(0, dot3(n_p, n_q)), and hmax drops a NaN second operand, so x is 0 (no dlog2) or positive and finite (a
                   normalised normal has finite components, 0 or NaN) -- n_inf class; test_an_infinite_normal_is_invisible_to_its_neighbours.
                   dexp2: (int)n -- behind !(y > -150) and y > 128, both of which catch NaN and +-inf, so n is in -150 .. 128
                   (z_neg: large positive exponents, z_denormal / z_zero: -inf, a_pinf: -inf, z_nan / x_nan: NaN).
                   u2f((n + 127) << 23): n1, n2 in -75 .. 64, so the biased exponents are 52 .. 191."""
import numpy as np
import pytest

import image_edges_util as E
from test_denoise_cpu import TOL, reference as dn_reference
from test_temporal_cpu import BASE, camera, noisy_beauty, reference as tp_reference, room_aov, room_history

f32 = np.float32
# |host - float64| on the finite words of the crafted frames outside the reach of the F32_ONLY classes, relative to max(1, |ref|):
# measured at most 3.3e-6 over every frame, pass count and parameter set below -- within the clean frames' TOL = 2e-5 (measured
# 2.8e-6 there), so the crafted frames keep TOL.  DESIGN.md records the figure.
EDGE_TOL = TOL
# The same for the host integration (poisoned room, crafted history records) on the pixels the float64 comparison keeps: measured at
# most 2.76e-5 (the poisoned room at the default cap and at 65536; 4.3e-6 on the crafted records); four times that.  The binary32 projection is a few ulps of (u, v) off the exact one, which moves the bilinear mean
# of the taps; the per-word bound of test_temporal_cpu (8 ulps + 1e-4 * the taps' spread) is asserted as well.
INTEGRATION_TOL = 1.1e-4
CAP = 0.5     # at least this share of the valid pixels' colour words is not NaN, i.e. compared on bits by same_or_nan


@pytest.fixture(scope="module")
def cases():
    return E.denoise_cases()


@pytest.fixture(scope="module")
def host(pkg, cases):
    """{(case name, passes, parameter set): host output} of every comparison the GPU file makes."""
    out = {}
    for (name, b, a, pl, passes) in cases:
        for pi, params in enumerate(E.PSETS):
            for p in passes:
                out[(name, p, pi)] = pkg.capi.denoise_host(b, a, threads=4, passes=p, **params)
    return out


def word_class(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


# ---------------------------------------------------------------------------------------------------- the cap
def test_at_least_half_of_the_colour_words_compare_on_bits(pkg, cases, host):
    assert len(cases) > 20
    seen = set()
    worst = 1.0
    for (name, b, a, pl, passes) in cases:
        valid = E.valid_mask32(b, a)
        seen |= {c for (_, _, c) in pl}
        for pi in range(len(E.PSETS)):
            for p in passes:
                share = E.comparable_share(host[(name, p, pi)], valid)
                worst = min(worst, share)
                assert share >= CAP, (name, p, pi, share)
    assert seen == set(E.NAMES), "every class sits in some frame"
    print("smallest share of colour words compared on bits: %.3f" % worst)
    b, a = E.denormal_plane()
    assert E.comparable_share(pkg.capi.denoise_host(b, a), E.valid_mask32(b, a)) == 1.0


def test_the_temporal_sequences_keep_half_of_their_colour_words_too(pkg):
    used = {}
    for (name, calls) in E.temporal_cases(pkg):
        chain = E.Chain(pkg.capi)
        for k, (b, a, cam, origin, new, kw) in enumerate(calls):
            out = chain.call(b, a, cam, origin, new, **kw)
            share = E.comparable_share(out, E.valid_mask32(chain.integrated, a))
            assert share >= CAP, (name, k, share)
            used[name] = int((E.bits(chain.integrated)[..., 3] != E.bits(b)[..., 3]).sum())
        if name == "denormal history":                        # the last call's blend of denormal history and denormal beauty: no zero, no normal
            took = E.bits(chain.integrated)[..., 3] != E.bits(b)[..., 3]
            w = E.bits(chain.integrated)[..., :3][took]
            assert took.sum() > 1000 and (w != 0).all() and (w < 0x00800000).all()
            assert (E.bits(out)[..., :3][took] != 0).all()
    # F = 0 gives lambda = 0 / 0, pixelSize = 0 gives u = x / 0: neither is ever inside the guard
    assert all((n > 0) == (name != "cap 0" and "zero_" not in name) for name, n in used.items()), used


def test_same_or_nan_is_fenced():
    a = np.zeros((2, 3, 4), f32)
    a[0, 0, 0] = np.nan; a[0, 1, 1] = np.inf; a.view(np.uint32)[1, 1, 3] = 0x7F800001
    b = a.copy()
    b.view(np.uint32)[0, 0, 0] = E.NAN_B                       # another NaN: accepted
    assert E.same_or_nan(b, a, "ok").sum() == 1
    for (idx, bits_) in [((0, 1, 1), 0xFF800000), ((0, 2, 2), E.NAN_A), ((0, 0, 0), 0x7F800000), ((1, 1, 3), 0x7FC00001), ((1, 2, 0), 0x80000000)]:
        c = b.copy()
        c.view(np.uint32)[idx] = bits_                         # inf sign, a NaN on one side only (either side), alpha NaN bits, zero sign
        with pytest.raises(AssertionError):
            E.same_or_nan(c, a, "bad")
        if idx != (1, 1, 3):
            with pytest.raises(AssertionError):
                E.same_or_nan(a, c, "bad")


# ---------------------------------------------------------------------------------------------------- float64
def test_host_filter_matches_the_float64_restatement_on_crafted_frames(pkg, cases, host):
    worst = 0.0
    for (name, b, a, pl, passes) in cases:
        for pi, params in enumerate(E.PSETS):
            for p in passes:
                got = host[(name, p, pi)]
                ref, valid = dn_reference(b, a, passes=p, **params)
                keep = ~E.near(b.shape[:2], pl, E.F32_ONLY, E.reach(p))
                g, r = got[..., :3][keep].astype(np.float64), ref[..., :3][keep]
                cg, cr = word_class(g), word_class(r)
                assert np.array_equal(cg, cr), (name, p, pi, "word classes differ in %d words" % int((cg != cr).sum()))
                fin = cg == 0
                err = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
                if err.size:
                    worst = max(worst, float(err.max()))
                    assert err.max() <= EDGE_TOL, (name, p, pi, float(err.max()))
    print("largest |host - float64| / max(1, |ref|) on the crafted frames: %.3g" % worst)


# ---------------------------------------------------------------------------------------------------- exact expectations
def isolated_frames():
    for v in range(E.variants_for(E.W0, E.H0, E.ISOLATED)):
        for edge in (False, True):
            yield E.frame(E.W0, E.H0, E.ISOLATED, v, edge)


def cell_of(shape, y, x, r):
    H, W = shape
    return (slice(max(0, y - r), min(H, y + r + 1)), slice(max(0, x - r), min(W, x + r + 1)))


def test_an_infinite_colour_poisons_exactly_its_reach_in_its_channel(pkg):
    """After P passes the NaN mask of a +-inf channel is valid & ~source & dilate(source): every valid pixel with a chain of taps back to
    the source (d_l = inf, E = 0, w = 0, C += 0 * inf).  The source keeps its texel: its centre tap has d_l = NaN, so W is NaN."""
    found = 0
    for (b, a, pl) in isolated_frames():
        valid = E.valid_mask32(b, a)
        for p in (1, 2):
            for params in E.PSETS:
                out = pkg.capi.denoise_host(b, a, passes=p, **params)
                for (y, x, name) in pl:
                    if name not in ("rgb_pinf", "rgb_ninf", "pinf_by_invalid"):
                        continue
                    found += 1
                    src = np.zeros(valid.shape, bool); src[y, x] = True
                    want = valid & ~src & E.dilate(valid, src, p)
                    win = cell_of(valid.shape, y, x, E.ISOLATED // 2 - 1)
                    nan = np.isnan(out[..., :3])
                    assert np.array_equal(nan[..., 0][win], want[win]), (name, y, x, p)
                    assert not nan[..., 1:][win].any(), (name, "NaN in that channel only")
                    assert np.array_equal(E.bits(out)[y, x], E.bits(b)[y, x]), (name, "the source keeps its texel")
                    assert want[win].sum() >= min(3, valid[win].sum() - 1)
    assert found >= 12


def test_a_nan_colour_poisons_nobody(pkg):
    """A pixel that taps a NaN colour has d_l = NaN, so W is NaN and not > 0: it keeps the previous pass's colour.  After one pass the
    valid pixels of the 5x5 around the source hold their beauty bits; after two, those at even offsets up to 2 do (tapped in both
    passes), and the other valid pixels at step-2 offsets hold their one-pass colour."""
    found = 0
    for (b, a, pl) in isolated_frames():
        valid = E.valid_mask32(b, a)
        one = pkg.capi.denoise_host(b, a, passes=1)
        two = pkg.capi.denoise_host(b, a, passes=2)
        H, W = valid.shape
        for (y, x, name) in pl:
            if name not in ("rgb_nan_a", "rgb_nan_b"):
                continue
            found += 1
            for dy in range(-4, 5):
                for dx in range(-4, 5):
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < H and 0 <= qx < W) or not valid[qy, qx]:
                        continue
                    if max(abs(dy), abs(dx)) <= 2:
                        assert np.array_equal(E.bits(one)[qy, qx], E.bits(b)[qy, qx]), (name, dy, dx, "pass 0 keeps it")
                    if dy % 2 == 0 and dx % 2 == 0:
                        keeps = b if max(abs(dy), abs(dx)) <= 2 else one
                        assert np.array_equal(E.bits(two)[qy, qx, :3], E.bits(keeps)[qy, qx, :3]), (name, dy, dx, "pass 1 keeps it")
            win = cell_of(valid.shape, y, x, E.ISOLATED // 2 - 1)
            lone = np.isnan(two[..., :3][win]).sum()
            assert lone == 1, (name, "the only NaN word of the cell is the source's")
    assert found >= 4


def test_an_infinite_normal_is_invisible_to_its_neighbours(pkg):
    """n_inf: normalize3 gives (NaN, 0, 0); hmax(0, NaN) = 0 in front of dpow makes every weight with it 0 (for its neighbours) or NaN
    (its own, through d_x): the neighbours stay finite and the pixel keeps its colour.  n_nan and n_1em30 are invalid pixels, copied
    through; n_1e30 gives n = 0 and all weights 0: it keeps its colour."""
    found = set()
    for (b, a, pl) in isolated_frames():
        valid = E.valid_mask32(b, a)
        for p in (1, 2):
            out = pkg.capi.denoise_host(b, a, passes=p)
            for (y, x, name) in pl:
                if name not in ("n_inf", "n_nan", "n_1e30", "n_1em30"):
                    continue
                found.add(name)
                assert valid[y, x] == (name in ("n_inf", "n_1e30")), name
                assert np.array_equal(E.bits(out)[y, x], E.bits(b)[y, x]), (name, "keeps its texel")
                win = cell_of(valid.shape, y, x, E.ISOLATED // 2 - 1)
                assert np.isfinite(out[..., :3][win]).all(), (name, "no NaN or inf reaches a neighbour")
    assert found == {"n_inf", "n_nan", "n_1e30", "n_1em30"}


def test_count_words_come_through_on_bits(pkg, cases, host):
    for (name, b, a, pl, passes) in cases:
        for p in passes:
            assert np.array_equal(E.bits(host[(name, p, 0)])[..., 3], E.bits(b)[..., 3]), (name, p)
        inv = ~E.valid_mask32(b, a)
        assert np.array_equal(E.bits(host[(name, passes[-1], 1)])[inv], E.bits(b)[inv]), (name, "invalid pixels are copied")
    words = {int(E.bits(b)[y, x, 3]) for (_, b, a, pl, _) in cases for (y, x, c) in pl if c.startswith("cnt_")}
    assert words == {0x7F800001, 0xFFC00000, 0x80000000, 0xFFFFFFFF}


def test_the_denormal_plane_stays_denormal(pkg):
    b, a = E.denormal_plane()
    tiny = np.finfo(f32).tiny
    for p in (1, 3, 5):
        out = pkg.capi.denoise_host(b, a, passes=p)
        rgb = out[..., :3]
        assert (rgb > 0).all() and (rgb < tiny).all(), "non-zero denormals everywhere"
        assert not np.array_equal(E.bits(out)[..., :3], E.bits(b)[..., :3])
        ref, _ = dn_reference(b, a, passes=p)
        assert np.abs(rgb - ref[..., :3]).max() <= 4 * 1.4e-45 * p + 1e-5 * 4e-40      # a few denormal ulps per pass


def test_thread_count_does_not_change_a_bit_on_the_dense_frame(pkg):
    b, a, pl = E.frame(E.W0, E.H0, E.DENSE, 0, True)
    one = pkg.capi.denoise_host(b, a, threads=1)
    for t in (3, 16):
        assert np.array_equal(E.bits(pkg.capi.denoise_host(b, a, threads=t)), E.bits(one)), t


# ---------------------------------------------------------------------------------------------------- temporal integration
def integrate(pkg, second, first, cam, **params):
    _, hist = pkg.capi.temporal_integrate_host(first[0], first[1], **params)
    return pkg.capi.temporal_integrate_host(second[0], second[1], hist, cam, **params) + (hist,)


def test_projection_edges_take_no_history(pkg):
    """A projection outside the guard, a NaN lambda and lambda = 0 give N_h = 0: the integrated texel is the beauty texel on bits and the
    record has count = nf.  The projections at fu = -1 and W - 1 (fv likewise) take the one column inside."""
    first, second, pl = E.projection_sequence()
    cam = E.crafted_camera(pkg, E.PW, E.PH)
    got, hist, prev = integrate(pkg, second, first, cam)
    b2 = second[0]
    nb = E.bits(b2)[..., 3]
    took = E.bits(got)[..., 3] != nb
    assert took.mean() > 0.8, "the shifted plane reprojects onto the history"
    cls = {name: (y, x) for (y, x, name) in pl}
    for name in E.NO_HISTORY:
        y, x = cls[name]
        assert np.array_equal(E.bits(got)[y, x], E.bits(b2)[y, x]), name
        assert hist["count"][y, x] == f32(nb[y, x]) and hist["valid"][y, x] == (1 if nb[y, x] else 0), name
    for name in ("fu_m05", "fu_wm1", "fu_wm05", "fv_hm1", "corner"):
        y, x = cls[name]
        assert took[y, x], (name, "the taps inside the rectangle count")
    for name in ("fu_m1", "fv_m1", "fu_m1_fv_m1"):                # fx = 0 (fy = 0): the whole weight lies on the column (row) outside, Sw = 0
        y, x = cls[name]
        assert np.array_equal(E.bits(got)[y, x], E.bits(b2)[y, x]), (name, "inside the guard, but the inside taps weigh 0")
    y, x = cls["n_00000000"]                                     # n = 0: count = N_h, alpha = ceilf(N_h), rgb = Hc
    assert took[y, x] and int(E.bits(got)[y, x, 3]) == int(np.ceil(hist["count"][y, x])) and 0 < hist["count"][y, x] <= 32
    y, x = cls["n_ffffffff"]                                     # nf = 2^32 absorbs N_h <= 32; n + ceilf(N_h) wraps modulo 2^32
    assert took[y, x] and hist["count"][y, x] == f32(2.0 ** 32) and 0 <= int(E.bits(got)[y, x, 3]) < 32
    # history_cap = 0: nothing is taken anywhere; 65536: the cap never binds here
    g0, h0, _ = integrate(pkg, second, first, cam, history_cap=0.0)
    assert np.array_equal(E.bits(g0), E.bits(b2))
    g1, h1, _ = integrate(pkg, second, first, cam, history_cap=65536.0)
    assert np.array_equal(E.bits(g1), E.bits(got))


@pytest.mark.parametrize("kind", ["zero_f", "zero_ps"])
def test_degenerate_previous_cameras(pkg, kind):
    """dot3(F, F) = 0 makes lambda +-inf or NaN, pixelSize = 0 makes u and v +-inf or NaN: whatever the rule gives, every thread count
    gives it, and pixels whose projection is not finite take no history."""
    first, second, pl = E.projection_sequence()
    cam = E.crafted_camera(pkg, E.PW, E.PH, kind)
    got, hist, prev = integrate(pkg, second, first, cam)
    for t in (1, 3):
        g, h = pkg.capi.temporal_integrate_host(second[0], second[1], prev, cam, threads=t)
        assert np.array_equal(E.bits(g), E.bits(got)) and np.array_equal(h.view(np.uint32), hist.view(np.uint32))
    if kind == "zero_ps":
        assert np.array_equal(E.bits(got), E.bits(second[0])), "u = x / 0 is never inside the guard"
    with np.errstate(all="ignore"):
        rgb, alpha, count, surface, amb, spread = tp_reference(second[0], second[1], prev, cam, (0, 0))
    ok = ~amb & ~E.near(got.shape[:2], pl, E.F32_ONLY, 0)
    assert np.array_equal(word_class(got[..., :3])[ok], word_class(rgb)[ok])
    assert np.array_equal(E.bits(got)[..., 3][ok], alpha[ok])


def integration_against_float64(got, hist, ref, ok, what):
    """The host integration against the float64 restatement on the pixels `ok`: the word classes first, then the finite colour words
    and the record's count to the per-word bound of test_temporal_cpu.check_against_reference (8 ulps of the result plus what 1e-4 px of
    projection error moves the bilinear means by), the alpha bits exactly, and the colour words to INTEGRATION_TOL.  Returns the
    largest colour error relative to max(1, |ref|)."""
    rgb, alpha, count, surface, amb, spread = ref
    ulps = lambda x: np.spacing(np.abs(x).astype(f32)).astype(np.float64)
    g, r = got[..., :3][ok].astype(np.float64), rgb[ok]
    cg, cr = word_class(g), word_class(r)
    assert np.array_equal(cg, cr), (what, "word classes differ in %d words" % int((cg != cr).sum()))
    fin = cg == 0
    assert fin.sum() > 1000, what
    with np.errstate(all="ignore"):
        bound = (8 * ulps(rgb) + 1e-4 * (spread[..., :3] + spread[..., 3:]))[ok]
        err = np.abs(g - r)
        assert np.all(err[fin] <= bound[fin]), (what, float((err[fin] / bound[fin]).max()))
        cb = (8 * ulps(count) + 1e-4 * spread[..., 3])[ok]
        cerr = np.abs(hist["count"][ok].astype(np.float64) - count[ok])
    assert np.all(cerr <= cb), (what, "count", float(cerr.max()))
    assert np.array_equal(E.bits(got)[..., 3][ok], alpha[ok]), (what, "alpha")
    rel = float((err[fin] / np.maximum(1.0, np.abs(r[fin]))).max())
    assert rel <= INTEGRATION_TOL, (what, rel)
    return rel


def test_integration_of_the_poisoned_room_matches_float64(pkg):
    (b0, a0, cam0, pl0), (b1, a1, cam1, pl1) = E.room_sequence(pkg)
    _, hist0 = pkg.capi.temporal_integrate_host(b0, a0)
    for params in ({}, {"history_cap": 65536.0}, {"history_cap": 0.0}):
        got, hist = pkg.capi.temporal_integrate_host(b1, a1, hist0, cam0, **params)
        with np.errstate(all="ignore"):
            rgb, alpha, count, surface, amb, spread = tp_reference(b1, a1, hist0, cam0, (0, 0), **params)
        assert amb.mean() < 0.25          # the first call's counts are whole numbers, so many bilinear means of them sit on ceilf's step
        # the bound scales with the taps' spread (test_temporal_cpu): pixels whose taps hold a huge count word or colour are left to the
        # class comparison of the crafted-record test and to device == host
        fin_spread = np.where(np.isfinite(spread), spread, np.inf)
        ok = ~amb & ~E.near(got.shape[:2], pl1, E.F32_ONLY, 0) & (fin_spread[..., :3].max(-1) + fin_spread[..., 3] < 50.0)
        assert ok.mean() > 0.6
        worst = integration_against_float64(got, hist, (rgb, alpha, count, surface, amb, spread), ok, ("room", params))
        print("poisoned room %r: largest |host - float64| / max(1, |ref|) = %.3g on %d pixels" % (params, worst, int(ok.sum())))
        if params.get("history_cap") == 0.0:
            assert np.array_equal(E.bits(got), E.bits(b1))
        else:
            assert (E.bits(got)[..., 3] != E.bits(b1)[..., 3]).mean() > 0.3, "the second call uses the poisoned history"
            assert np.isnan(got[..., :3]).any() and np.isinf(got[..., :3]).any(), "non-finite history colours arrive"
        surf32 = E.surface_mask32(a1)
        assert np.array_equal(E.bits(got)[~surf32], E.bits(b1)[~surf32]), "other pixels: the beauty texel"
        assert not hist.view(np.uint32).reshape(hist.shape + (12,))[~surf32].any()
        runs = [pkg.capi.temporal_integrate_host(b1, a1, hist0, cam0, threads=t, **params) for t in (1, 3, 16)]
        for g, h in runs:
            assert np.array_equal(E.bits(g), E.bits(got)) and np.array_equal(h.view(np.uint32), hist.view(np.uint32))


def test_crafted_history_records(pkg):
    """Records only the host entry can be given: count +inf, NaN, denormal, negative; valid == 2; non-finite colour, normal, position.
    Counted taps need valid == 1 and count > 0 (false for NaN and negative), so N_h stays in (0, cap] and ceilf(N_h) in range."""
    W, H = 64, 36
    cam = camera(pkg, W, H, BASE)
    aov = room_aov(cam, W, H, seed=7, specials=False)
    beauty = noisy_beauty(W, H, 8, zero_frac=0.5)
    clean = room_history(cam, W, H, seed=9, defects=False)
    kinds = {"count_inf": ("count", np.inf), "count_nan": ("count", np.nan), "count_denormal": ("count", 1e-40), "count_negative": ("count", -3.0),
             "valid_2": ("valid", 2), "color_inf": ("color", (np.inf, 0.5, 0.5)), "color_nan": ("color", (0.5, np.nan, 0.5)),
             "normal_nan": ("normal", (np.nan, 0.0, 1.0)), "normal_inf": ("normal", (np.inf, 0.0, 0.0)),
             "position_nan": ("position", (np.nan, 0.0, 0.0)), "position_inf": ("position", (np.inf, np.inf, -np.inf))}
    h = clean.copy()
    where = {}
    for k, (name, (field, value)) in enumerate(kinds.items()):
        y, x = 4 + 9 * (k // 4), 6 + 14 * (k % 4)
        h[field][y, x] = value
        where[name] = (y, x)
    base, _ = pkg.capi.temporal_integrate_host(beauty, aov, clean, cam)
    got, hist = pkg.capi.temporal_integrate_host(beauty, aov, h, cam)
    changed = (E.bits(got) != E.bits(base)).any(-1)
    for name, (y, x) in where.items():
        assert changed[max(0, y - 1):y + 2, max(0, x - 1):x + 2].any(), (name, "the record is tapped")
    far = np.ones(changed.shape, bool)
    for (y, x) in where.values():
        far[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = False
    assert not changed[far].any(), "a record reaches only the pixels that tap it"
    alpha = E.bits(got)[..., 3].astype(np.int64) - E.bits(beauty)[..., 3]
    assert alpha.min() >= 0 and alpha.max() <= 32, "ceilf(N_h) stays within the cap"
    assert np.isinf(got[..., 0]).any() and np.isnan(got[..., 1]).any()
    # rejected records leave their share to the other taps: the result stays finite around them
    for name in ("count_nan", "count_negative", "valid_2", "normal_nan", "normal_inf", "position_nan", "position_inf"):
        y, x = where[name]
        assert np.isfinite(got[y - 1:y + 2, x - 1:x + 2, :3]).all(), name
    # the same records seen from a moved camera (from the same one every projection sits on a cell boundary), against float64
    cur = camera(pkg, W, H, (0.6, 1.5, 1.0, -5.0, 198.0))
    aov = room_aov(cur, W, H, seed=7, specials=False)
    got, hist = pkg.capi.temporal_integrate_host(beauty, aov, h, cam)
    with np.errstate(all="ignore"):
        rgb, alpha64, count, surface, amb, spread = tp_reference(beauty, aov, h, cam, (0, 0))
    fin_spread = np.where(np.isfinite(spread), spread, np.inf)
    ok = ~amb & (fin_spread[..., :3].max(-1) + fin_spread[..., 3] < 50.0)
    assert ok.mean() > 0.8
    worst = integration_against_float64(got, hist, (rgb, alpha64, count, surface, amb, spread), ok, "crafted records")
    print("crafted records: largest |host - float64| / max(1, |ref|) = %.3g" % worst)
    # where a counted tap holds a non-finite colour the spread is not finite: the word classes still agree
    wild = ~amb & ~ok
    assert wild.sum() >= 2 and np.array_equal(word_class(got[..., :3])[wild], word_class(rgb)[wild])
    assert np.isinf(got[..., 0]).any() and np.isnan(got[..., 1]).any()
    for t in (1, 3, 16):
        g, hh = pkg.capi.temporal_integrate_host(beauty, aov, h, cam, threads=t)
        assert np.array_equal(E.bits(g), E.bits(got)) and np.array_equal(hh.view(np.uint32), hist.view(np.uint32))


def test_motion_records_move_or_are_ignored(pkg):
    """flags == 1 with a non-finite prev_position: the projection is NaN or outside, no history; flags == 2 and 0: the record is ignored."""
    (b0, a0, cam0, pl0), (b1, a1, cam1, pl1) = E.room_sequence(pkg)
    _, hist0 = pkg.capi.temporal_integrate_host(b0, a0)
    mv, plm = E.motion_plane_for(a1)
    plain, _ = pkg.capi.temporal_integrate_host(b1, a1, hist0, cam0)
    got, _ = pkg.capi.temporal_integrate_motion_host(b1, a1, mv, hist0, cam0)
    kinds = set()
    surf = E.surface_mask32(a1)
    for (y, x, name) in plm:
        if not surf[y, x]:
            continue
        kinds.add(name)
        if name in ("mv_flags2", "mv_flags2_nan", "mv_flags0"):
            assert np.array_equal(E.bits(got)[y, x], E.bits(plain)[y, x]), name
        else:
            assert np.array_equal(E.bits(got)[y, x], E.bits(b1)[y, x]), (name, "no history")
    assert len(kinds) == 7
    assert (E.bits(got) != E.bits(plain)).any(-1).mean() > 0.2, "the nudged records move the taps elsewhere"

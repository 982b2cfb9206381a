"""What the convergence tests share: the numpy restatement of the rule of include/gmupt.h ("Convergence"), written from the header and
independent of csrc/pt_converge.hpp; the crafted frame sequences; the wide-range sequences on which the order of the sum and the
seams of the reduction show, with the orders that are not the rule's; and the bit-for-bit comparison with the NaN fence."""
import numpy as np

SIZES = [(37, 5), (67, 19), (257, 257)]     # 185 pixels (less than one run), 1 273 (5 runs, ragged), 66 049 (259 runs: two reduce levels)
UPDATES = 6
F = np.float32
STATE_FLOATS = ("s", "mean", "m2")
INFO_INTS = ("pixels", "unsampled", "known", "nonfinite", "below", "converged")


def reduce_runs(x):
    """The order of a sum: entries padded with +0.0 to a multiple of 256, every run reduced by stride halving, level by level."""
    x = np.asarray(x, np.float64)
    while True:
        pad = (-len(x)) % 256
        x = np.concatenate([x, np.zeros(pad)]).reshape(-1, 256).copy()
        s = 128
        while s:
            x[:, :s] = x[:, :s] + x[:, s:2 * s]
            s //= 2
        x = x[:, 0].copy()
        if len(x) == 1:
            return x[0]


def rule(state, rgba, threshold=0.0, min_batches=2, allow_pixels=0):
    """One update of `state` ((H, W) records, in place) from `rgba` ((H, W, 4) float32): (info dict, (H, W) float32 error plane)."""
    shape = state.shape
    st = state.reshape(-1)
    px = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        n1 = px[:, 3].copy().view(np.uint32)
        y = (F(0.2126) * px[:, 0] + F(0.7152) * px[:, 1]) + F(0.0722) * px[:, 2]
        assert y.dtype == np.float32
        restart = n1 < st["n"]
        for name in st.dtype.names:
            st[name][restart] = 0
        bsz = n1 - st["n"]
        u = bsz != 0
        bf = bsz[u].astype(np.float64)
        s1 = n1[u].astype(np.float64) * y[u].astype(np.float64)
        t = s1 - st["s"][u]
        B = t / bf
        w1 = st["w"][u] + bsz[u]
        d = B - st["mean"][u]
        mean1 = st["mean"][u] + (bf / w1.astype(np.float64)) * d
        st["m2"][u] = st["m2"][u] + (bf * d) * (B - mean1)
        st["mean"][u] = mean1; st["s"][u] = s1; st["n"][u] = n1[u]; st["w"][u] = w1; st["k"][u] = st["k"][u] + np.uint32(1)
        known = st["k"] >= 2
        v = (st["m2"][known] / (st["k"][known] - np.uint32(1)).astype(np.float64)) / st["w"][known].astype(np.float64)
        v = np.where(v < 0, 0.0, v)
        err = np.full(len(st), F(-1.0), np.float32)
        err[known] = np.sqrt(v.astype(np.float32))
        finite = known & np.isfinite(err)
        below = finite & (st["k"] >= min_batches) & (err <= F(threshold))
        info = {"pixels": len(st), "unsampled": int((n1 == 0).sum()), "known": int(known.sum()), "nonfinite": int((known & ~finite).sum()),
                "below": int(below.sum())}
        info["converged"] = bool(info["pixels"] - info["below"] <= allow_pixels)
        info["max_error"] = float(err[finite].max()) if finite.any() else 0.0
        info["sum_error"] = float(reduce_runs(np.where(finite, err.astype(np.float64), 0.0)))
        m = info["known"] - info["nonfinite"]
        info["mean_error"] = info["sum_error"] / m if m else 0.0
        info["ms"] = 0.0
    return info, err.reshape(shape)


def crafted_frames(W, H, seed):
    """UPDATES read-outs of one W x H accumulation target with every case the rule distinguishes.  By flat pixel number i:
    i % 11 == 0 never gets a sample; i % 13 == 1 gets none in updates 2 and 4 (bsz == 0; its colour moves all the same); i % 17 == 2
    restarts at update 3 (the count drops); i % 19 == 3 is first seen at n = 500; i % 23 == 4 has a constant colour (err == 0).  Pixels
    5..9 hold a NaN, +inf, -inf, 3e38 and the count 0xFFFFFFFF (which then drops)."""
    rng = np.random.default_rng(seed)
    N = W * H
    i = np.arange(N)
    inc = rng.integers(1, 10, size=(UPDATES, N)).astype(np.int64)
    inc[2, i % 13 == 1] = 0; inc[4, i % 13 == 1] = 0
    drop = i % 17 == 2
    inc[3, drop] = 1                                               # below the two samples or more of updates 0 and 1
    counts = np.cumsum(inc, axis=0)
    counts[3:, drop] = np.cumsum(inc[3:, drop], axis=0)            # starts again from zero at update 3
    assert (counts[3, drop] < counts[2, drop]).all()
    counts[:, i % 19 == 3] += 500
    counts[:, i % 11 == 0] = 0
    base = rng.random((N, 3), dtype=np.float32)
    frames = []
    for u in range(UPDATES):
        noise = (rng.random((N, 3), dtype=np.float32) - F(0.5)) / np.sqrt(np.maximum(counts[u], 1)).astype(np.float32)[:, None]
        rgb = base + noise
        const = i % 23 == 4
        rgb[const] = base[const]
        rgb[i % 11 == 0] = 0
        a = counts[u].astype(np.uint32)
        if u >= 1:
            rgb[5, 1] = np.nan
        if u >= 2:
            rgb[6] = np.inf
            rgb[7, 0] = -np.inf
        rgb[8] = F(3e38) if u % 2 else F(-3e38)
        a[5:9] = np.cumsum(inc[:, 5:9], axis=0)[u]                  # the special colours sit on plainly counted pixels
        a[9] = [3, 7, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 12][u]
        frame = np.empty((N, 4), np.float32)
        frame[:, :3] = rgb
        frame[:, 3] = a.view(np.float32)
        assert np.array_equal(frame[:, 3].copy().view(np.uint32), a)   # the count bits survive the copy (0xFFFFFFFF is a NaN pattern)
        frames.append(frame.reshape(H, W, 4))
    return frames


# ---- frames on which the ORDER of the sum and the seams of the reduction show.  crafted_frames cannot show either: its errors are
# binary32 values of a narrow range summed in binary64, so no addition rounds and every order gives the same bits, and its special
# pixels sit in lanes 5..9 of the first run.

# 1, 255, 256 (one full run, no padding), 257 (a run and one pixel), 1 273, 65 536 (exactly 256 partials), 65 537 (257 partials: a
# second level whose last run has one entry) and 66 049 pixels
SEAM_SIZES = [(1, 1), (255, 1), (256, 1), (257, 1), (67, 19), (256, 256), (65537, 1), (257, 257)]
RUN = 256
LANES = (0, 31, 32, 63, 64, 127, 128, 191, 255)      # both sides of every stride of the block reduction (128, 64, 32) and the two ends
KINDS = ("nan", "+inf", "-inf", "3e38", "count", "zero", "denormal")
RUN_KINDS = ("nan", "count", "zero", "+inf", "-inf", "3e38", "nan", "denormal", "+inf")     # by place of a run, see special_kinds
NONFINITE_KINDS = ("nan", "+inf", "-inf", "3e38")    # known and not finite from the third update on
COUNT_TRACK = (3, 7, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 12)
ZERO_TRACK = (5, 9, 0, 0, 4, 8)                      # drops to exactly 0: restart, then bsz == 0, and the zeroed state must be kept
CARRIER_LANES = (0, 63, 64, 127, 128, 255)
CARRIER_PLACES = len(CARRIER_LANES) + 2              # the run lanes, then the first pixel of the last run and the last pixel


def _runs(n):
    return (n + RUN - 1) // RUN


def special_runs(n):
    """The runs that hold special pixels: the first, a middle one and the last; with more than 256 runs also runs 255 and 256, whose
    partials are the last entry of one run of the second level and the first entry of the next."""
    runs = _runs(n)
    out = {0, runs // 2, runs - 1}
    if runs > RUN:
        out |= {RUN - 1, RUN}
    return sorted(out)


def run_places(n, run, lanes=LANES):
    """The flat indices of `lanes` in `run`, clipped to the run's length, with the run's last pixel."""
    first = run * RUN
    length = min(RUN, n - first)
    assert length >= 1
    return sorted({first + l for l in lanes if l < length} | {first + length - 1})


def placed_specials(n):
    """Where the special pixels of an image of n pixels go: LANES of every run of special_runs(n); sorted, no duplicates."""
    return np.array(sorted({p for r in special_runs(n) for p in run_places(n, r)}), np.int64)


def special_kinds(n):
    """{flat index: kind}.  RUN_KINDS goes over the places of a special run in order, starting three further on in every next run: all
    seven kinds occur in one run, the kinds that end non-finite sit on both sides of the two strides that go through LDS (lanes 63,
    64, 127, 128), and a lane holds another kind in the next run."""
    out = {}
    for j, r in enumerate(special_runs(n)):
        for q, p in enumerate(run_places(n, r)):
            out[p] = RUN_KINDS[(q + 3 * j) % len(RUN_KINDS)]
    return out


def _special_pixel(kind, u, colour, count):
    """The (rgb, count) of a special pixel at update u; `colour` is its unscaled ordinary colour, `count` its plainly growing count."""
    rgb = np.array(colour, np.float32)
    if kind == "nan" and u >= 1:
        rgb[1] = np.nan
    elif kind == "+inf" and u >= 2:
        rgb[:] = np.inf
    elif kind == "-inf" and u >= 2:
        rgb[0] = -np.inf
    elif kind == "3e38":
        rgb[:] = F(3e38) if u % 2 else F(-3e38)
    elif kind == "count":
        count = COUNT_TRACK[u]
    elif kind == "zero":
        count = ZERO_TRACK[u]
        if count == 0:
            rgb[:] = 0
    elif kind == "denormal":
        rgb = (rgb * F(2.0 ** -100)) * F(2.0 ** -30)               # binary32 denormals: a flush to zero moves s, mean and m2
    return rgb, count


def wide_range_frames(W, H, seed, kinds=None):
    """crafted_frames' six updates and case classes (never sampled, no new samples, restart, late start, constant colour) with the
    colour of pixel i multiplied by 2^e(i), e(i) fixed over the sequence and drawn from -20..20: the errors then span 40 binades, the
    additions of the sum round, and the order shows in the bits; powers of two leave everything else about the frames exact.  The
    special pixels -- `kinds`, by default special_kinds(W * H) -- are not scaled."""
    rng = np.random.default_rng(seed)
    N = W * H
    i = np.arange(N)
    inc = rng.integers(1, 10, size=(UPDATES, N)).astype(np.int64)
    plain = np.cumsum(inc, axis=0)                                 # what a special pixel counts: new samples at every update
    inc[2, i % 13 == 1] = 0; inc[4, i % 13 == 1] = 0
    drop = i % 17 == 2
    inc[3, drop] = 1
    counts = np.cumsum(inc, axis=0)
    counts[3:, drop] = np.cumsum(inc[3:, drop], axis=0)
    assert (counts[3, drop] < counts[2, drop]).all()
    counts[:, i % 19 == 3] += 500
    counts[:, i % 11 == 0] = 0
    scale = np.ldexp(F(1), rng.integers(-20, 21, size=N)).astype(np.float32)
    base = rng.random((N, 3), dtype=np.float32)
    kinds = special_kinds(N) if kinds is None else kinds
    frames = []
    for u in range(UPDATES):
        noise = (rng.random((N, 3), dtype=np.float32) - F(0.5)) / np.sqrt(np.maximum(counts[u], 1)).astype(np.float32)[:, None]
        colour = base + noise
        const = i % 23 == 4
        colour[const] = base[const]
        rgb = colour * scale[:, None]
        rgb[i % 11 == 0] = 0
        a = counts[u].astype(np.uint32)
        for p, kind in kinds.items():
            rgb[p], a[p] = _special_pixel(kind, u, colour[p], int(plain[u, p]))
        frame = np.empty((N, 4), np.float32)
        frame[:, :3] = rgb
        frame[:, 3] = a.view(np.float32)
        assert np.array_equal(frame[:, 3].copy().view(np.uint32), a)
        frames.append(frame.reshape(H, W, 4))
    return frames


def carrier_places(n, raw=False):
    """The pixels that can carry the maximum, duplicates dropped (raw: all eight): CARRIER_LANES, then the first pixel of the last run and the last
    pixel of the image.  With 256 runs or more lane L sits in run L, so that the maximum travels from lane L of a k_cv_update block
    and from lane L of a k_cv_reduce block; otherwise in run 1 when there are four runs or more (no special run), else in run 0."""
    runs = _runs(n)
    out = []
    for l in CARRIER_LANES:
        run = min(l, runs - 1) if runs >= RUN else (1 if runs >= 4 else 0)
        out.append(min(run * RUN + l, n - 1) if run == runs - 1 else run * RUN + l)
    out += [(runs - 1) * RUN, n - 1]
    if raw:
        return out
    places = list(dict.fromkeys(out))
    assert len(places) == 1 or len(places) >= UPDATES, "a pixel would carry two updates"
    return places


def carrier_pixels(n, place):
    """The pixel that holds max_error after update u, for every u: the places in turn, starting at `place`."""
    places = carrier_places(n)
    return [places[(u + place) % len(places)] for u in range(UPDATES)]


def max_carrier(frames, place):
    """A copy of `frames` in which, for every update u, the pixel carrier_pixels(n, place)[u] is the one holder of the largest finite
    error.  Every carrier runs through the same two alternating colours, on a power-of-two scale above every other pixel's
    from the first update on -- 2^24 for the last carrier and 16 times more for each earlier one, so their errors are 16 times apart
    exactly -- and the carrier of update u has a NaN colour from update u + 1 on, which takes it out of
    the maximum (and into `nonfinite`) for good.  In a single-pixel image the one pixel carries every update."""
    H, W = frames[0].shape[:2]
    pixels = carrier_pixels(W * H, place)
    out = [f.copy() for f in frames]
    for p in dict.fromkeys(pixels):
        first, last = pixels.index(p), UPDATES - 1 - pixels[::-1].index(p)
        scale = F(2.0 ** (24 + 4 * (UPDATES - 1 - first)))
        for v in range(UPDATES):
            px = out[v].reshape(-1, 4)[p]
            px[:3] = np.array((0.25, 0.5, 0.75) if v % 2 else (0.75, 0.5, 0.25), np.float32) * scale
            if v > last:
                px[1] = np.nan
            px[3:] = np.array([3 * (v + 1)], np.uint32).view(np.float32)
    return out


# Per seam size: the seed of the sequence with the placed specials alone, the seed of the one with the carrier on top, and the place
# at which its carrier starts (all eight places occur over the sizes).  The seeds are the smallest, counted from 1, at which the
# numpy restatement's sum differs in bits from every order of other_orders() as test_converge_cpu.py demands: with binary32 errors
# 40 binades apart few additions of a binary64 sum round, so not every seed shows every order.
WIDE_SEQUENCES = {(1, 1): (1, 1, 0), (255, 1): (4, 4, 1), (256, 1): (22, 3, 2), (257, 1): (13, 8, 3), (67, 19): (35, 41, 4),
                  (256, 256): (88, 2, 5), (65537, 1): (26, 3, 6), (257, 257): (2, 2, 7)}
VARIANTS = ("specials", "carrier")


def wide_sequence(size, variant):
    W, H = size
    plain, carried, place = WIDE_SEQUENCES[size]
    if variant == "specials":
        return wide_range_frames(W, H, plain)
    return max_carrier(wide_range_frames(W, H, carried), place)


def error_entries(err):
    """What the pixels of an error plane enter into sum_error: the finite errors of the known pixels in binary64, +0.0 elsewhere."""
    e = np.asarray(err, np.float32).reshape(-1)
    return np.where(np.isfinite(e) & (e != F(-1.0)), e.astype(np.float64), 0.0)


def _by_levels(x, reduce_rows):
    """The level structure of the rule with another reduction of the (runs, 256) rows of a level."""
    x = np.asarray(x, np.float64)
    while True:
        x = reduce_rows(np.concatenate([x, np.zeros((-len(x)) % RUN)]).reshape(-1, RUN))
        if len(x) == 1:
            return x[0]


def _halving(x):
    x = x.copy()
    s = x.shape[-1] // 2
    while s:
        x[..., :s] = x[..., :s] + x[..., s:2 * s]
        s //= 2
    return x[..., 0].copy()


def _doubling(x):
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0].copy()


def _wave_first(x):
    w = _halving(x.reshape(-1, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def other_orders(x):
    """The binary64 sum of the entries x in orders that are NOT the rule's, {name: sum}: left to right (what atomics on one address or a
    serial loop give); numpy.sum (pairwise); stride doubling inside a run, neighbours first; every run as four waves of 64 reduced by
    stride halving and then added left to right; runs by the rule, but the partials of the first level added left to right."""
    x = np.asarray(x, np.float64)
    runs = _halving(np.concatenate([x, np.zeros((-len(x)) % RUN)]).reshape(-1, RUN))
    return {"sequential": float(np.add.accumulate(x)[-1]), "numpy": float(np.sum(x)), "doubling": float(_by_levels(x, _doubling)),
            "wave_first": float(_by_levels(x, _wave_first)), "flat_levels": float(np.add.accumulate(runs)[-1])}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def fenced_equal(got, want, fence):
    """Bit for bit; with `fence` a word that is NaN in `want` may be any NaN in `got` (the shade_util.compare convention)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    same = bits(got) == bits(want)
    if fence and got.dtype.kind == "f":
        same = same | (np.isnan(want) & np.isnan(got))
    return bool(same.all())


def differing(got_state, got_err, got_info, want_state, want_err, want_info, fence):
    """The names of what differs between two results of one update (state records, error plane, info dict)."""
    bad = []
    for name in ("n", "k", "w", "pad"):
        if not np.array_equal(got_state[name], want_state[name]):
            bad.append("state." + name)
    for name in STATE_FLOATS:
        if not fenced_equal(got_state[name], want_state[name], fence):
            bad.append("state." + name)
    if not fenced_equal(got_err, want_err, fence):
        bad.append("error")
    for name in INFO_INTS:
        if int(got_info[name]) != int(want_info[name]):
            bad.append("info." + name)
    if not fenced_equal(np.float32(got_info["max_error"]), np.float32(want_info["max_error"]), False):
        bad.append("info.max_error")
    for name in ("sum_error", "mean_error"):
        if not fenced_equal(np.float64(got_info[name]), np.float64(want_info[name]), False):
            bad.append("info." + name)
    return bad


PARAMS = [dict(), dict(threshold=0.02, min_batches=3, allow_pixels=40), dict(threshold=float("inf"), min_batches=2, allow_pixels=0)]


def host_chain(capi, frames, params=PARAMS):
    """gmupt_converge_host chained over `frames`: [(state copy, error plane, info)] per update, the parameters cycling through `params`."""
    H, W = frames[0].shape[:2]
    state = np.zeros((H, W), capi.converge_pixel_dtype)
    out = []
    for u, f in enumerate(frames):
        info, err = capi.converge_host(state, f, error=True, **params[u % len(params)])
        out.append((state.copy(), err, info))
    return out

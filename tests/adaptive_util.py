"""What the adaptive-sampling tests share: a numpy restatement of the two rules of include/gmupt_adaptive.h, written from
the header, and the crafted error planes."""
import numpy as np

F = np.float32
RUN = 256
T = 0.0078125                       # 2^-7: q = err / T is exact for the crafted values, so q * q lands where the plane says it does
SIZES = [(1, 1), (255, 1), (256, 1), (257, 1), (256, 256), (65537, 1), (257, 257)]   # 65 536, 65 537 and 66 049 pixels: a second scan level and its seam
MAX_REPEATS = (1, 3, 64)
LANES = (0, 63, 64, 255)
INFO_INTS = ("pixels", "active", "entries", "skipped_nonfinite", "max_rep")


def specials(max_repeat):
    """The values the rule has a case for, with what each is there for."""
    t = F(T)
    return np.array([
        -1.0, 0.0, -0.0, t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(0)),           # unknown, zero, at the threshold and its two neighbours
        2 * t, np.nextafter(2 * t, F(np.inf)), np.nextafter(2 * t, F(0)),                # q * q == 4 exactly, just past it, just short of it
        1.5 * t, F(1.25) * t,                                                            # 2.25 -> 3, 1.5625 -> 2
        8 * t, np.nextafter(8 * t, F(0)), np.nextafter(8 * t, F(np.inf)), 100 * t,       # q * q == 64: the largest cap, its neighbours, far beyond
        t * F(np.sqrt(F(max_repeat))), np.nextafter(t * F(np.sqrt(F(max_repeat))), F(np.inf)),   # at this plane's cap (to rounding)
        np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40, 1.4e-45,                    # non-finite, huge (q * q overflows), denormals
    ], dtype=F)


def places(n):
    """Lanes 0, 63, 64, 255 and the last pixel of the first, a middle and the last run of n pixels."""
    runs = (n + RUN - 1) // RUN
    out = []
    for run in sorted({0, runs // 2, runs - 1}):
        for lane in LANES:
            if run * RUN + lane < n:
                out.append(run * RUN + lane)
        out.append(min(n, (run + 1) * RUN) - 1)
    return sorted(set(out))


def plane(size, max_repeat, seed):
    """A (H, W) error plane: a quarter of the pixels draws from the special values, the rest is spread over 0 .. 12 T; the places of
    `places` take the special values in turn, starting at `seed`."""
    W, H = size
    n = W * H
    rng = np.random.default_rng(seed * 7919 + n)
    sp = specials(max_repeat)
    e = (rng.random(n, dtype=F) ** 2 * F(12 * T)).astype(F)
    pick = rng.random(n) < 0.25
    e[pick] = sp[rng.integers(0, len(sp), int(pick.sum()))]
    for i, p in enumerate(places(n)):
        e[p] = sp[(i + seed) % len(sp)]
    return e.reshape(H, W)


def uniform_planes(size):
    """Every pixel below the threshold (count == 0) and every pixel at the cap."""
    W, H = size
    return np.full((H, W), F(T) / 2, F), np.full((H, W), F(T) * 100, F)


def reps(err, threshold, max_repeat):
    """"Selection" of the header: the entries of every pixel."""
    e = np.asarray(err, F).reshape(-1)
    t = F(threshold)
    finite = np.isfinite(e)
    with np.errstate(all="ignore"):
        q = (e / t).astype(F)
        m = (q * q).astype(F)
        capped = m >= F(max_repeat)
        c = np.ceil(np.where(finite & ~capped, m, F(1))).astype(np.uint32)
    rep = np.where(capped, np.uint32(max_repeat), np.maximum(np.uint32(1), c)).astype(np.uint32)
    rep[finite & (e <= t)] = 0          # the monitor's `below` comparison
    rep[finite & (e < 0)] = 1           # unknown / unsampled
    rep[~finite] = 0
    return rep


def select(err, threshold, max_repeat=1, **_):
    """(list, info) of the header's selection."""
    e = np.asarray(err, F).reshape(-1)
    rep = reps(e, threshold, max_repeat)
    lst = np.repeat(np.arange(e.size, dtype=np.uint32), rep)
    info = {"pixels": e.size, "active": int((rep > 0).sum()), "entries": int(rep.sum()), "skipped_nonfinite": int((~np.isfinite(e)).sum()),
            "max_rep": int(rep.max())}
    return lst, info


def pixel_of(lst, uniform_every, w, h, k):
    """"Where path k goes" of the header, for an array of k (uint32 arithmetic)."""
    k = np.asarray(k, np.uint64) & np.uint64(0xFFFFFFFF)
    lst = np.asarray(lst, np.uint32)
    out = lst[(k % np.uint64(lst.size)).astype(np.int64)].astype(np.uint64)
    if uniform_every:
        u = (k % np.uint64(uniform_every)) == 0
        out[u] = k[u] % np.uint64(w * h)
    return out.astype(np.uint32)


def same(got_list, got_info, want_list, want_info):
    """What differs between two selections: [] when they are equal bit for bit."""
    bad = [f for f in INFO_INTS if int(got_info[f]) != int(want_info[f])]
    if got_list.shape != want_list.shape or not np.array_equal(got_list, want_list):
        bad.append("list")
    return bad


def rect_list(W, x0, y0, w, h):
    """The row-major list of the pixels of a rectangle of a frame W wide."""
    ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
    return (ys * W + xs).astype(np.uint32).reshape(-1)

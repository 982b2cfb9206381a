"""What the convergence tests share: the numpy restatement of the rule of include/gmupt.h ("Convergence"), written from the header and
independent of csrc/pt_converge.hpp; the crafted frame sequences; and the bit-for-bit comparison with the NaN fence."""
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

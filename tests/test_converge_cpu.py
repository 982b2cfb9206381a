"""gmupt_converge_host, the reference of the device convergence monitor (include/gmupt.h "Convergence"), against the independent numpy
restatement of the rule in converge_util.py -- state, error plane and info bit for bit over chained updates of crafted frames and of
the wide-range frames, whose preconditions (the order of the sum shows in the bits, the specials and the maximum sit at the seams of the
reduction) are checked on the restatement alone -- the
estimator's unbiasedness on synthetic samples, the argument errors, the stop rule at its boundaries, and ProgressiveSession.run_until on
stand-in renderers, alone and as two gloo ranks.  No device."""
import ctypes as C
import os
import re
import socket
import sys

import numpy as np
import pytest

import converge_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_converge_default_params", "gmupt_converge_host", "gmupt_converge_create", "gmupt_converge_destroy", "gmupt_converge_reset",
               "gmupt_converge_update", "gmupt_converge_update_image", "gmupt_converge_read_state", "gmupt_render_until"]


@pytest.mark.parametrize("size", CU.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_rule_equals_the_restatement_bit_for_bit(pkg, size):
    W, H = size
    frames = CU.crafted_frames(W, H, seed=W * 1000 + H)
    got = CU.host_chain(pkg.capi, frames)
    want_state = np.zeros((H, W), pkg.capi.converge_pixel_dtype)
    for u, f in enumerate(frames):
        want_info, want_err = CU.rule(want_state, f, **CU.PARAMS[u % len(CU.PARAMS)])
        state, err, info = got[u]
        bad = CU.differing(state, err, info, want_state, want_err, want_info, fence=False)
        assert not bad, (size, u, bad, info, want_info)
        assert info["ms"] == 0.0
    # the frames hold what they are meant to hold
    state, err, info = got[-1]
    flat, e = state.reshape(-1), err.reshape(-1)
    i = np.arange(W * H)
    assert info["pixels"] == W * H and info["unsampled"] == int((i % 11 == 0).sum()) and (flat["k"][i % 11 == 0] == 0).all()
    assert (flat["k"][(i % 13 == 1) & (i % 11 != 0) & (i % 17 != 2) & (i > 9)] == CU.UPDATES - 2).all(), "bsz == 0 leaves the state alone"
    assert (flat["k"][(i % 17 == 2) & (i % 11 != 0) & (i % 13 != 1) & (i > 9)] == 3).all(), "a count that drops restarts the pixel"
    first = got[0][0].reshape(-1)
    assert (first["n"][(i % 19 == 3) & (i % 11 != 0)] > 500).all() and (first["k"][(i % 19 == 3) & (i % 11 != 0)] == 1).all()
    const = (i % 23 == 4) & (i % 11 != 0) & (i > 9)
    assert const.any() and (CU.bits(e[const]) == 0).all(), "equal batches give err == +0"
    assert np.isnan(e[5]) and np.isnan(e[6]) and np.isnan(e[7]) and np.isinf(e[8]) and info["nonfinite"] >= 4
    assert got[3][0].reshape(-1)["n"][9] == 0xFFFFFFFF and flat["n"][9] == 12 and flat["k"][9] == 1
    assert (e[flat["k"] < 2] == -1.0).all() and info["known"] == int((flat["k"] >= 2).sum())


_SEAM_IDS = dict(ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else s)


@pytest.fixture(scope="module")
def restated(pkg):
    """(size, variant) -> (frames, [(state copy, error plane, info)] per update) of a wide-range sequence by the numpy restatement."""
    cache = {}

    def get(size, variant):
        if (size, variant) not in cache:
            frames = CU.wide_sequence(size, variant)
            state = np.zeros((size[1], size[0]), pkg.capi.converge_pixel_dtype)
            out = []
            for u, f in enumerate(frames):
                info, err = CU.rule(state, f, **CU.PARAMS[u % len(CU.PARAMS)])
                out.append((state.copy(), err, info))
            cache[(size, variant)] = (frames, out)
        return cache[(size, variant)]
    return get


def _same_bits(a, b):
    return bool(CU.bits(np.float64(a)) == CU.bits(np.float64(b)))


@pytest.mark.parametrize("variant", CU.VARIANTS)
@pytest.mark.parametrize("size", CU.SEAM_SIZES, **_SEAM_IDS)
def test_wide_range_frames_show_the_order_and_the_seams(restated, size, variant):
    """The preconditions of the host and device comparisons on the wide-range sequences, on the numpy restatement alone, so that those
    comparisons cannot pass vacuously.  The crafted frames' sum has the same bits in any order; here the rule's sum differs from each
    order of other_orders() at three or more of the five updates with known pixels, from all of them at once at one update or more.
    Void for the single pixel (one entry has one order).  "flat_levels" is left out for one run (it is the rule) and for two: the
    rule's second level pads two partials to a run, and the only addition of that run that is not x + 0.0 is p0 + p1."""
    W, H = size
    N = W * H
    frames, want = restated(size, variant)
    differs, at_once = {}, 0
    for u in range(1, CU.UPDATES):
        _, err, info = want[u]
        x = CU.error_entries(err)
        assert info["known"] > info["nonfinite"] or N == 1
        assert _same_bits(CU.reduce_runs(x), info["sum_error"]), "the entries are those of the sum"
        others = CU.other_orders(x)
        assert len(others) == 5
        if CU._runs(N) <= 2:
            del others["flat_levels"]
        d = {name: not _same_bits(v, info["sum_error"]) for name, v in others.items()}
        for name, v in d.items():
            differs[name] = differs.get(name, 0) + int(v)
        at_once += all(d.values())
    print(size, variant, differs, at_once)
    if N == 1:
        assert not any(differs.values())
    else:
        assert min(differs.values()) >= 3 and at_once >= 1, (differs, at_once)
    # the special pixels are where placed_specials() says; no ordinary pixel is non-finite
    kinds = CU.special_kinds(N)
    assert sorted(kinds) == CU.placed_specials(N).tolist() and set(kinds.values()) <= set(CU.KINDS)
    carriers = CU.carrier_pixels(N, CU.WIDE_SEQUENCES[size][2]) if variant == "carrier" else []
    state, err, info = want[-1]
    flat, e = state.reshape(-1), err.reshape(-1)
    nonfinite = np.flatnonzero((flat["k"] >= 2) & ~np.isfinite(e))
    assert info["nonfinite"] == len(nonfinite) and set(nonfinite.tolist()) <= set(kinds) | set(carriers)
    if variant == "specials":
        assert nonfinite.tolist() == sorted(p for p, kind in kinds.items() if kind in CU.NONFINITE_KINDS)
        if N >= 255:
            # the nine places of one run hold all seven kinds, six pixels of them non-finite; three runs or more are placed from 1 273 pixels on
            assert set(kinds.values()) == set(CU.KINDS) and info["nonfinite"] >= 6 and (info["nonfinite"] > 8 or N <= 257)
            assert {63, 64, 127, 128} <= set(nonfinite.tolist()), "both sides of the strides that go through LDS"
            assert (N - 1) in kinds and (CU._runs(N) - 1) * 256 in kinds
        if CU._runs(N) > 256:
            assert {255 * 256 + 255, 256 * 256} <= set(nonfinite.tolist()), "the last entry of a run of the second level, the first of the next"
        for p, kind in kinds.items():
            if kind == "zero":   # 5, 9, 0, 0, 4, 8
                for u in (2, 3):
                    assert CU.bits(frames[u].reshape(-1, 4)[p, 3]) == 0, "counted as unsampled"
                    assert not want[u][0].reshape(-1)[p:p + 1].view(np.uint8).any() and want[u][1].reshape(-1)[p] == -1.0
                assert (flat["n"][p], flat["k"][p], flat["w"][p]) == (8, 2, 8) and e[p] >= 0, "it recovers"
            if kind == "denormal":
                rgb = frames[-1].reshape(-1, 4)[p, :3]
                assert (rgb != 0).all() and (np.abs(rgb) < np.float32(2.0 ** -126)).all() and flat["s"][p] != 0 and e[p] == 0
            if kind == "count":
                assert want[3][0].reshape(-1)["n"][p] == 0xFFFFFFFF and (flat["n"][p], flat["k"][p]) == (12, 1)
    else:
        # max_error is held by one pixel, the carrier of the update
        for u in range(1, CU.UPDATES):
            _, err_u, info_u = want[u]
            eu = err_u.reshape(-1)
            finite = np.isfinite(eu) & (eu != -1.0)
            top = eu[finite].max()
            assert np.flatnonzero(finite & (eu == top)).tolist() == [carriers[u]], (u, carriers)
            assert np.float32(info_u["max_error"]) == top and top >= np.float32(2.0 ** 20)
        assert len(set(carriers)) == (1 if N == 1 else CU.UPDATES)


def test_every_carrier_place_occurs(pkg):
    """Over the seam sizes the maximum travels from each of the eight places, at an update with known pixels."""
    seen = set()
    for size in CU.SEAM_SIZES:
        n = size[0] * size[1]
        if n > 1:
            held = CU.carrier_pixels(n, CU.WIDE_SEQUENCES[size][2])[1:]
            seen |= {j for j, p in enumerate(CU.carrier_places(n, raw=True)) if p in held}
    assert seen == set(range(CU.CARRIER_PLACES))
    assert CU.carrier_places(66049, raw=True) == [0, 63 * 257, 64 * 257, 127 * 257, 128 * 257, 255 * 257, 66048, 66048]
    assert CU.carrier_places(1273) == [256, 319, 320, 383, 384, 511, 1024, 1272] and CU.carrier_places(255) == [0, 63, 64, 127, 128, 254]
    assert CU.placed_specials(257).tolist() == [0, 31, 32, 63, 64, 127, 128, 191, 255, 256] and CU.placed_specials(1).tolist() == [0]
    assert CU.special_runs(66049) == [0, 129, 255, 256, 258] and CU.special_runs(65536) == [0, 128, 255]


@pytest.mark.parametrize("variant", CU.VARIANTS)
@pytest.mark.parametrize("size", CU.SEAM_SIZES, **_SEAM_IDS)
def test_host_rule_equals_the_restatement_on_wide_range_frames(pkg, restated, size, variant):
    """As test_host_rule_equals_the_restatement_bit_for_bit, on frames on which a host reference that summed in another order fails."""
    frames, want = restated(size, variant)
    got = CU.host_chain(pkg.capi, frames)
    for u in range(CU.UPDATES):
        state, err, info = got[u]
        want_state, want_err, want_info = want[u]
        bad = CU.differing(state, err, info, want_state, want_err, want_info, fence=True)
        assert not bad, (size, variant, u, bad, info, want_info)
        assert info["ms"] == 0.0


def test_the_estimate_is_unbiased(pkg):
    """4 096 pixels, each the running mean of iid uniform samples on [0, a_p) -- per-sample variance sigma^2 = a_p^2 / 12 of the grey value,
    hence of its luminance (the three weights sum to 1) -- read out after each of K = 16 batches of 8 samples.  err^2 * w is the weighted
    sample variance S^2 of the batch means, an unbiased estimator of sigma^2.  Tolerance, from the estimator's own sampling distribution:
    the batch means are close to normal, so (K - 1) S^2 / sigma^2 is close to chi-square with K - 1 degrees of freedom and S^2 / sigma^2 has
    the relative standard deviation sqrt(2 / (K - 1)) per pixel (the negative excess kurtosis of a mean of 8 uniforms only lowers it); the
    mean over P independent pixels has that divided by sqrt(P); six of those standard deviations: 6 * sqrt(2 / 15) / 64 = 0.0342.  The
    rounding of the stored binary32 mean, about (n / bsz) * 2^-24 = 1e-6 of the mean per batch, is four orders below the batch means'
    spread."""
    capi = pkg.capi
    P, K, b = 4096, 16, 8
    rng = np.random.default_rng(20240229)
    a = rng.uniform(0.2, 1.0, P)
    x = rng.random((K * b, P)) * a
    state = np.zeros((64, 64), capi.converge_pixel_dtype)
    for j in range(1, K + 1):
        n = j * b
        frame = np.empty((P, 4), np.float32)
        frame[:, :3] = x[:n].mean(axis=0).astype(np.float32)[:, None]
        frame[:, 3] = np.full(P, n, np.uint32).view(np.float32)
        info, err = capi.converge_host(state, frame.reshape(64, 64, 4), error=True)
    assert info["known"] == P and info["nonfinite"] == 0 and (state["k"] == K).all() and (state["w"] == K * b).all()
    ratio = err.reshape(-1).astype(np.float64) ** 2 * (K * b) / (a * a / 12.0)
    tol = 6.0 * np.sqrt(2.0 / (K - 1)) / np.sqrt(P)
    print("mean of err^2 * w / sigma^2 over %d pixels: %.5f (1 +- %.4f)" % (P, ratio.mean(), tol))
    assert abs(ratio.mean() - 1.0) <= tol


def _known_state(capi, errs_k):
    """A one-row state whose pixels already hold (err^2, k): an update with unchanged counts reports exactly these errors."""
    state = np.zeros((1, len(errs_k)), capi.converge_pixel_dtype)
    rgba = np.zeros((1, len(errs_k), 4), np.float32)
    for p, (e, k) in enumerate(errs_k):
        state[0, p] = (10, k, 10, 0, 0.0, 0.0, float(e) ** 2 * (k - 1) * 10.0)
    rgba[0, :, 3] = np.full(len(errs_k), 10, np.uint32).view(np.float32)
    return state, rgba


def test_stop_rule_at_its_boundaries(pkg):
    capi = pkg.capi
    state, rgba = _known_state(capi, [(0.25, 2), (0.25, 3), (0.5, 3), (0.5, 2), (0.125, 4), (0.125, 2)])
    before = state.copy()
    info, err = capi.converge_host(state, rgba, error=True, threshold=0.25)
    assert state.tobytes() == before.tobytes(), "bsz == 0: the state is unchanged"
    assert err.tolist() == [[0.25, 0.25, 0.5, 0.5, 0.125, 0.125]]
    assert info["known"] == 6 and info["below"] == 4 and info["max_error"] == 0.5 and info["sum_error"] == 1.75 and not info["converged"]
    assert info["mean_error"] == 1.75 / 6
    # pixels - below == allow_pixels converges, one pixel more does not
    assert capi.converge_host(state, rgba, threshold=0.25, allow_pixels=2)["converged"]
    assert not capi.converge_host(state, rgba, threshold=0.25, allow_pixels=1)["converged"]
    # err == threshold counts as below, the next binary32 below the threshold does not
    assert capi.converge_host(state, rgba, threshold=float(np.nextafter(np.float32(0.25), np.float32(0))))["below"] == 2
    # min_batches: pixels with two batches stop counting at 3
    assert capi.converge_host(state, rgba, threshold=0.25, min_batches=2)["below"] == 4
    three = capi.converge_host(state, rgba, threshold=0.25, min_batches=3)
    assert three["below"] == 2 and three["known"] == 6
    assert capi.converge_host(state, rgba, threshold=1.0, min_batches=3, allow_pixels=3)["converged"]
    assert not capi.converge_host(state, rgba, threshold=1.0, min_batches=3, allow_pixels=2)["converged"]
    # the defaults only report: threshold 0, nothing below unless its error is zero
    d = capi.converge_params()
    assert (d.threshold, d.min_batches, d.allow_pixels) == (0.0, 2, 0)
    assert capi.converge_host(state, rgba)["below"] == 0
    # unknown pixels are never below, whatever the threshold
    fresh = np.zeros((1, 6), capi.converge_pixel_dtype)
    info = capi.converge_host(fresh, rgba, threshold=float("inf"))
    assert info["known"] == 0 and info["below"] == 0 and info["max_error"] == 0.0 and info["mean_error"] == 0.0 and not info["converged"]


def test_argument_errors_leave_the_outputs_untouched(pkg):
    capi = pkg.capi
    lib = capi.lib()
    frames = CU.crafted_frames(8, 4, 1)
    state = np.zeros((4, 8), capi.converge_pixel_dtype)
    capi.converge_host(state, frames[0]); capi.converge_host(state, frames[1])
    err = np.full((4, 8), 7.0, np.float32)
    info = capi.ConvergeInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    before = (bytes(info), state.tobytes(), err.tobytes())
    ps, pf, pe = (a.ctypes.data_as(C.c_void_p) for a in (state, frames[2], err))
    ok = capi.converge_params()
    few, nan = capi.converge_params(min_batches=1), capi.converge_params(threshold=float("nan"))
    cases = [(None, pf, 8, 4, C.byref(ok), pe, C.byref(info)), (ps, None, 8, 4, C.byref(ok), pe, C.byref(info)), (ps, pf, 8, 4, C.byref(ok), pe, None),
             (ps, pf, 0, 4, C.byref(ok), pe, C.byref(info)), (ps, pf, 8, 0, C.byref(ok), pe, C.byref(info)),
             (ps, pf, 65536, 65536, C.byref(ok), pe, C.byref(info)), (ps, pf, 8, 4, C.byref(few), pe, C.byref(info)),
             (ps, pf, 8, 4, C.byref(nan), pe, C.byref(info))]
    for args in cases:
        assert lib.gmupt_converge_host(*args) == capi.ERR_INVALID_ARGUMENT, args
        assert b"gmupt_converge_host" in lib.gmupt_last_error()
        assert (bytes(info), state.tobytes(), err.tobytes()) == before, args
    with pytest.raises(TypeError):
        capi.converge_params(sigma=1.0)
    # the device entry points refuse a missing handle before any device is touched
    h = C.c_void_p(0x1234)
    n = C.c_uint32(77)
    assert lib.gmupt_converge_create(None, C.byref(h)) == capi.ERR_INVALID_ARGUMENT and not h.value
    assert lib.gmupt_converge_create(None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_reset(None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_update(None, C.byref(ok), None, C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_update_image(None, pf, 8, 4, C.byref(ok), None, C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_converge_read_state(None, ps, state.nbytes) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_until(None, None, None, C.byref(ok), 1, 8, C.byref(n), C.byref(info)) == capi.ERR_INVALID_ARGUMENT and n.value == 77
    assert (bytes(info), state.tobytes(), err.tobytes()) == before
    lib.gmupt_converge_destroy(None)


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS and getattr(lib, name, None) is not None, name
    assert "Convergence" in header and "Noise floor" in header and "Missed restart" in header
    assert C.sizeof(pkg.capi.ConvergeInfo) == 56 and pkg.capi.ConvergeInfo.ms.offset == 48 and pkg.capi.converge_pixel_dtype.itemsize == 40


# ---- ProgressiveSession.run_until on stand-ins: "anything with the same methods"
class _Monitor:
    def __init__(self, converges_at):
        self.converges_at, self.checks, self.resets, self.closed, self.params = converges_at, 0, 0, False, None

    def update(self, **params):
        self.checks += 1
        self.params = params
        done = self.checks >= self.converges_at
        return {"pixels": 4, "below": 4 if done else 1, "converged": done, "max_error": 0.0 if done else 1.0}

    def reset(self):
        self.resets += 1
        self.checks = 0

    def close(self):
        self.closed = True


class _Renderer:
    def __init__(self, converges_at):
        self.monitor, self.made, self.iterations, self.size = _Monitor(converges_at), 0, 0, None

    def converge(self):
        self.made += 1
        return self.monitor

    def set_camera(self, buf):
        pass

    def iterate(self):
        self.iterations += 1

    def resize(self, w, h):
        self.size = (w, h)


class _Camera:
    class _Buffer:
        lightCount = 0

    def __init__(self):
        self.buffer, self.resets = self._Buffer(), 0

    def update(self, dt=0.0):
        pass

    def reset_accumulation(self):
        self.resets += 1

    def update_resolution(self, w, h):
        pass


class _LightBuffer:
    def update(self, lights):
        self.lights = lights


def test_session_run_until_on_stand_ins(pkg):
    S = pkg.progressive.ProgressiveSession
    r = _Renderer(converges_at=3)
    s = S(r, _Camera(), 8, 8, preview_every=0)
    info = s.run_until(0.01, check_every=4, max_frames=100, min_batches=3, allow_pixels=2)
    assert info["converged"] and info["frames"] == 12 and r.iterations == 12 and s.frames == 12, "stops at the first converged check"
    assert r.monitor.params == {"threshold": 0.01, "min_batches": 3, "allow_pixels": 2} and r.made == 1
    # max_frames: the monitor would need two more checks
    r.monitor.converges_at = 6
    info = s.run_until(0.01, check_every=4, max_frames=10)
    assert not info["converged"] and info["frames"] == 10 and r.iterations == 22 and r.monitor.checks == 5 and r.made == 1
    # fewer frames than one check: nothing but the frame count
    assert s.run_until(0.01, check_every=4, max_frames=3) == {"converged": False, "frames": 3}
    with pytest.raises(ValueError):
        s.run_until(0.01, check_every=0)
    # the events that restart the accumulation reset the monitor
    assert r.monitor.resets == 0
    s.set_lights(_LightBuffer(), [1, 2], 2)
    assert r.monitor.resets == 1 and s.camera.buffer.lightCount == 2
    s.resize(16, 8)
    assert r.monitor.resets == 2 and r.size == (16, 8)
    assert s.run_until(0.01, check_every=2, max_frames=100)["frames"] == 12      # six checks from the reset on
    s.close()
    assert r.monitor.closed and s.converge is None
    # a session that never ran run_until has no monitor to reset or close
    q = S(_Renderer(1), _Camera(), 8, 8, preview_every=0)
    q.set_lights(_LightBuffer(), [], 0); q.resize(4, 4); q.close()
    assert q.renderer.made == 0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, converges_at, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    import gmupt_pkg
    import test_converge_cpu as T
    pkg = gmupt_pkg.load()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = T._Renderer(converges_at[rank])
    s = pkg.progressive.ProgressiveSession(r, T._Camera(), 8, 8, rank=rank, world=world, dist=dist, preview_every=0)
    info = s.run_until(0.01, check_every=2, max_frames=40)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([info["frames"], int(info["converged"]), r.monitor.checks, r.iterations]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_leave_in_the_same_frame(tmp_path, pkg):
    """Rank 0's stand-in converges three checks before rank 1's: both return after rank 1's check."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), (2, 5), str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(str(tmp_path / ("rank%d.npy" % k))).tolist() for k in (0, 1))
    assert a == [10, 1, 5, 10] and b == [10, 1, 5, 10], (a, b)

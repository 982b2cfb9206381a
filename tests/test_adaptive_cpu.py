"""CPU tests of adaptive sampling (include/gmupt_adaptive.h): the host rules gmupt_adaptive_select_host and
gmupt_adaptive_pixel_host against the numpy restatement of adaptive_util.py bit for bit, the argument errors, and
ProgressiveSession.run_until(adaptive=True) on stand-in renderers, alone and as two gloo ranks.  No device."""
import ctypes as C
import os
import re
import socket
import sys

import numpy as np
import pytest

import adaptive_util as AU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_adaptive_default_params", "gmupt_adaptive_select_host", "gmupt_adaptive_pixel_host", "gmupt_adaptive_create", "gmupt_adaptive_destroy",
               "gmupt_adaptive_select", "gmupt_adaptive_set_list", "gmupt_adaptive_read_list", "gmupt_renderer_set_adaptive", "gmupt_render_adaptive"]


def test_the_restatement_on_values_worked_by_hand():
    t = AU.F(AU.T)
    up, down = np.nextafter(t, AU.F(np.inf)), np.nextafter(t, AU.F(0))
    e = np.array([-1, 0, t, up, down, 2 * t, np.nextafter(2 * t, AU.F(np.inf)), 1.5 * t, 8 * t, 100 * t, np.nan, np.inf, -np.inf, 3e38, 1e-40, -1e-40], AU.F)
    assert AU.reps(e, t, 64).tolist() == [1, 0, 0, 2, 0, 4, 5, 3, 64, 64, 0, 0, 0, 64, 0, 1]
    assert AU.reps(e, t, 3).tolist() == [1, 0, 0, 2, 0, 3, 3, 3, 3, 3, 0, 0, 0, 3, 0, 1]
    assert AU.reps(e, t, 1).tolist() == [1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1]
    lst = np.array([5, 6, 7], np.uint32)
    assert AU.pixel_of(lst, 0, 4, 4, [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32]).tolist() == [5, 6, 7, 5, 5, 5]
    assert AU.pixel_of(lst, 7, 4, 4, [0, 7, 8, 21]).tolist() == [0, 7, 7, 5]


@pytest.mark.parametrize("max_repeat", AU.MAX_REPEATS)
@pytest.mark.parametrize("size", AU.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_selection_equals_the_restatement(pkg, size, max_repeat):
    for seed in range(3):
        e = AU.plane(size, max_repeat, seed)
        got = pkg.capi.adaptive.adaptive_select_host(e, threshold=AU.T, max_repeat=max_repeat)
        want = AU.select(e, AU.T, max_repeat)
        assert not AU.same(*got, *want), (size, max_repeat, seed, got[1], want[1])
        assert got[1]["ms"] == 0.0
    n = size[0] * size[1]
    if n > 3 * 256:
        sp, where = AU.specials(max_repeat), AU.places(n)
        assert len(where) >= 9 and {p % 256 for p in where} >= {0, 63, 64, 255} and n - 1 in where, "three runs: the four lanes (where the run has them) and the last pixel of each"
        assert want[1]["skipped_nonfinite"] > 0 and want[1]["max_rep"] == max_repeat and 0 < want[1]["active"] < n and len(sp) > 20
    below, cap = AU.uniform_planes(size)
    lst, info = pkg.capi.adaptive.adaptive_select_host(below, threshold=AU.T, max_repeat=max_repeat)
    assert lst.size == 0 and info["entries"] == 0 and info["active"] == 0 and info["max_rep"] == 0 and not AU.same(lst, info, *AU.select(below, AU.T, max_repeat))
    lst, info = pkg.capi.adaptive.adaptive_select_host(cap, threshold=AU.T, max_repeat=max_repeat)
    assert info["entries"] == n * max_repeat and info["active"] == n and not AU.same(lst, info, *AU.select(cap, AU.T, max_repeat))


def test_host_mapping_equals_the_restatement(pkg):
    rng = np.random.default_rng(5)
    w, h = 11, 6
    for count in (1, 5, 66, 97):
        lst = rng.integers(0, w * h, count).astype(np.uint32)
        ks = np.concatenate([np.arange(0, 300), np.arange(2 ** 32 - 150, 2 ** 32 + 150), rng.integers(0, 2 ** 32, 200)]).astype(np.uint64)
        for every in (0, 1, 7):
            want = AU.pixel_of(lst, every, w, h, ks)
            got = [pkg.capi.adaptive.adaptive_pixel_host(lst, every, w, h, int(k)) for k in ks]
            assert got == want.tolist(), (count, every)
            if every == 1:
                assert got == [int(k % 2 ** 32) % (w * h) for k in ks]


def test_argument_errors_leave_the_outputs_untouched(pkg):
    capi = pkg.capi
    lib = capi.lib()
    err = AU.plane((8, 4), 3, 0)
    out = np.full(8 * 4 * 3, 0xABABABAB, np.uint32)
    info = capi.adaptive.AdaptiveInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    before = (bytes(info), out.tobytes())
    pe, po = err.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    ok = capi.adaptive.adaptive_params(threshold=AU.T, max_repeat=3)
    bad = [capi.adaptive.adaptive_params(), capi.adaptive.adaptive_params(threshold=-1.0), capi.adaptive.adaptive_params(threshold=float("nan")), capi.adaptive.adaptive_params(threshold=float("inf")),
           capi.adaptive.adaptive_params(threshold=AU.T, max_repeat=0), capi.adaptive.adaptive_params(threshold=AU.T, max_repeat=65)]
    cases = [(None, 8, 4, C.byref(ok), po, out.size, C.byref(info)), (pe, 8, 4, C.byref(ok), po, out.size, None), (pe, 8, 4, None, po, out.size, C.byref(info)),
             (pe, 0, 4, C.byref(ok), po, out.size, C.byref(info)), (pe, 8, 0, C.byref(ok), po, out.size, C.byref(info)),
             (pe, 65536, 65536, C.byref(ok), po, out.size, C.byref(info)), (pe, 16384, 16384, C.byref(ok), po, out.size, C.byref(info)),   # 3 * 2^28 entries
             (pe, 8, 4, C.byref(ok), po, 1, C.byref(info))]                                                                               # too little room
    cases += [(pe, 8, 4, C.byref(b), po, out.size, C.byref(info)) for b in bad]
    for args in cases:
        assert lib.gmupt_adaptive_select_host(*args) == capi.ERR_INVALID_ARGUMENT, args
        assert b"gmupt_adaptive_select_host" in lib.gmupt_last_error()
        assert (bytes(info), out.tobytes()) == before, args
    assert AU.select(err, AU.T, 3)[1]["entries"] > 1, "the case with room for one entry is a refusal"
    # the mapping
    lst = np.array([1, 2, 40], np.uint32)
    pl = lst.ctypes.data_as(C.c_void_p)
    pix = C.c_uint32(77)
    for args in [(None, 3, 0, 8, 4, 0, C.byref(pix)), (pl, 3, 0, 8, 4, 0, None), (pl, 0, 0, 8, 4, 0, C.byref(pix)), (pl, 3, 0, 0, 4, 0, C.byref(pix)),
                 (pl, 3, 0, 65536, 65536, 0, C.byref(pix)), (pl, 3, 0, 8, 4, 2, C.byref(pix))]:      # the last: entry 40 of a 32-pixel rectangle
        assert lib.gmupt_adaptive_pixel_host(*args) == capi.ERR_INVALID_ARGUMENT, args
        assert b"gmupt_adaptive_pixel_host" in lib.gmupt_last_error() and pix.value == 77
    with pytest.raises(TypeError):
        capi.adaptive.adaptive_params(sigma=1.0)
    # the device entry points refuse a missing handle before any device is touched
    h = C.c_void_p(0x1234)
    n = C.c_uint32(77)
    cinfo = capi.ConvergeInfo()
    C.memset(C.byref(cinfo), 0xAB, C.sizeof(cinfo))
    cbefore = bytes(cinfo)
    assert lib.gmupt_adaptive_create(None, C.byref(h)) == capi.ERR_INVALID_ARGUMENT and not h.value
    assert lib.gmupt_adaptive_create(None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_select(None, pe, 8, 4, C.byref(ok), C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_set_list(None, pl, 3, 8, 4, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_adaptive_read_list(None, po, out.nbytes, C.byref(n)) == capi.ERR_INVALID_ARGUMENT and n.value == 77
    assert lib.gmupt_renderer_set_adaptive(None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_render_adaptive(None, None, None, None, None, C.byref(ok), 1, 8, C.byref(n), C.byref(cinfo), C.byref(info)) == capi.ERR_INVALID_ARGUMENT
    assert n.value == 77 and bytes(cinfo) == cbefore and (bytes(info), out.tobytes()) == before
    lib.gmupt_adaptive_destroy(None)


def test_new_symbols_are_declared_bound_and_exported(pkg):
    main = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    header = open(os.path.join(ROOT, "include", "gmupt_adaptive.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    assert "Adaptive sampling" in main and "gmupt_adaptive.h" in main and "uneven counts" in main
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.adaptive.SYMBOLS and name not in pkg.capi.SYMBOLS and getattr(lib, name, None) is not None, name
    assert "Adaptive sampling" in header and "Known bias" in header and "err <= prm.threshold" in header
    assert C.sizeof(pkg.capi.adaptive.AdaptiveParams) == 12 and C.sizeof(pkg.capi.adaptive.AdaptiveInfo) == 32 and pkg.capi.adaptive.AdaptiveInfo.ms.offset == 24
    d = pkg.capi.adaptive.adaptive_params()
    assert (d.threshold, d.max_repeat, d.uniform_every) == (0.0, 1, 0)


# ---- ProgressiveSession.run_until(adaptive=True) on stand-ins: "anything with the same methods"
class _Monitor:
    def __init__(self, converges_at):
        self.converges_at, self.checks, self.resets, self.closed, self.params = converges_at, 0, 0, False, None

    def update(self, error=False, **params):
        self.checks += 1
        self.params = params
        done = self.checks >= self.converges_at
        info = {"pixels": 4, "below": 4 if done else 1, "converged": done, "max_error": 0.0 if done else 1.0}
        return (info, ("plane", self.checks)) if error else info

    def reset(self):
        self.resets += 1
        self.checks = 0

    def close(self):
        self.closed = True


class _Plan:
    def __init__(self):
        self.selected, self.closed = [], False

    def select(self, error, **params):
        self.selected.append((error, params))
        return {"pixels": 4, "active": 3, "entries": 5}

    def close(self):
        self.closed = True


class _Renderer:
    def __init__(self, converges_at):
        self.monitor, self.plan, self.made, self.plans, self.iterations, self.size = _Monitor(converges_at), _Plan(), 0, 0, 0, None
        self.attached, self.log = None, []          # log: per iteration, whether a plan was attached

    def converge(self):
        self.made += 1
        return self.monitor

    def adaptive(self):
        self.plans += 1
        return self.plan

    def set_adaptive(self, plan):
        self.attached = plan

    def set_camera(self, buf):
        pass

    def iterate(self):
        self.iterations += 1
        self.log.append(self.attached is not None)

    def resize(self, w, h):
        self.size = (w, h)

    def bind_scene(self, sb):
        pass

    def refit(self):
        return {"ms": 0.0}


class _Camera:
    class _Buffer:
        lightCount = 0
        iterationCounter = 1

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


class _Closable:
    def close(self):
        pass


class _Scene:
    nodes, tris, verts = _Closable(), _Closable(), _LightBuffer()      # verts: anything with update(array)


def test_session_run_until_adaptive_on_stand_ins(pkg):
    S = pkg.progressive.ProgressiveSession
    r = _Renderer(converges_at=3)
    s = S(r, _Camera(), 8, 8, preview_every=0)
    info = s.run_until(0.01, check_every=4, max_frames=100, min_batches=3, allow_pixels=2, adaptive=True, max_repeat=8, uniform_every=5)
    assert info["converged"] and info["frames"] == 12 and r.made == 1 and r.plans == 1
    assert r.monitor.params == {"threshold": 0.01, "min_batches": 3, "allow_pixels": 2}
    # a plan after each of the two checks that did not end the loop, made from that check's error plane, used by the frames after it
    assert [e for e, _ in r.plan.selected] == [("plane", 1), ("plane", 2)]
    assert r.plan.selected[0][1] == {"threshold": 0.01, "max_repeat": 8, "uniform_every": 5}
    assert r.log == [False] * 4 + [True] * 8 and info["plan"]["entries"] == 5
    assert r.attached is None, "a converged return detaches: the image needs no plan any more"
    # each of the four events that reset the monitor detaches the plan
    def attach():
        r.monitor.converges_at = 99
        s.run_until(0.01, check_every=2, max_frames=2, adaptive=True)
        assert r.attached is r.plan
    s.set_lights(_LightBuffer(), [1, 2], 2)
    assert r.attached is None and r.monitor.resets == 1
    attach()
    s.resize(16, 8)
    assert r.attached is None and r.monitor.resets == 2
    attach()
    s._adopt(_Scene(), _Closable(), _Closable(), None)
    assert r.attached is None and r.monitor.resets == 3
    attach()
    s.set_vertices(_Scene(), np.zeros((3, 3), np.float32))      # upload, refit, restart: _after_vertices
    assert r.attached is None and r.monitor.resets == 4
    # a frame that clears the target detaches; a run_until without `adaptive` does too
    attach()
    s.camera.buffer.iterationCounter = 0
    s.frame()
    assert r.attached is None and r.log[-1] is False
    s.camera.buffer.iterationCounter = 1
    attach()
    n = len(r.plan.selected)
    s.run_until(0.01, check_every=2, max_frames=4)
    assert r.attached is None and len(r.plan.selected) == n and r.log[-4:] == [False] * 4
    # the default is the loop as it was: no plan is made
    q = S(_Renderer(2), _Camera(), 8, 8, preview_every=0)
    assert q.run_until(0.01, check_every=2, max_frames=10)["frames"] == 4 and q.renderer.plans == 0 and q.adaptive is None
    q.close()
    attach()
    s.close()
    assert r.attached is None and r.plan.closed and r.monitor.closed and s.adaptive is None


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, converges_at, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    import gmupt_pkg
    import test_adaptive_cpu as T
    pkg = gmupt_pkg.load()
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = T._Renderer(converges_at[rank])
    s = pkg.progressive.ProgressiveSession(r, T._Camera(), 8, 8, rank=rank, world=world, dist=dist, preview_every=0)
    info = s.run_until(0.01, check_every=2, max_frames=40, adaptive=True, max_repeat=4)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([info["frames"], int(info["converged"]), r.monitor.checks, r.iterations, len(r.plan.selected),
                                                                  sum(r.log)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_plan_their_own_band_and_leave_together(tmp_path, pkg):
    """Rank 0's stand-in converges three checks before rank 1's: both return after rank 1's check, and each has planned its own band
    after every check but the last -- rank 0 also after the checks at which it alone was done."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), (2, 5), str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(str(tmp_path / ("rank%d.npy" % k))).tolist() for k in (0, 1))
    assert a == [10, 1, 5, 10, 4, 8] and b == [10, 1, 5, 10, 4, 8], (a, b)

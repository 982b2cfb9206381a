"""The surface of the thin lens without a device: its header, the structure layout, the exports and the bindings, the argument errors
of the host entry points, and ProgressiveSession.set_lens on stand-ins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lens_util as LU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_lens_default_params", "gmupt_renderer_set_lens", "gmupt_renderer_get_lens", "gmupt_lens_ray_host", "gmupt_lens_focus_at"]


def test_new_symbols_are_declared_bound_and_exported(pkg):
    main = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    header = open(os.path.join(ROOT, "include", "gmupt_lens.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    assert "gmupt_lens.h" in main and "pinhole centre ray" in main
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.lens.SYMBOLS and name not in pkg.capi.SYMBOLS and getattr(lib, name, None) is not None, name
    for words in ("What stays a pinhole", "does NOT clear the frame", "survives gmupt_resize", "6.2831853f", "GMUPT_STAGE_SHADE"):
        assert words in header, words
    L = pkg.capi.lens.Lens
    assert C.sizeof(L) == 8 and L.aperture_radius.offset == 0 and L.focus_distance.offset == 4
    d = pkg.capi.lens.lens_params()
    assert (d.aperture_radius, d.focus_distance) == (0.0, 1.0)
    with pytest.raises(TypeError):
        pkg.capi.lens.lens_params(fstop=2.8)
    sources = open(os.path.join(ROOT, "gmu-path-tracer_amd", "build.py")).read()
    for f in ("csrc/pt_lens.hip", "csrc/pt_lens.cpp", "csrc/gmupt_capi_lens.hip", "csrc/pt_lens.hpp", "../include/gmupt_lens.h"):
        assert '"%s"' % f in sources, f


def test_argument_errors_leave_the_outputs_untouched(pkg):
    capi = pkg.capi
    lib = capi.lib()
    cam = LU.camera(capi, 32, 18, LU.POSES[0])
    cb = cam.buffer_copy()
    cam.close()
    ray = capi.Ray()
    C.memset(C.byref(ray), 0xAB, C.sizeof(ray))
    was = bytes(ray)
    nan, inf = float("nan"), float("inf")
    for a, f in [(nan, 1.0), (inf, 1.0), (-inf, 1.0), (-1e-30, 1.0), (0.1, nan), (0.1, inf), (0.1, 0.0), (0.1, -0.0), (0.1, -2.0)]:
        l = LU.lens_struct(capi, a, f)
        assert lib.gmupt_lens_ray_host(C.byref(cb), C.byref(l), 0, 0, 0, C.byref(ray)) == capi.ERR_INVALID_ARGUMENT, (a, f)
        assert b"gmupt_lens_ray_host" in lib.gmupt_last_error() and bytes(ray) == was
    ok = LU.lens_struct(capi, 0.1, 2.0)
    for args in [(None, C.byref(ok), 0, 0, 0, C.byref(ray)), (C.byref(cb), None, 0, 0, 0, C.byref(ray)), (C.byref(cb), C.byref(ok), 0, 0, 0, None)]:
        assert lib.gmupt_lens_ray_host(*args) == capi.ERR_INVALID_ARGUMENT
    assert bytes(ray) == was
    # aperture 0 is a pinhole whatever the focus says: accepted
    assert lib.gmupt_lens_ray_host(C.byref(cb), C.byref(LU.lens_struct(capi, 0.0, 2.0)), 3, 1, 1, C.byref(ray)) == 0
    assert list(ray.origin) == list(cb.position)[:3]
    # the renderer's entry points refuse a missing handle before any device is touched
    assert lib.gmupt_renderer_set_lens(None, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_renderer_get_lens(None, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert lib.gmupt_lens_focus_at(None, 1.0, 1.0, 0, C.byref(ok)) == capi.ERR_INVALID_ARGUMENT
    assert (ok.aperture_radius, ok.focus_distance) == (np.float32(0.1), 2.0)
    lib.gmupt_lens_default_params(None)


class _Camera:
    class _Buffer:
        lightCount = 2
        iterationCounter = 5

    def __init__(self):
        self.buffer, self.resets = self._Buffer(), 0

    def reset_accumulation(self):
        self.resets += 1


class _Monitor:
    resets = 0

    def reset(self):
        self.resets += 1

    def close(self):
        pass


def test_session_set_lens_is_an_event_that_restarts(pkg, monkeypatch):
    """On stand-ins: the lens reaches the renderer through capi.lens, the camera's accumulation and the monitor restart, the temporal
    history is left alone, and the arguments are checked."""
    L = pkg.capi.lens
    calls = []
    monkeypatch.setattr(L, "set_lens", lambda r, lens: calls.append(("set", r, lens.aperture_radius, lens.focus_distance)))
    monkeypatch.setattr(L, "focus_at", lambda r, px, py, lights, aperture_radius=0.0: calls.append(("focus", px, py, lights)) or L.lens_params(aperture_radius=aperture_radius, focus_distance=9.0))
    renderer, cam = object(), _Camera()
    s = pkg.progressive.ProgressiveSession(renderer, cam, 8, 8, preview_every=0)
    s.converge = _Monitor()

    class _Temporal:
        resets = 0

        def reset(self):
            self.resets += 1

        def close(self):
            pass
    s.temporal = _Temporal()
    lens = s.set_lens(0.25, focus=4.0)
    assert (lens.aperture_radius, lens.focus_distance) == (0.25, 4.0) and calls == [("set", renderer, 0.25, 4.0)]
    assert cam.resets == 1 and s.converge.resets == 1 and s.temporal.resets == 0
    s.set_lens(0.25, focus_at=(3, 4))
    assert calls[1:] == [("focus", 3, 4, 2), ("set", renderer, 0.25, 9.0)] and cam.resets == 2
    s.set_lens(0)
    assert calls[-1] == ("set", renderer, 0.0, 1.0) and cam.resets == 3
    for bad in (dict(), dict(focus=1.0, focus_at=(1, 1))):
        with pytest.raises(ValueError):
            s.set_lens(0.25, **bad)
    assert cam.resets == 3 and len(calls) == 4

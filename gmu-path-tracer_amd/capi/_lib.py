"""The loaded libgmupt.so.  This module alone holds the current library: every call site calls lib() at call time, so that use_build
switches all of them at once."""
import ctypes as C
import os

from .. import build as _build
from ._abi import _EXTRA_SYMBOLS, SYMBOLS, GmuptError

_current = None
_libs = {}
_devices_created = 0   # gmupt_device_create calls of this process (a process that uses the GPU must not spawn a compiler)


def _load(path):
    if path not in _libs:
        handle = C.CDLL(path)
        for name, (res, args) in list(SYMBOLS.items()) + list(_EXTRA_SYMBOLS.items()):
            fn = getattr(handle, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _libs[path] = handle
    return _libs[path]


def lib():
    """Loads libgmupt.so (building it first if the sources are newer).  Fails loudly when it cannot."""
    global _current
    if _current is None:
        path = os.environ.get("GMUPT_LIB") or _build.LIB   # GMUPT_LIB: A/B timing of differently configured builds
        if not os.environ.get("GMUPT_LIB") and (not os.path.exists(path) or (os.path.exists("/opt/rocm/bin/hipcc") and _build.needs_build())):
            path = _build.build()
        _current = _load(path)
    return _current


class use_build:
    """Context manager: inside the block every call of this module goes to a test build of the same sources (build.TEST_BUILDS,
    e.g. "variants" = the library with the whole traversal ladder).  Objects created inside must be closed inside."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _current
        path = _build.lib_path(self.name)
        if not os.path.exists(path) or (os.path.exists("/opt/rocm/bin/hipcc") and _build.needs_build(self.name)):
            if _devices_created:
                # a process that has initialised the GPU must not start hipcc (fork + exec): the GPU box refuses it.  __graft_entry__.build()
                # prebuilds every test build; a stale one is an error here, not something to repair on the fly
                raise GmuptError("test build %r is missing or older than its sources and this process already uses the GPU: run __graft_entry__.build() first" % self.name)
            path = _build.build(name=self.name)
        self.saved = lib()
        _current = _load(path)
        return _current

    def __exit__(self, *exc):
        global _current
        _current = self.saved
        return False


def _check(rc):
    if rc != 0:
        raise GmuptError("gmupt error %d: %s" % (rc, lib().gmupt_last_error().decode(errors="replace")), rc)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)

"""The exported surface of libgmupt.so: every function include/gmupt.h declares resolves in the library, whichever C-API translation
unit (csrc/gmupt_capi*.hip, csrc/gmupt_capi_host.cpp) defines it.  No device involved."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED_BEFORE_THE_SPLIT = 87   # distinct gmupt_\w+( names in include/gmupt.h when gmupt_capi.hip was still one file


def test_every_declared_function_resolves(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    declared = sorted(set(re.findall(r"\b(gmupt_\w+)\(", header)))
    assert len(declared) >= DECLARED_BEFORE_THE_SPLIT, len(declared)
    lib = pkg.capi.lib()
    missing = [name for name in declared if getattr(lib, name, None) is None]
    assert not missing, "libgmupt.so does not export %s" % missing

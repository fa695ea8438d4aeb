"""The switch of the dense assembly at the ABI (no GPU needed): the library exports povar_set_sc_assembly and povar_sc_assembly,
the header declares them, and the ctypes binding has both methods; a null context is an error, not a crash."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_assembly_switch():
    from povar_amd import capi
    capi.build()
    lib = capi.lib()
    text = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("povar_set_sc_assembly", "povar_sc_assembly"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\bint\s+%s\s*\(\s*povar_ctx\s*\*" % name, text), f"{name} is not declared in povar_hip.h"
    assert callable(getattr(capi.Context, "set_sc_assembly", None)) and callable(getattr(capi.Context, "sc_assembly", None))
    assert lib.povar_set_sc_assembly(None, C.c_int32(2)) < 0 and lib.povar_last_error()
    assert lib.povar_sc_assembly(None) < 0

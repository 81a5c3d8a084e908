"""The many-sizes read-out without a GPU (include/lqr_sizes.h): the header declares exactly its three calls, the binding's table equals
the header, the engine exports them, and no other header or table names them."""
import os
import re
import subprocess

import lqr_ctypes as L
import test_imgtype_abi as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_sizes.h")
FUNCS = {
    "lqrx_carver_size_range": dict(ret="gint", args=["LqrCarver*", "gint*", "gint*"]),
    "lqrx_carver_read_sizes_device": dict(ret="LqrRetVal", args=["LqrCarver*", "gint*", "gint", "void**"]),
    "lqrx_carver_read_sizes": dict(ret="LqrRetVal", args=["LqrCarver*", "gint*", "gint", "void**"]),
}
CTYPES_OF = {"LqrCarver*": L.C.c_void_p, "gint*": L.C.POINTER(L.C.c_int), "void**": L.C.POINTER(L.C.c_void_p), "gint": L.C.c_int,
             "LqrRetVal": L.C.c_int}
OTHER_HEADERS = ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h", "lqr_energy.h", "lqr_vmap.h", "lqr_control.h")
OTHER_TABLES = ("SYMBOLS", "COLDEPTH_SYMBOLS", "IMGTYPE_SYMBOLS", "MASK_SYMBOLS", "ENERGY_SYMBOLS", "VMAP_SYMBOLS", "CONTROL_SYMBOLS")


def test_header_declares_exactly_the_three_calls_and_states_the_contract():
    d = IA.declared(HEADER)
    assert d == FUNCS
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src)
    for phrase in ("byte for byte", "pure read", "attached carver", "any order", "multiple of the SAMPLE size", "LQR_ERROR", "LQR_NOMEM",
                   "IMAGE orientation", "delta_max"):
        assert phrase in src, phrase


def test_binding_table_equals_the_header_and_no_other_header_or_table_names_the_calls():
    assert set(L.SIZES_SYMBOLS) == set(FUNCS)
    for name, (res, args) in L.SIZES_SYMBOLS.items():
        assert res == CTYPES_OF[FUNCS[name]["ret"]] and args == [CTYPES_OF[a] for a in FUNCS[name]["args"]], name
        for table in OTHER_TABLES:
            assert name not in getattr(L, table), (table, name)
    for other in OTHER_HEADERS:
        src = open(os.path.join(ROOT, "include", other)).read()
        for name in FUNCS:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")) == sorted(OTHER_HEADERS + ("lqr_hip.h", "lqr_sizes.h"))
    assert all(hasattr(L.Carver, m) for m in ("size_range", "read_sizes", "read_sizes_device"))
    assert callable(L.bind_sizes) and callable(L.engine_sizes_api)


def test_engine_exports_the_three_calls_and_the_shim_call():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in tuple(FUNCS) + ("lqrhip_read_sizes",):
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    api = L.engine_sizes_api()
    assert all(callable(getattr(api, name)) for name in FUNCS)


def test_size_range_of_a_null_carver():
    assert L.engine_sizes_api().lqrx_carver_size_range(None, None, None) == -1

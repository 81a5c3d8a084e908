"""The object-removal surface without a GPU (include_ext/lqr_remove.h): the header declares exactly its two calls and two macros and
compiles as C, the binding's table equals the header, the header is not in include/, the engine exports the calls and the shim's scan
behind them, lqr.h and its symbol table are as they were, and every call refuses bad arguments before any device work."""
import os
import re
import subprocess

import lqr_ctypes as L
import remove_cases as RC
import test_abi as TA
import test_imgtype_abi as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "lqr_remove.h")
FUNCS = {
    "lqrx_carver_discard_scan": dict(ret="LqrRetVal", args=["LqrCarver*", "gint", "gfloat", "gint*", "gint*"]),
    "lqrx_carver_remove_discarded": dict(ret="LqrRetVal", args=["LqrCarver*", "gint", "gfloat", "gint", "gint", "gint*", "gint*", "gint*"]),
}
MACROS = {"LQRX_REMOVE_MIN_STEP": "16", "LQRX_ORIENTATION_AUTO": "(-1)"}
CTYPES_OF = {"LqrCarver*": L.C.c_void_p, "gint*": L.C.POINTER(L.C.c_int), "gint": L.C.c_int, "gfloat": L.C.c_float, "LqrRetVal": L.C.c_int}
SHIM_FUNCS = ("lqrhip_discard_scan", "lqrhip_discard_launches")
OTHER_TABLES = ("SYMBOLS", "COLDEPTH_SYMBOLS", "IMGTYPE_SYMBOLS", "MASK_SYMBOLS", "ENERGY_SYMBOLS", "VMAP_SYMBOLS", "CONTROL_SYMBOLS", "SIZES_SYMBOLS",
                "FORWARD_SYMBOLS", "STATIC_SYMBOLS", "CLIPFORWARD_SYMBOLS")


def test_header_declares_exactly_its_two_calls_and_two_macros_and_states_the_contract():
    assert IA.declared(HEADER) == FUNCS
    src = open(HEADER).read()
    macros = dict(re.findall(r"^#define\s+(LQRX?_\w+)\s+(\S+)\s*$", src, re.M))
    assert macros == MACROS
    assert re.search(r'#include\s+"lqr.h"', src)
    for phrase in ("LOWER BOUND", "PURE READ", "a tie goes to 0", "bit for bit", "LQR_USRCANCEL", "LQR_NOMEM", "L - 2", "SCALEBACK_MODE_LQRBACK",
                   "THE ROUNDS ARE PART OF THE RESULT", "attached carver", "tests/remove_cases.py"):
        assert phrase in src, phrase
    assert RC.MIN_STEP == int(MACROS["LQRX_REMOVE_MIN_STEP"]) == L.LQRX_REMOVE_MIN_STEP
    assert RC.ORIENTATION_AUTO == -1 == L.LQRX_ORIENTATION_AUTO


def test_header_lies_beside_include_and_compiles_as_c_with_both_on_the_path(tmp_path):
    # include/'s list of headers is closed (tests/test_sizes_abi.py): this one has a directory of its own and finds lqr.h through -I
    assert os.path.dirname(HEADER) == os.path.join(ROOT, "include_ext") and not os.path.exists(os.path.join(ROOT, "include", "lqr_remove.h"))
    prog = tmp_path / "use_remove.c"
    prog.write_text('#include "lqr_remove.h"\n'
                    "int main(void) { LqrRetVal (*f)(LqrCarver *, gint, gfloat, gint *, gint *) = lqrx_carver_discard_scan; (void) f;\n"
                    "                 LqrRetVal (*g)(LqrCarver *, gint, gfloat, gint, gint, gint *, gint *, gint *) = lqrx_carver_remove_discarded; (void) g;\n"
                    "                 return LQRX_REMOVE_MIN_STEP + LQRX_ORIENTATION_AUTO - 15; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include_ext"), "-c", str(prog), "-o", str(tmp_path / "use_remove.o")], check=True)


def test_binding_table_equals_the_header_and_no_other_header_or_table_names_the_calls():
    assert set(L.REMOVE_SYMBOLS) == set(FUNCS)
    for name, (res, args) in L.REMOVE_SYMBOLS.items():
        assert res == CTYPES_OF[FUNCS[name]["ret"]] and args == [CTYPES_OF[a] for a in FUNCS[name]["args"]], name
        for table in OTHER_TABLES:
            assert name not in getattr(L, table), (table, name)
    for d in ("include", "include_ext"):
        for other in sorted(os.listdir(os.path.join(ROOT, d))):
            if other == "lqr_remove.h" or other == "lqr_hip.h":
                continue
            src = open(os.path.join(ROOT, d, other)).read()
            for name in FUNCS:
                assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert all(hasattr(L.Carver, m) for m in ("discard_scan", "remove_discarded"))
    assert callable(L.bind_remove) and callable(L.engine_remove_api)


def test_lqr_h_and_its_symbol_table_are_as_they_were():
    assert set(L.SYMBOLS) == set(TA.declared("lqr.h", r"\b(lqrx?_[a-z_0-9]+)\s*\("))
    assert len(L.SYMBOLS) == 62 and not any("discard" in name for name in L.SYMBOLS)


def test_engine_exports_the_two_calls_and_the_shim_calls_and_binds_them():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in tuple(FUNCS) + SHIM_FUNCS:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    declared = TA.declared("lqr_hip.h", r"\b(lqrhip_[a-z_0-9]+)\s*\(")
    assert all(name in declared for name in SHIM_FUNCS)
    api = L.engine_remove_api()
    assert all(callable(getattr(api, name)) for name in FUNCS) and callable(api.lqrhip_discard_launches)


def test_null_and_bad_arguments_are_refused_before_any_device_work(capfd):
    api = L.engine_remove_api()
    m, n = L.C.c_int(-5), L.C.c_int(-5)
    assert api.lqrx_carver_discard_scan(None, 0, 0.0, L.C.byref(m), L.C.byref(n)) == L.LQR_ERROR
    assert api.lqrx_carver_remove_discarded(None, 0, 0.0, 10, 0, None, None, None) == L.LQR_ERROR
    assert (m.value, n.value) == (-5, -5)
    err = capfd.readouterr().err
    assert err.count("lqrx_carver_remove_discarded refused") == 1 and len(err.strip().splitlines()) == 1      # one line (the scan is a read-out: silent)

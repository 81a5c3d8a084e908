"""The static-seam surface without a GPU (include_ext/lqr_static.h): the header declares exactly its five calls and compiles as C with
both include directories on the path, the binding's table equals the header, the engine exports the calls and the shim's calls behind
them, every other header and symbol table is as it was, and NULL arguments are refused before any device work."""
import os
import re
import subprocess

import lqr_ctypes as L
import static_cases as SC
import test_abi as TA
import test_imgtype_abi as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "lqr_static.h")
MAP_ARGS = ["LqrCarver**", "gint", "gint", "gint", "gfloat", "gint", "gfloat"]
FUNCS = {
    "lqrx_carvers_static_energy_device": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "gint", "gfloat", "gfloat*"]),
    "lqrx_carvers_static_energy": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "gint", "gfloat", "gfloat*"]),
    "lqrx_carvers_static_map": dict(ret="LqrVMap*", args=MAP_ARGS),
    "lqrx_carvers_load_static": dict(ret="LqrRetVal", args=MAP_ARGS),
    "lqrx_carvers_resize_static": dict(ret="LqrRetVal", args=MAP_ARGS),
}
CTYPES_OF = {"LqrVMap*": L.C.c_void_p, "gfloat*": L.C.c_void_p, "gint": L.C.c_int, "gfloat": L.C.c_float, "LqrRetVal": L.C.c_int,
             "LqrCarver**": L.C.POINTER(L.C.c_void_p)}
SHIM_FUNCS = ("lqrhip_static_begin", "lqrhip_static_groups", "lqrhip_static_fold", "lqrhip_static_finish", "lqrhip_static_energy",
              "lqrhip_static_release")
OTHER_HEADERS = ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h", "lqr_energy.h", "lqr_vmap.h", "lqr_control.h", "lqr_sizes.h")
OTHER_TABLES = ("SYMBOLS", "COLDEPTH_SYMBOLS", "IMGTYPE_SYMBOLS", "MASK_SYMBOLS", "ENERGY_SYMBOLS", "VMAP_SYMBOLS", "CONTROL_SYMBOLS", "SIZES_SYMBOLS",
                "FORWARD_SYMBOLS")


def test_header_declares_exactly_the_five_calls_and_states_the_contract():
    assert IA.declared(HEADER) == FUNCS
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src) and re.search(r'#include\s+"lqr_vmap.h"', src)
    for phrase in ("bit for bit", "IMAGE orientation", "max_t S_t", "alpha lies in [0, 1]", "LQR_EF_NULL", "bias_factor 2", "ALSO ACCEPTS INITIALISED",
                   "NOT INTERRUPTED", "NO PROGRESS CALLBACKS", "LQR_USRCANCEL", "LQR_NOMEM", "flattened first", "STAY FLATTENED", "no frame is transposed",
                   "attached carver", "65535", "through host memory"):
        assert phrase in src, phrase


def test_header_lies_beside_include_and_compiles_as_c_with_both_on_the_path(tmp_path):
    assert os.path.dirname(HEADER) == os.path.join(ROOT, "include_ext") and not os.path.exists(os.path.join(ROOT, "include", "lqr_static.h"))
    prog = tmp_path / "use_static.c"
    prog.write_text('#include "lqr_static.h"\n'
                    "int main(void) { LqrRetVal (*f)(LqrCarver **, gint, gint, gint, gfloat, gint, gfloat) = lqrx_carvers_load_static; (void) f;\n"
                    "                 LqrVMap *(*g)(LqrCarver **, gint, gint, gint, gfloat, gint, gfloat) = lqrx_carvers_static_map; (void) g;\n"
                    "                 LqrRetVal (*e)(LqrCarver **, gint, gint, gfloat, gfloat *) = lqrx_carvers_static_energy; (void) e; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include_ext"), "-c", str(prog), "-o", str(tmp_path / "use_static.o")], check=True)


def test_binding_table_equals_the_header_and_no_other_header_or_table_names_the_calls():
    assert set(L.STATIC_SYMBOLS) == set(FUNCS)
    for name, (res, args) in L.STATIC_SYMBOLS.items():
        assert res == CTYPES_OF[FUNCS[name]["ret"]] and args == [CTYPES_OF[a] for a in FUNCS[name]["args"]], name
        for table in OTHER_TABLES:
            assert name not in getattr(L, table), (table, name)
    for other in OTHER_HEADERS:
        src = open(os.path.join(ROOT, "include", other)).read()
        for name in FUNCS:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    fwd = open(os.path.join(ROOT, "include_ext", "lqr_forward.h")).read()
    assert not any(re.search(r"\b%s\s*\(" % name, fwd) for name in FUNCS)
    assert all(callable(getattr(L, f)) for f in ("bind_static", "engine_static_api", "static_energy", "static_energy_device", "static_map",
                                                 "load_static", "resize_static"))


def test_lqr_h_and_its_symbol_table_are_as_they_were():
    assert set(L.SYMBOLS) == set(TA.declared("lqr.h", r"\b(lqrx?_[a-z_0-9]+)\s*\("))
    assert len(L.SYMBOLS) == 62 and not any("static" in name for name in L.SYMBOLS)


def test_engine_exports_the_five_calls_and_the_shim_calls_and_binds_them():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in tuple(FUNCS) + SHIM_FUNCS:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    declared = TA.declared("lqr_hip.h", r"\b(lqrhip_[a-z_0-9]+)\s*\(")
    assert all(name in declared for name in SHIM_FUNCS)
    api = L.engine_static_api()
    assert all(callable(getattr(api, name)) for name in FUNCS)


def test_null_arguments_are_refused_before_any_device_work(capfd):
    api = L.engine_static_api()
    assert api.lqrx_carvers_static_energy_device(None, 1, 0, 0.3, None) == L.LQR_ERROR
    assert api.lqrx_carvers_static_energy(None, 1, 0, 0.3, None) == L.LQR_ERROR
    assert not api.lqrx_carvers_static_map(None, 1, 1, 0, 0.3, 1, 0.0)
    assert api.lqrx_carvers_load_static(None, 1, 1, 0, 0.3, 1, 0.0) == L.LQR_ERROR
    assert api.lqrx_carvers_resize_static(None, 1, 3, 3, 0.3, 1, 0.0) == L.LQR_ERROR
    one = (L.C.c_void_p * 1)(None)
    assert api.lqrx_carvers_static_energy(one, 1, 0, 0.3, None) == L.LQR_ERROR                # a NULL frame in the list
    err = capfd.readouterr().err
    assert err.count("refused") == 6 and len(err.strip().splitlines()) == 6                  # one line each


def test_kernel_constants_are_the_ones_the_model_and_the_cases_were_sized_for():
    src = open(os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc", "lqr_common.h")).read()
    K = {name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, src, re.M).group(1)) for name in ("STATIC_TILE", "STATIC_GROUP", "EO_TILE")}
    assert K == dict(STATIC_TILE=SC.TILE, STATIC_GROUP=SC.GROUP, EO_TILE=SC.TILE)
    hip = open(os.path.join(ROOT, "include", "lqr_hip.h")).read()
    assert int(re.search(r"#define\s+LQRHIP_STATIC_MAX_FRAMES\s+(\d+)", hip).group(1)) == 65535
    # the tile and its halo as doubles, the bias tile and the table of v / 255: static LDS, within the 64 KB a workgroup has without an attribute
    assert (SC.TILE + 2) * (SC.TILE + 3) * 8 + SC.TILE * (SC.TILE + 1) * 4 + 256 * 8 <= 64 * 1024

"""The clip's forward-seam surface without a GPU (include_ext/lqr_clipforward.h): the header declares exactly its four calls and compiles
as C with both include directories on the path, the binding's table equals the header, the engine exports the calls and the shim's calls
behind them, every other header and symbol table is as it was, NULL arguments are refused before any device work, and the kernels'
constants are the ones the cases were sized for."""
import os
import re
import subprocess

import clipforward_cases as CC
import lqr_ctypes as L
import test_abi as TA
import test_imgtype_abi as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "lqr_clipforward.h")
FUNCS = {
    "lqrx_clip_forward_map_device": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "gint", "gint", "gfloat", "gint*"]),
    "lqrx_clip_forward_map": dict(ret="LqrVMap*", args=["LqrCarver**", "gint", "gint", "gint", "gfloat"]),
    "lqrx_clip_load_forward": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "gint", "gint", "gfloat"]),
    "lqrx_clip_resize_forward": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "gint", "gint", "gfloat"]),
}
CTYPES_OF = {"LqrVMap*": L.C.c_void_p, "gint*": L.C.c_void_p, "gint": L.C.c_int, "gfloat": L.C.c_float, "LqrRetVal": L.C.c_int,
             "LqrCarver**": L.C.POINTER(L.C.c_void_p)}
SHIM_FUNCS = ("lqrhip_clipfwd_begin", "lqrhip_clipfwd_seams", "lqrhip_clipfwd_finish", "lqrhip_clipfwd_map", "lqrhip_clipfwd_read_map",
              "lqrhip_clipfwd_release", "lqrhip_clipfwd_launches")
OTHER_HEADERS = ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h", "lqr_energy.h", "lqr_vmap.h", "lqr_control.h", "lqr_sizes.h")
OTHER_TABLES = ("SYMBOLS", "COLDEPTH_SYMBOLS", "IMGTYPE_SYMBOLS", "MASK_SYMBOLS", "ENERGY_SYMBOLS", "VMAP_SYMBOLS", "CONTROL_SYMBOLS", "SIZES_SYMBOLS",
                "FORWARD_SYMBOLS", "STATIC_SYMBOLS")


def test_header_declares_exactly_the_four_calls_and_states_the_contract():
    assert IA.declared(HEADER) == FUNCS
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src) and re.search(r'#include\s+"lqr_vmap.h"', src)
    for phrase in ("bit for bit", "IMAGE orientation", "max_t P_t", "temporal * T", "a finite float >= 0", "Ties: up, then left, then right",
                   "ALSO ACCEPTS INITIALISED", "NO PROGRESS CALLBACKS", "LQR_USRCANCEL", "LQR_NOMEM", "flattened first", "STAY FLATTENED",
                   "no frame is transposed", "attached carver", "65535", "16384", "without a trip through the\n * host", "slices\n * of 16 seams"):
        assert phrase in src, phrase


def test_header_lies_beside_include_and_compiles_as_c_with_both_on_the_path(tmp_path):
    assert os.path.dirname(HEADER) == os.path.join(ROOT, "include_ext") and not os.path.exists(os.path.join(ROOT, "include", "lqr_clipforward.h"))
    prog = tmp_path / "use_clipforward.c"
    prog.write_text('#include "lqr_clipforward.h"\n'
                    "int main(void) { LqrRetVal (*f)(LqrCarver **, gint, gint, gint, gfloat) = lqrx_clip_load_forward; (void) f;\n"
                    "                 LqrVMap *(*g)(LqrCarver **, gint, gint, gint, gfloat) = lqrx_clip_forward_map; (void) g;\n"
                    "                 LqrRetVal (*d)(LqrCarver **, gint, gint, gint, gfloat, gint *) = lqrx_clip_forward_map_device; (void) d;\n"
                    "                 LqrRetVal (*r)(LqrCarver **, gint, gint, gint, gfloat) = lqrx_clip_resize_forward; (void) r; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include_ext"), "-c", str(prog), "-o", str(tmp_path / "use_clipforward.o")], check=True)


def test_binding_table_equals_the_header_and_no_other_header_or_table_names_the_calls():
    assert set(L.CLIPFORWARD_SYMBOLS) == set(FUNCS)
    for name, (res, args) in L.CLIPFORWARD_SYMBOLS.items():
        assert res == CTYPES_OF[FUNCS[name]["ret"]] and args == [CTYPES_OF[a] for a in FUNCS[name]["args"]], name
        for table in OTHER_TABLES:
            assert name not in getattr(L, table), (table, name)
    for other in [os.path.join("include", h) for h in OTHER_HEADERS] + [os.path.join("include_ext", h) for h in ("lqr_forward.h", "lqr_static.h")]:
        src = open(os.path.join(ROOT, other)).read()
        for name in FUNCS:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert all(callable(getattr(L, f)) for f in ("bind_clipforward", "engine_clipforward_api", "clip_forward_map", "clip_forward_map_device",
                                                 "clip_load_forward", "clip_resize_forward"))


def test_the_other_tables_are_as_they_were():
    assert set(L.SYMBOLS) == set(TA.declared("lqr.h", r"\b(lqrx?_[a-z_0-9]+)\s*\("))
    assert len(L.SYMBOLS) == 62 and len(L.FORWARD_SYMBOLS) == 5 and len(L.STATIC_SYMBOLS) == 5
    assert not any("clip" in name for table in OTHER_TABLES for name in getattr(L, table))


def test_engine_exports_the_four_calls_and_the_shim_calls_and_binds_them():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in tuple(FUNCS) + SHIM_FUNCS:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    declared = TA.declared("lqr_hip.h", r"\b(lqrhip_[a-z_0-9]+)\s*\(")
    assert all(name in declared for name in SHIM_FUNCS)
    api = L.engine_clipforward_api()
    assert all(callable(getattr(api, name)) for name in FUNCS) and callable(api.lqrhip_clipfwd_launches)


def test_null_arguments_are_refused_before_any_device_work(capfd):
    api = L.engine_clipforward_api()
    api.lqrhip_clipfwd_launches(1)
    assert api.lqrx_clip_forward_map_device(None, 1, 1, 0, 1.0, None) == L.LQR_ERROR
    assert not api.lqrx_clip_forward_map(None, 1, 1, 0, 1.0)
    assert api.lqrx_clip_load_forward(None, 1, 1, 0, 1.0) == L.LQR_ERROR
    assert api.lqrx_clip_resize_forward(None, 1, 3, 3, 1.0) == L.LQR_ERROR
    one = (L.C.c_void_p * 1)(None)
    assert api.lqrx_clip_load_forward(one, 1, 1, 0, 1.0) == L.LQR_ERROR                      # a NULL frame in the list
    assert api.lqrx_clip_resize_forward(one, 1, 3, 3, 1.0) == L.LQR_ERROR
    err = capfd.readouterr().err
    assert err.count("refused") == 6 and len(err.strip().splitlines()) == 6                  # one line each
    assert api.lqrhip_clipfwd_launches(0) == 0


def test_kernel_constants_are_the_ones_the_cases_were_sized_for():
    K = CC.kernel_constants()
    assert K["CLIPFWD_GROUP"] == CC.GROUP == 16 and K["CLIPFWD_REFRESH_THREADS"] % 64 == 0 and K["CLIPFWD_FOLD_THREADS"] == 256
    # the sweep, the walk and the removal are sized as the forward build's: the cases' line lengths and line counts cross those
    assert (K["FWD_THREADS"], K["FWD_MAX_PXT"], K["FWD_WALK_ROWS"], K["FWD_SLICE_SEAMS"]) == (1024, 16, 64, 16)
    assert K["FWD_THREADS"] * K["FWD_MAX_PXT"] == 16384
    names = dict(CC.cases())
    lengths = {FC_line(s)[0] for s in names.values()}
    assert {2, 3, 1023, 1024, 1025, 4097, 8193, 16384} <= lengths
    assert {1, 2, 64, 65, 66, 193} <= {FC_line(s)[1] for s in names.values()}
    assert {1, 2, CC.GROUP, CC.GROUP + 1} <= {s["n"] for s in names.values()}
    hip = open(os.path.join(ROOT, "include", "lqr_hip.h")).read()
    assert int(re.search(r"#define\s+LQRHIP_FORWARD_MAX_LINES\s+(\d+)", hip).group(1)) == 65535
    # the sweep's dynamic LDS at the widest line, with its static LDS (the cone, the path, the pick), fits a workgroup's 160 KB
    assert 2 * 16384 * 4 + K["FWD_WALK_ROWS"] * 2 * K["FWD_WALK_ROWS"] + 4 * K["FWD_WALK_ROWS"] + 8 * (K["FWD_THREADS"] // 64) + 4 <= 160 * 1024


def FC_line(spec):
    import forward_cases as FC
    return FC.line_shape(spec)

"""The forward-energy surface without a GPU (include_ext/lqr_forward.h): the header declares exactly its five calls, the binding's table
equals the header, the engine exports them and the shim's calls behind them, lqr.h and its symbol table are as they were, every call
refuses bad arguments before any device work, and the cases of tests/forward_cases.py cross every boundary of the kernels' constants."""
import os
import re
import subprocess

import forward_cases as FC
import lqr_ctypes as L
import test_abi as TA
import test_imgtype_abi as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "lqr_forward.h")
FUNCS = {
    "lqrx_carver_forward_map_device": dict(ret="LqrRetVal", args=["LqrCarver*", "gint", "gint", "gint*"]),
    "lqrx_carver_forward_map": dict(ret="LqrVMap*", args=["LqrCarver*", "gint", "gint"]),
    "lqrx_carver_forward_maps_device": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "gint", "gint", "gint**"]),
    "lqrx_carver_load_forward": dict(ret="LqrRetVal", args=["LqrCarver*", "gint", "gint"]),
    "lqrx_carver_resize_forward": dict(ret="LqrRetVal", args=["LqrCarver*", "gint", "gint"]),
}
CTYPES_OF = {"LqrCarver*": L.C.c_void_p, "LqrVMap*": L.C.c_void_p, "gint*": L.C.c_void_p, "gint": L.C.c_int, "LqrRetVal": L.C.c_int,
             "LqrCarver**": L.C.POINTER(L.C.c_void_p), "gint**": L.C.POINTER(L.C.c_void_p)}
SHIM_FUNCS = ("lqrhip_forward_begin", "lqrhip_forward_seams", "lqrhip_forward_finish", "lqrhip_forward_map", "lqrhip_forward_read_map",
              "lqrhip_forward_release", "lqrhip_forward_launches", "lqrhip_forward_intensity", "lqrhip_read_forward_intensity")
OTHER_HEADERS = ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h", "lqr_energy.h", "lqr_vmap.h", "lqr_control.h", "lqr_sizes.h")
OTHER_TABLES = ("SYMBOLS", "COLDEPTH_SYMBOLS", "IMGTYPE_SYMBOLS", "MASK_SYMBOLS", "ENERGY_SYMBOLS", "VMAP_SYMBOLS", "CONTROL_SYMBOLS", "SIZES_SYMBOLS")


def test_header_declares_exactly_the_five_calls_and_states_the_contract():
    assert IA.declared(HEADER) == FUNCS
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src) and re.search(r'#include\s+"lqr_vmap.h"', src)
    for phrase in ("bit for bit", "up, then left, then right", "IMAGE orientation", "ALSO ACCEPTS AN INITIALISED CARVER", "warm start",
                   "NO PROGRESS CALLBACKS", "LQR_USRCANCEL", "LQR_NOMEM", "flattened first", "not transposed", "attached carver"):
        assert phrase in src, phrase


def test_header_lies_beside_include_and_compiles_as_c_with_both_on_the_path(tmp_path):
    # include/'s list of headers is closed (tests/test_sizes_abi.py): this one has a directory of its own and finds lqr.h through -I
    assert os.path.dirname(HEADER) == os.path.join(ROOT, "include_ext") and not os.path.exists(os.path.join(ROOT, "include", "lqr_forward.h"))
    prog = tmp_path / "use_forward.c"
    prog.write_text('#include "lqr_forward.h"\n'
                    "int main(void) { LqrRetVal (*f)(LqrCarver *, gint, gint) = lqrx_carver_load_forward; (void) f;\n"
                    "                 LqrVMap *(*g)(LqrCarver *, gint, gint) = lqrx_carver_forward_map; (void) g; return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "include_ext"), "-c", str(prog), "-o", str(tmp_path / "use_forward.o")], check=True)


def test_binding_table_equals_the_header_and_no_other_header_or_table_names_the_calls():
    assert set(L.FORWARD_SYMBOLS) == set(FUNCS)
    for name, (res, args) in L.FORWARD_SYMBOLS.items():
        assert res == CTYPES_OF[FUNCS[name]["ret"]] and args == [CTYPES_OF[a] for a in FUNCS[name]["args"]], name
        for table in OTHER_TABLES:
            assert name not in getattr(L, table), (table, name)
    for other in OTHER_HEADERS:
        src = open(os.path.join(ROOT, "include", other)).read()
        for name in FUNCS:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert all(hasattr(L.Carver, m) for m in ("forward_map", "forward_map_device", "load_forward", "resize_forward", "forward_intensity"))
    assert callable(L.bind_forward) and callable(L.engine_forward_api) and callable(L.forward_maps_device)


def test_lqr_h_and_its_symbol_table_are_as_they_were():
    assert set(L.SYMBOLS) == set(TA.declared("lqr.h", r"\b(lqrx?_[a-z_0-9]+)\s*\("))
    assert len(L.SYMBOLS) == 62 and not any("forward" in name for name in L.SYMBOLS)


def test_engine_exports_the_five_calls_and_the_shim_calls_and_binds_them():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in tuple(FUNCS) + SHIM_FUNCS:
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    declared = TA.declared("lqr_hip.h", r"\b(lqrhip_[a-z_0-9]+)\s*\(")
    assert all(name in declared for name in SHIM_FUNCS)
    api = L.engine_forward_api()
    assert all(callable(getattr(api, name)) for name in FUNCS)
    assert callable(api.lqrhip_forward_launches) and callable(api.lqrhip_read_forward_intensity)


def test_null_arguments_are_refused_before_any_device_work(capfd):
    api = L.engine_forward_api()
    assert api.lqrx_carver_forward_map_device(None, 1, 0, None) == L.LQR_ERROR
    assert not api.lqrx_carver_forward_map(None, 1, 0)
    assert api.lqrx_carver_forward_maps_device(None, 0, 1, 0, None) == L.LQR_ERROR
    assert api.lqrx_carver_load_forward(None, 1, 0) == L.LQR_ERROR
    assert api.lqrx_carver_resize_forward(None, 3, 3) == L.LQR_ERROR
    err = capfd.readouterr().err
    assert err.count("refused") == 4 and len(err.strip().splitlines()) == 4      # one line each (resize_forward of NULL has none to name)


def test_kernel_constants_are_the_ones_the_cases_were_sized_for():
    K = FC.kernel_constants()
    assert K == dict(FWD_THREADS=1024, FWD_MAX_PXT=16, FWD_WALK_ROWS=64, FWD_REMOVE_THREADS=256, FWD_REMOVE_PX=4, LDS_ATTR_BYTES=65536,
                     FWD_SLICE_SEAMS=16)
    assert K["FWD_THREADS"] * K["FWD_MAX_PXT"] == 16384          # LQRHIP_MAX_FRAME_WIDTH: the widest line has a form
    assert int(re.search(r"#define\s+LQRHIP_MAX_FRAME_WIDTH\s+(\d+)", open(os.path.join(ROOT, "include", "lqr_hip.h")).read()).group(1)) == 16384
    assert 2 * 16384 * 4 + 16 * 1024 <= 160 * 1024               # the two rows of M and the kernel's static LDS fit a compute unit's


def test_cases_cross_every_boundary_of_the_kernels():
    K = FC.kernel_constants()
    crossed = {}
    for name, spec in FC.cases():
        if spec["pre"] is None:
            for b in FC.boundaries(spec, K):
                crossed.setdefault(b, []).append(name)
    B = K["FWD_WALK_ROWS"]
    # every form of the sweep the committed sizes reach, each at the first length that needs it; the LDS attribute; the walk with no
    # block, one, a full one, one of a single row, several; a removal of several rounds; a build of several slices; both extreme depths
    for need in ("pxt1", "pxt1_edge", "pxt2", "pxt2_edge", "pxt4", "pxt4_edge", "pxt8", "pxt8_edge", "pxt16", "pxt16_edge", "lds_attr", "lds_max", "walk_blocks_0",
                 "walk_blocks_1", "walk_blocks_many", "walk_block_full", "walk_block_of_one_row", "remove_rounds_many", "slices_many",
                 "depth_max", "depth_1"):
        assert crossed.get(need), need
    lines = {FC.line_shape(spec) for _, spec in FC.cases() if spec["pre"] is None}
    assert {L_ for L_, H in lines if H <= 8} >= {2, 3, 63, 64, 65, 1023, 1025, 4096, 4097, 8193, 16384}
    by_name = dict(FC.cases())
    assert {by_name[n]["o"] for n in crossed["lds_max"]} == {0, 1}          # the widest line, read along the rows and across them
    assert {H for L_, H in lines if L_ <= 70} >= {1, 2, B - 1, B, B + 1, 3 * B + 1}
    # both orientations, every pixel kind the issue names, both signs of the bias, both states beforehand
    specs = [s for _, s in FC.cases()]
    assert {s["o"] for s in specs} == {0, 1} and {s["pre"] for s in specs} == {None, "transposed", "notflat"}
    assert {(s["ch"], s["depth"]) for s in specs} >= {(1, 0), (2, 0), (3, 0), (4, 0), (3, 1), (4, 2)}
    assert any(s["type"] == FC.IT.CMYK for s in specs) and any(FC.is_luma(s) for s in specs)
    assert any((s["bias"] or 0) > 0 for s in specs) and any((s["bias"] or 0) < 0 for s in specs)
    assert {s["content"] for s in specs} == {"grey4", "flat", "float"}

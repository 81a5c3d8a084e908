"""The carver-control calls without a GPU: include/lqr_control.h against liblqr 0.4.1's own prototypes and enum values
(tests/golden/ref/abi.json), the binding's table against the header, and the engine's exports."""
import ctypes as C
import os
import re
import subprocess

import lqr_ctypes as L
import test_coldepth_abi as CA
import test_imgtype_abi as IA
import test_masks_abi as MA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_control.h")
ABI = CA.ABI
LIBLQR_FUNCS = ("lqr_carver_cancel", "lqr_carver_set_use_cache", "lqr_carver_set_no_dump_vmaps", "lqr_carver_list_foreach",
                "lqr_carver_list_foreach_recursive", "lqr_carver_set_gradient_function")
EXT_FUNCS = {
    "lqrx_carver_cancelled": dict(ret="gint", args=["LqrCarver*"]),
    "lqrx_carver_cancel_clear": dict(ret="LqrRetVal", args=["LqrCarver*"]),
}
CTYPES_OF = dict(MA.CTYPES_OF, **{"LqrCarverList*": C.c_void_p, "LqrCarverFunc": L.CARVER_FUNC, "LqrDataTok": L.DATA_TOK, "gboolean": C.c_int,
                                  "LqrGradFuncType": C.c_int, "void": None})


def test_header_declares_liblqrs_six_prototypes_and_the_two_extensions():
    d = IA.declared(HEADER)
    assert set(d) == set(LIBLQR_FUNCS) | set(EXT_FUNCS)
    for name in LIBLQR_FUNCS:
        assert name in ABI["functions"] and d[name] == ABI["functions"][name], name
    for name, proto in EXT_FUNCS.items():
        assert d[name] == proto, name
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src)
    for phrase in ("ANY thread", "NO EFFECT", "attach order", "LQR_USRCANCEL", "last COMPLETED session", "lqrx_carver_cancel_clear", "WITHOUT one"):
        assert phrase in src, phrase


def test_enum_values_and_the_callback_and_token_types_are_liblqrs():
    src = CA._strip_comments(open(HEADER).read())
    m = re.search(r"typedef enum _LqrGradFuncType \{(.*?)\} LqrGradFuncType;", src, re.S)
    members = [re.match(r"(\w+)\s*=\s*(\d+)$", x.strip()).groups() for x in m.group(1).split(",") if x.strip()]
    assert [(n, int(v)) for n, v in members] == [(n, i) for i, n in enumerate(ABI["enums"]["LqrGradFuncType"])]
    assert re.search(r"typedef LqrRetVal \(\*LqrCarverFunc\)\s*\(LqrCarver \*\w+, LqrDataTok \w+\);", src)
    # liblqr's token: a union of a carver, a gint and a pointer -- one word, which is how the binding passes it
    m = re.search(r"typedef union _LqrDataTok \{(.*?)\} LqrDataTok;", src, re.S)
    assert [re.sub(r"\s+", " ", x.strip()) for x in m.group(1).split(";") if x.strip()] == ["LqrCarver *carver", "gint integer", "gpointer data"]
    assert ABI["functions"]["lqr_carver_list_foreach"]["args"][2] == "LqrDataTok"


def test_size_of_the_token_is_one_pointer(tmp_path):
    prog = tmp_path / "tok.c"
    prog.write_text('#include <stdio.h>\n#include "lqr_control.h"\nint main(void) { LqrDataTok t; t.data = 0; t.integer = 7;\n'
                    '    printf("%u %u %d %d\\n", (unsigned) sizeof(LqrDataTok), (unsigned) sizeof(void *), t.integer, (int) LQR_GF_NULL); return 0; }\n')
    exe = str(tmp_path / "tok")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(prog), "-o", exe], check=True)
    size, ptr, seven, gf_null = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert size == ptr == C.sizeof(L.DATA_TOK) and seven == 7 and gf_null == 5


def test_binding_table_equals_the_header_and_the_other_headers_and_tables_stay_as_they_were():
    d = IA.declared(HEADER)
    assert set(L.CONTROL_SYMBOLS) == set(d)
    for name, (res, args) in L.CONTROL_SYMBOLS.items():
        assert res == CTYPES_OF[d[name]["ret"]] and args == [CTYPES_OF[a] for a in d[name]["args"]], name
        for table in (L.SYMBOLS, L.COLDEPTH_SYMBOLS, L.IMGTYPE_SYMBOLS, L.MASK_SYMBOLS, L.ENERGY_SYMBOLS, L.VMAP_SYMBOLS):
            assert name not in table, name
    for other in ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h", "lqr_energy.h", "lqr_vmap.h"):
        src = open(os.path.join(ROOT, "include", other)).read()
        for name in d:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert (L.LQR_GF_NORM, L.LQR_GF_NORM_BIAS, L.LQR_GF_SUMABS, L.LQR_GF_XABS, L.LQR_GF_YABS, L.LQR_GF_NULL) == tuple(range(6))
    for m in ("cancel", "cancelled", "cancel_clear", "cancel_at_update", "set_use_cache", "set_no_dump_vmaps", "set_gradient_function", "list_foreach"):
        assert hasattr(L.Carver, m), m
    assert callable(L.bind_control)


def test_engine_exports_the_six_symbols_and_the_extensions():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in LIBLQR_FUNCS + tuple(EXT_FUNCS):
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    # with these six, the only public liblqr 0.4.1 function the engine does not export is the custom energy
    public = [n for n in ABI["functions"] if n.startswith("lqr_") and not n.endswith("_attached")]
    exported = set(re.findall(r"\bT (lqr_\w+)$", syms, re.M))
    headers = "".join(open(os.path.join(ROOT, "include", h)).read() for h in os.listdir(os.path.join(ROOT, "include")))
    missing = [n for n in public if re.search(r"\b%s\s*\(" % n, headers) is None]
    assert all(n in exported for n in LIBLQR_FUNCS) and "lqr_carver_set_energy_function" in missing

"""The image-type surface without a GPU: include/lqr_imagetype.h against liblqr 0.4.1's own prototypes (tests/golden/ref/abi.json),
tests/c/cmyka_replay.c compiled with -Werror against it, the engine's exports, the channel limit, the soundness of the
genuine-code vectors under tests/golden/imgtype/, and the numpy model of the value the energy reads (tests/imgtype_cases.py) against
the genuine lqr_carver_read_brightness / lqr_carver_read_luma, bit for bit -- what the identity tests of
tests/test_imgtype_gpu.py rest on."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import coldepth_cases as CD
import imgtype_cases as IT
import lqr_ctypes as L
import test_coldepth_abi as CA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_imagetype.h")
ABI = CA.ABI
GOLD = os.path.join(ROOT, "tests", "golden", "imgtype")
LIBLQR_FUNCS = ("lqr_carver_set_image_type", "lqr_carver_set_alpha_channel", "lqr_carver_set_black_channel")
FUNCS = LIBLQR_FUNCS + ("lqrx_set_max_channels",)
MAX_FILE = IT.MAX_FILE                  # the largest golden file committed before these
MAN = json.load(open(os.path.join(GOLD, "MANIFEST.json")))


def declared(path):
    src = re.sub(r"^\s*#.*$", "", CA._strip_comments(open(path).read()), flags=re.M)       # (no preprocessor lines)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(lqrx?_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src):
        ret = re.sub(r"\s+", "", m.group(1))
        args = [] if m.group(3).strip() in ("", "void") else [CA._type_of(a) for a in m.group(3).split(",")]
        out[m.group(2)] = dict(ret=ret, args=args)
    return out


def engine_lib():
    if not os.path.exists(L.ENGINE_LIB):
        import __graft_entry__ as g
        g.build()
    return L.ENGINE_LIB


def test_header_declares_exactly_the_four_calls_with_liblqrs_prototypes():
    d = declared(HEADER)
    assert set(d) == set(FUNCS)
    for name in LIBLQR_FUNCS:
        assert d[name] == ABI["functions"][name], name
    assert d["lqrx_set_max_channels"] == dict(ret="gint", args=["gint"])
    assert re.search(r'#include\s+"lqr_coldepth.h"', open(HEADER).read())


def test_the_other_headers_and_symbol_tables_stay_as_they_were():
    lqr_h = open(os.path.join(ROOT, "include", "lqr.h")).read()
    assert set(declared(os.path.join(ROOT, "include", "lqr_coldepth.h"))) == set(CA.FUNCS)
    for name in FUNCS:
        assert not re.search(r"\b%s\s*\(" % name, lqr_h), name
        assert name not in L.SYMBOLS and name not in L.COLDEPTH_SYMBOLS
        assert name in L.IMGTYPE_SYMBOLS
    assert set(L.IMGTYPE_SYMBOLS) == set(FUNCS)
    assert len(L.COLDEPTH_SYMBOLS) == 8 and set(L.COLDEPTH_SYMBOLS) == set(CA.FUNCS)


def test_engine_exports_the_image_type_calls():
    syms = subprocess.run(["nm", "-D", "--defined-only", engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in FUNCS + ("lqrhip_carver_set_read",):
        assert re.search(r"\bT %s$" % name, syms, re.M), name


@pytest.mark.parametrize("glib", [False, True])
def test_cmyka_replay_compiles_with_werror_against_both_headers(tmp_path, glib):
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "c", "cmyka_replay.c"), "-o", str(tmp_path / "cmyka_replay.o")]
    if glib:
        hdr = tmp_path / "glib_standin.h"
        hdr.write_text("typedef int gint; typedef unsigned int guint; typedef unsigned char guchar; typedef char gchar;\n"
                       "typedef float gfloat; typedef double gdouble; typedef int gboolean; typedef void *gpointer;\n")
        cmd[1:1] = ["-DLQR_NO_GLIB_TYPEDEFS", "-include", str(hdr)]
    subprocess.run(cmd, check=True)


def test_channel_limit_range_return_value_and_default():
    """in a process of its own (the limit is process-wide): the default refuses five channels before any device work and says which
    limit is in force; values outside 4 .. 64 are refused; the previous value comes back either way"""
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.lqr_carver_new_ext.restype = ctypes.c_void_p
lib.lqr_carver_new_ext.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
lib.lqr_carver_new.restype = ctypes.c_void_p
lib.lqr_carver_new.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
buf = (ctypes.c_double * 4096)()
assert not lib.lqr_carver_new_ext(buf, 4, 4, 5, 2)
assert not lib.lqr_carver_new(buf, 4, 4, 5)
s = lib.lqrx_set_max_channels
assert s(3) == 4 and s(65) == 4 and s(-1) == 4 and s(0) == 4
assert s(4) == 4 and s(64) == 4 and s(200) == 64 and s(9) == 64 and s(9) == 9
assert not lib.lqr_carver_new_ext(buf, 4, 4, 10, 0)
assert not lib.lqr_carver_new_ext(buf, 4, 4, 5, 4)
assert s(4) == 9
assert not lib.lqr_carver_new_ext(buf, 4, 4, 5, 2)
"""
    r = subprocess.run([sys.executable, "-c", code, engine_lib()],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stderr.splitlines() if "channels" in ln]
    assert any("1 .. 4 channels" in ln for ln in lines) and any("1 .. 9 channels" in ln for ln in lines), r.stderr
    assert all("lqrx_set_max_channels" in ln for ln in lines)


# ---- the vectors --------------------------------------------------------------------------------------------------------------
def test_manifest_lists_every_vector_with_its_checksum_and_size_limits():
    listed = MAN["vectors"] + MAN["mid"]
    files = {v["file"] for v in listed}
    assert files == {f for f in os.listdir(GOLD) if f.endswith(".npz")}
    assert len(files) == len(listed)
    assert [v["name"] for v in MAN["vectors"]] == [n for n, _ in IT.cases()]
    assert [v["name"] for v in MAN["mid"]] == [n for n, _ in IT.mid_cases()]
    for v, (_, spec) in zip(listed, IT.cases() + IT.mid_cases()):
        assert v["spec"] == json.loads(json.dumps(spec)), v["name"]
        data = open(os.path.join(GOLD, v["file"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"], v["file"]
        assert len(data) <= MAX_FILE, v["file"]
        assert v["heap"] == [0, 0], v["name"]
        assert v["rets"] == [1] * len(v["spec"]["steps"]), v["name"]
        assert v["same_as_shipped"] in (True, False)
        if v["spec"].get("preserve"):
            assert v["input_unchanged"] is True, v["name"]
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD)) < 8 << 20


def test_small_vectors_cover_the_matrix():
    specs = dict(IT.cases())
    assert all(s["w"] <= 56 and s["h"] <= 44 for s in specs.values())
    for depth in (0, 1, 2, 3):
        d = CD.DEPTH_NAMES[depth]
        for lname, ch, _ in IT.LAYOUTS:
            mine = [s for n, s in specs.items() if n.startswith("%s_%s_e" % (lname, d))]
            assert len(mine) == 2 and all(s["ch"] == ch and s["depth"] == depth for s in mine), (lname, d)
            assert sorted(s["nrg"] in (3, 4, 5) for s in mine) == [False, True], (lname, d)
        assert "interactive_%s" % d in specs
    states = {n: IT.state_of(s) for n, s in specs.items()}
    keys = {st.key() for st in states.values()}
    assert {(IT.CMY, -1, -1), (IT.CMYK, -1, 3), (IT.CMYKA, 4, 3), (IT.CUSTOM, -1, -1), (IT.CUSTOM, 1, -1), (IT.CUSTOM, -1, 8),
            (IT.CUSTOM, 5, 2), (IT.CUSTOM, -1, 4), (IT.CUSTOM, 3, -1)} <= keys
    every = list(specs.values())
    assert any(s.get("bias") and s.get("rigmask") for s in every)
    assert {s.get("delta", 1) for s in every} >= {1, 2, 5}
    assert {s.get("res_order", 0) for s in every} == {0, 1}
    assert any(s.get("preserve") for s in every) and any(s.get("edge") and s["depth"] >= 2 for s in every)
    assert any(s.get("enl_step") == 1.3 for s in every) and any(st != "flatten" and st[0] > s["w"] for s in every for st in s["steps"])
    assert {s["aux_ch"] for s in every if s.get("aux_depth") is not None} == {5, 7}
    # seams per direction and step
    for n, s in specs.items():
        w, h = s["w"], s["h"]
        for st in s["steps"]:
            if st != "flatten" and s.get("enl_step") != 1.3:
                assert abs(st[0] - w) <= 12 and abs(st[1] - h) <= 12, n
                w, h = st


def test_setter_returns_and_types_follow_the_rules_on_every_vector():
    """what the genuine setters returned and the type they left, call by call, is what imgtype_cases.TypeState (the rules
    lqr_imagetype.h documents) says; so are the defaults by channel count"""
    refused = 0
    for v in MAN["vectors"] + MAN["mid"]:
        spec = v["spec"]
        st = IT.TypeState(spec["ch"])
        assert v["default_type"] == st.type, v["name"]
        want = []
        for op in IT.initial_ops(spec) + [op for at, op in spec.get("type_at", []) if at > 0]:
            ret = st.apply(op)
            refused += ret == 0
            want.append([ret, st.type])
        assert want == v["type_rets"], v["name"]
        z = np.load(os.path.join(GOLD, v["file"]))
        rec = json.loads(str(z["record"]))
        if spec.get("aux_depth") is not None:
            sa = IT.TypeState(spec["aux_ch"])
            assert rec["aux_default_type"] == sa.type
            assert rec["aux_type_rets"] == [[sa.apply(op), sa.type] for op in spec["aux_ops"]], v["name"]
    assert refused >= 6
    assert {IT.TypeState(ch).type for ch in (1, 2, 3, 4, 5, 6, 7, 9)} == {IT.GREY, IT.GREYA, IT.RGB, IT.RGBA, IT.CMYKA, IT.CUSTOM}


def test_numpy_model_equals_the_genuine_read_planes_bit_for_bit():
    with_planes = [v for v in MAN["vectors"] if v["read_planes"]]
    assert [v["name"] for v in with_planes] == sorted(IT.PLANE_CASES, key=[n for n, _ in IT.cases()].index) and len(with_planes) >= 12
    seen = set()
    for v in with_planes:
        z = np.load(os.path.join(GOLD, v["file"]))
        st = IT.state_of(v["spec"])
        seen.add((v["spec"]["depth"], st.type == IT.CUSTOM, st.alpha >= 0, st.black >= 0))
        for luma, key in ((False, "in_read_bright"), (True, "in_read_luma")):
            got = IT.model_value(z["img"], v["spec"]["depth"], st, luma)
            assert got.dtype == np.float64 and z[key].dtype == np.float64 and got.shape == z[key].shape
            assert np.array_equal(got.view(np.uint64), z[key].view(np.uint64)), (v["name"], key)
    assert {d for d, *_ in seen} == {0, 1, 2, 3}
    assert {(c, a, k) for _, c, a, k in seen} >= {(False, False, False), (False, False, True), (False, True, True), (True, False, False),
                                                   (True, True, False), (True, False, True), (True, True, True)}


def test_mid_vectors_cross_the_boundaries_of_the_new_code_and_the_small_ones_none():
    K = CA.kernel_constants()
    lag1 = K["FROZEN_LAG_MAX"] // 4
    mid = dict(IT.mid_cases())
    lab = {n: IT.boundaries(s, K) for n, s in mid.items()}
    for lname, px in (("cmyka_8i", 5), ("custom7_8i", 7), ("cmyka_16i", 10), ("cmyka_32f", 20), ("custom6_64f", 48)):
        for k, chunks in ((2, 2), (3, 3)):
            got = lab["all%d_%s" % (k, lname)]
            assert (mid["all%d_%s" % (k, lname)]["w"], mid["all%d_%s" % (k, lname)]["h"]) == (
                (340, 12) if k == 2 else (600, 6) if px == 48 else (600, 12))       # 600 x 6: imgtype_cases.mid_cases says why
            want = {"shrink:c%d" % chunks, "relayout:c%d" % chunks, "flatten:c%d" % chunks, "readout:c%d" % chunks, "enlarge:c%d" % chunks,
                    "inflate:b%d" % px, "compact:b%d" % px, "seams>%d" % lag1, "catchup:c%d" % chunks}
            assert want <= got, (lname, k, sorted(want - got))
    assert "transpose:b5" in lab["enlv_cmyka_8i"] and "transpose:b14" in lab["enlv_custom7_16i"]
    assert {"rows:b3", "seams>%d" % lag1, "catchup:c1"} <= lab["tall_cmyk_8i"] and mid["tall_cmyk_8i"]["depth"] == 0
    # the 8I instantiations are reached by 8I specs that read through the value plane
    for n in ("all2_cmyka_8i", "all3_cmyka_8i", "all2_custom7_8i", "all3_custom7_8i", "enlv_cmyka_8i", "tall_cmyk_8i"):
        assert mid[n]["depth"] == 0 and IT.reads_value(mid[n], IT.state_of(mid[n]))
    small = set()
    for _, spec in IT.cases():
        small |= IT.boundaries(spec, K)
    assert small and all(x.endswith(":c1") or x in ("rows:b1", "ragged", "nt12", "nt36") for x in small), small


def test_files_stay_within_the_limits():
    for f in os.listdir(GOLD):
        assert os.path.getsize(os.path.join(GOLD, f)) <= MAX_FILE, f

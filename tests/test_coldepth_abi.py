"""The colour-depth surface without a GPU: include/lqr_coldepth.h against liblqr 0.4.1's own prototypes and enum values
(tests/golden/ref/abi.json), tests/c/float_replay.c compiled with -Werror against it, the engine's exports, and the
soundness of the genuine-code vectors under tests/golden/coldepth/."""
import hashlib
import json
import os
import re
import subprocess

import pytest

import lqr_ctypes as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_coldepth.h")
ABI = json.load(open(os.path.join(ROOT, "tests", "golden", "ref", "abi.json")))
GOLD = os.path.join(ROOT, "tests", "golden", "coldepth")
FUNCS = ("lqr_carver_new_ext", "lqr_carver_scan_ext", "lqr_carver_scan_line_ext", "lqr_carver_scan", "lqr_carver_get_col_depth",
         "lqr_carver_get_image_type", "lqr_carver_get_bpp", "lqr_carver_set_preserve_input_image")


def _strip_comments(s):
    return re.sub(r"/\*.*?\*/", "", s, flags=re.S)


def _type_of(decl):
    """'LqrCarver *r' -> 'LqrCarver*', 'void **rgb' -> 'void**'"""
    decl = decl.strip()
    m = re.match(r"^(.*?)([A-Za-z_][A-Za-z_0-9]*)$", decl)
    t = m.group(1) if m and m.group(1).strip() else decl
    return re.sub(r"\s+", "", t.replace("const", ""))


def declared():
    src = _strip_comments(open(HEADER).read())
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(lqrx?_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src):
        ret = re.sub(r"\s+", "", m.group(1))
        args = [] if m.group(3).strip() in ("", "void") else [_type_of(a) for a in m.group(3).split(",")]
        out[m.group(2)] = dict(ret=ret, args=args)
    return out


def test_header_declares_exactly_the_colour_depth_calls_with_liblqrs_prototypes():
    d = declared()
    assert set(d) == set(FUNCS)
    for name in FUNCS:
        assert d[name] == ABI["functions"][name], name


def test_header_enums_have_liblqrs_members_and_values():
    src = _strip_comments(open(HEADER).read())
    for enum in ("LqrColDepth", "LqrImageType"):
        body = re.search(r"typedef\s+enum\s+_%s\s*\{(.*?)\}\s*%s\s*;" % (enum, enum), src, re.S).group(1)
        members = [(n, int(v)) for n, v in re.findall(r"(LQR_[A-Z0-9_]+)\s*=\s*(\d+)", body)]
        assert members == [(n, i) for i, n in enumerate(ABI["enums"][enum])], enum


def test_lqr_h_and_the_symbol_table_stay_as_they_were():
    """the plug-in's surface does not grow: the colour-depth calls live in their own header and table"""
    lqr_h = open(os.path.join(ROOT, "include", "lqr.h")).read()
    for name in FUNCS:
        assert not re.search(r"\b%s\s*\(" % name, lqr_h), name
        assert name not in L.SYMBOLS
        assert name in L.COLDEPTH_SYMBOLS


def test_engine_exports_the_colour_depth_calls():
    if not os.path.exists(L.ENGINE_LIB):
        import __graft_entry__ as g
        g.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", L.ENGINE_LIB], capture_output=True, text=True, check=True).stdout
    for name in FUNCS + ("lqrhip_carver_create_ext", "lqrhip_carver_set_read_luma"):
        assert re.search(r"\bT %s$" % name, syms, re.M), name


@pytest.mark.parametrize("glib", [False, True])
def test_float_replay_compiles_with_werror_against_both_headers(tmp_path, glib):
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "c", "float_replay.c"), "-o", str(tmp_path / "float_replay.o")]
    if glib:        # the header under a GLib stand-in, as tests/test_c_replay.py builds the plug-in's replay
        hdr = tmp_path / "glib_standin.h"
        hdr.write_text("typedef int gint; typedef unsigned int guint; typedef unsigned char guchar; typedef char gchar;\n"
                       "typedef float gfloat; typedef double gdouble; typedef int gboolean; typedef void *gpointer;\n")
        cmd[1:1] = ["-DLQR_NO_GLIB_TYPEDEFS", "-include", str(hdr)]
    subprocess.run(cmd, check=True)


def test_manifest_lists_every_vector_with_its_checksum_and_size_limits():
    man = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
    files = {v["file"] for v in man["vectors"]}
    on_disk = {f for f in os.listdir(GOLD) if f.endswith(".npz")}
    assert files == on_disk
    assert len(files) == len(man["vectors"])
    for v in man["vectors"]:
        path = os.path.join(GOLD, v["file"])
        data = open(path, "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"], v["file"]
        assert len(data) < 512 * 1024, v["file"]
        assert v["heap"] == [0, 0], v["name"]                     # the genuine code's heap check was clean
        if v["spec"].get("preserve"):
            assert v["input_unchanged"] is True, v["name"]        # ... and it neither wrote nor freed a preserved buffer
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD)) < 8 << 20


def test_vectors_cover_every_depth_channel_count_and_energy():
    import coldepth_cases as CD
    man = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
    assert [v["name"] for v in man["vectors"]] == [n for n, _ in CD.cases()]
    specs = [v["spec"] for v in man["vectors"]]
    for depth in (1, 2, 3):
        mine = [s for s in specs if s["depth"] == depth]
        assert {s["ch"] for s in mine} == {1, 2, 3, 4}
        assert {s["nrg"] for s in mine} == set(range(7))
        assert any(s.get("preserve") for s in mine) and any(not s.get("preserve") for s in mine)
        assert any(s.get("edge") for s in mine) and any(s.get("bias") and s.get("rigmask") for s in mine)
        assert {s.get("delta", 1) for s in mine} >= {1, 2, 5}
    assert any(s.get("aux_depth") is not None and s["aux_depth"] != s["depth"] for s in specs)


def test_a_wrong_depth_or_channel_count_is_refused_before_any_device_work():
    """lqr_carver_new_ext checks its arguments first: no GPU is needed to see NULL"""
    if not os.path.exists(L.ENGINE_LIB):
        import __graft_entry__ as g
        g.build()
    import ctypes
    lib = ctypes.CDLL(L.ENGINE_LIB)
    lib.lqr_carver_new_ext.restype = ctypes.c_void_p
    lib.lqr_carver_new_ext.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    buf = (ctypes.c_double * 64)()
    assert not lib.lqr_carver_new_ext(buf, 4, 4, 5, 2)
    assert not lib.lqr_carver_new_ext(buf, 4, 4, 3, 4)
    assert not lib.lqr_carver_new_ext(buf, 4, 4, 3, -1)


# ---- the mid-size vectors (tests/golden/coldepth_mid/) and the boundaries they cross ------------------------------------------
MID = os.path.join(ROOT, "tests", "golden", "coldepth_mid")
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")


def test_mid_manifest_lists_every_vector_with_its_checksum_and_size_limits():
    import coldepth_cases as CD
    man = json.load(open(os.path.join(MID, "MANIFEST.json")))
    listed = man["vectors"] + man["planes"]
    files = {v["file"] for v in listed}
    assert files == {f for f in os.listdir(MID) if f.endswith(".npz")}
    assert len(files) == len(listed)
    assert [v["name"] for v in man["vectors"]] == [n for n, _ in CD.mid_cases()]
    assert [v["name"] for v in man["planes"]] == [n for n, _ in CD.plane_cases()]
    for v, (_, spec) in zip(listed, CD.mid_cases() + CD.plane_cases()):
        assert v["spec"] == json.loads(json.dumps(spec)), v["name"]
        data = open(os.path.join(MID, v["file"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"], v["file"]
        assert len(data) < 1 << 20, v["file"]
        assert v["heap"] == [0, 0], v["name"]
        if "rets" in v:
            assert v["rets"] == [1] * len(v["spec"]["steps"]), v["name"]
        if v["spec"].get("preserve"):
            assert v["input_unchanged"] is True, v["name"]
    assert sum(os.path.getsize(os.path.join(MID, f)) for f in os.listdir(MID)) < 10 << 20


def kernel_constants():
    """EU_ROWS, EU_LOGB, FROZEN_LAG_MAX from the sources; the delta_x thresholds of k_emap_update's instantiations (both forms of the
    working plane go through the one function, eu_samples) and the lag rule as the planner itself answers (csrc/lqr_plan.h through
    tests/c/plan_main.cc, built by tests/test_plan.py)"""
    import test_plan
    common = open(os.path.join(CSRC, "lqr_common.h")).read()
    plan = open(os.path.join(CSRC, "lqr_plan.h")).read()
    K = {}
    for name, src in (("EU_ROWS", common), ("EU_LOGB", common), ("FROZEN_LAG_MAX", plan)):
        (K[name],) = {int(v) for v in re.findall(r"^#define\s+%s\s+(\d+)" % name, src, re.M)}
    rules = [ln.split() for ln in test_plan.run_plan("rules\n").splitlines()]
    nt = [(int(d), int(v)) for kind, d, v in rules if kind == "nt"]          # samples per row for delta_x 0 .. LQRHIP_MAX_DELTA
    assert [d for d, _ in nt] == list(range(17)) and [v for _, v in nt] == sorted(v for _, v in nt)
    last = {v: d for d, v in nt}                                             # the largest delta_x of each sample count
    K["NT"] = [(10 ** 9 if d == 16 else d, v) for v, d in sorted(last.items())]
    # the lag of a group: a quarter up to 4 carvers -- the seam step's plan says when the frozen planes are caught up
    lag = {int(n): int(v) for kind, n, v in rules if kind == "lag"}
    assert lag == {n: K["FROZEN_LAG_MAX"] // 4 if n <= 4 else K["FROZEN_LAG_MAX"] for n in range(1, 9)}, lag
    # the chunk of every rank loop a deep carver runs: k_wk_init_visible and k_frozen_catchup; k_vs_commit, k_inflate, k_compact, k_compact_jobs
    for unit, loops in (("k_energy.hip", 2), ("k_oneoff.hip", 4)):
        src = open(os.path.join(CSRC, unit)).read()
        assert re.findall(r"for \(int base = 0; base < \w+; base \+= (\d+)\)", src) == ["256"] * loops, unit
        assert len(re.findall(r"\bbase \+= ", src)) == loops, unit
    return K


def test_kernel_constants_are_the_ones_the_cases_were_sized_for():
    assert kernel_constants() == dict(EU_ROWS=62, EU_LOGB=8, FROZEN_LAG_MAX=128, NT=[(2, 12), (8, 36), (10 ** 9, 68)])


def test_mid_vectors_cross_every_boundary_of_the_deep_kernels_and_the_small_ones_none():
    import coldepth_cases as CD
    K = kernel_constants()
    lag1, lagn = K["FROZEN_LAG_MAX"] // 4, K["FROZEN_LAG_MAX"]
    wide_nt = ["nt%d" % s for _, s in K["NT"][1:]]
    sizes = {1: (6, 8), 2: (8, 12, 16), 3: (8, 16, 24, 32)}
    fam = {n for depth in (1, 2, 3) for n in CD.family_names(depth)}
    for depth in (1, 2, 3):
        single, group = set(), set()
        for name, spec in CD.mid_cases():
            if spec["depth"] != depth:
                continue
            single |= CD.boundaries(spec, K)
            if name in fam:
                assert spec["w"] > 256 and len(CD.family_names(depth)) >= 5
                group |= CD.boundaries(spec, K, group=5)
        want = ["%s:c%d" % (p, n) for p in ("shrink", "enlarge", "flatten", "relayout", "readout", "catchup") for n in (2, 3)]
        want += ["rows:b2", "rows:b3", "seams>%d" % lag1, "ragged"] + wide_nt
        want += ["%s:b%d" % (p, b) for p in ("inflate", "compact") for b in sizes[depth]]
        assert not [x for x in want if x not in single], (depth, [x for x in want if x not in single])
        assert {"seams>%d" % lagn, "catchup:c2", "ragged"} <= group, (depth, group)
    assert any("transpose:b%d" % b in CD.boundaries(s, K) for _, s in CD.mid_cases() for b in (12, 16))
    # the statement the mid-size vectors rest on: the small ones stay inside one chunk, one block and the lag, and below delta_x 9
    old = set()
    for _, spec in CD.cases():
        old |= CD.boundaries(spec, K)
        assert spec.get("delta", 1) < 9
    assert old and all(x.endswith(":c1") or x in ("rows:b1", "ragged", "nt12", "nt36") for x in old), old
    # plane vectors: more than one chunk and block, both counts past the lag (so a catch-up precedes each), one not a multiple of EU_LOGB
    for _, spec in CD.plane_cases():
        assert spec["w"] - max(CD.PLANE_SEAMS) > 0 and spec["w"] > 256 and spec["h"] > K["EU_ROWS"]
    assert min(CD.PLANE_SEAMS) > lag1 and max(CD.PLANE_SEAMS) > 2 * lag1 and any(k % K["EU_LOGB"] for k in CD.PLANE_SEAMS)
    for depth in (1, 2, 3):
        mine = [s for _, s in CD.plane_cases() if s["depth"] == depth]
        assert any(s["nrg"] in (0, 1, 2) and s["ch"] >= 3 for s in mine) and any(s["nrg"] in (3, 4, 5) and s["ch"] >= 3 for s in mine)
        assert any(s.get("delta", 1) >= 9 and s.get("rigidity") for s in mine)

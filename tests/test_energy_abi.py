"""The energy read-outs without a GPU: include/lqr_energy.h against liblqr 0.4.1's own prototypes (tests/golden/ref/abi.json), the
binding's table against the header, the engine's exports, tests/c/energy_replay.c compiled with -Werror against the header, the
soundness of the genuine-code vectors under tests/golden/energy/, and the numpy model of the calls (tests/energy_cases.py) against
every genuine plane and picture recorded there, bit for bit -- what the device tests of tests/test_energy_gpu.py rest on."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import energy_cases as EC
import imgtype_cases as IT
import lqr_ctypes as L
import test_coldepth_abi as CA
import test_imgtype_abi as IA
import test_masks_abi as MA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_energy.h")
ABI = CA.ABI
GOLD = os.path.join(ROOT, "tests", "golden", "energy")
LIBLQR_FUNCS = ("lqr_carver_get_energy", "lqr_carver_get_true_energy", "lqr_carver_get_energy_image")
EXT_FUNCS = {
    "lqrx_carver_get_energy_device": dict(ret="LqrRetVal", args=["LqrCarver*", "void*", "gint", "gint"]),
    "lqrx_carver_get_energy_image_device": dict(ret="LqrRetVal", args=["LqrCarver*", "void*", "gint", "LqrColDepth", "LqrImageType"]),
}
MAN = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
CTYPES_OF = dict(MA.CTYPES_OF, LqrImageType=L.C.c_int)


def test_header_declares_exactly_liblqrs_three_prototypes_and_the_two_extensions():
    d = IA.declared(HEADER)
    assert set(d) == set(LIBLQR_FUNCS) | set(EXT_FUNCS)
    for name in LIBLQR_FUNCS:
        assert d[name] == ABI["functions"][name], name
    for name, proto in EXT_FUNCS.items():
        assert d[name] == proto, name
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src) and re.search(r'#include\s+"lqr_coldepth.h"', src)
    # the comment states the rules a caller cannot guess
    for phrase in ("e_max starts at 0", "TRANSPOSED AND LEFT THAT", "LQR_CUSTOM_IMAGE", "NaN", "attached"):
        assert phrase in src, phrase


def test_binding_table_equals_the_header_and_the_other_tables_and_headers_stay_as_they_were():
    d = IA.declared(HEADER)
    assert set(L.ENERGY_SYMBOLS) == set(d)
    for name, (res, args) in L.ENERGY_SYMBOLS.items():
        assert res == CTYPES_OF[d[name]["ret"]] and args == [CTYPES_OF[a] for a in d[name]["args"]], name
        for table in (L.SYMBOLS, L.COLDEPTH_SYMBOLS, L.IMGTYPE_SYMBOLS, L.MASK_SYMBOLS):
            assert name not in table, name
    for other in ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h"):
        src = open(os.path.join(ROOT, "include", other)).read()
        for name in d:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert set(IA.declared(os.path.join(ROOT, "include", "lqr_coldepth.h"))) == set(CA.FUNCS)
    assert set(IA.declared(os.path.join(ROOT, "include", "lqr_imagetype.h"))) == set(IA.FUNCS)
    assert set(IA.declared(os.path.join(ROOT, "include", "lqr_masks.h"))) == set(MA.LIBLQR_FUNCS) | set(MA.EXT_FUNCS)
    assert "lqrx_carver_get_energy" in L.SYMBOLS                 # the old hook keeps its place
    assert all(hasattr(L.Carver, m) for m in ("get_energy", "get_energy_image", "get_energy_device", "get_energy_image_device", "energy_call"))


def test_engine_exports_every_name():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in LIBLQR_FUNCS + tuple(EXT_FUNCS) + ("lqrhip_energy_out", "lqrx_carver_get_energy"):
        assert re.search(r"\bT %s$" % name, syms, re.M), name


@pytest.mark.parametrize("glib", [False, True])
def test_energy_replay_compiles_with_werror_against_both_headers(tmp_path, glib):
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "tests", "c", "energy_replay.c"), "-o", str(tmp_path / "energy_replay.o")]
    if glib:        # the header under a GLib stand-in, as tests/test_c_replay.py builds the plug-in's replay
        hdr = tmp_path / "glib_standin.h"
        hdr.write_text("typedef int gint; typedef unsigned int guint; typedef unsigned char guchar; typedef char gchar;\n"
                       "typedef float gfloat; typedef double gdouble; typedef int gboolean; typedef void *gpointer;\n")
        cmd[1:1] = ["-DLQR_NO_GLIB_TYPEDEFS", "-include", str(hdr)]
    subprocess.run(cmd, check=True)


# ---- the vectors --------------------------------------------------------------------------------------------------------------
def test_manifest_lists_every_vector_with_its_checksum_and_size_limits():
    listed = MAN["vectors"] + MAN["findings"]
    files = {v["file"] for v in listed}
    assert files == {f for f in os.listdir(GOLD) if f.endswith(".npz")} and len(files) == len(listed)
    assert [v["name"] for v in MAN["vectors"]] == [n for n, _ in EC.cases()]
    assert [v["name"] for v in MAN["findings"]] == [n for n, _ in EC.finding_cases()]
    for v, (_, spec) in zip(listed, EC.cases() + EC.finding_cases()):
        assert v["spec"] == spec, v["name"]
        data = open(os.path.join(GOLD, v["file"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"], v["file"]
        assert len(data) <= IT.MAX_FILE, v["file"]
        assert v["heap"] == [0, 0] and v["heap_shipped"] == [0, 0], v["name"]
        assert v["step_rets"] == [1] * len(spec["steps"]), v["name"]
        assert v["same_as_shipped"] in (True, False)
        z = np.load(os.path.join(GOLD, v["file"]))
        assert json.loads(str(z["spec"])) == spec
        img, _ = EC.make_input(spec)
        assert img.dtype == z["img"].dtype and np.array_equal(img, z["img"]), v["name"]      # inputs come from the spec alone
        rec = json.loads(str(z["record"]))
        assert rec["rets"] == v["rets"] and rec["orientation"] == v["orientation"] and rec["intact"] == v["intact"], v["name"]
    assert all(v["model_equal"] for v in listed)
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD)) < 1 << 20


def test_numpy_model_equals_every_recorded_genuine_plane_and_picture_bit_for_bit():
    total = 0
    for v in MAN["vectors"] + MAN["findings"]:
        z = np.load(os.path.join(GOLD, v["file"]))
        n, differ = EC.model_check(v["spec"], z)
        assert not differ and n == v["model_compared"], (v["name"], differ)
        assert n == sum(op[0] in ("norm", "image") and r == [1, 1] for op, r in zip(v["spec"]["ops"], v["rets"])), v["name"]     # no skip list
        total += n
    assert total >= 100


def test_what_the_vectors_say_about_the_rules():
    vec = {v["name"]: (v, np.load(os.path.join(GOLD, v["file"]))) for v in MAN["vectors"] + MAN["findings"]}
    # nothing is ever written past the result, and a failing call writes nothing
    for v, _ in vec.values():
        flat = [x for i in v["intact"] if i is not None for x in (i if isinstance(i, list) else [i])]
        assert all(flat), v["name"]
    # the carver is left in the orientation asked for; 0 -> 1 -> 0
    for v, _ in vec.values():
        for op, o, r in zip(v["spec"]["ops"], v["orientation"], v["rets"]):
            if op[0] in ("true", "norm", "image") and r in (1, [1, 1]):
                assert o == op[1], (v["name"], op)
    assert vec["ef2"][0]["orientation"] == [0, 1, 1, 0, 0]
    # the true energy does not depend on the call order, the two orientations differ (another gradient direction)
    z = vec["ef2"][1]
    assert np.array_equal(z["true@0"], z["true@3"]) and np.array_equal(z["true@0"], z["out@4"]) and not np.array_equal(z["true@0"], z["true@1"])
    # a shrunk carver asked for its own orientation stays as it is (no flattening): the read-out has the carved size
    v, z = vec["shrunk"]
    assert z["out@1"].shape == (33, 57) and json.loads(str(z["record"]))["after_ops"]["orientation"] == 1
    assert vec["shrunk_regrown"][1]["out@2"].shape == (33, 61) and vec["enlarged"][1]["out@1"].shape == (33, 75)
    assert vec["height_changed"][1]["out@1"].shape == (28, 65)
    # e_max starts at 0: an all-negative plane normalises to [0, < 1]; a constant negative one to 0; constant zero stays 0
    z = vec["bias_neg_null"][1]
    assert (z["true@1"] < 0).all() and z["out@1"].min() == 0 and 0.5 < z["out@1"].max() < 1
    assert (vec["const_negative"][1]["true@1"] < 0).all() and not vec["const_negative"][1]["out@1"].any()
    assert not vec["const_null"][1]["true@0"].any() and not vec["const_null"][1]["out@0"].any()
    assert not vec["const_colour"][1]["out@0"].any()
    # a single non-negative value stays its squashed self in the float form, and is 0 in the picture
    z = vec["size_1x1"][1]
    assert z["true@0"][0, 0] > 0 and z["out@0"][0, 0] == EC.squash(z["true@0"])[0, 0] and not z["out@2"].any()
    # LQR_CUSTOM_IMAGE, an orientation other than 0 / 1, a NULL buffer: LQR_ERROR
    assert vec["formats"][0]["rets"][-2:] == [[1, 0], [1, 0]] and all(r == [1, 1] for r in vec["formats"][0]["rets"][:-2])
    assert vec["bad_arguments"][0]["rets"] == [[0, 0], 0, [0, 0], 0, 0, 0, [1, 1]] and set(vec["bad_arguments"][0]["orientation"]) == {0}
    assert {(op[2], op[3]) for op in vec["formats"][0]["spec"]["ops"][:-2]} == {(d, t) for d in range(4) for t in range(7)}
    # 0.24875-like values truncate: an 8-bit picture is never above the rounded one
    z = vec["formats"][1]
    n = EC.normalised(z["true@2"])
    assert z["out@2"].dtype == np.uint8 and (z["out@2"][:, :, 0] <= np.rint(n * 255)).all() and (z["out@2"][:, :, 0] < np.rint(n * 255)).any()
    # served before lqr_carver_init, and the carver still initialises and carves afterwards
    assert vec["late_alone"][0]["rets"] == [[1, 1], 1, [1, 1]] and vec["late_then_resize"][0]["rets"] == [[1, 1], 1]
    assert vec["late_then_resize"][0]["step_rets"] == [1, 1]
    # the attached carver follows the root: it was carved to the root's size by the root's seams
    z = vec["attached"][1]
    assert z["aux_image1"].shape[:2] == z["image1"].shape[:2] == (14, 27)
    # a frame one pixel wide: liblqr's gradient reads the neighbour outside it -- the pixel of the next row, nothing (0) after the last --
    # and reports that difference (the engine: 0, include/lqr_energy.h)
    for name, keys in (("size_1x1", ("true@0", "true@1")), ("size_1xn_o0", ("true@0",)), ("size_nx1_o1", ("true@0",))):
        z = vec[name][1]
        seq = (z["img"].astype(np.float64) / 255.0).mean(axis=2).ravel()
        for k in keys:
            assert np.allclose(z[k].ravel(), np.abs(np.append(seq[1:], 0.0) - seq), rtol=1e-6, atol=1e-9) and z[k].all(), (name, k)
    # liblqr serves an attached carver (the engine does not: include/lqr_energy.h), and transposes it ALONE
    assert vec["attached_same_orientation"][0]["rets"] == [1, 1] and vec["attached_other_orientation"][0]["rets"] == [1]
    assert vec["attached_other_orientation"][0]["orientation"] == [0]


def test_cases_cover_what_the_issue_lists():
    specs = dict(EC.cases())
    every = list(specs.values())
    assert {s["nrg"] for s in every} == set(range(7)) and {s["depth"] for s in every} == {0, 1, 2, 3}
    assert {s.get("type") for s in every} >= {IT.CMYK} and any(s["ch"] == 5 for s in every)
    assert {(s["w"], s["h"]) for s in every} >= {(1, 9), (9, 1), (130, 3), (7, 5)}
    assert {(s["w"], s["h"]) for _, s in EC.finding_cases()} >= {(1, 1), (1, 9), (9, 1)}
    assert all(s["w"] <= 130 and s["h"] <= 33 for s in every)
    kinds = {op[0] for s in every for op in s["ops"]}
    assert kinds == {"resize", "init", "bias", "true", "norm", "image", "null"}
    assert {op[1] for s in every for op in s["ops"] if op[0] == "bias"} == {"pos", "neg", "mixed", "negconst"}
    assert any(s.get("aux") for s in every) and sum(bool(s.get("late_init")) for s in every) == 2
    assert any(s["steps"] and s["ops"][-1] == ["norm", 1] and not s.get("late_init") and not s.get("aux") for s in every)

"""The computed-mask surface without a GPU: include/lqr_masks.h against liblqr 0.4.1's own prototypes (tests/golden/ref/abi.json), the
binding's table against the header, the engine's exports, the soundness of the genuine-code vectors under tests/golden/masks/, and
the numpy model of the mask calls (tests/mask_cases.py) against every genuine plane recorded there, bit for bit -- what the device
tests of tests/test_masks_gpu.py rest on."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np

import imgtype_cases as IT
import lqr_ctypes as L
import mask_cases as MC
import test_coldepth_abi as CA
import test_imgtype_abi as IA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_masks.h")
ABI = CA.ABI
GOLD = os.path.join(ROOT, "tests", "golden", "masks")
LIBLQR_FUNCS = ("lqr_carver_bias_add_xy", "lqr_carver_bias_add_area", "lqr_carver_bias_add", "lqr_carver_bias_add_rgb", "lqr_carver_bias_clear",
                "lqr_carver_rigmask_add_xy", "lqr_carver_rigmask_add_area", "lqr_carver_rigmask_add", "lqr_carver_rigmask_add_rgb",
                "lqr_carver_rigmask_clear")
EXT_FUNCS = {
    "lqrx_carver_bias_add_area_device": dict(ret="LqrRetVal", args=["LqrCarver*", "void*", "LqrColDepth", "gint", "gint", "gint", "gint", "gint"]),
    "lqrx_carver_rigmask_add_area_device": dict(ret="LqrRetVal", args=["LqrCarver*", "void*", "LqrColDepth", "gint", "gint", "gint", "gint"]),
    "lqrx_carver_get_bias": dict(ret="LqrRetVal", args=["LqrCarver*", "gfloat*"]),
    "lqrx_carver_get_rigmask": dict(ret="LqrRetVal", args=["LqrCarver*", "gfloat*"]),
}
MAN = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
CTYPES_OF = {"LqrCarver*": L.C.c_void_p, "gdouble*": L.C.c_void_p, "guchar*": L.C.c_void_p, "gfloat*": L.C.c_void_p, "void*": L.C.c_void_p,
             "gint": L.C.c_int, "gdouble": L.C.c_double, "LqrColDepth": L.C.c_int, "LqrRetVal": L.C.c_int, "void": None}


def test_header_declares_exactly_liblqrs_prototypes_and_the_four_extensions():
    d = IA.declared(HEADER)
    assert set(d) == set(LIBLQR_FUNCS) | set(EXT_FUNCS)
    for name in LIBLQR_FUNCS:
        assert d[name] == ABI["functions"][name], name
    for name, proto in EXT_FUNCS.items():
        assert d[name] == proto, name
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src) and re.search(r'#include\s+"lqr_coldepth.h"', src)


def test_binding_table_equals_the_header_and_the_other_tables_stay_as_they_were():
    d = IA.declared(HEADER)
    assert set(L.MASK_SYMBOLS) == set(d)
    for name, (res, args) in L.MASK_SYMBOLS.items():
        assert res == CTYPES_OF[d[name]["ret"]] and args == [CTYPES_OF[a] for a in d[name]["args"]], name
        assert name not in L.SYMBOLS and name not in L.COLDEPTH_SYMBOLS and name not in L.IMGTYPE_SYMBOLS
    lqr_h = open(os.path.join(ROOT, "include", "lqr.h")).read()
    for name in d:
        assert not re.search(r"\b%s\s*\(" % name, lqr_h), name


def test_engine_exports_every_name():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in LIBLQR_FUNCS + tuple(EXT_FUNCS) + ("lqrhip_debug_mask_flushes", "lqrhip_mask_add_f", "lqrhip_mask_scatter"):
        assert re.search(r"\bT %s$" % name, syms, re.M), name


# ---- the vectors --------------------------------------------------------------------------------------------------------------
def test_manifest_lists_every_vector_with_its_checksum_and_size_limits():
    listed = MAN["vectors"] + MAN["findings"]
    files = {v["file"] for v in listed}
    assert files == {f for f in os.listdir(GOLD) if f.endswith(".npz")} and len(files) == len(listed)
    assert [v["name"] for v in MAN["vectors"]] == [n for n, _ in MC.cases()]
    assert [v["name"] for v in MAN["findings"]] == [n for n, _ in MC.finding_cases()]
    for v, (_, spec) in zip(listed, MC.cases() + MC.finding_cases()):
        assert v["spec"] == spec, v["name"]
        data = open(os.path.join(GOLD, v["file"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"], v["file"]
        assert len(data) <= IT.MAX_FILE, v["file"]
        assert v["heap"] == [0, 0] and v["heap_shipped"] == [0, 0], v["name"]
        assert v["step_rets"] == [1] * len(spec["steps"]), v["name"]
        assert v["same_as_shipped"] in (True, False)
        z = np.load(os.path.join(GOLD, v["file"]))
        assert json.loads(str(z["spec"])) == spec
        img, _ = MC.make_input(spec)
        assert img.dtype == z["img"].dtype and np.array_equal(img, z["img"]), v["name"]      # inputs come from the spec alone
    assert all(v["model_equal"] for v in MAN["vectors"]) and not any(v["model_equal"] for v in MAN["findings"])
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD)) < 6 << 20


def _model_walk(spec, z):
    """mask_cases.Model through the ops of a spec: return values against the record, every recorded plane the model can know against
    the model; returns the number of planes compared"""
    _, extra = MC.make_input(spec)
    m = MC.Model(spec, extra["masks"])
    rec = json.loads(str(z["record"]))
    compared = 0

    def check(kb, kr, what):
        nonlocal compared
        if not m.valid:                 # a resize carved non-zero planes: only the genuine code knows them; go on from what it had
            m.adopt(z[kb], z[kr])
            return
        for which, key in (("bias", kb), ("rig", kr)):
            got = m.plane(which)
            assert got.dtype == np.float32 and z[key].dtype == np.float32 and got.shape == z[key].shape, (what, key)
            assert np.array_equal(got.view(np.uint32), z[key].view(np.uint32)), (what, key)
            compared += 1

    for i, op in enumerate(spec["ops"]):
        on_aux = op[0] == "aux"
        kind = op[1] if on_aux else op[0]
        want = 0 if on_aux else m.apply(op)                 # (every op on an attached carver in the cases is one liblqr refuses)
        if kind == "planes":
            check("bias@%d" % i, "rig@%d" % i, (spec["seed"], i))
        elif kind in ("bias_xy", "rig_xy"):
            assert [v for v, _ in rec["rets"][i]] == [want] and sum(n for _, n in rec["rets"][i]) > 0, (op, rec["rets"][i])
        else:
            assert rec["rets"][i] == want, (op, rec["rets"][i])
    if "bias" in z.files and m.valid:
        check("bias", "rig", (spec["seed"], "end"))
    return compared


def test_numpy_model_equals_every_recorded_genuine_plane_bit_for_bit():
    total = 0
    for v in MAN["vectors"]:
        z = np.load(os.path.join(GOLD, v["file"]))
        n = _model_walk(v["spec"], z)
        assert n == v["model_planes"], v["name"]
        total += n
    assert total >= 100
    # the planes no model can know -- non-zero ones carved by a resize -- are those of the two interrupted runs and nothing else
    unknown = [v["name"] for v in MAN["vectors"] if v["planes"] and v["model_planes"] == 0]
    assert unknown == ["xy_interrupted"], unknown


def test_findings_are_liblqrs_offsets_on_a_transposed_carver_and_nothing_else():
    """orientation 1, max(0, x_off) != max(0, y_off): the genuine planes are NOT the documented ones, they are exactly the documented
    ones of the call with x_off and y_off exchanged (include/lqr_masks.h)"""
    assert len(MAN["findings"]) == 2
    for v in MAN["findings"]:
        z = np.load(os.path.join(GOLD, v["file"]))
        assert json.loads(str(z["record"]))["after_ops"]["orientation"] == 1
        assert v["swapped_offsets_model_equal"] is True
        assert _model_walk(MC.swapped_offsets(v["spec"]), z) == 2
        _, extra = MC.make_input(v["spec"])
        m = MC.Model(v["spec"], extra["masks"])
        for op in v["spec"]["ops"]:
            m.apply(op)
        assert not np.array_equal(m.plane("bias"), z["bias"]) and not np.array_equal(m.plane("rig"), z["rig"])
    # every transposed case among the vectors proper keeps to offsets on which the two placements agree
    for name, spec in MC.cases():
        if name.startswith("transposed"):
            for op in spec["ops"]:
                offs = op[3:5] if op[0] in ("bias_f", "bias_rgb_area") else op[2:4] if op[0] in ("rig_f", "rig_rgb_area") else None
                if offs and offs[0] is not None:
                    assert max(0, offs[0]) == max(0, offs[1]), (name, op)


def test_clear_then_resize_is_the_unmasked_carve():
    a, b = (np.load(os.path.join(GOLD, "masks_%s.npz" % n)) for n in ("unmasked", "clear_resize"))
    specs = dict(MC.cases())
    assert specs["unmasked"]["seed"] == specs["clear_resize"]["seed"] and np.array_equal(a["img"], b["img"])
    for k in ("image0", "vmap0", "energy"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert not b["bias"].any() and not b["rig"].any()


def test_cases_cover_what_the_mask_code_can_get_wrong():
    specs = dict(MC.cases())
    assert {specs["width_%d" % w]["w"] for w in (255, 256, 257, 300)} == {255, 256, 257, 300}
    every = list(specs.values())
    assert any(s["h"] == 2 for s in every) and any(m[:2] == [1, 1] for s in every for m in s["masks"].values())
    assert any(m[1] == 1 for s in every for m in s["masks"].values()) and any(m[1] == 2 for s in every for m in s["masks"].values())
    assert all(s["w"] <= 340 and s["h"] <= 300 and s["w"] * s["h"] <= 12000 for s in every)
    factors = [op[2] for s in every for op in s["ops"] if op[0] == "bias_f"]
    assert min(factors) < 0 and 0 in factors and max(factors) >= 1000000
    offs = [(op[3], op[4]) for s in every for op in s["ops"] if op[0] == "bias_f" and op[3] is not None]
    assert any(x < 0 and y < 0 for x, y in offs) and any(x > 0 and y > 0 for x, y in offs)
    assert {(s["delta"], s["rigidity"] != 0) for n, s in specs.items() if n.startswith("delta")} == {(1, False), (1, True), (2, False), (2, True)}
    assert {s["depth"] for s in every} == {0, 1, 2}
    assert any(s.get("aux") for s in every) and any(s.get("late_init") for s in every)
    kinds = {op[0] for s in every for op in s["ops"]}
    assert kinds >= {"resize", "flatten", "init", "planes", "aux", "bias_f", "rig_f", "bias_rgb", "rig_rgb", "bias_rgb_area", "rig_rgb_area", "bias_xy",
                     "rig_xy", "bias_clear", "rig_clear"}
    runs = {tuple(r[:1]) for s in every for r in s["runs"].values()}
    assert runs == {("rowmajor",), ("shuffle",), ("repeat",), ("some",)}
    assert specs["xy_repeat3"]["runs"]["a"][2:] == [234, 3, 700]
    # orientation 1 when the masks arrive, and carvers that are not flat
    for n in ("transposed", "transposed_tall", "transposed_height_first"):
        z = np.load(os.path.join(GOLD, "masks_%s.npz" % n))
        assert json.loads(str(z["record"]))["after_ops"]["orientation"] == 1, n
    assert specs["after_enlarge"]["ops"][0][1] > specs["after_enlarge"]["w"] and specs["after_shrink"]["ops"][0][1] < specs["after_shrink"]["w"]
    # the refused calls were refused by the genuine code
    for v in MAN["vectors"]:
        if v["name"] == "attached":
            assert v["rets"][:4] == [0, [[0, 5]], 0, 0] and v["rets"][4:] == [1, 1]
        if v["name"] == "late_init":
            assert v["rets"][:4] == [0, [[0, 40]], 0, 0] and v["rets"][4:7] == [1, [[1, 40]], 1] and v["rets"][8:] == [1, 1, 1]

"""Seam-map loading without a GPU: include/lqr_vmap.h against liblqr 0.4.1's own prototypes (tests/golden/ref/abi.json), the binding's
table against the header, the engine's exports, the soundness of the genuine-code vectors under tests/golden/vmap/, what the specs
alone cover, and the numpy model of a loaded map (tests/vmap_cases.py) against every genuine image recorded there, bit for bit -- what
the permutation-map tests of tests/test_vmap_load_gpu.py rest on."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np

import coldepth_cases as CD
import imgtype_cases as IT
import lqr_ctypes as L
import test_coldepth_abi as CA
import test_imgtype_abi as IA
import test_masks_abi as MA
import vmap_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lqr_vmap.h")
ABI = CA.ABI
GOLD = os.path.join(ROOT, "tests", "golden", "vmap")
LIBLQR_FUNCS = ("lqr_vmap_new", "lqr_vmap_load", "lqr_vmap_internal_dump")
EXT_FUNCS = {
    "lqrx_vmap_load_device": dict(ret="LqrRetVal", args=["LqrCarver*", "gint*", "gint", "gint", "gint", "gint"]),
    "lqrx_vmap_load_batch": dict(ret="LqrRetVal", args=["LqrCarver**", "gint", "LqrVMap*"]),
}
MAN = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
CTYPES_OF = dict(MA.CTYPES_OF, **{"LqrVMap*": L.C.c_void_p, "gint*": L.C.c_void_p, "LqrCarver**": L.C.POINTER(L.C.c_void_p)})


def _entries():
    return MAN["vectors"] + MAN["findings"]


def _load(v):
    return np.load(os.path.join(GOLD, v["file"]))


def test_header_declares_liblqrs_three_prototypes_and_the_two_extensions():
    d = IA.declared(HEADER)
    assert set(d) == set(LIBLQR_FUNCS) | set(EXT_FUNCS)
    for name in LIBLQR_FUNCS:
        assert name in ABI["functions"] and d[name] == ABI["functions"][name], name
    for name, proto in EXT_FUNCS.items():
        assert d[name] == proto, name
    src = open(HEADER).read()
    assert re.search(r'#include\s+"lqr.h"', src)
    for phrase in ("VALIDATED", "exactly once", "enl_step is 2.0", "REFUSED UP FRONT", "attached", "LQR_NOMEM", "Connected seams are NOT"):
        assert phrase in src, phrase


def test_binding_table_equals_the_header_and_the_other_headers_and_tables_stay_as_they_were():
    d = IA.declared(HEADER)
    assert set(L.VMAP_SYMBOLS) == set(d)
    for name, (res, args) in L.VMAP_SYMBOLS.items():
        assert res == CTYPES_OF[d[name]["ret"]] and args == [CTYPES_OF[a] for a in d[name]["args"]], name
        for table in (L.SYMBOLS, L.COLDEPTH_SYMBOLS, L.IMGTYPE_SYMBOLS, L.MASK_SYMBOLS, L.ENERGY_SYMBOLS):
            assert name not in table, name
    for other in ("lqr.h", "lqr_coldepth.h", "lqr_imagetype.h", "lqr_masks.h", "lqr_energy.h"):
        src = open(os.path.join(ROOT, "include", other)).read()
        for name in d:
            assert not re.search(r"\b%s\s*\(" % name, src), (other, name)
    assert all(hasattr(L.Carver, m) for m in ("vmap_load", "vmap_load_device", "vmap_internal_dump")) and callable(L.vmap_load_batch)
    assert callable(L.bind_vmap)


def test_engine_exports_all_five_symbols_and_the_shim_calls():
    syms = subprocess.run(["nm", "-D", "--defined-only", IA.engine_lib()], capture_output=True, text=True, check=True).stdout
    for name in LIBLQR_FUNCS + tuple(EXT_FUNCS) + ("lqrhip_vmap_stage", "lqrhip_vmap_load", "lqrhip_vmap_release", "lqr_vmap_dump"):
        assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_manifest_lists_every_vector_with_its_checksum_and_size_limits():
    listed = _entries()
    files = {v["file"] for v in listed}
    assert files == {f for f in os.listdir(GOLD) if f.endswith(".npz")} and len(files) == len(listed)
    assert [v["name"] for v in MAN["vectors"]] == [n for n, _ in VC.cases()]
    assert [v["name"] for v in MAN["findings"]] == [n for n, _ in VC.finding_cases()]
    for v, (_, spec) in zip(listed, VC.cases() + VC.finding_cases()):
        assert v["spec"] == spec, v["name"]
        data = open(os.path.join(GOLD, v["file"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"], v["file"]
        assert len(data) <= IT.MAX_FILE and spec["w"] <= VC.MAX_W and spec["h"] <= VC.MAX_H, v["file"]
        assert v["heap"] == [0, 0] and v["heap_shipped"] == [0, 0], v["name"]
        z = _load(v)
        assert json.loads(str(z["spec"])) == spec
        img, _ = VC.make_input(spec)
        assert img.dtype == z["img"].dtype and np.array_equal(img, z["img"]), v["name"]      # inputs come from the spec alone
        rec = json.loads(str(z["record"]))
        assert rec["rets"] == v["rets"] and rec["map_meta"] == v["map_meta"], v["name"]
        if spec["map"]["kind"] == "perm":
            m = VC.perm_map(spec["seed"], spec["w"], spec["h"], spec["map"]["d"], spec["map"]["o"])
            assert np.array_equal(m["data"], z["map"]) and rec["map_meta"] == [m["depth"], m["orientation"]]
        assert v["map_valid"] and VC.valid_map(dict(data=z["map"], depth=rec["map_meta"][0], orientation=rec["map_meta"][1]), spec["w"], spec["h"])
    assert all(v["model_equal"] for v in listed)
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD)) < 1 << 20


def test_numpy_model_equals_every_recorded_genuine_image_bit_for_bit():
    total = perm = 0
    for v in _entries():
        z = _load(v)
        n, differ = VC.model_check(v["spec"], z["img"], z)
        assert not differ and n == v["model_compared"], (v["name"], differ)
        total += n
        perm += n if v["spec"]["map"]["kind"] == "perm" else 0
    assert total >= 60 and perm >= 20          # ... of them on maps that are not seam-connected


def test_what_the_vectors_say_about_liblqr():
    vec = {v["name"]: (v, _load(v), json.loads(str(_load(v)["record"]))) for v in _entries()}
    for name, (v, z, rec) in vec.items():
        spec = v["spec"]
        for i, op in enumerate(spec["ops"]):
            g = rec["getters"][i]
            if op[0] == "load" and rec["rets"][i] == 1:
                # depth and orientation are the map's, enl_step is 2.0 (the carver was configured with 1.5), the map comes back
                assert (g["depth"], g["orientation"], g["enl_step"]) == (rec["map_meta"][0], rec["map_meta"][1], 2.0), (name, i)
                if name not in ("second_load_at_50", "second_load_at_30") or i == 0:
                    assert (g["width"], g["height"], g["ref_width"], g["ref_height"]) == (spec["w"], spec["h"], spec["w"], spec["h"]), (name, i)
                    assert np.array_equal(z["redump@%d" % i], z["map"]) and rec["redump_meta"][str(i)] == rec["map_meta"], (name, i)
    # every vector the engine reproduces returns LQR_OK throughout, but for the load onto an initialised carver
    for v in MAN["vectors"]:
        want = [0 if (op[0] == "load" and "init" in [o[0] for o in v["spec"]["ops"][:i]]) else 1 for i, op in enumerate(v["spec"]["ops"])]
        assert v["rets"] == want, v["name"]
    # an initialised carver: LQR_ERROR, nothing changes
    v, z, rec = vec["initialised"]
    assert rec["rets"] == [1, 0] and rec["getters"][0] == rec["getters"][1]
    assert vec["init_then_load_refused"][2]["rets"] == [1, 1, 1, 1, 0, 1]
    # init after a load and a deeper resize: LQR_OK and the depth grows (10 -> 15, 7 -> 12) ...
    v, z, rec = vec["init_after_load_h"]
    assert rec["rets"] == [1, 1, 1, 1, 1, 0] and rec["getters"][2]["depth"] == 15 and rec["getters"][2]["width"] == 25
    assert vec["init_after_load_v"][2]["getters"][2]["depth"] == 12 and vec["init_after_load_v"][2]["getters"][2]["orientation"] == 1
    # ... but liblqr's further seams are found on the wrong pixels: the map it dumps afterwards is not one (a finding, include/lqr_vmap.h 5)
    for name in ("init_after_load_h", "init_after_load_v"):
        v, z, rec = vec[name]
        d, o = rec["redump_meta"]["3"]
        assert not VC.valid_map(dict(data=z["dump@3"], depth=d, orientation=o), v["spec"]["w"], v["spec"]["h"]), name
    # the attached carver follows the resizes
    z = vec["attached_h"][1]
    assert z["aux_image@1"].shape == z["image@1"].shape == (24, 34, 3)
    # lqr_vmap_internal_dump appends
    rec = vec["h_40x24_d10"][2]
    assert sorted(rec["lists"].values()) == [1, 2] and np.array_equal(vec["h_40x24_d10"][1]["idump@8"], vec["h_40x24_d10"][1]["map"])
    # where the engine does not follow (include/lqr_vmap.h items 2 and 3): outside the range liblqr fails and then refuses sizes that
    # had worked; in a two-direction request it carries out the width and transposes first; a second load onto a resized carver is
    # accepted and applies the map to the resized image
    assert vec["beyond_range"][0]["rets"] == [1, 1, 0, 0, 0] and vec["below_range"][0]["rets"] == [1, 0, 0]
    rec = vec["other_direction"][2]
    assert rec["rets"] == [1, 0, 0] and (rec["getters"][1]["width"], rec["getters"][1]["orientation"], rec["getters"][1]["depth"]) == (35, 1, 0)
    for name, w1 in (("second_load_at_50", 50), ("second_load_at_30", 30)):
        rec = vec[name][2]
        assert rec["rets"] == [1, 1, 1] and (rec["getters"][2]["ref_width"], rec["getters"][2]["depth"]) == (w1, 10), name


def test_cases_cover_what_the_issue_lists():
    specs = dict(VC.cases())
    every = list(specs.values())
    recorded = every + [s for _, s in VC.finding_cases()]         # (init after a load and a deeper resize is recorded as a finding)
    depth_of = lambda s: s["map"]["d"] if s["map"]["kind"] == "perm" else abs(s["w"] - s["map"]["to"][0]) + abs(s["h"] - s["map"]["to"][1])     # noqa: E731
    orient_of = lambda s: s["map"]["o"] if s["map"]["kind"] == "perm" else int(s["map"]["to"][1] != s["h"])                                    # noqa: E731
    assert {orient_of(s) for s in every} == {0, 1}
    assert any(depth_of(s) == 1 for s in every) and any(orient_of(s) == 0 and depth_of(s) == s["w"] - 2 for s in every)
    # a load after a resize; init after a load (both directions); an attached carver
    assert any([op[0] for op in s["ops"]].count("load") >= 2 and s["ops"][1][0] == "resize" and "init" not in [op[0] for op in s["ops"]] for s in every)
    inits = [s for s in recorded if ["load"] in s["ops"] and ["init"] in s["ops"] and s["ops"].index(["init"]) > s["ops"].index(["load"])]
    deeper = [s for s in inits if any(op[0] == "resize" and (op[2] if orient_of(s) else op[1]) < (s["h"] if orient_of(s) else s["w"]) - depth_of(s) for op in s["ops"])]
    assert {orient_of(s) for s in deeper} == {0, 1} and len(inits) > len(deeper)
    assert any(s.get("aux") for s in every)
    # a deep (32F) and a five-channel carver; maps that are not seam-connected in both orientations; more than 256 columns
    assert any(s["depth"] == 2 for s in every) and any(s["ch"] == 5 for s in every) and {s["depth"] for s in every} == {0, 1, 2, 3}
    assert {s["map"]["o"] for s in every if s["map"]["kind"] == "perm"} == {0, 1} and any(s["w"] > 256 for s in every)
    assert all(s["w"] <= VC.MAX_W and s["h"] <= VC.MAX_H for s in every)
    assert {op[0] for s in every for op in s["ops"]} == {"load", "resize", "init", "idump"}
    assert any(s["ops"].index(["init"]) > s["ops"].index(["load"]) for s in every if ["init"] in s["ops"])


def test_model_rules_on_a_hand_made_line():
    p = np.array([[10], [20], [31], [40]], np.uint8)
    v = np.array([2, 0, 1, 0], np.int32)
    line = lambda n: VC.model_line(p, v, 2, n)[:, 0].tolist()      # noqa: E731
    assert line(4) == [10, 20, 31, 40] and line(3) == [10, 20, 40] and line(2) == [20, 40]
    assert line(5) == [10, 20, 25, 31, 40] and line(6) == [10, 10, 20, 25, 31, 40]
    f = np.array([[0.1], [0.7]], np.float32)
    assert VC.model_line(f, np.array([0, 1], np.int32), 1, 3)[1, 0] == np.float32((np.float32(0.1) + np.float32(0.7)) * np.float32(0.5))
    assert VC.valid_map(dict(data=v[None, :], depth=2, orientation=0), 4, 1)
    assert not VC.valid_map(dict(data=np.array([[2, 2, 1, 0]]), depth=2, orientation=0), 4, 1)
    assert not VC.valid_map(dict(data=np.array([[3, 0, 1, 0]]), depth=2, orientation=0), 4, 1)
    assert CD.bits(f).dtype == np.uint8

"""tests/golden/control/ without a GPU: the manifest is consistent with the files and with tests/control_cases.py, and every value the
engine's rules predict (control_cases.predict: return values, number of progress events, sizes, what the armed cancel returned) is the
one recorded from the genuine liblqr -- or the vector is listed as a finding with the reason (a cancelled carver's state, where the
engine departs on purpose, include/lqr_control.h).

What the genuine vectors pinned: a cancel outside a call returns LQR_OK and changes nothing; a cancel from the n-th update callback ends
the resize with LQR_USRCANCEL after n update events and no end event, in either direction, either order and in both steps of an
enlargement; afterwards lqr_carver_resize and lqr_carver_flatten return LQR_USRCANCEL, lqr_vmap_dump gives a map, both scans serve and
lqr_carver_cancel returns LQR_OK; on an attached carver lqr_carver_cancel returns LQR_ERROR, idle or not, and the resize runs on.
NOT pinned (not recorded): the energy read-outs and lqr_vmap_load on a cancelled carver; the engine returns LQR_USRCANCEL there too."""
import hashlib
import json
import os

import numpy as np

import control_cases as CC
import lqr_ctypes as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "control")
MAN = json.load(open(os.path.join(GOLD, "MANIFEST.json")))


def _load(v):
    z = np.load(os.path.join(GOLD, v["file"]))
    return z, json.loads(str(z["record"]))


def test_manifest_lists_every_vector_with_its_checksum():
    listed = MAN["vectors"] + MAN["findings"]
    assert {v["file"] for v in listed} == {f for f in os.listdir(GOLD) if f.endswith(".npz")} and len({v["file"] for v in listed}) == len(listed)
    assert [v["name"] for v in MAN["vectors"]] == [n for n, _ in CC.cases()]
    assert [v["name"] for v in MAN["findings"]] == [n for n, _ in CC.finding_cases()]
    for v, (_, spec) in zip(listed, CC.cases() + CC.finding_cases()):
        assert v["spec"] == spec, v["name"]
        data = open(os.path.join(GOLD, v["file"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == v["sha256"] and len(data) <= 256 << 10, v["file"]
        assert v["heap"] == [0, 0] and v["heap_shipped"] == [0, 0] and v["rets_shipped_same"], v["name"]
        z, rec = _load(v)
        assert json.loads(str(z["spec"])) == spec and rec["rets"] == v["rets"] and rec["hooks"] == v["hooks"], v["name"]
        img, _ = CC.make_input(spec)
        assert np.array_equal(img, z["img"]) and (spec["w"], spec["h"]) == (64, 48), v["name"]
    assert MAN["rules"] == CC.RULES_NOTE and MAN["gradient_to_builtin"] == {str(k): e for k, e in CC.GRADIENT_TO_BUILTIN.items()}
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD)) < 1 << 20


def test_the_rules_predict_every_recorded_value_or_the_vector_is_a_finding():
    for v in MAN["vectors"] + MAN["findings"]:
        _, rec = _load(v)
        p = CC.predict(v["spec"])
        finding = v in MAN["findings"]
        assert rec["hooks"] == p["hooks"], v["name"]
        for i, op in enumerate(v["spec"]["ops"]):
            what = (v["name"], i, op)
            if p["rets"][i] is not None:
                assert rec["rets"][i] == p["rets"][i], what                # return values: pinned everywhere, findings included
            assert rec["n_events"][i] == p["n_events"][i], what            # ... and so are the progress events
            g = rec["getters"][i]
            if not finding:
                assert (g["width"], g["height"]) == tuple(p["sizes"][i]), what
        if finding:
            # the reason: from the cancelled resize on, the genuine carver sits inside the session it was building
            assert v["finding"] == "half_built_state" and v["differs_from_rules"] and all(d.startswith("size@") for d in v["differs_from_rules"]), v["name"]
            k = v["rets"].index(L.LQR_USRCANCEL)
            assert all(int(d.split("@")[1].split()[0]) >= k for d in v["differs_from_rules"]), v["name"]
            assert ("end", "done") not in [tuple(e) for e in rec["events"][-1:]]
        else:
            assert v["differs_from_rules"] == [] and "finding" not in v, v["name"]


def test_what_the_vectors_say_about_liblqr():
    vec = {v["name"]: _load(v) for v in MAN["vectors"] + MAN["findings"]}
    # after a cancel: resize 3, flatten 3, dump a map, both scans serve, cancel OK, resize 3
    for name, _ in CC.finding_cases():
        rets = vec[name][1]["rets"]
        k = rets.index(3)
        assert rets[k:] == [3, 3, 3, 1, [1, 1], 1, 3], name
        assert vec[name][1]["hooks"] == {str(k): [1, 1]}, name
    # on an attached carver: LQR_ERROR, and nothing is cancelled
    assert vec["cancel_aux_idle"][1]["rets"] == [0, 1] and vec["cancel_aux_in_resize"][1]["rets"] == [None, 1, 1]
    assert vec["cancel_aux_in_resize"][1]["hooks"] == {"1": [1, 0]}
    # set_no_dump_vmaps: the second resize appends nothing, the third (dumping again) does
    assert vec["set_no_dump_vmaps"][1]["lists"]["dumped_depths"] == [6, 4]
    # the cancelled run with dumps holds the first direction's map only
    assert vec["cancel_with_dumps"][1]["lists"]["dumped_depths"][:1] == [20]
    # foreach: attach order, the token handed through, stops at the first value that is not LQR_OK and returns it; _recursive alike
    rec = vec["foreach"][1]
    assert rec["rets"] == [1, 1, 0, 2, 3]
    assert [rec["lists"]["foreach@%d" % i][0] for i in range(5)] == [[0, 1, 2], [0, 1, 2], [0, 1], [0, 1], [0, 1]]
    assert all(t == 1 for i in range(5) for t in rec["lists"]["foreach@%d" % i][1])
    assert vec["foreach_empty"][1]["rets"] == [1, 1]
    # set_use_cache(FALSE): image and map are those of the same resize with the cache on
    a, b = vec["use_cache_off"][0], vec["idle_cancel_then_resize"][0]
    assert np.array_equal(a["image@1"], b["image@3"])


def test_gradient_functions_select_the_builtin_energies_the_table_says(oracle):
    """the genuine energy plane under every LqrGradFuncType equals the oracle's under the builtin the engine maps it to, bit for bit"""
    planes = {}
    for gf, ef in CC.GRADIENT_TO_BUILTIN.items():
        v = next(x for x in MAN["vectors"] if x["name"] == "gradient_%d" % gf)
        z, _ = _load(v)
        if ef not in planes:
            c = L.Carver(oracle, z["img"])
            c.configure(nrg_func=ef)
            planes[ef] = c.energy()
            c.destroy()
        assert np.array_equal(planes[ef].view(np.uint32), z["energy@1"].view(np.uint32)), gf
    assert sorted(set(CC.GRADIENT_TO_BUILTIN.values())) == [0, 1, 2, 6]

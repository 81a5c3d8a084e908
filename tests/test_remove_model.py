"""The object-removal rule itself, without a GPU (tests/remove_cases.py is the specification the engine is held to), run on the CPU oracle:
the model's scan equals a brute-force count; with side-switch frequency 0 the result equals one lqr_carver_resize to the final size and
does not depend on the round size; `restore` gives back the starting size with nothing marked; and the case list meets the conditions
that keep it from going soft."""
import numpy as np
import pytest

import lqr_ctypes as L
import remove_cases as RC

CASES = dict(RC.cases())


model = RC.model


def brute(bias, strength, orientation):
    """(marked, need) by loops over the pixels"""
    h, w = bias.shape
    lines = [[(y, x) for x in range(w)] for y in range(h)] if orientation == 0 else [[(y, x) for y in range(h)] for x in range(w)]
    per_line = [sum(1 for y, x in line if np.float32(bias[y, x]) < np.float32(-strength)) for line in lines]
    return sum(per_line), max(per_line)


@pytest.mark.parametrize("name", ["blobs_w", "lshape_h", "edges_w", "strength_below", "strength_exact", "preserve_h", "auto_tie", "nobias_auto", "pre_transposed_w"])
def test_the_models_scan_equals_a_brute_force_count(name):
    spec = CASES[name]
    c = RC.build(L.oracle_api(), spec, L.OracleCarver)
    got = {o: RC.scan(c, o, spec["strength"]) for o in (0, 1, RC.ORIENTATION_AUTO)}
    bias = c.get_bias()
    want = {o: brute(bias, spec["strength"], o) for o in (0, 1)}
    assert got[0] == want[0] + (0,) and got[1] == want[1] + (1,)
    auto = 1 if want[1][1] < want[0][1] else 0
    assert got[RC.ORIENTATION_AUTO] == want[auto] + (auto,)
    c.destroy()


def test_auto_reports_the_smaller_need_and_a_tie_goes_to_0():
    assert model("auto_rect")["orientation_used"] == 0 and model("auto_lshape")["orientation_used"] == 1
    assert model("auto_fullrow")["orientation_used"] == 1 and model("auto_tie")["orientation_used"] == 0
    c = RC.build(L.oracle_api(), CASES["auto_tie"], L.OracleCarver)
    assert RC.scan(c, 0, 0.0)[1] == RC.scan(c, 1, 0.0)[1] > 0
    c.destroy()


def single_resize(spec, res):
    """one lqr_carver_resize of the same carver to the size the removal ended at"""
    c = RC.build(L.oracle_api(), spec, L.OracleCarver)
    if not RC.is_flat(c):
        assert c.flatten() == L.LQR_OK
    g = c.getters()
    o, k = res["orientation_used"], res["seams"]
    assert c.resize(*((g["width"], g["height"] - k) if o else (g["width"] - k, g["height"]))) == L.LQR_OK
    out = RC.observe(c, {})
    c.destroy()
    return out


NO_SWITCH = [n for n, s in CASES.items() if s["switch"] == 0 and not s["restore"]]


@pytest.mark.parametrize("name", NO_SWITCH)
def test_without_side_switches_the_result_is_one_resize_to_the_final_size_whatever_the_round_size(name):
    res, one = model(name), model(name, 1)
    assert res["ret"] == L.LQR_OK
    for k in ("ret", "orientation_used", "seams", "left"):
        assert res[k] == one[k], k
    assert all(res["getters"][k] == one["getters"][k] for k in ("width", "height", "orientation"))      # (the depth is the rounds' sum)
    assert np.array_equal(res["image"], one["image"]) and all(np.array_equal(a, b) for a, b in zip(res["aux"], one["aux"]))
    if res["seams"]:
        want = single_resize(CASES[name], res)
        assert np.array_equal(res["image"], want["image"]) and all(np.array_equal(a, b) for a, b in zip(res["aux"], want["aux"]))
        assert {k: res["getters"][k] for k in ("width", "height", "orientation")} == {k: want["getters"][k] for k in ("width", "height", "orientation")}
        # the removal's map holds the seams of its rounds, the single resize's only those it needed: they agree on the seams both hold
        a, b = res["vmap"]["data"], want["vmap"]["data"]
        assert np.array_equal(np.where(a <= res["seams"], a, 0), np.where(b <= res["seams"], b, 0))


@pytest.mark.parametrize("name", [n for n, s in CASES.items() if s["restore"]])
def test_restore_gives_back_the_starting_size_with_nothing_marked(name):
    spec, res = CASES[name], model(name)
    assert res["ret"] == L.LQR_OK
    assert (res["getters"]["width"], res["getters"]["height"]) == (spec["w"], spec["h"])
    assert res["image"].shape[:2] == (spec["h"], spec["w"])
    if res["left"] == 0:
        assert not RC.marked_of(res["bias_after"], spec["strength"]).any()


def test_the_case_list_meets_its_conditions():
    res = {n: model(n) for n in CASES}
    assert all(r["ret"] == L.LQR_OK for r in res.values())
    assert sum(1 for r in res.values() if r["seams"] > 0 and r["left"] == 0) >= 6
    capped = [n for n, r in res.items() if r["left"] > 0]
    assert len(capped) >= 2 and any(CASES[n]["mask"] in ("fullrow", "fullcol") for n in capped) and any(CASES[n]["max_seams"] < 48 for n in capped)
    assert sum(1 for r in res.values() if len(r["rounds"]) > 1) >= 4
    assert sum(1 for n, r in res.items() if CASES[n]["mask"] != "none" and CASES[n]["o"] in (0, 1) and not CASES[n]["preserve"] and not CASES[n]["weak"]
               and r["left"] == 0 and r["seams"] > RC.guess_seams(CASES[n])) >= 4
    assert sum(1 for r in res.values() if r["regrown"]) >= 2
    # side switches: the rounds are part of the result
    differ = 0
    for n, r in res.items():
        if CASES[n]["switch"] == 2 and not CASES[n]["restore"] and r["seams"]:
            one = single_resize(CASES[n], r)
            differ += not np.array_equal(r["image"], one["image"])
    assert differ >= 2
    # what the GPU test's shapes are for: every state beforehand, every way a mask arrives, AUTO, the pixel kinds
    specs = list(CASES.values())
    assert {s["pre"] for s in specs} == {None, "transposed", "shrunk"} and {s["via"] for s in specs} == {"rgb", "f", "xy", "device"}
    assert {s["o"] for s in specs} == {0, 1, RC.ORIENTATION_AUTO} and {s["ch"] for s in specs} >= {1, 3, 4}
    assert any(s["attach"] for s in specs) and any(s["delta"] == 2 and s["rigidity"] for s in specs)

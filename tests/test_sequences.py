"""The reference of the call-sequence tests alone (tests/sequence_cases.py), without a GPU: every committed seed's program is run on
the shadow -- the CPU oracle and its bookkeeping -- and the run must be self-consistent, cover the states it claims to cover, and
seldom end early.

Coverage is counted over (op kind, state before the op).  The state classes are flat, shrunk, regrown inside the map, enlarged,
transposed-flat and transposed-not-flat, each crossed with four flags: initialised or not, bias or not, rigidity mask or not,
attached carver or not.  What is asserted: every cell (op kind, class, flag, value) that sequence_cases.feasible() does not rule out
-- its docstring states what cannot exist and why -- is met at least MIN times over the committed seeds.  The generator gets there by
giving every (op kind, class) target ROUNDS seeds whose flags follow sequence_cases.flag_plan.  The table is printed (pytest -s shows
it; NOTES/sequence-tests.md has a copy): per op kind and class, the count with / without each flag, "-" where the cell cannot exist.
"""
import collections
import json

import numpy as np
import pytest

import sequence_cases as S
import sizes_cases as SC
import vmap_cases as VC

MIN = 5                 # occurrences of every (op kind, state class) and (op kind, flag value) pair
MIN_LIFTABLE = 20       # liftable programs that visit each lift-eligible class
MAX_EARLY = 0.10        # share of programs that end early on an error return


@pytest.fixture(scope="module")
def runs():
    """seed -> (program, the shadow's observations); every op's self-consistency is checked as it is made"""
    out = {}
    for seed in S.SEEDS:
        prog = S.program(seed)
        out[seed] = (prog, S.run(None, prog))
    return out


def test_the_generator_is_deterministic_and_programs_round_trip_through_json(runs):
    for seed, (a, _) in runs.items():                   # every committed seed: a second draw, the JSON round trip, the ranges
        assert S.program(seed) == a and json.loads(json.dumps(a)) == a, seed
        assert 4 <= len(a["ops"]) <= 10, (seed, len(a["ops"]))
        i, c = a["image"], a["config"]
        assert (24 <= i["w"] <= 90 or 257 <= i["w"] <= 330) and (8 <= i["h"] <= 60 or 63 <= i["h"] <= 130) and 1 <= i["ch"] <= 4, seed
        assert c["delta"] in (1, 2, 3) and c["rigidity"] in (0.0, 1.0, 8.0) and c["switch_freq"] in (0, 1, 2, 3) and c["enl_step"] in (1.2, 1.5, 2.0), seed
        assert c["nrg"] in range(7) and c["res_order"] in (0, 1), seed
    assert S.program(3) != S.program(3 + len(S.TARGETS))        # (same target, other draw)


def test_new_sessions_have_3_to_40_seams_and_no_side_falls_below_5(runs):
    """a resize that digs below the map it has, the way the carver lies, starts a session: 3 .. 40 seams, a share above 32"""
    sessions = []
    for seed, (prog, seen) in runs.items():
        for op, obs in zip(prog["ops"], seen):
            g0, g1 = obs["state"]["g"], obs["getters"]
            if S.ok_ret(obs["ret"]):
                assert g1["width"] >= S.MIN_SIDE and g1["height"] >= S.MIN_SIDE, (seed, op)
            if op[0] == "resize" and g0["orientation"] == g1["orientation"] and obs["mode"] == "oracle":
                side = "height" if g0["orientation"] else "width"
                lo0 = g0["ref_" + side] - g0["depth"]
                if g1[side] < lo0:
                    sessions.append(lo0 - g1[side])
    assert sessions and min(sessions) >= S.MIN_SEAMS and max(sessions) <= 40, (min(sessions), max(sessions))
    assert sum(n > 32 for n in sessions) >= len(sessions) // 20


def test_the_shadow_is_self_consistent_after_every_op(runs):
    """the image at the last flat point under the map equals what the oracle shows: the bookkeeping that referees read_sizes, the
    reopened carvers and the forward loads; and the read_sizes prediction at the current size is the image"""
    checked = 0
    for seed, (prog, seen) in runs.items():
        for i, (op, obs) in enumerate(zip(prog["ops"], seen)):
            if not S.ok_ret(obs["ret"]):
                break
            g = obs["getters"]
            size = g["height"] if g["orientation"] else g["width"]
            what = "seed %d op %d %s" % (seed, i, op)
            want = VC.model(obs["base"], obs["vmap"], size)
            assert want.shape == obs["image"].shape and np.array_equal(want, obs["image"]), what
            assert np.array_equal(SC.fast_model(obs["base"], obs["vmap"], size), obs["image"]), what
            if obs["aux"] is not None:
                assert np.array_equal(VC.model(obs["aux_base"], obs["vmap"], size), obs["aux"]), what
            if obs["mode"] == "model" or not obs["state"]["init"]:
                assert obs["range"][1] <= size <= obs["range"][2], what                 # (a loaded map serves its own sizes only)
            checked += 1
    assert checked > 4 * len(runs)


def coverage(runs):
    cells, lift = collections.Counter(), collections.Counter()
    for prog, seen in runs.values():
        for op, obs in zip(prog["ops"], seen):
            st = obs["state"]
            for f in S.FLAGS:
                cells[op[0], st["cls"], f, bool(st[f])] += 1
        if S.liftable(seen) and all(S.ok_ret(o["ret"]) for o in seen):
            for cls in {o["state"]["cls"] for o in seen} | {S.classify(seen[-1]["getters"])}:
                lift[cls] += 1
    return cells, lift


def test_every_op_kind_runs_in_every_state_its_precondition_allows(runs):
    cells, lift = coverage(runs)
    show = lambda k, c, f, v: "%d" % cells[k, c, f, v] if S.feasible(k, c, f, v) else "-" if not cells[k, c, f, v] else "(%d)" % cells[k, c, f, v]   # noqa: E731
    lines = ["%-16s%-20s" % ("op kind", "class") + "".join("%12s" % (f + " +/-") for f in S.FLAGS)]
    for kind in S.OPS:
        for c in S.OPS[kind]["classes"]:
            lines.append("%-16s%-20s" % (kind, c) + "".join("%12s" % ("%s/%s" % (show(kind, c, f, True), show(kind, c, f, False))) for f in S.FLAGS))
    lines.append("liftable programs per class: " + ", ".join("%s %d" % (c, lift[c]) for c in S.LIFT_CLASSES))
    print("\n" + "\n".join(lines))
    feasible = [(k, c, f, v) for k in S.OPS for c in S.CLASSES for f in S.FLAGS for v in (True, False) if S.feasible(k, c, f, v)]
    short = ["%s in %s with %s %s: %d" % (x + (cells[x],)) for x in feasible if cells[x] < MIN]
    short += ["liftable programs in %s: %d" % (c, lift[c]) for c in S.LIFT_CLASSES if lift[c] < MIN_LIFTABLE]
    assert not short, short
    # what the rule calls impossible is a small, stated set: the kinds' own preconditions, and uninitialised carvers that are not flat
    for k in S.OPS:
        for c in S.OPS[k]["classes"]:
            for f in S.FLAGS:
                assert S.feasible(k, c, f, True) or S.feasible(k, c, f, False), (k, c, f)
            assert S.feasible(k, c, "aux", True) and S.feasible(k, c, "aux", False), (k, c)


def test_few_programs_end_early_and_none_before_its_third_op(runs):
    early = [(seed, len(seen)) for seed, (prog, seen) in runs.items() if not S.ok_ret(seen[-1]["ret"])]
    for seed, (prog, seen) in runs.items():
        assert all(S.ok_ret(o["ret"]) for o in seen[:-1]), seed
        assert len(seen) == len(prog["ops"]), seed          # (an error return is the last op the generator drew)
    assert len(early) <= MAX_EARLY * len(runs), early
    assert all(n >= 3 for _, n in early), early
    assert early                                            # (the error path is run at all)

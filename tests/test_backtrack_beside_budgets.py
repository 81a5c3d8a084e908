"""k_carve_v<NRG, DELTA> (the backtrack and the energy update beside the carve, one launch: csrc/k_carve.hip) in the built library's
code-object metadata, in the manner of tests/test_kernel_budgets.py (CPU test, no GPU needed).

The launch is the carve's: its bandwidth rests on five waves per SIMD, that is 96 registers, and on five workgroups per compute unit,
that is at most 32 KB of static LDS each (160 KB per compute unit).  The walk role and the energy role are compiled into the same
kernel and registers are allocated per kernel, so either can take the carve over the boundary "without a word"."""
import os
import re

import pytest

import kernel_meta as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("LQR_BUDGET_LIB") or os.path.join(ROOT, "gimp-lqr-plugin_amd", "liblqr-hip.so")
FORMS = sorted("k_carve_v<%d, %d>" % (nrg, delta) for nrg in range(7) for delta in (1, 2))
MAX_REGS = 96
MAX_LDS = 32 * 1024


@pytest.fixture(scope="module")
def meta():
    if not KM.tools_available():
        pytest.skip("no LLVM object tools on this machine")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return KM.kernels(LIB)


def test_every_form_exists_and_no_other(meta):
    assert sorted(n for n in meta if n.startswith("k_carve_v<")) == FORMS


def violations(meta):
    bad = []
    for name in FORMS:
        d = meta[name]
        regs = d["vgpr_count"] + d["agpr_count"]
        if regs > MAX_REGS:
            bad.append("%s: %d VGPRs + AGPRs, budget %d (five waves per SIMD)" % (name, regs, MAX_REGS))
        if d["private_segment_fixed_size"] or d["vgpr_spill_count"] or d["sgpr_spill_count"]:
            bad.append("%s: %d B of scratch, %d VGPRs and %d SGPRs spilled; budget: none" % (
                name, d["private_segment_fixed_size"], d["vgpr_spill_count"], d["sgpr_spill_count"]))
        if d["group_segment_fixed_size"] > MAX_LDS:
            bad.append("%s: %d B of static LDS, budget %d (five workgroups per compute unit)" % (name, d["group_segment_fixed_size"], MAX_LDS))
    return bad


def test_every_form_is_within_the_carves_budget(meta):
    bad = violations(meta)
    assert not bad, "\n".join(bad)


def test_checker_is_red_on_doctored_metadata(meta):
    import copy
    fat = copy.deepcopy(meta)
    fat[FORMS[0]]["vgpr_count"] = 102
    fat[FORMS[1]]["private_segment_fixed_size"] = 20
    fat[FORMS[1]]["vgpr_spill_count"] = 5
    fat[FORMS[2]]["group_segment_fixed_size"] = 40 * 1024
    bad = violations(fat)
    assert len(bad) == 3 and all(re.match(re.escape(f), b) for f, b in zip(FORMS, bad)), bad


def test_no_flag_of_the_walk_role_goes_through_flat(meta):
    """the chase and the publishing wave talk through LDS (LDS_FLAG, lqr_common.h): a FLAT access there would drain the chase's prefetch"""
    counts = KM.instruction_counts(LIB)
    for name in FORMS:
        assert counts[name].get("flat_load_dword", 0) == 0 and counts[name].get("flat_store_dword", 0) == 0, (name, counts[name])

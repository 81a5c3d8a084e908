"""k_carve_u<NRG> (the energy update beside the carve, one launch: csrc/k_carve.hip) in the built library's code-object metadata,
without a GPU.  The carve role must keep k_carve's 5 waves per SIMD -- its bandwidth rests on them -- so every instantiation stays
within 96 VGPRs, without scratch or spills, and within 12 KB of LDS (the energy role's staging rows and table of v / 255: five
workgroups per compute unit hold 57.6 of 160 KB).  All seven energy functions are instantiated.  k_carve itself is the kernel it was:
the same registers and, with the compiler the figures were recorded with, the same instructions (scripts/kernel_diff.py shows the same
between two builds)."""
import hashlib
import os

import pytest

import kernel_meta as KM
from test_kernel_budgets import LIB, compiler_is_the_recorded_one

# k_carve at the commit before k_carve_u: sha256 of its disassembly (mnemonics and operands, one per line) and its length
K_CARVE_SHA256_16, K_CARVE_INSTRUCTIONS = "3a24787451ae55cc", 2569


@pytest.fixture(scope="module")
def meta():
    if not KM.tools_available():
        pytest.skip("no LLVM object tools on this machine")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return KM.kernels(LIB)


def test_every_form_keeps_the_carves_occupancy(meta):
    forms = {n: d for n, d in meta.items() if n.startswith("k_carve_u<")}
    assert sorted(forms) == ["k_carve_u<%d>" % i for i in range(7)], sorted(forms)
    for name, d in forms.items():
        print(name, d)
        assert d["vgpr_count"] + d["agpr_count"] <= 96, (name, d)
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (name, d)
        assert d["group_segment_fixed_size"] <= 12 * 1024, (name, d)
        assert d["max_flat_workgroup_size"] == 256, (name, d)


def test_no_form_reaches_lds_or_memory_through_flat_instructions(meta):
    counts = KM.instruction_counts(LIB)
    for i in range(7):
        c = counts["k_carve_u<%d>" % i]
        assert c["flat_load_dword"] == 0 and c["flat_store_dword"] == 0, (i, c)


def test_k_carve_is_unchanged(meta):
    d = meta["k_carve"]
    assert (d["vgpr_count"], d["agpr_count"], d["group_segment_fixed_size"], d["private_segment_fixed_size"], d["vgpr_spill_count"]) == (96, 0, 0, 0, 0), d
    text = KM.disassembly(LIB)["k_carve"]
    same = len(text) == K_CARVE_INSTRUCTIONS and hashlib.sha256("\n".join(text).encode()).hexdigest()[:16] == K_CARVE_SHA256_16
    if not same and not compiler_is_the_recorded_one():
        pytest.xfail("k_carve's instructions were recorded with another compiler release (%d instructions here)" % len(text))
    assert same, "k_carve changed: %d instructions, recorded %d" % (len(text), K_CARVE_INSTRUCTIONS)

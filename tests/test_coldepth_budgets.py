"""Register budgets of the kernels a colour-depth carver runs -- the value / deep forms (csrc/lqr_pixel.h) of the kernels in
csrc/k_energy.hip and csrc/k_oneoff.hip -- checked at build time from the library's code-object metadata (tests/kernel_meta.py),
as tests/test_kernel_budgets.py does for the 8-bit ones: none may use scratch, the energy update next to the seam keeps the
8 waves per SIMD of its 8-bit form, and every kernel the shim launches for a deep carver is there under its name, and no other:
the value forms exist for energies 0, 1, 2 and 6 (on the value plane 3, 4, 5 are 0, 1, 2; plane_nrg in csrc/lqr_shim.hip)."""
import os
import re

import pytest

import kernel_meta as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("LQR_BUDGET_LIB") or os.path.join(ROOT, "gimp-lqr-plugin_amd", "liblqr-hip.so")

# (regular expression on the demangled name, max VGPRs + AGPRs, instances expected, why)
BUDGETS = [
    (r"^k_wk_init<PixValue<[123]> ?>$", 48, 3, "E1 on the value plane: a streaming pass"),
    (r"^k_wk_init_visible<PixValue<[123]> ?>$", 64, 3, "E1 on a multi-size image: one block per row"),
    (r"^k_emap_full<[0-6], true>$", 32, 4, "E3/E4: one pixel per thread"),
    (r"^k_emap_update<[0-6], 12, true>$", 64, 4, "delta_x <= 2: 8 waves per SIMD, as k_emap_update<N, 12, false>"),
    (r"^k_emap_update<[0-6], (36|68), true>$", 512, 8, "delta_x 3 .. 16: the 8-bit kernel's staging, 8-byte samples"),
    (r"^k_frozen_catchup<true>$", 48, 1, "the frozen value plane brought forward"),
    (r"^k_inflate<true>$", 64, 1, "E14 with the depth's averaging and the fused level check"),
    (r"^k_transpose_px$", 48, 1, "E11 for pixels wider than 4 bytes"),
    (r"^k_compact<true>$", 64, 1, "E12 read-out of pixels wider than 4 bytes"),
    (r"^k_compact_jobs<true>$", 64, 1, "E11 flatten of pixels wider than 4 bytes"),
]


@pytest.fixture(scope="module")
def meta():
    if not KM.tools_available():
        pytest.skip("no LLVM object tools on this machine")
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    return KM.kernels(LIB)


def test_colour_depth_kernels_are_within_budget_and_use_no_scratch(meta):
    bad = []
    for pat, max_regs, count, why in BUDGETS:
        found = [n for n in meta if re.search(pat, n)]
        if len(found) != count:
            bad.append("%s: %d kernels, expected %d" % (pat, len(found), count))
        for n in found:
            d = meta[n]
            regs = d["vgpr_count"] + d["agpr_count"]
            if regs > max_regs or d["private_segment_fixed_size"] or d["vgpr_spill_count"]:
                bad.append("%s: %d VGPRs, %d B scratch, %d spilled VGPRs -- budget %d / 0 / 0: %s" % (
                    n, regs, d["private_segment_fixed_size"], d["vgpr_spill_count"], max_regs, why))
    assert not bad, "\n".join(bad)

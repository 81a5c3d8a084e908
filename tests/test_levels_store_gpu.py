"""The level kernel writes back only the rows of a level that changed (csrc/k_levels_body.inc; lqrhip_set_levels_store), against the
form that writes every row and against the oracle.

Every case carves the same inputs as a lock-step group on the level kernel (update mode 5, one stream, the slot count pinned) with the
hook at 0 (every row of every processed tile-level, as before) and at 1 (of an interior tile only the rows on which an own pixel
changed), as sessions of 1, 2, .. seams, and compares what the seam loop left after the last seam of each -- the state after every seam
-- bit for bit: the seams, the energies, cumulative minima and back pointers (lqrx_set_debug's planes), the flags of the last seam, the
pixels, and the level kernel's event counters 0 .. 4.  The longest session is then compared with the oracle, planes included.  Counters
5 and 6 are the rows written back and the rows skipped: nothing is skipped with the hook at 0, and both hooks count the same rows.

Only k_band_levels2 (two slots per workgroup) has the form: the one-slot family k_band_levels ignores the hook and writes every row
(keeping the change bits costs the groups it serves more than the stores it would save), so with one slot per workgroup both runs
are the same kernel doing the same, nothing is skipped, and the comparison holds trivially.

Shapes (width x height) 130 x 33, 200 x 70, 520 x 100, 1100 x 65 as tests/test_levels_pair_gpu.py, and 131 x 33, whose last own lane
holds one pixel inside and one outside the frame (a tile that is not interior: written whole).  Slots per image 2, 3, 8 and 12, groups of
1, 2, 9 and 17 images, one and two slots per workgroup (k_band_levels and k_band_levels2)."""
import ctypes

import numpy as np
import pytest

import datasets as D
from test_carve_beside_gpu import oracle_ref, same_state
from test_forms_gpu import assert_same
from test_levels_pair_gpu import carve_group, images, level_stats

pytestmark = pytest.mark.gpu

SHAPES = [(130, 33), (200, 70), (520, 100), (1100, 65), (131, 33)]
SLOTS = [2, 3, 8, 12]
GROUPS = [1, 2, 9, 17]


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    for f in ("lqrhip_set_levels_store", "lqrhip_set_levels_wg_slots", "lqrhip_set_band_levels", "lqrhip_set_update_mode", "lqrhip_set_sub_batches"):
        getattr(lb, f).restype, getattr(lb, f).argtypes = None, [ctypes.c_int]
    lb.lqrhip_band_levels_stats.restype, lb.lqrhip_band_levels_stats.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_debug_seam_flags.restype = ctypes.c_int
    lb.lqrhip_debug_seam_flags.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
    lb.lqrhip_set_sub_batches(1); lb.lqrhip_set_update_mode(5)
    lb.lqrhip_fault_stats((ctypes.c_ulonglong * 8)(), 1)
    yield lb
    lb.lqrhip_set_levels_store(-1); lb.lqrhip_set_levels_wg_slots(-1); lb.lqrhip_set_band_levels(-1); lb.lqrhip_set_update_mode(-1)
    lb.lqrhip_set_sub_batches(0)
    engine.lqrx_set_debug(0)


def check(oracle, engine, lib, imgs, P, wg_slots, seams, what, prefixes=None, masks=None, **kw):
    """both hooks after each session of `prefixes` seams; returns the level kernel's counters of the (every-row, changed-rows) runs of the
    longest session"""
    w = imgs[0].shape[1]
    masks = masks or [None] * len(imgs)
    lib.lqrhip_set_band_levels(P); lib.lqrhip_set_levels_wg_slots(wg_slots)
    engine.lqrx_set_debug(1)
    last, events = None, {}
    for k in prefixes or range(1, seams + 1):
        outs = {}
        for mode in (0, 1):
            lib.lqrhip_set_levels_store(mode)
            level_stats(lib)
            outs[mode] = carve_group(engine, imgs, masks, w - k, kw)
            events[mode] = level_stats(lib)
            faults = (ctypes.c_ulonglong * 8)()
            lib.lqrhip_fault_stats(faults, 0)
            assert not any(faults[i] for i in (0, 1, 4, 6)), "%s: a session was redone %s" % (what, list(faults))
            print("%s, %d seams, hook %d: events %s, rows written %d, skipped %d" % (what, k, mode, events[mode][:5], events[mode][5], events[mode][6]))
        assert events[0][:5] == events[1][:5], "%s after %d seams: the level kernel's events %s writing every row, %s writing the changed ones" % (what, k, events[0][:5], events[1][:5])
        assert events[0][6] == 0, "%s after %d seams: %d rows skipped with the hook at 0" % (what, k, events[0][6])
        assert events[0][5] == events[1][5] + events[1][6], "%s after %d seams: rows %s with the hook at 0, %s at 1" % (what, k, events[0][5:7], events[1][5:7])
        # (the update behind a session's last seam is not run, and a side switch replaces one by a full DP)
        assert events[1][2] > 0 or k < 3,"%s after %d seams: the level kernel did not run" % (what, k)
        for i, (a, b) in enumerate(zip(outs[0], outs[1])):
            same_state(a, b, "%s, image %d after %d seams" % (what, i, k))
            assert a["flags"] == b["flags"], "%s, image %d after %d seams: flags %s writing every row, %s writing the changed ones" % (what, i, k, a["flags"], b["flags"])
        last = outs[1]
    for i, (im, mk, got) in enumerate(zip(imgs, masks, last)):
        assert_same(oracle_ref(oracle, im, mk, got["getters"]["width"], kw), got, "%s, image %d against the oracle" % (what, i))
    return events


# every shape with every slot count and both families; the group size goes round with them, so that each size meets each shape
@pytest.mark.parametrize("wg_slots", [1, 2])
@pytest.mark.parametrize("P", SLOTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_slots_and_groups(oracle, engine, lib, w, h, P, wg_slots):
    n = GROUPS[(SHAPES.index((w, h)) + SLOTS.index(P) + wg_slots) % len(GROUPS)]
    check(oracle, engine, lib, images(w, h, n, 5000 + w + P), P, wg_slots, 3, "%d x %d x %d, %d slots, %d per workgroup" % (n, w, h, P, wg_slots), switch_freq=0)


@pytest.mark.parametrize("rigidity", [0.0, 4.0])
@pytest.mark.parametrize("P,wg_slots", [(3, 1), (8, 2)])
def test_both_sides_across_a_side_switch_with_and_without_rigidity(oracle, engine, lib, P, wg_slots, rigidity):
    """side switch frequency 2: the first half of the session picks the leftmost of equal minima, the second the rightmost (LR false and
    true), with a full DP between them"""
    check(oracle, engine, lib, images(520, 100, 9, 5100), P, wg_slots, 6, "side switch, %d slots, rigidity %g" % (P, rigidity), prefixes=[2, 3, 4, 6], switch_freq=2, rigidity=rigidity)


@pytest.mark.parametrize("variant", ["delta2", "delta2-rigidity", "rigmask"])
def test_the_other_row_functions(oracle, engine, lib, variant):
    """dp_row_g: delta_x 2 (a level is 16 rows) with and without rigidity, and a rigidity mask at delta_x 1 (RIGM: 16 rows too)"""
    w, h = 520, 100
    kw = {"delta2": dict(delta_x=2), "delta2-rigidity": dict(delta_x=2, rigidity=4.0), "rigmask": dict(rigidity=6.0, rigmask=D.top_half_mask(w, h))}[variant]
    check(oracle, engine, lib, images(w, h, 9, 5200), 8, 1, 4, variant, prefixes=[2, 3, 4], switch_freq=0, **kw)


def test_everything_changes_and_an_image_stops(oracle, engine, lib):
    """the flat image of test_an_image_that_stops_stops_alike: the first seam takes its one strongly negative pixel on row 0 away, the
    whole cone below it changes (no row of its tiles is skipped) and with 2 slots per image the image stops; it must stop at the same
    row (the same images stopped, the same tile-levels processed) and leave the same planes after the sweep"""
    w, h = 1100, 300
    flat = np.full((h, w, 4), 128, np.uint8)
    flat[..., 3] = 255
    dot = np.zeros((h, w), np.uint8)
    dot[0, w // 2] = 255
    imgs, masks = [flat, D.noise(w, h, 5301)], [dot, np.zeros((h, w), np.uint8)]
    for wg_slots in (1, 2):
        events = check(oracle, engine, lib, imgs, 2, wg_slots, 3, "a stopped image, %d slots per workgroup" % wg_slots, prefixes=[2, 3], masks=masks, switch_freq=0, disc_coeff=100000)
        assert events[1][0] == events[0][0] > 0, events


@pytest.mark.parametrize("wg_slots", [1, 2])
def test_rows_are_skipped_on_noise_and_counted(oracle, engine, lib, wg_slots):  # (one slot per workgroup: counted, never skipped)
    """noise images of four levels: a seam's band crosses most rows of the tiles it runs through, so with the hook at 1 most rows are
    still written (about four in five at 4K) and some -- those of tiles that are active only because the band is within reach of their
    halo -- are skipped; with the hook at 0 none is skipped (check asserts it) and the totals agree"""
    w, h = 520, 100
    events = check(oracle, engine, lib, [D.noise(w, h, 5400 + i) for i in range(9)], 8, wg_slots, 4, "counters, %d slots per workgroup" % wg_slots, prefixes=[4], switch_freq=0)
    assert events[1][5] > 0 and (events[1][6] > 0 if wg_slots == 2 else events[1][6] == 0), events
    assert events[0][6] == 0 and events[0][5] == events[1][5] + events[1][6], events

"""k_band_levels2: two slots of an image per 256-thread workgroup (csrc/k_levels2.hip; lqrhip_set_levels_wg_slots), against the
one-slot form k_band_levels and against the oracle.

Every case carves the same inputs as a lock-step group on the level kernel (update mode 5, the slot count pinned) with the hook at 1
and at 2, as sessions of 1, 2, .. seams, and compares what the seam loop left after the last seam of each -- the state after every
seam -- bit for bit: the seams (the visibility map), the energies, cumulative minima and back pointers (lqrx_set_debug's planes), the
flags of the last seam, the pixels.  The longest session is then compared with the oracle, planes included, and
lqrhip_levels_pair_launches must say that the form ran (never with the hook at 1).

Shapes (width x height) 130 x 33, 200 x 70, 520 x 100 and 1100 x 65: 3, 4, 9 and 18 tiles of 64 columns, 2 to 4 levels of 32 rows, the
last one partial.  Slots per image 2, 3, 4, 7, 8 and 12: odd counts (the last workgroup's second slot does not exist), more slots than
tiles, and half the slots equal to a band's width.  Groups of 1, 2, 9 and 17 images: beyond the eight an XCD round takes, and no
multiple of eight."""
import ctypes

import numpy as np
import pytest

import datasets as D
import harness as H
import lqr_ctypes as L
from test_carve_beside_gpu import oracle_ref, same_state
from test_forms_gpu import assert_same, read_out

pytestmark = pytest.mark.gpu

SHAPES = [(130, 33), (200, 70), (520, 100), (1100, 65)]
SLOTS = [2, 3, 4, 7, 8, 12]
GROUPS = [1, 2, 9, 17]


@pytest.fixture()
def lib(engine):
    lb = engine.lib
    for f in ("lqrhip_set_levels_wg_slots", "lqrhip_set_band_levels", "lqrhip_set_update_mode", "lqrhip_band_levels_debug", "lqrhip_set_sub_batches", "lqrhip_set_no_spin"):
        getattr(lb, f).restype, getattr(lb, f).argtypes = None, [ctypes.c_int]
    lb.lqrhip_levels_pair_launches.restype, lb.lqrhip_levels_pair_launches.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    lb.lqrhip_band_levels_stats.restype, lb.lqrhip_band_levels_stats.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lb.lqrhip_fault_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lb.lqrhip_debug_seam_flags.restype = ctypes.c_int
    lb.lqrhip_debug_seam_flags.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
    lb.lqrhip_set_sub_batches(1); lb.lqrhip_set_update_mode(5)
    lb.lqrhip_fault_stats((ctypes.c_ulonglong * 8)(), 1)
    yield lb
    lb.lqrhip_set_levels_wg_slots(-1); lb.lqrhip_set_band_levels(-1); lb.lqrhip_set_update_mode(-1); lb.lqrhip_band_levels_debug(0)
    lb.lqrhip_set_sub_batches(0); lb.lqrhip_debug_inject(0, 0, 0); lb.lqrhip_set_no_spin(0)
    engine.lqrx_set_debug(0)


def level_stats(lib, reset=True):
    st = (ctypes.c_ulonglong * 8)()
    assert lib.lqrhip_band_levels_stats(st, 1 if reset else 0) == 0
    return [int(x) for x in st]


def carve_group(api, imgs, masks, nw, kw):
    """the images as one lock-step group down to nw columns: what the seam loop left, per image, the last seam's flags included"""
    cs = [H.init_carver(api, im, nw, im.shape[0], disc=mk, **kw)[0] for im, mk in zip(imgs, masks)]
    ret = L.resize_batch(api, cs, nw, imgs[0].shape[0])
    outs = [read_out(c, ret) for c in cs]
    for c, o in zip(cs, outs):
        f = [ctypes.c_int(-1) for _ in range(3)]
        assert api.lib.lqrhip_debug_seam_flags(c.p, *[ctypes.byref(x) for x in f]) == 0
        o["flags"] = tuple(x.value for x in f)          # (origin, origin before the last seam, its side)
    for c in cs:
        c.destroy()
    return outs


def images(w, h, n, seed):
    return [D.photo_like(w, h, seed + i) if i % 2 else D.noise(w, h, seed + i) for i in range(n)]


def check(oracle, engine, lib, imgs, P, seams, what, prefixes=None, masks=None, **kw):
    """both forms after each session of `prefixes` seams; returns the level kernel's event counters of the (one-slot, two-slot) runs"""
    w = imgs[0].shape[1]
    masks = masks or [None] * len(imgs)
    lib.lqrhip_set_band_levels(P)
    engine.lqrx_set_debug(1)
    last, events = None, {}
    for k in prefixes or range(1, seams + 1):
        outs = {}
        for slots in (1, 2):
            lib.lqrhip_set_levels_wg_slots(slots)
            lib.lqrhip_levels_pair_launches(1); level_stats(lib)
            outs[slots] = carve_group(engine, imgs, masks, w - k, kw)
            ran, events[slots] = lib.lqrhip_levels_pair_launches(1), level_stats(lib)
            faults = (ctypes.c_ulonglong * 8)()
            lib.lqrhip_fault_stats(faults, 0)
            assert not any(faults[i] for i in (0, 1, 4, 6)), "%s: a session was redone %s" % (what, list(faults))
            print("%s, %d seams, %d slots per workgroup: %d two-slot launches, events %s" % (what, k, slots, ran, events[slots][:5]))
            # (the update behind a session's last seam is not run, and a side switch replaces one by a full DP)
            assert ran == 0 if slots == 1 else (ran > 0 or k < 3), (what, k, slots, ran)
        assert events[1] == events[2], "%s after %d seams: the level kernel's events %s with one slot per workgroup, %s with two" % (what, k, events[1], events[2])
        for i, (a, b) in enumerate(zip(outs[1], outs[2])):
            same_state(a, b, "%s, image %d after %d seams" % (what, i, k))
            assert a["flags"] == b["flags"], "%s, image %d after %d seams: flags %s with one slot per workgroup, %s with two" % (what, i, k, a["flags"], b["flags"])
        last = outs[2]
    for i, (im, mk, got) in enumerate(zip(imgs, masks, last)):
        assert_same(oracle_ref(oracle, im, mk, got["getters"]["width"], kw), got, "%s, image %d against the oracle" % (what, i))
    return events


# every shape with every slot count; the group size goes round with them, so that each size meets each shape and each parity of P
@pytest.mark.parametrize("P", SLOTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_slots_and_groups(oracle, engine, lib, w, h, P):
    n = GROUPS[(SHAPES.index((w, h)) + SLOTS.index(P)) % len(GROUPS)]
    check(oracle, engine, lib, images(w, h, n, 4000 + w + P), P, 3, "%d x %d x %d, %d slots" % (n, w, h, P), switch_freq=0)


@pytest.mark.parametrize("rigidity", [0.0, 4.0])
@pytest.mark.parametrize("P", [3, 8])
def test_both_sides_across_a_side_switch_with_and_without_rigidity(oracle, engine, lib, P, rigidity):
    """side switch frequency 2: the first half of the session picks the leftmost of equal minima, the second the rightmost (LR false and
    true), with a full DP between them"""
    check(oracle, engine, lib, images(520, 100, 9, 4100), P, 6, "side switch, %d slots, rigidity %g" % (P, rigidity), prefixes=[2, 3, 4, 6], switch_freq=2, rigidity=rigidity)


@pytest.mark.parametrize("switch", [4, 8])
@pytest.mark.parametrize("P", [3, 8])
def test_debug_switches(oracle, engine, lib, P, switch):
    """4: no near copy of the hand-over words; 8: an image's workgroups on different XCDs"""
    lib.lqrhip_band_levels_debug(switch)
    check(oracle, engine, lib, images(1100, 65, 9, 4200), P, 3, "debug switch %d, %d slots" % (switch, P), switch_freq=0)


def test_an_image_that_stops_stops_alike(oracle, engine, lib):
    """a flat image whose one strongly negative pixel on row 0 owns a cone of cumulative minima that widens by two columns per row: the
    first seam takes that pixel away, the whole cone changes, and with 2 slots per image a band of five tiles puts three on one slot --
    the image stops there and the sweep redoes the rows below.  Asserted on the one-slot form first; the two-slot form must count the
    same events (images stopped, tile-levels processed: the same row) and leave the same planes after the sweep"""
    w, h = 1100, 300
    flat = np.full((h, w, 4), 128, np.uint8)
    flat[..., 3] = 255
    dot = np.zeros((h, w), np.uint8)
    dot[0, w // 2] = 255
    imgs, masks = [flat, D.noise(w, h, 4301)], [dot, np.zeros((h, w), np.uint8)]
    lib.lqrhip_set_band_levels(2); lib.lqrhip_set_levels_wg_slots(1)
    engine.lqrx_set_debug(1)
    level_stats(lib)
    carve_group(engine, imgs, masks, w - 3, dict(switch_freq=0, disc_coeff=100000))
    stopped = level_stats(lib)[0]
    assert stopped > 0, "the one-slot form stopped no image on this input: the case is empty"
    events = check(oracle, engine, lib, imgs, 2, 3, "a stopped image", prefixes=[2, 3], masks=masks, switch_freq=0, disc_coeff=100000)
    assert events[2][0] == events[1][0] > 0, events


@pytest.mark.parametrize("kind", [1, 2])
def test_a_session_redone_after_a_fault_is_exact(oracle, engine, lib, kind):
    """an injected spin time-out (1) or failed activity prediction (2) with the form forced: the session is rolled back and carved again
    on the kernels without spin waits -- never this form -- and is exact, as in tests/test_faults_gpu.py"""
    w, h, n = 520, 100, 9
    imgs = images(w, h, n, 4400)
    st = (ctypes.c_ulonglong * 8)()
    lib.lqrhip_set_band_levels(8); lib.lqrhip_set_levels_wg_slots(2)
    engine.lqrx_set_debug(1)
    lib.lqrhip_levels_pair_launches(1)
    carve_group(engine, imgs, [None] * n, w - 9, dict(switch_freq=0))
    clean = lib.lqrhip_levels_pair_launches(1)             # what one session launches when nothing goes wrong
    assert clean >= 8, clean
    lib.lqrhip_fault_stats(st, 1)
    lib.lqrhip_debug_inject(kind, 4, 1)                    # the fault falls into seam step 4; the session's end finds it
    outs = carve_group(engine, imgs, [None] * n, w - 9, dict(switch_freq=0))
    lib.lqrhip_fault_stats(st, 1)
    lib.lqrhip_set_no_spin(0)
    injected, rolled_back, redone = int(st[5]), int(st[4]), int(st[6])
    assert injected == 1 and rolled_back >= 1 and redone >= 1, list(st)
    ran = lib.lqrhip_levels_pair_launches(1)
    assert 0 < ran <= clean, (ran, clean)                  # the failed session's launches; the redone session adds none
    for i, (im, got) in enumerate(zip(imgs, outs)):
        assert got["ret"] == L.LQR_OK
        assert_same(oracle_ref(oracle, im, None, w - 9, dict(switch_freq=0)), got, "redone session after fault %d, image %d" % (kind, i))

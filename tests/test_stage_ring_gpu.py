"""The pinned transfer ring at its real size (-m gpu): 16 slots of 4 MiB (gimp-lqr-plugin_amd/csrc/lqr_stage.h, as lqr_shim.hip makes it).
Every image enters and leaves the engine through it.  tests/test_stage.py drives the ring's logic around every boundary of a ring of
4 x 64 bytes on the CPU; this guards the real constants through the C ABI alone: a one-channel 8-bit carver of seeded random bytes is
made (the upload) and read back with lqrx_carver_read_image (the download), and every byte is compared.  The shapes are the smallest
that cross each boundary; the largest moves 128 MiB each way."""
import numpy as np
import pytest

import lqr_ctypes as L

pytestmark = pytest.mark.gpu

SHAPES = [                  # w, h, what it crosses
    (1, 1, "one byte"),
    (2047, 2049, "one byte short of a slot"),
    (2048, 2048, "one slot exactly"),
    (2049, 2048, "a slot and a short chunk"),
    (8191, 8193, "one byte short of the whole ring"),
    (8192, 8192, "the ring exactly"),
    (8192, 8193, "17 chunks: the first slot reused"),
    (16384, 8193, "33 chunks: two wraps"),
]


@pytest.mark.parametrize("w,h", [s[:2] for s in SHAPES], ids=["%dx%d" % s[:2] for s in SHAPES])
def test_an_image_comes_back_through_the_ring_byte_for_byte(engine, w, h):
    img = np.random.default_rng(w * 100003 + h).integers(0, 256, (h, w, 1), dtype=np.uint8)
    c = L.Carver(engine, img, init=False)           # no working planes: the base layout alone
    try:
        out = c.read_image()
    finally:
        c.destroy()
        engine.lib.lqrhip_pool_trim()               # up to 0.8 GiB per case: not left in the cache for the rest of the suite
    assert out.shape == img.shape
    assert np.array_equal(out, img), "%d of %d bytes differ, the first at %d" % (
        np.count_nonzero(out != img), img.size, int(np.flatnonzero(out.ravel() != img.ravel())[0]))

"""The static-seam rule without a GPU (include_ext/lqr_static.h, tests/static_cases.py): the gradient model is the CPU oracle's
lqr_carver_get_true_energy, n = 1 and the two ends of alpha isolate the terms, S does not see the order of the frames and T does, and
on a clip in which a bright block crosses a dark picture no static seam touches any position of the block -- while the seams of the first
frame alone do."""
import numpy as np
import pytest

import coldepth_cases as CD
import forward_cases as FC
import imgtype_cases as IT
import lqr_ctypes as L
import static_cases as SC

F = np.float32
bits = CD.bits


def clip(n, w=37, h=21, ch=3, seed=5):
    rng = np.random.default_rng([seed, n, w, h, ch])
    return [CD.base_image(rng, w, h, ch) for _ in range(n)]


@pytest.mark.parametrize("nrg", range(7))
@pytest.mark.parametrize("w,h", [(33, 17), (9, 1), (1, 9), (2, 2)])
def test_the_gradient_model_is_the_oracles_true_energy(oracle, nrg, w, h):
    """8-bit RGB with a bias, both orientations; a frame one pixel wide is where liblqr (and its restatement) reads outside the frame
    and the engine, which the model follows, has no gradient along the line (include/lqr_energy.h): those are left to the GPU test"""
    img = CD.base_image(np.random.default_rng([11, nrg, w, h]), w, h, 3)
    bias = np.random.default_rng([12, w, h]).uniform(-1.0, 1.0, (h, w)).astype(F)
    st = IT.TypeState(3)
    for o in (0, 1):
        if (h if o else w) == 1:
            continue
        c = L.OracleCarver(oracle, img, init=False)
        c.configure(nrg_func=nrg)
        assert c.bias_add_f(bias.astype(np.float64), 2) == 1
        want = c.get_energy(o, true=True)
        c.destroy()
        got = SC.true_energy(IT.model_value(img, 0, st, SC.is_luma(nrg)), nrg, o, bias)
        assert np.array_equal(bits(got), bits(want)), (nrg, o)


def test_one_frame_gives_alpha_times_its_energy():
    (img,) = clip(1)
    st = IT.TypeState(3)
    S = SC.true_energy(IT.model_value(img, 0, st, False), 0, 0)
    for alpha in (0.0, 0.3, 1.0):
        E = SC.static_energy([img], 0, st, 0, 0, alpha)
        assert np.array_equal(bits(E), bits((F(alpha) * S).astype(F) + F(0)))          # T = 0: fl(1 - alpha) * 0 = 0
    assert np.array_equal(bits(SC.static_energy([img], 0, st, 0, 0, 1.0)), bits(S))


@pytest.mark.parametrize("o", (0, 1))
def test_alpha_one_and_zero_isolate_the_two_terms(o):
    imgs, st = clip(5), IT.TypeState(3)
    S, T = SC.planes(imgs, 0, st, 1, o)
    assert np.array_equal(bits(SC.static_energy(imgs, 0, st, 1, o, 1.0)), bits(S))
    assert np.array_equal(bits(SC.static_energy(imgs, 0, st, 1, o, 0.0)), bits(T))
    each = [SC.true_energy(IT.model_value(im, 0, st, False), 1, o) for im in imgs]
    assert np.array_equal(bits(S), bits(np.max(each, axis=0)))
    I = [FC.intensity(im, 0, st, False) for im in imgs]
    assert np.array_equal(bits(T), bits(np.max([np.abs(I[t] - I[t - 1]) for t in range(1, 5)], axis=0)))
    assert S.any() and T.any() and (T >= 0).all()


def test_the_order_of_the_frames_matters_to_t_only():
    imgs, st = clip(4), IT.TypeState(3)
    S, T = SC.planes(imgs, 0, st, 0, 0)
    swapped = [imgs[0], imgs[2], imgs[1], imgs[3]]
    S2, T2 = SC.planes(swapped, 0, st, 0, 0)
    assert np.array_equal(bits(S), bits(S2)) and not np.array_equal(bits(T), bits(T2))
    assert np.array_equal(bits(SC.static_energy(imgs, 0, st, 0, 0, 1.0)), bits(SC.static_energy(swapped, 0, st, 0, 0, 1.0)))
    assert not np.array_equal(bits(SC.static_energy(imgs, 0, st, 0, 0, 0.3)), bits(SC.static_energy(swapped, 0, st, 0, 0, 0.3)))
    # reversing a clip reverses the differences: the same T
    S3, T3 = SC.planes(imgs[::-1], 0, st, 0, 0)
    assert np.array_equal(bits(S3), bits(S)) and np.array_equal(bits(T3), bits(T))


def test_no_static_seam_touches_a_block_that_crosses_the_clip_and_the_first_frames_seams_do(oracle):
    """96 x 24, six frames, an 8 x 8 block of 255 on black moving left to right; 24 vertical seams, the oracle as the seam finder"""
    frames, union = SC.crossing_block()
    st = IT.TypeState(1)
    E = SC.static_energy(frames, 0, st, 2, 0, SC.PAPER_ALPHA)
    assert (E[union] > 0).any() and not E[:, :3].any()
    m = SC.key_map(oracle, L.OracleCarver, E, 24, 0)
    assert m["depth"] == 24 and m["orientation"] == 0 and FC.valid_levels(m["data"], 24)
    assert not (SC.seam_pixels(m) & union).any()
    # the key frame alone: its energy knows the block where it stands in frame 0 and nothing of where it goes
    E0 = SC.static_energy(frames[:1], 0, st, 2, 0, SC.PAPER_ALPHA)
    m0 = SC.key_map(oracle, L.OracleCarver, E0, 24, 0)
    assert FC.valid_levels(m0["data"], 24) and (SC.seam_pixels(m0) & union).any()

"""The cases of tests/sizes_cases.py without a GPU: its vectorised model equals vmap_cases.model (which tests/test_vmap_abi.py pins to
the genuine liblqr) at every size, depth and orientation on small images, and the cases cover what they are meant to."""
import numpy as np

import coldepth_cases as CD
import sizes_cases as SC
import vmap_cases as VC


def test_vectorised_model_equals_the_pinned_model():
    n = 0
    for px, (ch, depth, _) in SC.PIXELS.items():
        for o in (0, 1):
            w, h, d = 23 + px % 3, 9 + o, 7
            rng = np.random.default_rng([41, px, o])
            img = CD.to_depth(rng, CD.base_image(rng, w, h, ch), depth)
            m = VC.perm_map(50 + px, w, h, d, o)
            length = h if o else w
            for size in range(length - d, length + d + 1):
                want, got = VC.model(img, m, size), SC.fast_model(img, m, size)
                assert want.dtype == got.dtype and want.shape == got.shape and np.array_equal(CD.bits(want), CD.bits(got)), (px, o, size)
                n += 1
    assert n == 8 * 2 * 15


def test_cases_cover_the_boundaries():
    cs = SC.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    w0s = {c["line"] + c["d"] for c in cs}
    assert w0s >= {255, 256, 257, 1023, 1024, 1025, SC.CHUNK - 1, SC.CHUNK + 1}
    assert {c["lines"] for c in cs} >= {1, 2, 31, 32, 33, 65}
    assert {c["px"] for c in cs} == {1, 2, 3, 4, 5, 8, 16, 32} and {c["o"] for c in cs} == {0, 1}
    for o in (0, 1):
        mine = [c for c in cs if c["o"] == o]
        assert {len(SC.sizes_of(c)) for c in mine} >= {1, 64, 65}
        assert any(c["how"] == "repeats" and len(set(SC.sizes_of(c))) < len(SC.sizes_of(c)) for c in mine)
        assert any(c["how"] == "full" and SC.sizes_of(c) == list(range(c["line"] - c["d"], c["line"] + c["d"] + 1)) for c in mine)
        assert {off for c in mine for off in c["offsets"]} == {0, 1}
        assert {c["px"] for c in mine if 1 in c["offsets"]} == set(SC.PIXELS)
    for c in cs:
        w, h = (c["line"] + c["d"], c["lines"]) if c["o"] == 0 else (c["lines"], c["line"] + c["d"])
        assert w <= 1100 and h <= 1100 and min(w, h) <= 70, c["name"]
        assert all(c["line"] - c["d"] <= s <= c["line"] + c["d"] for s in SC.sizes_of(c))

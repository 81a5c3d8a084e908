"""The forward-energy rule itself, without a GPU (tests/forward_cases.py is the specification the engine is held to): on every frame
size up to 5 x 4 the model's first seam is a cheapest connected seam -- found by enumerating them all, each charged what its removal
inserts plus P -- and among the cheapest the one the tie rule names; its maps are valid; an all-equal image gives the maps the tie rule
predicts."""
import itertools

import numpy as np
import pytest

import forward_cases as FC

F = np.float32
SIZES = [(L, H) for L in range(1, 6) for H in range(1, 5)]


def frames(L, H, kind, n=12):
    rng = np.random.default_rng([L, H, 1 if kind == "grey4" else 2])
    for i in range(n):
        if kind == "grey4":
            I = (rng.integers(0, 4, (H, L)) / 4.0).astype(F)
            P = (rng.integers(-2, 3, (H, L)) / 8.0).astype(F) if i % 2 else np.zeros((H, L), F)
        else:
            I = rng.random((H, L)).astype(F)
            P = (rng.normal(0, 0.3, (H, L))).astype(F) if i % 2 else np.zeros((H, L), F)
        yield I, P


def step_cost(I, x, y, px):
    """what removing pixel (x, y) inserts when the seam's pixel on the line above is px (None: there is no line above)"""
    wc = I.shape[1]
    l, r = I[y, max(x - 1, 0)], I[y, min(x + 1, wc - 1)]
    c = F(abs(F(r - l)))
    if px is None or px == x:
        return c
    u = I[y - 1, x]
    return F(c + F(abs(F(u - l)))) if px == x - 1 else F(c + F(abs(F(u - r))))


def seam_cost(I, P, xs):
    """the seam's cost, summed from the top in the order of the recurrence"""
    c = F(P[0, xs[0]] + step_cost(I, xs[0], 0, None))
    for y in range(1, len(xs)):
        c = F(P[y, xs[y]] + F(c + step_cost(I, xs[y], y, xs[y - 1])))
    return c


def connected_seams(L, H):
    for x0 in range(L):
        for steps in itertools.product((-1, 0, 1), repeat=H - 1):
            xs = [x0]
            for s in steps:
                xs.append(xs[-1] + s)
            if all(0 <= x < L for x in xs):
                yield tuple(xs)


def named_seam(I, P):
    """the tie rule applied to the enumeration: the least cost of a seam ending at every pixel, then from the smallest cheapest x of the
    last line upwards the first of up, left, right through which that least cost is reached"""
    H, L = I.shape
    best = {}
    for y in range(H):
        for xs in connected_seams(L, y + 1):
            c = seam_cost(I, P, xs)
            key = (xs[-1], y)
            if key not in best or c < best[key]:
                best[key] = c
    last = [best[(x, H - 1)] for x in range(L)]
    x = int(np.flatnonzero(np.array(last) == min(last))[0])
    xs = [x]
    for y in range(H - 1, 0, -1):
        cand = [(px, F(best[(px, y - 1)] + step_cost(I, x, y, px))) for px in (x, x - 1, x + 1) if 0 <= px < L]
        least = min(c for _, c in cand)
        x = next(px for px, c in cand if c == least)
        xs.append(x)
    return tuple(reversed(xs)), min(last)


@pytest.mark.parametrize("kind", ["grey4", "float"])
@pytest.mark.parametrize("L,H", SIZES)
def test_first_seam_is_a_cheapest_one_and_the_one_the_tie_rule_names(L, H, kind):
    for I, P in frames(L, H, kind):
        xs = tuple(int(x) for x in FC.seam_of(I, P))
        costs = {s: seam_cost(I, P, s) for s in connected_seams(L, H)}
        assert xs in costs
        least = min(costs.values())
        assert costs[xs] == least, (I, P, xs)
        M, _ = FC.sweep(I, P)
        assert M.min() == least and M[xs[-1]] == least
        want, want_cost = named_seam(I, P)
        assert want_cost == least and xs == want, (I, P, xs, want)


def test_grey4_frames_do_have_ties():
    """the tie rule is only tested where cheapest seams tie: at least a quarter of the frames that have more than one seam must"""
    tied = several = 0
    for L, H in SIZES:
        for I, P in frames(L, H, "grey4"):
            costs = [seam_cost(I, P, s) for s in connected_seams(L, H)]
            several += len(costs) > 1
            tied += sum(1 for c in costs if c == min(costs)) > 1
    assert several >= 150 and 4 * tied >= several, (tied, several)


@pytest.mark.parametrize("kind", ["grey4", "float"])
def test_maps_are_valid_and_each_seam_is_the_first_seam_of_what_is_left(kind):
    for L, H in SIZES:
        for I, P in frames(L, H, kind, n=4):
            for depth in range(1, L):
                lv = FC.levels(I, P, depth)
                assert lv.shape == (H, L) and lv.dtype == np.int32 and FC.valid_levels(lv, depth)
                # level k lies where the first seam of the frame without levels 1 .. k - 1 lies
                for k in range(1, depth + 1):
                    keep = (lv == 0) | (lv >= k)
                    Ik, Pk = I[keep].reshape(H, L - k + 1), P[keep].reshape(H, L - k + 1)
                    xs = FC.seam_of(Ik, Pk)
                    assert all((lv[y][keep[y]] == k)[xs[y]] for y in range(H))
                if depth > 1:       # a deeper map extends a shallower one
                    shallow = FC.levels(I, P, depth - 1)
                    assert np.array_equal(np.where(lv == depth, 0, lv), shallow)


@pytest.mark.parametrize("o", [0, 1])
def test_an_all_equal_image_gives_the_map_the_tie_rule_predicts(o):
    """every cost is 0: the seam ends at column 0 and goes straight up, so seam k takes what was the k-th pixel of every line"""
    for w, h in ((5, 4), (9, 3), (2, 7), (12, 1)):
        L = h if o else w
        for depth in sorted({1, L - 1} & set(range(1, L))):      # (a line of one pixel has no seam to give)
            m = FC.forward_map(np.full((h, w), 0.5, F), None, depth, o)
            lines = m["data"].T if o else m["data"]
            want = np.tile(np.where(np.arange(L) < depth, np.arange(L) + 1, 0), (lines.shape[0], 1))
            assert m["data"].shape == (h, w) and np.array_equal(lines, want)
            assert m["depth"] == depth and m["orientation"] == o


def test_a_low_bias_column_draws_the_seam_and_orientation_1_is_the_transposed_problem():
    rng = np.random.default_rng(9)
    I = rng.random((6, 9)).astype(F)
    lo = np.zeros((6, 9), F)
    lo[:, 6] = -1000.0
    m = FC.forward_map(I, lo, 1, 0)
    assert np.array_equal(np.flatnonzero(m["data"][3]), [6]) and (m["data"][:, 6] == 1).all()
    # orientation 1 is orientation 0 of the transposed image
    a, b = FC.forward_map(I, lo, 3, 1), FC.forward_map(I.T, lo.T, 3, 0)
    assert np.array_equal(a["data"], b["data"].T)


def test_values_that_are_not_finite_still_give_a_valid_map():
    rng = np.random.default_rng(11)
    I = rng.random((5, 8)).astype(F)
    I[1, 2], I[3, 5], I[0, 0] = np.nan, np.inf, -np.inf
    for depth in (1, 4, 7):
        assert FC.valid_levels(FC.levels(I, np.zeros_like(I), depth), depth)
    assert FC.valid_levels(FC.levels(np.full((3, 4), np.nan, F), np.zeros((3, 4), F), 3), 3)

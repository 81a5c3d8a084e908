"""The rule of include_ext/lqr_clipforward.h as tests/clipforward_cases.py states it, without a GPU: for one frame and for identical
frames it is forward_cases' rule; with temporal 0 the order of the frames does not matter; forming the costs of two columns per line again
after a seam equals forming all of them again; by enumeration the first seam is a cheapest connected seam under the clip's costs, and the
one the tie rule names; and on the clip of static_cases.crossing_block() the clip's seams leave the block alone where frame 0's own do not."""
import itertools

import numpy as np
import pytest

import clipforward_cases as CC
import forward_cases as FC
import static_cases as SC

F = np.float32


def clip(seed, n, H, L, kind="grey4"):
    rng = np.random.default_rng(seed)
    if kind == "grey4":
        return (rng.integers(0, 4, (n, H, L)) / 4.0).astype(F)
    return rng.random((n, H, L)).astype(F)


def bias_terms(seed, n, H, L):
    rng = np.random.default_rng([seed, 9])
    return ((rng.integers(0, 4, (n, H, L)) - 1) * 0.375 / L).astype(F)


@pytest.mark.parametrize("temporal", [0.0, 0.7, 5.0])
@pytest.mark.parametrize("with_bias", [False, True])
def test_one_frame_and_identical_frames_are_the_forward_rule(temporal, with_bias):
    for seed, (H, L, d) in enumerate([(7, 23, 22), (1, 9, 4), (12, 5, 4), (30, 40, 17)]):
        for kind in ("grey4", "float"):
            I = clip(100 + seed, 1, H, L, kind)
            P = bias_terms(seed, 1, H, L) if with_bias else np.zeros((1, H, L), F)
            want = FC.levels(I[0], P[0], d)
            assert np.array_equal(CC.levels(I, P, d, temporal), want), (seed, kind)
            assert np.array_equal(CC.levels(np.repeat(I, 3, 0), np.repeat(P, 3, 0), d, temporal), want), (seed, kind)


def test_with_temporal_0_any_permutation_of_the_frames_gives_the_same_map():
    for seed, (n, H, L, d) in enumerate([(3, 6, 14, 9), (4, 9, 11, 10), (3, 1, 8, 5)]):
        I, P = clip(200 + seed, n, H, L, "float" if seed % 2 else "grey4"), bias_terms(200 + seed, n, H, L)
        want = CC.levels(I, P, d, 0.0)
        assert FC.valid_levels(want, d)
        for perm in itertools.permutations(range(n)):
            assert np.array_equal(CC.levels(I[list(perm)], P[list(perm)], d, 0.0), want), (seed, perm)


def test_the_two_column_refresh_equals_full_recomputation_down_to_width_1():
    shapes = [(n, H, L) for n in (1, 2, 3) for H in (1, 2, 3, 7) for L in (3, 4, 5, 9, 16)]
    for seed, (n, H, L) in enumerate(shapes):
        for kind, temporal in (("grey4", 1.0), ("float", 0.3)):
            I, P = clip(300 + seed, n, H, L, kind), bias_terms(300 + seed, n, H, L) if seed % 2 else np.zeros((n, H, L), F)
            assert np.array_equal(CC.levels_two_columns(I, P, L - 1, temporal), CC.levels(I, P, L - 1, temporal)), (n, H, L, kind)


def all_seams(H, wc):
    """every connected seam: a column per line, neighbours at most one apart"""
    seams = [[x] for x in range(wc)]
    for _ in range(H - 1):
        seams = [s + [x] for s in seams for x in (s[-1] - 1, s[-1], s[-1] + 1) if 0 <= x < wc]
    return seams


def seam_cost(s, CU, CL, CR, Q):
    """M along a seam given top-down, in the recurrence's own order of operations"""
    m = Q[0, s[0]] + CU[0, s[0]]
    for y in range(1, len(s)):
        step = s[y] - s[y - 1]              # the parent lies at s[y-1]: left of the pixel when the seam stepped right
        m = Q[y, s[y]] + (m + (CU if step == 0 else CL if step == 1 else CR)[y, s[y]])
    return m


def test_by_enumeration_the_first_seam_is_a_cheapest_one_and_the_one_the_tie_rule_names():
    """dyadic values: every sum is exact, so the cost of a seam does not depend on rounding and the cheapest is well defined"""
    rng = np.random.default_rng(404)
    for n in (1, 2, 3):
        for H in range(1, 5):
            for wc in range(2, 6):
                for rep in range(6):
                    I = (rng.integers(0, 4, (n, H, wc)) / 4.0).astype(F)
                    P = (rng.integers(-1, 3, (n, H, wc)) / 8.0).astype(F) if rep % 2 else np.zeros((n, H, wc), F)
                    CU, CL, CR = CC.costs(I)
                    Q = CC.q_plane(I, P, 0.5)
                    got = list(CC.seam_of(CU, CL, CR, Q))
                    seams = all_seams(H, wc)
                    cost = [seam_cost(s, CU, CL, CR, Q) for s in seams]
                    best = min(cost)
                    assert seam_cost(got, CU, CL, CR, Q) == best, (n, H, wc, rep)
                    # among the cheapest: the smallest end column; then, walking up, up before left before right
                    cand = [s for s, c in zip(seams, cost) if c == best]
                    end = min(s[-1] for s in cand)
                    assert got[-1] == end
                    M = [None] * H          # M(x, y) by enumeration of the seams that end at (x, y)
                    for y in range(H):
                        sub = all_seams(y + 1, wc)
                        M[y] = [min(seam_cost(s, CU, CL, CR, Q) for s in sub if s[-1] == x) for x in range(wc)]
                    for y in range(H - 1, 0, -1):
                        x = got[y]
                        opts = [(M[y - 1][x] + CU[y, x], 0)]
                        if x > 0:
                            opts.append((M[y - 1][x - 1] + CL[y, x], -1))
                        if x < wc - 1:
                            opts.append((M[y - 1][x + 1] + CR[y, x], 1))
                        least = min(o[0] for o in opts)
                        assert got[y - 1] - x == [o[1] for o in opts if o[0] == least][0], (n, H, wc, rep, y)


@pytest.mark.parametrize("depth,orientation,alone", [(20, 0, 80), (8, 1, 8)])
def test_the_clips_seams_leave_the_crossing_block_alone_where_frame_0s_own_do_not(depth, orientation, alone):
    frames, union = SC.crossing_block()
    st = FC.type_state(dict(ch=1))
    Is = [FC.intensity(f, 0, st, False) for f in frames]
    m = CC.clip_forward_map(Is, None, depth, orientation, 1.0)
    assert FC.valid_levels(m["data"].T if orientation else m["data"], depth)
    assert CC.block_hits(m, union) == 0
    own = FC.forward_map(Is[0], None, depth, orientation)
    assert CC.block_hits(own, union) == alone
    if orientation == 0:
        first = np.zeros(union.shape, bool)
        first[8:16, 4:12] = True
        assert bool(np.all(frames[0][first] == 255)) and CC.block_hits(own, first) == 48

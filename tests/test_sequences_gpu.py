"""Random call sequences across the carver API on the MI355X (tests/sequence_cases.py has the ops, their references and what is
left out; tests/test_sequences.py checks the reference alone and what the seeds cover).

Every committed seed's program runs on the engine beside its shadow.  After EVERY op: the return value, the getters (orientation and
depth among them), scan_by_row, lqrx_carver_size_range, the image byte for byte, the dumped map, the attached carver's image, the
op's own output (bits for floats), the guard bytes around every host buffer handed in and the elements before and behind every
device tensor.  At the end of every program the device pool has every block back and no session was rolled back.  A program that
never asks for a size above the reference size runs again on its 16I and 64F twins.  The assertion message carries the seed, the op's
index and the program.
"""
import pytest

import lqr_ctypes as L
import sequence_cases as S

pytestmark = pytest.mark.gpu

CHUNK = 20
CHUNKS = [S.SEEDS[i:i + CHUNK] for i in range(0, len(S.SEEDS), CHUNK)]


@pytest.fixture(scope="module")
def eng():
    return L.engine_api()


_reference = {}


def reference(chunk):
    """[(program, the shadow's observations)] of a chunk; the last chunk asked for is kept (the twins of a chunk run one after the other)"""
    if chunk not in _reference:
        _reference.clear()
        _reference[chunk] = []
        for seed in CHUNKS[chunk]:
            prog = S.program(seed)
            _reference[chunk].append((prog, S.run(None, prog)))
    return _reference[chunk]


def run_program(eng, prog, seen, depth=0):
    """the program beside its reference, then the pool and roll-back checks (sequence_cases.run_checked)"""
    return S.run_checked(eng, prog, depth, seen)


@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=lambda i: "seeds%d-%d" % (CHUNKS[i][0], CHUNKS[i][-1]))
def test_sequences_equal_their_reference_after_every_op(eng, chunk):
    for prog, seen in reference(chunk):
        run_program(eng, prog, seen)


@pytest.mark.parametrize("depth", [1, 3], ids=["16i", "64f"])
@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=lambda i: "seeds%d-%d" % (CHUNKS[i][0], CHUNKS[i][-1]))
def test_lifted_twins_equal_the_lifted_reference(eng, chunk, depth):
    ran = 0
    for prog, seen in reference(chunk):
        if S.liftable(seen):
            run_program(eng, prog, seen, depth)
            ran += 1
    assert ran                      # (tests/test_sequences.py counts them per state class)

"""Randomised run of call sequences across the carver API (tests/sequence_cases.py): programs from seeds beyond the committed list,
the engine beside the shadow (the CPU oracle and its bookkeeping), compared after EVERY op, the device pool and the roll-back counter checked at the end of every program; a liftable program also on
its 16I and 64F twins.  For soaks: tests/test_sequences_gpu.py runs the committed seeds.

    python scripts/fuzz_sequences.py [seconds] [seed]
"""
import sys

sys.path.insert(0, "tests")

import fuzz_common as FC
import lqr_ctypes as L
import sequence_cases as S

budget = FC.Budget(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0)      # FUZZ_COUNT=n: exactly n cases, no wall-clock exit
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
e = L.engine_api()
fails = FC.Failures(e.lib)
n = ops = twins = early = 0
while budget.more(n):
    prog = S.program(len(S.SEEDS) + 1000000 * seed + n)
    what = "seed %d: %d ops on %dx%d ch%d %s" % (prog["seed"], len(prog["ops"]), prog["image"]["w"], prog["image"]["h"], prog["image"]["ch"], prog["config"])
    try:
        seen = S.run_checked(e, prog)
        ops += len(seen)
        early += not S.ok_ret(seen[-1]["ret"])
        if S.liftable(seen):
            for depth in (1, 3):
                S.run_checked(e, prog, depth, seen)
                twins += 1
    except Exception as ex:
        # (sequence_cases words every difference, the end-of-program pool and roll-back checks included, with "differ": FC.Failures
        # labels those MISMATCH, and anything else -- an exception of the harness itself -- ERROR)
        fails.record(n, what, ex)
    n += 1
FC.summary("sequence fuzz", n, budget, fails, seed, " (%d ops compared, %d lifted twins, %d sequences ended by an error both libraries returned)" % (ops, twins, early))
sys.exit(1 if fails.total else 0)

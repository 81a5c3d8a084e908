"""The launch shim's pinned transfer ring and its helper threads (gimp-lqr-plugin_amd/csrc/lqr_stage.h: StageRing) without a GPU.
tests/c/stage_main.cc includes the header alone -- it is plain C++17 -- and supplies a fake device: heap blocks for device memory and
for the pinned slots, a DMA thread that executes the queued copies in order with a deterministic pseudo-random yield before each, and
events that are complete once the queue has passed them.  The same source is built twice with -Werror as a stand-alone program, under
ThreadSanitizer and under AddressSanitizer + UndefinedBehaviorSanitizer.  With 4 slots of 64 bytes and 3 helpers it checks: round trips
of 0 .. 64 003 bytes around every boundary of the ring (exactly full +- 1, the first slot reused, two wraps with a short last chunk, a
thousand chunks), from and into heap blocks of exactly that size that are freed on the line after the call returns; the same on rings
of one and of two slots, where a slot is refilled right after it was handed over; a 6-chunk transfer in each direction with its kth
device operation failing, for every k: the call returns that error, the DMA queue is empty and no helper has work when it does, and
the next transfer on the same ring is correct; a pinned allocation that fails for slot k releases every slot made so far and the next
call creates the ring; and for uploads of 1, 3 and 6 chunks the device operations issued are, one by one, those of the h2d_staged the
ring was moved out of."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")


@pytest.mark.parametrize("sanitizers", [["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["tsan", "asan-ubsan"])
def test_the_transfer_ring_keeps_its_promises(sanitizers):
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_stage_"), "stage_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + sanitizers +
                   ["-I" + CSRC, os.path.join(ROOT, "tests", "c", "stage_main.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip() and r.stdout.strip() == "stage ok", r.stdout[-2000:] + r.stderr[-4000:]

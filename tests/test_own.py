"""The launch shim's ownership types (gimp-lqr-plugin_amd/csrc/lqr_own.h: DevBuf, a device block with one owner, and Scratch, the
temporaries of one call) without a GPU.  tests/c/own_main.cc includes the header alone -- it is plain C++17 -- defines the three
functions the shim supplies over malloc / free with a journal, and is compiled with -Werror under AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program.  It checks: a move empties its source and gives the target's old block back
exactly once; ensure keeps a block that is large enough, otherwise gives back before it takes, and says whether it grew; a failed
allocation leaves a buffer empty; a Scratch that ends without done() waits for its stream before the first block goes back, one that
ends with done() does not wait at all; of three temporaries, whichever allocation fails, exactly the blocks already taken go back;
and the program ends with no live block (LeakSanitizer)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gimp-lqr-plugin_amd", "csrc")


def test_the_ownership_types_keep_their_rules():
    exe = os.path.join(tempfile.mkdtemp(prefix="lqr_own_"), "own_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "c", "own_main.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip() and r.stdout.strip() == "own ok", r.stdout[-2000:] + r.stderr[-4000:]

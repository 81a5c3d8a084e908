"""The carver's state word (gimp-lqr-plugin_amd/host/lqr_state.c) without a GPU: the C file is compiled alone with a stand-alone main
(tests/c/state_main.c) and run as a child process, once under AddressSanitizer and UndefinedBehaviorSanitizer (every transition, and
whose word an attached carver reads) and once under ThreadSanitizer with a second thread that cancels at arbitrary moments: a cancel
that hit a busy state is seen by the next check, leaving to idle never erases it, a cancel on an idle word changes nothing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gimp-lqr-plugin_amd", "host")
CALLS = 300000


def build(tmp_path_factory, name, sanitize):
    out = str(tmp_path_factory.mktemp(name) / "state_main")
    subprocess.run(["gcc", "-std=c99", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                    "-I" + HOST, os.path.join(HOST, "lqr_state.c"), os.path.join(ROOT, "tests", "c", "state_main.c"), "-o", out, "-lpthread"], check=True)
    return out


@pytest.fixture(scope="module")
def exe_asan(tmp_path_factory):
    return build(tmp_path_factory, "state_asan", "address,undefined")


@pytest.fixture(scope="module")
def exe_tsan(tmp_path_factory):
    return build(tmp_path_factory, "state_tsan", "thread")


def test_every_transition_and_the_attached_carvers(exe_asan):
    r = subprocess.run([exe_asan, "transitions"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout + r.stderr
    assert r.stdout.startswith("state transitions ok ")


def test_a_second_thread_cancels_at_arbitrary_moments(exe_tsan):
    r = subprocess.run([exe_tsan, "race", str(CALLS)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout + r.stderr      # (a data race is ThreadSanitizer's report on stderr and its exit code)
    f = r.stdout.split()
    assert f[:3] == ["state", "race", "ok"]
    calls, cancelled, in_call, idle = int(f[4]), int(f[6]), int(f[8]), int(f[10])
    # both kinds of cancel happened: ones that found a call running (some seen by the call's own checks) and ones that found none
    assert calls == CALLS and 0 < in_call <= cancelled <= calls and idle > 0


def test_state_sources_are_bookkeeping_and_the_host_checks_where_it_says():
    for name in ("lqr_state.c", "lqr_state.h"):
        src = open(os.path.join(HOST, name)).read()
        assert "hip" not in src.lower() and "malloc" not in src and "calloc" not in src and "printf" not in src and "#include <std" not in src, name
        assert "__atomic" in src or name.endswith(".h")
    host = open(os.path.join(HOST, "lqr_carver.c")).read()
    cancel = host[host.index("LqrRetVal lqr_carver_cancel("):]
    cancel = cancel[:cancel.index("\n}") + 2]
    assert "lqr_state_cancel" in cancel and "lqrhip_" not in cancel and "->attached" not in cancel     # the word, and nothing else
    loop = host[host.index("static LqrRetVal group_build_vsmap("):host.index("static LqrRetVal session_run(")]
    assert loop.count("CANCEL_POINT(g)") == 2 and loop.index("CANCEL_POINT(g)") < loop.index("lqrhip_seam_step") < loop.index("lqrhip_session_check")
    assert "CANCEL_POINT" not in loop[loop.index("lqrhip_session_check"):]          # never after the self-check
    mk = open(os.path.join(ROOT, "gimp-lqr-plugin_amd", "Makefile")).read()
    assert "$(BUILD)/lqr_state.o: host/lqr_state.c host/lqr_state.h" in mk

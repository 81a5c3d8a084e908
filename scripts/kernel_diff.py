#!/usr/bin/env python3
"""Compare the kernels of two builds of liblqr-hip.so: what a refactor of the kernels has to show before any GPU time is spent.

    python scripts/kernel_diff.py OLD.so NEW.so [--map old_name=new_name ...]

For every kernel of either library (demangled name without the parameter list; --map pairs a kernel that was renamed) one line
with the VGPR (+ AGPR) / SGPR / LDS / scratch figures of both and whether the instruction streams are equal.  A stream is the
kernel's disassembly up to its last s_endpgm, without addresses and encodings (tests/kernel_meta.py disassembly): what follows is
padding, which differs between a template instantiation and a plain function.  Streams that differ are reported with the number of
lines a unified diff changes.  The tool compares two libraries and nothing else; a summary line counts each outcome."""
import argparse
import difflib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import kernel_meta as KM  # noqa: E402


def stream(ins):
    """the instructions up to the last s_endpgm"""
    last = max((i for i, s in enumerate(ins) if s.split()[0] == "s_endpgm"), default=len(ins) - 1)
    return ins[:last + 1]


def figures(d):
    return "%4d %4d %6d %7d" % (d["vgpr_count"] + d["agpr_count"], d["sgpr_count"], d["group_segment_fixed_size"], d["private_segment_fixed_size"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="a kernel of OLD under its name in NEW (may be given many times)")
    args = ap.parse_args()
    renamed = dict(m.split("=", 1) for m in args.map)
    meta = [KM.kernels(args.old), KM.kernels(args.new)]
    text = [KM.disassembly(args.old), KM.disassembly(args.new)]
    for old, new in renamed.items():
        assert old in meta[0] and new in meta[1], "--map %s=%s: no such kernel" % (old, new)
    rows = [(o, renamed.get(o, o)) for o in sorted(meta[0])]
    taken = {n for _, n in rows}
    rows += [(None, n) for n in sorted(meta[1]) if n not in taken]
    tally = {}
    cols = "vgpr sgpr    lds scratch"
    print("# figures of OLD (%s), then of NEW (%s)" % (os.path.basename(os.path.dirname(os.path.abspath(args.old))), os.path.basename(os.path.dirname(os.path.abspath(args.new)))))
    print("%-14s  %-24s  %-24s  %s" % ("# stream", cols, cols, "kernel (old -> new where renamed)"))
    for o, n in rows:
        if o is None or n not in meta[1]:
            verdict = "only new" if o is None else "only old"
        else:
            a, b = stream(text[0][o]), stream(text[1][n])
            changed = sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            verdict = "equal" if a == b else "differs %d/%d" % (changed, len(a))
        tally[verdict.split()[0]] = tally.get(verdict.split()[0], 0) + 1
        name = n if o in (None, n) else "%s -> %s" % (o, n)
        print("%-14s  %-24s  %-24s  %s" % (verdict, figures(meta[0][o]) if o else "-", figures(meta[1][n]) if n in meta[1] else "-", name))
    print("# %d kernels old, %d new: %s" % (len(meta[0]), len(meta[1]), ", ".join("%d %s" % (v, k) for k, v in sorted(tally.items()))))


if __name__ == "__main__":
    main()

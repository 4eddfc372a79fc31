#!/usr/bin/env python3
"""What the entries that read a context's slice state return after every ordered pair of the entries that change it: one line
per call of every case of tests/ctx_sequences.py --
    <case id> <call> <return code> <first 16 hex digits of the SHA-256 of the call's output bytes>
tests/ctx_sequences_expected.txt is this script's output at the commit BEFORE the slice state became one struct with named
transitions (bf_ctx_state.h); tests/test_gpu_ctx_sequences.py holds every later build to it.  One context at a time.

usage: ctx_sequence_table.py [--lib PATH] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the library to load instead of the tree's")
    ap.add_argument("--out", default=None, help="write the table here instead of standard output")
    args = ap.parse_args()
    import ctx_sequences as cs
    from better_flow_amd import accel
    t0 = time.time()
    text = "\n".join(cs.table(accel, args.lib)) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    sys.stderr.write("%d lines in %.1f s\n" % (text.count("\n"), time.time() - t0))


if __name__ == "__main__":
    main()

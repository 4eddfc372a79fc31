#!/usr/bin/env python3
"""Which loop bf_run takes, case by case: one line per case of tests/loop_form_cases.py --
    <case id> loop_form scatter_format k1_head k1_threads k1_events_per_thread k3_mode k3_capped finish_updates_per_stencil_launch
(bf_get_stat after the case's run; the last column from the run's launch counts, tests/loop_form_cases.py).  tests/loop_forms_expected.txt is this script's output at the commit BEFORE the loop form
became one enum and one rule; tests/test_gpu_loop_forms.py holds every later build to it.  One context at a time: the persistent
kernel is for a context alone in its process.

usage: loop_form_table.py [--lib PATH] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the library to load instead of the tree's")
    ap.add_argument("--out", default=None, help="write the table here as well")
    args = ap.parse_args()
    import loop_form_cases as lc
    from better_flow_amd import accel
    lines = [lc.format_row(c, lc.case_row(accel, c, args.lib)) for c in lc.CASES]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

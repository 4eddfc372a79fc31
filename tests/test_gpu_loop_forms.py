"""Which loop bf_run takes and which kernel variants it launches, case by case (tests/loop_form_cases.py), against
tests/loop_forms_expected.txt: the output of scripts/loop_form_table.py at the commit before the loop form became one enum and
one pure rule (bf_rules::loop_choice).  Line for line: the plan decides as it did."""
import gc
import os

import pytest

import loop_form_cases as lc

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_forms_expected.txt")


def test_loop_forms_equal_the_recorded_table(accel_mod):
    with open(TABLE) as f:
        want = f.read().splitlines()
    assert len(want) == len(lc.CASES)
    gc.collect()   # (a context an earlier test dropped without closing would count as alive)
    got = [lc.format_row(c, lc.case_row(accel_mod, c)) for c in lc.CASES]   # one context at a time: the persistent kernel's condition
    for g, w in zip(got, want):
        print(g)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]

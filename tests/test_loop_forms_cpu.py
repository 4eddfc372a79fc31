"""The loop form on the host (no GPU): bf_rules::loop_choice (better_flow_amd/csrc/bf_plan_rules.h), fed the cases of
tests/loop_form_cases.py as plain numbers by tests/cpp/test_plan.cpp, against tests/loop_forms_expected.txt -- the table the
device recorded before the form became one enum and one rule.  The sweep of the rule over every combination of its facts runs
with the binary's other sweeps (tests/test_plan_cpu.py)."""
import os
import subprocess

import loop_form_cases as lc
from test_plan_cpu import test_plan_exe  # noqa: F401  (the fixture that compiles tests/cpp/test_plan.cpp)

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_forms_expected.txt")
FORMS = {0: "atomic", 1: "binned", 2: "one_kernel", 3: "persistent", 4: "delta"}


def expected_table():
    rows = {}
    with open(TABLE) as f:
        for ln in f:
            w = ln.split()
            rows[w[0]] = dict(zip(lc.COLUMNS + ("finish_updates",), (int(x) for x in w[1:])))
            assert len(w) == len(lc.COLUMNS) + 2, ln
    return rows


def test_cases_are_the_table_and_reach_every_form_and_home():
    table = expected_table()
    assert [c["id"] for c in lc.CASES] == list(table) and len(table) == len(lc.CASES)
    assert 30 <= len(lc.CASES) <= 50 and all(c["n"] <= 50000 for c in lc.CASES)
    assert {r["loop_form"] for r in table.values()} == set(FORMS)
    assert {c["home"] for c in lc.CASES} == {"tail", "head", "separate"}
    for key in ("binned", "fused", "persist", "delta_scatter", "sep_update", "bin_compact", "bin_split"):
        assert {0, 2} <= {c["opts"].get(key) for c in lc.CASES}, key


def test_pure_rule_gives_the_recorded_forms(test_plan_exe):  # noqa: F811
    lines = "".join(lc.facts_line(c) for c in lc.CASES)
    out = subprocess.run([test_plan_exe, "forms"], input=lines.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(lc.CASES), out
    table = expected_table()
    for c, ln in zip(lc.CASES, out):
        cid, form, name, home, fmt = ln.split()
        want = table[c["id"]]
        assert cid == c["id"] and FORMS[int(form)] == name
        assert int(form) == want["loop_form"], ln
        assert int(fmt) == want["scatter_format"], ln
        assert home == c["home"], ln
        if name == "binned":   # the table tells the three homes apart
            assert (home == "head") == (want["k1_head"] == 1), ln
            assert (home == "separate") == (want["finish_updates"] == 1), ln
        else:
            assert want["k1_head"] == -1 and home == ("tail" if name in ("atomic", "delta") else "head"), ln

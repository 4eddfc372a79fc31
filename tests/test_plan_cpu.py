"""The plan's rules on the host (no GPU): tests/cpp/test_plan.cpp sweeps better_flow_amd/csrc/bf_plan_rules.h -- every variant the
rules can ask for is compiled, every compiled variant can be asked for, and the reachable set is tests/variants_reachable.txt --
and the rows of tests/test_gpu_variants.py land, by those rules on 256 CUs, on the variants they claim and cover the table."""
import os
import subprocess

import pytest

import test_gpu_variants as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "test_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_plan.cpp"), "-o", exe])
    return exe


def test_plan_sweep_matches_the_committed_table(test_plan_exe):
    r = subprocess.run([test_plan_exe, tv.TABLE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and out.splitlines()[-1] == "ok", out[-4000:]
    swept = {tuple(int(x) for x in ln.split()) for ln in out.splitlines() if ln and ln[0].isdigit()}
    assert swept == tv.reachable_table() and len(swept) == 36


def test_gpu_rows_land_on_their_variants_and_cover_the_table(test_plan_exe):
    lines = "".join("%d %d %d %d %d %d 0\n" % (key + (head, fmt)) for key, head, fmt, _, _ in tv.ROWS)
    out = subprocess.run([test_plan_exe, "rows"], input=lines.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(tv.ROWS)
    for row, ln in zip(tv.ROWS, out):
        key, head, fmt, k1, k3 = row
        w = ln.split()
        assert w[:2] == ["ok", "1"], (tv.row_id(row), ln)
        assert tuple(int(x) for x in w[3:7]) == (head,) + k1 + (fmt,), (tv.row_id(row), ln)
        assert tuple(int(x) for x in w[8:11]) == k3, (tv.row_id(row), ln)
        assert tuple(int(x) for x in w[12:14]) == tv.SLICES[key], (tv.row_id(row), ln)
    assert {(head,) + k1 + (fmt,) for _, head, fmt, k1, _ in tv.ROWS} == tv.reachable_table()
    assert {k3 for *_, k3 in tv.ROWS} == {(hs, mode, capped) for hs in range(5) for mode in range(3) for capped in range(2)}
    assert len({tv.row_id(r) for r in tv.ROWS}) == len(tv.ROWS) and {r[0] for r in tv.ROWS} == set(tv.SLICES)


@pytest.mark.parametrize("key", sorted(tv.SLICES), ids=lambda k: "%dx%d_s%d_n%d" % (k[1], k[0], k[2], k[3]))
def test_gpu_slices_are_shaped_as_promised(oracle_lib, key):
    """Exactly n events over the whole sensor, a bin at least twice as full as the average, bins without events (asserted inside);
    and the solver has something to do on it: the oracle's loop runs to the cap of the GPU rows, warps included."""
    sl = tv.variant_slice(key)
    assert len(sl["t"]) == key[3] and (sl["t"][1:] >= sl["t"][:-1]).all()
    H, W, s, n = key
    o = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
    rc, lp, _ = o.run(o.set_cloud(s, H, W), oracle_lib.Model(), max_iter=tv.K, res_x=H, res_y=W, trace_cap=tv.K + 2, min_events=10)
    assert rc == 0 and lp.itercount == tv.K + 1, (key, rc, lp.itercount)

"""The stencil launch's block -> tile map on the host (no GPU): tests/cpp/test_tile_order.cpp sweeps bf_rules::tile_of_block
(better_flow_amd/csrc/bf_plan_rules.h) -- a bijection for every tile count 1 .. 4096 and on the BASELINE grids, one contiguous run
of tiles per residue class mod 8, class sizes within 1, and on config 2's grid all vertically adjacent tile pairs but at most
seven tile rows' worth inside one class (none with the launch order)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_tile_order_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_order") / "test_tile_order")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_tile_order.cpp"), "-o", exe])
    return exe


def test_tile_order_sweep(test_tile_order_exe):
    r = subprocess.run([test_tile_order_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and out.splitlines()[-1] == "ok", out[-4000:]
    # config 2: 49 x 17 tiles, 816 vertical pairs
    cfg2 = [ln for ln in out.splitlines() if ln.startswith("#") and "49 x 17 tiles" in ln]
    assert len(cfg2) == 1 and " 816 vertical pairs" in cfg2[0] and cfg2[0].rstrip().endswith(" 0 in launch order"), cfg2

"""Where bf_run_groups solves a group, on the host (no GPU): tests/cpp/test_group_route.cpp holds bf_rules::group_route
(better_flow_amd/csrc/bf_group_rules.h) to a table of cases -- the guards, exactly 156 KiB (96 x 104) stays on the LDS path, one
more row goes wide with "groups_wide" on and is BF_ERR_CAPACITY with it off, a window beyond max_rows is BF_ERR_CAPACITY either
way, zero events -- and, with the option off, to the guards of k_group_optimizer over a sweep.  The program is built with
-fsanitize=address,undefined and runs stand-alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_group_route.cpp")


def test_group_route_table_and_sweep(tmp_path):
    exe = str(tmp_path / "test_group_route")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SOURCE, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and out.splitlines()[-1] == "ok", out[-4000:]
    assert "FAILED" not in out
    # (the table ran for both settings of the option, and the sweep went somewhere)
    assert out.count("one more row") == 2 and " wide " in out and " capacity " in out
    swept = [l for l in out.splitlines() if l.startswith("sweep:")]
    assert swept and int(swept[0].split()[1]) > 10000 and swept[0].split()[3] == "0"

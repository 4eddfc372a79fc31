"""The result-block layouts of the entries on the K models' vote planes, on the host (no GPU): tests/cpp/test_group_blocks.cpp
holds better_flow_amd/csrc/bf_group_blocks.h -- the one place the kernels and the host code ask where a word of a block sits --
to the documented word order, the strides, the buffer sizes at K = 64 as literals and a set of spot values from the formulas
that were written out by hand before.  The header is pure (plain g++ compiles it); the program is built with
-fsanitize=address,undefined and runs stand-alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_group_blocks.cpp")


def test_group_block_layouts(tmp_path):
    exe = str(tmp_path / "test_group_blocks")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SOURCE, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0 and out.splitlines()[-1] == "ok", out[-4000:]
    assert "FAILED" not in out
    # (every K went through: the merge block alone names 2 (1 + 4 + 63^2 + 64^2) + 8 = 16148 words, each one checked)
    checked = [l for l in out.splitlines() if l.startswith("checked:")]
    assert checked and int(checked[0].split()[1]) > 16148

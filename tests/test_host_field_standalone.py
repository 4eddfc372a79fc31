"""include/bf_global_field.h on the host alone: tests/cpp/test_cell_field.cpp, a stand-alone program built with the address
and undefined-behaviour sanitizers, against the numpy restatement (tests/global_field_ref.py), bit for bit.  No GPU, no
library."""
import os
import subprocess

import numpy as np

import global_field_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(values):
    return np.array(values, dtype=np.float64).view(np.uint64)


def test_shared_header_against_the_restatement(tmp_path):
    exe = str(tmp_path / "test_cell_field")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cell_field.cpp"), "-o", exe])
    rng = np.random.default_rng(31)
    gx, gy = rng.uniform(-0.3, 0.3, (3, 3)), rng.uniform(-0.3, 0.3, (3, 3))
    fx, fy = rng.uniform(-1, 1, (3, 4)), rng.uniform(-1, 1, (3, 4))
    bx, by = np.where(F.FILL_MASK, fx, np.nan), np.where(F.FILL_MASK, fy, np.nan)
    inp = str(tmp_path / "in.txt")
    with open(inp, "w") as f:
        f.write(" ".join(float(v).hex() for v in np.concatenate([gx.ravel(), gy.ravel()])) + "\n")
        f.write(" ".join(str(int(m)) for m in F.FILL_MASK.ravel()) + "\n")
        f.write(" ".join("nan" if np.isnan(v) else float(v).hex() for v in np.concatenate([bx.ravel(), by.ravel()])) + "\n")
    r = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]     # any sanitizer report fails
    lines = [ln.split() for ln in r.stdout.decode().splitlines()]

    axis = np.array([[int(v) for v in ln[1:]] for ln in lines if ln[0] == "axis"])
    assert len(axis) == 4 * 24
    for size in (8, 5, 1, 7):
        a0, a1, w = F.axis(np.arange(24), size, -(-24 // size))
        got = axis[axis[:, 0] == size]
        assert np.array_equal(got[:, 1], np.arange(24))
        assert np.array_equal(got[:, 2], a0) and np.array_equal(got[:, 3], a1) and np.array_equal(got[:, 4], w), size

    field = [ln for ln in lines if ln[0] == "field"]
    assert len(field) == 24 * 24
    X, Y = np.meshgrid(np.arange(24), np.arange(24), indexing="ij")
    assert [(int(ln[1]), int(ln[2])) for ln in field] == list(zip(X.ravel().tolist(), Y.ravel().tolist()))
    nx, ny = F.field_at(X.ravel(), Y.ravel(), 8, 8, 3, 3, gx, gy)
    assert np.array_equal(_bits([float.fromhex(ln[3]) for ln in field]), nx.view(np.uint64))
    assert np.array_equal(_bits([float.fromhex(ln[4]) for ln in field]), ny.view(np.uint64))
    assert len(np.unique(nx)) > 9                                     # interpolated, not nine steps

    fill = [ln for ln in lines if ln[0] == "fill"]
    wx, wy = F.fill_cells(F.FILL_MASK, bx, by)
    assert np.array_equal(_bits([float.fromhex(ln[2]) for ln in fill]), wx.ravel().view(np.uint64))
    assert np.array_equal(_bits([float.fromhex(ln[3]) for ln in fill]), wy.ravel().view(np.uint64))
    none = [ln for ln in lines if ln[0] == "none"]
    assert len(none) == 12 and all(float.fromhex(ln[2]) == 0.0 and float.fromhex(ln[3]) == 0.0 for ln in none)

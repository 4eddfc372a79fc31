"""OptimizerGlobal on the CPU: the numpy restatement (tests/global_ref.py) against hand-computed clouds and a literal
loop transcription of optimizer_global.cpp, the ABI of the new structs, and the new symbols in the library."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import global_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the candidate grid ----

def test_default_grid_is_the_reference_loop():
    xs, ys = G.default_grid()
    assert (len(xs), len(ys)) == (180, 80)     # not the 181 x 81 the reference prints
    v, want = -0.09, []
    while v < 0.09:
        want.append(v)
        v += 0.001
    assert xs == want
    assert xs[0] == -0.09 and ys[0] == -0.04
    # accumulated, not exact: the value next to zero is a rounding residue, and the last one overshoots 0.089
    assert xs[90] != 0.0 and abs(xs[90]) < 1e-15
    assert ys[40] != 0.0 and abs(ys[40]) < 1e-15
    assert xs[-1] != 0.089 and abs(xs[-1] - 0.089) < 1e-12


def test_fixed_point_score_is_floor_of_the_double():
    rng = np.random.default_rng(0)
    cnt = rng.integers(1, 63 * 63 + 1, 20000)
    s = cnt * rng.integers(1, 256, 20000) - rng.integers(0, 255, 20000)
    s = np.maximum(s, cnt)
    got = G.score_fixed(s, cnt)
    want = [math.floor((int(a) / int(b)) * 2.0 ** 32) for a, b in zip(s, cnt)]
    assert got.tolist() == want
    assert G.score_fixed([0], [0]).tolist() == [0]


# ---- a literal transcription of optimizer_global.cpp:4-101 (loops, no numpy vectorisation) ----

def _literal_project_all(fr_x, fr_y, t, w, nx, ny, nz=G.NZ):
    s, mw = w["scale"], w["metric_wsize"]
    Rb, Cb = w["scale_bordered_img_x"], w["scale_bordered_img_y"]
    img = [[0] * Cb for _ in range(Rb)]
    pr_x, pr_y = G.project(fr_x, fr_y, t, nx, ny, nz)
    acc = []
    for px, py in zip(pr_x, pr_y):
        x = math.trunc(px * s - w["x_min"] * s)
        y = math.trunc(py * s - w["y_min"] * s)
        if x >= w["scale_img_x"] - s or x < 0 or y >= w["scale_img_y"] - s or y < 0:
            acc.append(None)
            continue
        acc.append((x, y))
        x += s // 2 + mw // 2
        y += s // 2 + mw // 2
        for jx in range(x - s // 2, x + s // 2 + 1):
            for jy in range(y - s // 2, y + s // 2 + 1):
                if img[jx][jy] < 255:
                    img[jx][jy] += 1
    img = np.array(img, dtype=np.int64)
    if s > 1:   # the stated Gaussian, written out with an explicit BORDER_REFLECT_101
        taps = G.TAPS[s // 2]
        n2 = sum(taps) ** 2
        h = s // 2

        def refl(i, n):
            while i < 0 or i >= n:
                i = -i if i < 0 else 2 * (n - 1) - i
            return i
        out = np.zeros_like(img)
        for i in range(Rb):
            for j in range(Cb):
                a = 0
                for da in range(-h, h + 1):
                    for db in range(-h, h + 1):
                        a += taps[da + h] * taps[db + h] * img[refl(i + da, Rb), refl(j + db, Cb)]
                out[i, j] = (a + n2 // 2) // n2
        img = out
    scores = []
    for p in acc:
        if p is None:
            scores.append(None)
            continue
        cx, cy = p[0] + mw // 2 + s // 2, p[1] + mw // 2 + s // 2
        tot = cnt = 0
        for j in range(cx - mw // 2, cx + mw // 2 + 1):
            for i in range(cy - mw // 2, cy + mw // 2 + 1):
                if img[j, i] <= 0:
                    continue
                cnt += 1
                tot += int(img[j, i])
        scores.append((tot, cnt))
    return img.astype(np.uint8), acc, scores


def _nine():
    fr_x = np.array([3, 4, 5, 3, 4, 5, 9, 9, 10], dtype=np.int64)
    fr_y = np.array([2, 2, 2, 6, 6, 7, 3, 3, 8], dtype=np.int64)
    t = np.array([0, 1000, 2000, 300000, 9000000, 12000000, 0, 0, 4000000], dtype=np.int64)
    return fr_x, fr_y, t


@pytest.mark.parametrize("scale,mw", [(1, 3), (3, 5), (3, 15), (5, 3), (7, 1)])
@pytest.mark.parametrize("nxny", [(0.0, 0.0), (0.05, -0.03), (-0.2, 0.1)])
def test_restatement_matches_the_literal_loops(scale, mw, nxny):
    fr_x, fr_y, t = _nine()
    g = G.Global(fr_x, fr_y, t, scale, mw)
    img, cur, S = g.project_all(*nxny)
    limg, acc, sc = _literal_project_all(fr_x, fr_y, t, g.w, *nxny)
    assert np.array_equal(img, limg)
    wantS = 0
    for p, q in zip(acc, sc):
        if p is None:
            continue
        tot, cnt = q
        f = np.float32(tot / cnt if cnt else 0.0)
        assert cur[p[0], p[1]] == f
        wantS += (tot << 32) // cnt if cnt else 0
    assert S == wantS


# ---- hand-built clouds ----

def test_one_event_is_never_accepted():
    # the bounding box of one event is one sensor pixel: scale_img - scale == 0, so x < 0 is needed
    g = G.Global([7], [9], [0], 3, 5)
    assert (g.w["scale_img_x"], g.w["scale_bordered_img_x"]) == (3, 8)
    img, cur, S = g.project_all(0.0, 0.0)
    assert S == 0 and not img.any() and not cur.any()
    assert g.max_score.tolist() == [0.0]
    assert g.best_pr_x.tolist() == [7.0] and g.best_pr_y.tolist() == [9.0]


def test_two_events_edge_rejection_and_score():
    # scale 1, window 3: (0, 0) lands on pixel (0, 0); (2, 2) lies exactly on the scale_img - scale edge and is rejected
    g = G.Global([0, 2], [0, 2], [0, 0], 1, 3)
    assert g.w["scale_img_x"] == 3 and g.w["scale_bordered_img_x"] == 6
    img, cur, S = g.project_all(0.0, 0.0)
    want = np.zeros((6, 6), np.uint8)
    want[1, 1] = 1                       # shifted by scale / 2 + metric_wsize / 2 = 1
    assert np.array_equal(img, want)
    assert cur[0, 0] == 1.0 and cur.sum() == 1.0
    assert S == 1 << 32
    assert g.max_score.tolist() == [1.0, 0.0]
    assert g.best_pr_x.tolist() == [0.0, 2.0]


def test_saturation_at_255():
    fr_x = [0] * 300 + [1, 2]
    fr_y = [0] * 300 + [1, 2]
    g = G.Global(fr_x, fr_y, [0] * 302, 1, 3)
    img, cur, S = g.project_all(0.0, 0.0)
    assert img[1, 1] == 255 and img[2, 2] == 1 and img.sum() == 256
    # the window of (0, 0) holds 255 and 1: mean 128; that of (1, 1) holds 255, 1 (its own) -> also 128
    assert cur[0, 0] == 128.0 and cur[1, 1] == 128.0
    assert S == 301 * (128 << 32)
    assert g.max_score[:301].tolist() == [128.0] * 301 and g.max_score[301] == 0.0


def test_strict_greater_keeps_the_first_candidate():
    # every t = 0: the projection does not depend on (nx, ny), every candidate scores the same
    fr_x, fr_y, _ = _nine()
    g = G.Global(fr_x, fr_y, np.zeros(9, np.int64), 3, 5)
    s1 = g.project_all(0.01, 0.02)[2]
    first = g.max_score.copy()
    s2 = g.project_all(-0.03, 0.0)[2]
    assert s1 == s2 and np.array_equal(g.max_score, first)
    acc = g.max_score > 0
    assert acc.tolist() == [True] * 8 + [False]   # (10, 8) is on the bounding box's far edge: rejected
    assert (g.best_nx[acc] == 0.01).all() and (g.best_ny[acc] == 0.02).all()


def test_search_argmax_and_uv():
    fr_x, fr_y, t = _nine()
    g = G.Global(fr_x, fr_y, t, 3, 5)
    xs, ys = G.sweep_values(-0.02, 0.02, 0.01), G.sweep_values(-0.01, 0.01, 0.01)
    surf, (bnx, bny, bs) = g.search(xs, ys)
    k = int(np.argmax(surf))
    assert (bnx, bny, bs) == (xs[k // len(ys)], ys[k % len(ys)], surf.max())
    u, v = g.best_uv()
    for i in range(9):
        assert (u[i], v[i]) == G.compute_uv(g.best_nx[i], g.best_ny[i])
    assert G.compute_uv(0.0127, 0.0) == pytest.approx((10.0, 0.0))    # nx = u * NZ / 1e5


# ---- ABI ----

_PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "bf_accel.h"
#define F(S, M) printf(#S " " #M " %zu\n", offsetof(S, M))
int main(void) {
    printf("bf_global_window size %zu\n", sizeof(bf_global_window));
    printf("bf_global_search_opts size %zu\n", sizeof(bf_global_search_opts));
    printf("bf_global_result size %zu\n", sizeof(bf_global_result));
    F(bf_global_window, scale); F(bf_global_window, metric_wsize); F(bf_global_window, x_min); F(bf_global_window, y_min);
    F(bf_global_window, x_max); F(bf_global_window, y_max); F(bf_global_window, scale_img_x); F(bf_global_window, scale_img_y);
    F(bf_global_window, scale_bordered_img_x); F(bf_global_window, scale_bordered_img_y);
    F(bf_global_search_opts, x_low); F(bf_global_search_opts, x_hi); F(bf_global_search_opts, x_step);
    F(bf_global_search_opts, y_low); F(bf_global_search_opts, y_hi); F(bf_global_search_opts, y_step); F(bf_global_search_opts, nz);
    F(bf_global_result, best_nx); F(bf_global_result, best_ny); F(bf_global_result, best_sum); F(bf_global_result, n_x);
    F(bf_global_result, n_y);
    return 0;
}
'''


def test_struct_mirrors_match_the_header(tmp_path):
    from better_flow_amd import accel
    src = tmp_path / "probe.cpp"
    src.write_text(_PROBE)
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        s, m, v = line.split()
        got[(s, m)] = int(v)
    for cname, mirror in (("bf_global_window", accel.GlobalWindow), ("bf_global_search_opts", accel.GlobalSearchOpts),
                          ("bf_global_result", accel.GlobalResult)):
        assert got[(cname, "size")] == ctypes.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert got[(cname, fname)] == getattr(mirror, fname).offset, (cname, fname)
        assert len(mirror._fields_) == sum(1 for (s, m) in got if s == cname and m != "size")


def test_library_exports_the_search():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    for name in ("bf_global_search_opts_default", "bf_global_set_window", "bf_global_project_all", "bf_global_search",
                 "bf_global_get_events"):
        assert hasattr(lib, name), name
    o = accel.GlobalSearchOpts()
    lib.bf_global_search_opts_default(ctypes.byref(o))
    assert (o.x_low, o.x_hi, o.x_step, o.y_low, o.y_hi, o.y_step, o.nz) == (-0.09, 0.09, 0.001, -0.04, 0.04, 0.001, 127.0)
    # no context: an argument error, not a crash
    assert lib.bf_global_set_window(None, 5, 21, None) == accel.BF_ERR_ARG

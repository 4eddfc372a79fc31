"""The projection of a grouping on the CPU: the ABI of the new structs and symbol, the table of DESIGN section 17 as exact
integers on the restatement (tests/project_groups_ref.py) -- the contrast sum N^2 separates the right grouping from every single
model and from the wrong pairing --, mutations of the restatement's rules on hand-made cases, bf::ObjectRenderer's host path
(host/better_flow/object_render.h) through the oracle-backed C-ABI stand-in, also as a stand-alone ASan / UBSan program, and the
command line's new flags on the oracle-backed build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import project_groups_ref as pr
import segment_scene as scene
from test_gpu_groups import seeded_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RES = (scene.H, scene.W)


# ---- (a) ABI ----

def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    from better_flow_amd import accel
    mirrors = {"bf_project_opts": accel.ProjectOpts, "bf_group_score": accel.GroupScore, "bf_project_info": accel.ProjectInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bf_accel.h"',
             'static const unsigned char pal[BF_PROJECT_PALETTE_SIZE][3] = BF_PROJECT_PALETTE;', 'int main(void) {']
    for cname, m in mirrors.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in m._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['for (int k = 0; k < BF_PROJECT_PALETTE_SIZE; ++k) printf("palette.%d %d,%d,%d\\n", k, pal[k][0], pal[k][1], pal[k][2]);',
              "return 0; }"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, m in mirrors.items():
        assert int(got[cname]) == ctypes.sizeof(m), cname
        for f, _ in m._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(m, f).offset, (cname, f)
    assert [ctypes.sizeof(m) for m in mirrors.values()] == [32, 32, 48]
    # the palette: the header's, the binding's and the restatement's are one table of 12 distinct colours
    header = [tuple(int(v) for v in got["palette.%d" % k].split(",")) for k in range(12)]
    assert header == [tuple(c) for c in accel.PROJECT_PALETTE] == [tuple(c) for c in pr.PALETTE.tolist()]
    assert len(set(header)) == 12 and all(max(c) == 255 for c in header)


def test_symbol_exported_and_bound():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert "bf_project_groups" in accel.EXPORTS and hasattr(lib, "bf_project_groups")
    assert callable(accel.Accel.project_groups)
    out = (ctypes.c_int32 * 16)()
    assert lib.bf_abi_struct_sizes(out, 16) == 10   # (its ten entries stay)


# ---- (b) the scene on the restatement: the table of DESIGN section 17 ----

@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def table(sc):
    """sum N^2 per row of the table and scale."""
    ids, ms = pr.scene_truth(sc)
    zero = ar.model_of_velocity((0.0, 0.0))
    one = np.zeros_like(ids)
    out = {}
    for s in (1, 3):
        out[s] = dict(truth=pr.project(sc, ids, ms, s, RES)["info"]["sum_sq"],
                      background_one_group=pr.project(sc, one, ms[:1], s, RES)["info"]["sum_sq"],
                      background_both_groups=pr.project(sc, ids, [ms[0], ms[0]], s, RES)["info"]["sum_sq"],
                      zero=pr.project(sc, one, [zero], s, RES)["info"]["sum_sq"],
                      swapped=pr.project(sc, ids, ms[::-1], s, RES)["info"]["sum_sq"])
    return out


def test_the_table_in_exact_integers(table):
    print(table)
    assert table[1] == dict(truth=647362, background_one_group=356908, background_both_groups=356908, zero=363092, swapped=313173)
    assert table[3] == dict(truth=5837588, background_one_group=3135808, background_both_groups=3135808, zero=3267828, swapped=2770511)


def test_four_assignment_rounds_from_the_true_models(sc):
    ids, ms = pr.scene_truth(sc)
    gid = ar.rounds(sc, ms, 3, RES, 4)[-1][0]
    r = pr.project(sc, gid, ms, 3, RES)
    assert (r["info"]["unassigned"], r["info"]["sum_sq"]) == (15, 5889285)


@pytest.mark.parametrize("scale", [1, 3])
def test_the_right_grouping_scores_1_5_times_any_single_model_and_the_swap_below_one(table, scale):
    t = table[scale]
    singles = [t["background_one_group"], t["background_both_groups"], t["zero"]]
    assert all(t["truth"] >= 1.5 * v for v in singles), t
    assert all(t["swapped"] < v for v in singles), t


def test_splitting_the_patch_under_one_model_keeps_the_total_and_lowers_the_groups_sum(sc):
    ids, ms = pr.scene_truth(sc)
    whole = pr.project(sc, ids, ms, 3, RES)
    patch = np.flatnonzero(ids == 1)
    split = ids.copy()
    split[patch[1::2]] = 2
    two = pr.project(sc, split, ms + [ms[1]], 3, RES)
    assert two["info"]["sum_sq"] == whole["info"]["sum_sq"] and two["count"].tobytes() == whole["count"].tobytes()
    assert sum(s["sum_sq"] for s in two["scores"]) < sum(s["sum_sq"] for s in whole["scores"])
    assert two["scores"][1]["events"] + two["scores"][2]["events"] == whole["scores"][1]["events"]


# ---- (c) hand-made cases and mutations ----

def hand(points, ids):
    """Events at t = 0 (no model moves them) on a 6 x 8 sensor: points = [(row, column), ...]."""
    sl = dict(fr_x=np.array([p[0] for p in points], np.int32), fr_y=np.array([p[1] for p in points], np.int32),
              t=np.zeros(len(points), np.int64))
    return sl, np.array(ids, np.int32)


STILL = gr.oracle.Model()


def test_two_groups_tied_on_a_pixel_give_the_smaller_id():
    sl, ids = hand([(2, 3), (2, 3), (2, 3), (2, 3), (4, 4)], [1, 2, 2, 1, 2])
    r = pr.project(sl, ids, [STILL] * 3, 1, (6, 8))
    w = ar.window(1, (6, 8), 0)
    x, y = 2 + int(w["x_shift"]), 3 + int(w["y_shift"])
    assert r["count"][x, y] == 4 and r["label"][x, y] == 1
    assert [s["pixels_owned"] for s in r["scores"]] == [0, 1, 1] and [s["pixels_hit"] for s in r["scores"]] == [0, 1, 2]
    up = pr.project(sl, ids, [STILL] * 3, 1, (6, 8), mutate="ties_up")
    assert up["label"][x, y] == 2 and up["label"].tobytes() != r["label"].tobytes()
    assert up["count"].tobytes() == r["count"].tobytes()


def test_an_empty_group_and_a_group_entirely_outside():
    sl, ids = hand([(2, 3), (2, 4), (3, 3)], [0, 2, 2])
    sl["t"][:] = 20_000_000
    away = ar.model_of_velocity((100000.0, 0.0))   # 2000 rows in 20 ms
    r = pr.project(sl, ids, [STILL, STILL, away], 3, (6, 8))
    assert [s["events"] for s in r["scores"]] == [1, 0, 2] and [s["inside"] for s in r["scores"]] == [1, 0, 0]
    assert r["info"]["outside"] == 2 and r["info"]["pixels"] == 9 and r["info"]["sum"] == 9 and r["info"]["sum_sq"] == 9
    assert r["scores"][1] == dict(events=0, inside=0, pixels_hit=0, pixels_owned=0, max=0, sum_sq=0)
    assert set(r["label"].ravel().tolist()) == {-1, 0}


def test_ids_of_minus_one_are_in_no_plane():
    sl, ids = hand([(2, 3), (2, 3), (4, 5)], [0, -1, -1])
    r = pr.project(sl, ids, [STILL], 1, (6, 8))
    assert r["info"]["unassigned"] == 2 and r["info"]["sum"] == 1 and r["scores"][0]["events"] == 1
    m = pr.project(sl, ids, [STILL], 1, (6, 8), mutate="count_unassigned")
    assert m["info"]["sum"] == 3 and m["count"].tobytes() != r["count"].tobytes() and m["info"]["unassigned"] == 0


def test_the_colour_saturates_at_gain_and_takes_the_owners_level():
    pts = [(2, 3)] * 40 + [(2, 3)] * 3 + [(4, 4)] * 2
    sl, ids = hand(pts, [0] * 40 + [1] * 3 + [1] * 2)
    w = ar.window(1, (6, 8), 0)
    px = lambda p: (p[0] + int(w["x_shift"]), p[1] + int(w["y_shift"]))
    r = pr.project(sl, ids, [STILL, STILL], 1, (6, 8), gain=8)
    assert r["bgr"][px((2, 3))].tolist() == [255, 255, 255]                    # 40 * 8 saturates group 0's white
    assert r["bgr"][px((4, 4))].tolist() == [0, 0, 255 * 16 // 255]            # group 1's red at level 2 * 8
    assert r["bgr"][px((0, 0))].tolist() == [0, 0, 0] and r["label"][px((0, 0))] == -1
    low = pr.project(sl, ids, [STILL, STILL], 1, (6, 8), gain=3)
    assert low["bgr"][px((2, 3))].tolist() == [120, 120, 120]                  # 40 * 3 = 120 <= 255: the owner's 40, not N = 43
    tot = pr.project(sl, ids, [STILL, STILL], 1, (6, 8), gain=3, mutate="label_by_total")
    assert tot["bgr"][px((2, 3))].tolist() == [129, 129, 129] and tot["bgr"].tobytes() != low["bgr"].tobytes()
    assert tot["label"].tobytes() == low["label"].tobytes()


def test_group_colours_repeat_after_twelve():
    pts = [(k // 7 + 1, k % 7) for k in range(14)]
    sl, ids = hand(pts, list(range(14)))
    r = pr.project(sl, ids, [STILL] * 14, 1, (6, 8), gain=255)
    w = ar.window(1, (6, 8), 0)
    px = lambda p: (p[0] + int(w["x_shift"]), p[1] + int(w["y_shift"]))
    assert r["bgr"][px(pts[12])].tolist() == r["bgr"][px(pts[0])].tolist() == pr.PALETTE[0].tolist()
    assert r["bgr"][px(pts[13])].tolist() == pr.PALETTE[1].tolist() and r["label"][px(pts[13])] == 13


def test_sums_wrap_modulo_two_to_the_64():
    assert pr.sum_sq(np.array([1 << 32, 3], dtype=np.uint64)) == 9
    assert pr.sum_sq(np.array([(1 << 32) - 1] * 2, dtype=np.uint64)) == (2 * ((1 << 32) - 1) ** 2) % (1 << 64)


# ---- (d) bf::ObjectRenderer's host path against the restatement ----

def build_program(out_dir, sanitize):
    exe = os.path.join(out_dir, "test_object_render" + ("_san" if sanitize else ""))
    extra = SAN if sanitize else []
    obj = exe + "_oracle.o"
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-ffp-contract=off"] + extra + ["-c", os.path.join(ROOT, "oracle", "bf_oracle.c"),
                                                                                    "-o", obj])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra"] + extra + [
        "-I" + os.path.join(ROOT, "better_flow_amd", "host"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
        os.path.join(ROOT, "tests", "cpp", "test_object_render.cpp"), os.path.join(ROOT, "tests", "shim", "bf_accel_oracle_shim.cpp"), obj,
        "-lm", "-o", exe])
    return exe


def ids64(n):
    """Ids -1 .. 63 spread over the slice, groups 5 and 40 empty."""
    ids = ((np.arange(n) * 7) % 65 - 1).astype(np.int32)
    ids[(ids == 5) | (ids == 40)] = -1
    return ids


def program_case(exe, tmp, name, sl, ids, models, scale, res, margin=0, gain=8, expect_path="host"):
    """Runs the program on one case and compares everything it writes with the restatement."""
    from better_flow_amd import accel
    d = os.path.join(str(tmp), name)
    os.makedirs(d)
    ev, idf, mf, prefix = os.path.join(d, "events.txt"), os.path.join(d, "ids.i32"), os.path.join(d, "models.bin"), os.path.join(d, "out_")
    with open(ev, "w") as f:
        for a, b, c in zip(sl["fr_x"].tolist(), sl["fr_y"].tolist(), sl["t"].tolist()):
            f.write("%d %d %d\n" % (a, b, c))
    np.asarray(ids, np.int32).tofile(idf)
    with open(mf, "wb") as f:
        for m in models:
            f.write(bytes(accel.Model(**{k: getattr(m, k) for k, _ in gr.oracle.Model._fields_})))
    r = subprocess.run([exe, ev, idf, mf, str(len(models)), str(scale), str(res[0]), str(res[1]), str(margin), str(gain), prefix],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode().splitlines()[0] == "path " + expect_path
    ref = pr.project(sl, ids, models, scale, res, margin, gain)
    assert np.fromfile(prefix + "count.u32", dtype=np.uint32).tobytes() == ref["count"].tobytes(), name
    assert np.fromfile(prefix + "label.i32", dtype=np.int32).tobytes() == ref["label"].tobytes(), name
    assert np.fromfile(prefix + "bgr.u8", dtype=np.uint8).tobytes() == ref["bgr"].tobytes(), name
    scores = [accel.GroupScore.from_buffer_copy(open(prefix + "scores.bin", "rb").read()[32 * k:32 * k + 32]) for k in range(len(models))]
    assert [[getattr(s, f) for f in pr.SCORE_FIELDS] for s in scores] == [[s[f] for f in pr.SCORE_FIELDS] for s in ref["scores"]], name
    info = accel.ProjectInfo.from_buffer_copy(open(prefix + "info.bin", "rb").read())
    assert {k: getattr(info, k) for k in pr.INFO_FIELDS} == ref["info"], name
    # the writers
    R, C = ref["count"].shape
    ppm = open(prefix + "img.ppm", "rb").read()
    head = b"P6\n%d %d\n255\n" % (C, R)
    assert ppm.startswith(head) and ppm[len(head):] == ref["bgr"][:, :, ::-1].tobytes(), name
    pgm = open(prefix + "label.pgm", "rb").read()
    head = b"P5\n%d %d\n65535\n" % (C, R)
    assert pgm.startswith(head) and pgm[len(head):] == (ref["label"] + 1).astype(">u2").tobytes(), name
    lines = [ln.split() for ln in open(prefix + "scores.txt").read().splitlines()]
    assert [[int(v) for v in ln] for ln in lines[:-1]] == [[k] + [s[f] for f in pr.SCORE_FIELDS] for k, s in enumerate(ref["scores"])]
    assert lines[-1][0] == "info" and [int(v) for v in lines[-1][1:]] == [ref["info"][f] for f in pr.INFO_FIELDS], name
    return ref


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_object_renderer_host_path_equals_the_restatement(sc, tmp_path, sanitize):
    exe = build_program(str(tmp_path), sanitize)
    ids, ms = pr.scene_truth(sc)
    for scale in (1, 3):
        ref = program_case(exe, tmp_path, "scene%d" % scale, sc, ids, ms, scale, RES)
        assert ref["info"]["sum_sq"] == {1: 647362, 3: 5837588}[scale]
    program_case(exe, tmp_path, "k64", sc, ids64(len(sc["t"])), seeded_models(64), 3, RES, margin=2, gain=40)
    empty = dict(fr_x=np.zeros(0, np.int32), fr_y=np.zeros(0, np.int32), t=np.zeros(0, np.int64))
    ref = program_case(exe, tmp_path, "zero", empty, np.zeros(0, np.int32), ms, 3, (12, 16))
    assert not ref["count"].any() and (ref["label"] == -1).all() and not any(ref["info"].values())


# ---- (e) the command line on the oracle-backed build ----

@pytest.fixture(scope="module")
def oracle_cli():
    sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))
    import build as shim_build
    return shim_build.build()


def test_cli_help_lists_the_flags(oracle_cli, tmp_path):
    out = subprocess.run([oracle_cli, "--help"], cwd=str(tmp_path), stdout=subprocess.PIPE, timeout=60).stdout.decode()
    for flag in ("--objects-img", "--objects-img-gain=<n>"):
        assert flag in out, flag


@pytest.mark.parametrize("args", (["--objects-img"], ["--objects-img", "--objects-img-gain=4"], ["--objects=2", "--objects-img", "--objects-img-gain=0"]),
                         ids=("alone", "alone_with_gain", "gain_zero"))
def test_cli_objects_img_refusals(oracle_cli, tmp_path, args):
    from better_flow_amd import synth
    out = tmp_path / "out"
    out.mkdir()
    txt = str(tmp_path / "ev.txt")
    synth.write_txt(txt, synth.make_slice(3000, 64, 64, 0.03, seed=5))
    r = subprocess.run([oracle_cli] + args + ["--quiet", "--img-prefix", str(out), txt], cwd=str(out), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 1 and b"--objects-img" in r.stderr, (r.returncode, r.stderr[-500:])
    assert os.listdir(str(out)) == []


def test_cli_on_a_library_without_the_entries_still_names_the_proposal_first(oracle_cli, tmp_path):
    from better_flow_amd import synth
    out = tmp_path / "out"
    out.mkdir()
    txt = str(tmp_path / "ev.txt")
    synth.write_txt(txt, synth.make_slice(3000, 64, 64, 0.03, seed=5))
    r = subprocess.run([oracle_cli, "--objects=2", "--objects-img", "--quiet", "--img-prefix", str(out), txt], cwd=str(out),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"bf_propose_models" in r.stderr and b"bf_project_groups" not in r.stderr, (r.returncode, r.stderr[-500:])
    assert os.listdir(str(out)) == []

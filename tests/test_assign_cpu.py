"""The assignment step on the CPU: the ABI of the new structs and symbol, the claims of DESIGN section 15 as conditions on the
restatement (tests/assign_ref.py) -- assignment alone separates the two motions of the scene when the candidates are near the
truth, and alternating it with the grouped fit (tests/groups_ref.py on the CPU oracle) grows the seed DESIGN section 14 shows to
be useless into the whole object --, mutations of the restatement's rules, and bf::MotionAssigner's host paths
(host/better_flow/motion_assign.h) through the oracle-backed C-ABI stand-in, also as a stand-alone ASan / UBSan program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import oracle
import segment_scene as scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RES, GUARD, MIN_EVENTS, HARD_CAP = (scene.H, scene.W), (90, 120), 100, 20000
SEED = (11.0, -45.0)   # DESIGN section 14's failed fit on the segmentation's component


# ---- (a) ABI ----

def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    from better_flow_amd import accel
    mirrors = {"bf_assign_opts": accel.AssignOpts, "bf_assign_info": accel.AssignInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bf_accel.h"', 'int main(void) {']
    for cname, m in mirrors.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in m._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["return 0; }"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, m in mirrors.items():
        assert int(got[cname]) == ctypes.sizeof(m), cname
        for f, _ in m._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(m, f).offset, (cname, f)
    assert (ctypes.sizeof(accel.AssignOpts), ctypes.sizeof(accel.AssignInfo)) == (32, 32)


def test_symbol_exported_and_bound():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert "bf_assign_groups" in accel.EXPORTS and hasattr(lib, "bf_assign_groups")
    assert callable(accel.Accel.assign_groups)


# ---- (b) the scene on the restatement ----

@pytest.fixture(scope="module")
def sc():
    return scene.make()


def candidates(v):
    return [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity(v)]


@pytest.fixture(scope="module")
def true_rounds(sc):
    out = ar.rounds(sc, candidates(scene.V_PATCH), 3, RES, 4)
    for r in out:
        r[0].setflags(write=False)
    return out


def test_window_is_the_sensor_widened_by_the_margin():
    w = ar.window(3, RES, 0)
    assert (w["R"], w["C"], w["wsx"], w["wsy"]) == (270, 360, 267, 357)
    w = ar.window(5, RES, 6)
    assert (w["x_min"], w["x_max"], w["R"], w["C"]) == (-6, scene.H + 5, 5 * (scene.H + 11) + 5, 5 * (scene.W + 11) + 5)


def test_true_flows_separate_the_scene(sc, true_rounds):
    rp = [ar.recall_purity(sc, r[0]) for r in true_rounds]
    print("candidates = the true flows: (recall, purity) per round", [(round(a, 3), round(b, 3)) for a, b in rp])
    assert rp[0][0] >= 0.85 and rp[0][1] >= 0.95
    assert rp[3][0] >= 0.99 and rp[3][1] >= 0.95
    info = true_rounds[0][3]
    assert info["assigned"] + info["unassigned"] == len(sc["t"]) == info["changed"] + info["unassigned"]
    assert true_rounds[0][2].sum() == len(sc["t"])


def test_a_candidate_100_px_s_off_still_collects_the_patch(sc):
    rs = ar.rounds(sc, candidates((300.0, -200.0)), 3, RES, 4)
    rp = [ar.recall_purity(sc, r[0]) for r in rs]
    print("candidate (300, -200): (recall, purity) per round", [(round(a, 3), round(b, 3)) for a, b in rp])
    assert rp[3][0] >= 0.97


# ---- (c) alternation on the oracle ----

@pytest.fixture(scope="module")
def alternation(sc):
    return ar.alternate(sc, candidates(SEED), 3, RES, GUARD, MIN_EVENTS, HARD_CAP, rounds_per_fit=2, max_alternations=5)


def test_alternation_grows_the_failed_seed_to_the_object(sc, alternation):
    models, gid, records = alternation
    for i, r in enumerate(records):
        print("alternation %d: changed %d, counts %s, iterations %s, flows %s" % (i + 1, r["changed"], r["counts"], r["iterations"],
                                                                                 r["flows"]))
    rec, pur = ar.recall_purity(sc, gid)
    print("recall %.4f, purity %.4f" % (rec, pur))
    assert len(records) <= 5
    assert rec >= 0.99
    flow = [r for r in records if r["flows"]][-1]["flows"][1]
    assert abs(flow[0] - scene.V_PATCH[0]) <= 5.0 and abs(flow[1] - scene.V_PATCH[1]) <= 5.0, flow


# ---- (d) mutations ----

def test_one_event_moved_by_a_pixel_changes_the_result(sc, true_rounds):
    """Event i's time changed by the time the patch's candidate needs to cross one sensor pixel: its pixel under that
    candidate moves, so its own score or a neighbour's leave-one-out count does."""
    ms = candidates(scene.V_PATCH)
    base = true_rounds[0]
    w = ar.window(3, RES, 0)
    i = int(np.flatnonzero(sc["is_patch"] & (base[0] == 1) & (sc["t"] < 20_000_000))[0])
    moved = dict(sc)
    moved["t"] = sc["t"].copy()
    moved["t"][i] += int(1e9 / 300.0)   # |V_PATCH's column velocity| = 300 px/s: one sensor pixel, three window pixels
    _, X0, Y0 = ar.pixels(sc, ms[1], w, 3)
    _, X1, Y1 = ar.pixels(moved, ms[1], w, 3)
    assert (X0[i], Y0[i]) != (X1[i], Y1[i])
    r = ar.assign(moved, ms, 3, RES)
    assert r[0].tobytes() != base[0].tobytes() or r[1].tobytes() != base[1].tobytes()


def test_dropping_the_leave_one_out_changes_the_result(sc, true_rounds):
    r = ar.assign(sc, candidates(scene.V_PATCH), 3, RES, mutate="no_loo")
    assert r[1].tobytes() != true_rounds[0][1].tobytes()
    assert r[3]["unassigned"] < true_rounds[0][3]["unassigned"]   # an event alone on its pixel scores 1 with itself


def test_breaking_ties_towards_the_larger_k_changes_the_result(sc, true_rounds):
    r = ar.assign(sc, candidates(scene.V_PATCH), 3, RES, mutate="ties_up")
    assert r[1].tobytes() == true_rounds[0][1].tobytes()
    assert r[0].tobytes() != true_rounds[0][0].tobytes()


# ---- (e) bf::MotionAssigner's host paths against the restatement ----

def build_program(out_dir, sanitize):
    exe = os.path.join(out_dir, "test_motion_assign" + ("_san" if sanitize else ""))
    extra = SAN if sanitize else []
    obj = exe + "_oracle.o"
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-ffp-contract=off"] + extra + ["-c", os.path.join(ROOT, "oracle", "bf_oracle.c"),
                                                                                    "-o", obj])
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra"] + extra + [
        "-I" + os.path.join(ROOT, "better_flow_amd", "host"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
        os.path.join(ROOT, "tests", "cpp", "test_motion_assign.cpp"), os.path.join(ROOT, "tests", "shim", "bf_accel_oracle_shim.cpp"), obj,
        "-lm", "-o", exe])
    return exe


def flat(r):
    gid, score, counts, info = r
    return np.concatenate([gid, score, counts, np.array([info[k] for k in ("models", "rows", "cols", "assigned", "unassigned", "changed",
                                                                            "max_score")] + [0])]).astype(np.int32)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_motion_assigner_host_paths_equal_the_restatement(sc, alternation, tmp_path, sanitize):
    from better_flow_amd import accel
    exe = build_program(str(tmp_path), sanitize)
    ev, mf, prefix = str(tmp_path / "events.txt"), str(tmp_path / "models.bin"), str(tmp_path / "out_")
    with open(ev, "w") as f:
        for a, b, c in zip(sc["fr_x"].tolist(), sc["fr_y"].tolist(), sc["t"].tolist()):
            f.write("%d %d %d\n" % (a, b, c))
    cand = candidates(SEED)
    with open(mf, "wb") as f:
        for m in cand:
            f.write(bytes(accel.Model(**{k: getattr(m, k) for k, _ in oracle.Model._fields_})))
    r = subprocess.run([exe, ev, mf, "2", "3", str(scene.H), str(scene.W), "0", "1", str(GUARD[0]), str(GUARD[1]), str(MIN_EVENTS),
                        str(HARD_CAP), "2", "5", prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode().splitlines()[0] == "path host"
    # assign: byte for byte
    first = ar.assign(sc, cand, 3, RES)
    second = ar.assign(sc, cand, 3, RES, prior=first[0])
    assert np.fromfile(prefix + "first.i32", dtype=np.int32).tobytes() == flat(first).tobytes()
    assert np.fromfile(prefix + "second.i32", dtype=np.int32).tobytes() == flat(second).tobytes()
    # alternate: the Python alternation of (c)
    models, gid, records = alternation
    assert np.fromfile(prefix + "gid.i32", dtype=np.int32).tobytes() == gid.tobytes()
    raw = open(prefix + "models.bin", "rb").read()
    sz = ctypes.sizeof(accel.Model)
    assert len(raw) == 2 * sz
    for k in range(2):
        got = accel.Model.from_buffer_copy(raw[k * sz:(k + 1) * sz])
        for f, _ in oracle.Model._fields_:
            a, b = getattr(got, f), getattr(models[k], f)
            assert np.array(a).tobytes() == np.array(b).tobytes() or a == b, (k, f, a, b)
    rec = np.fromfile(prefix + "records.i32", dtype=np.int32).reshape(-1, 1 + 3 + 2)
    exp = [[r["changed"]] + r["counts"] + (r["iterations"] if r["iterations"] else [-1, -1]) for r in records]
    assert rec.tolist() == exp

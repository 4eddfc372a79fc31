"""The proposal step on the CPU: the ABI of the new structs and symbol, the claims of DESIGN section 16 as conditions on the
restatement (tests/propose_ref.py on the numpy search of tests/global_ref.py) -- the modes of the per-event best flow are the
scene's two motions, and the alternation of DESIGN section 15 from them meets that section's own bars --, mutations of the
restatement's rules, hand-made states, bf::ModelProposer::propose_from_best (host/better_flow/model_proposer.h) as a stand-alone
program, also under ASan / UBSan, and the command-line flag on the oracle-backed build, which has no device entries."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import assign_ref as ar
import global_ref as gref
import propose_ref as pr
import segment_scene as scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
RES, GUARD, MIN_EVENTS, HARD_CAP = (scene.H, scene.W), (90, 120), 100, 20000
STEP_PX_S = 0.04 / 1.27e-3   # one step of the 0.04 lattice: 31.5 px / s
# (u, v, smoothed votes) of the scene's first four proposals at r = 1, suppress = 2
TABLE = [(-63.0, 94.5, 3878), (409.4, -315.0, 1621), (503.9, -346.5, 746), (503.9, -252.0, 617)]
TABLE_INDEX = [597, 1124, 1231, 1234]


# ---- (a) ABI ----

def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    from better_flow_amd import accel
    mirrors = {"bf_propose_opts": accel.AccelProposeOpts, "bf_proposal": accel.Proposal, "bf_propose_info": accel.ProposeInfo}
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
    assert [ctypes.sizeof(m) for m in mirrors.values()] == [32, 48, 32]
    assert pr.flat_proposals([]).dtype.itemsize == 48


def test_symbol_exported_and_bound():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    assert "bf_propose_models" in accel.EXPORTS and hasattr(lib, "bf_propose_models")
    assert callable(accel.Accel.propose_models)


# ---- (b) the scene on the restatement ----

@pytest.fixture(scope="module")
def sc():
    return scene.make()


def searched(sc, scale, step):
    xs = gref.sweep_values(-0.72, 0.72, step)
    g = gref.Global(sc["fr_x"], sc["fr_y"], sc["t"], scale=scale, metric_wsize=5)
    g.search(xs, xs)
    for a in (g.max_score, g.best_nx, g.best_ny):
        a.setflags(write=False)
    return g, xs


@pytest.fixture(scope="module")
def state(sc):
    """The scene after the numpy search at scale 1 over the 36 x 36 lattice (3.5 s): computed once, never changed."""
    return searched(sc, 1, 0.04)


@pytest.fixture(scope="module")
def state_fine(sc):
    """... and over the 72 x 72 lattice of step 0.02."""
    return searched(sc, 1, 0.02)


def run(state, **kw):
    g, xs = state
    return pr.propose(g.max_score, g.best_nx, g.best_ny, xs, xs, **kw)


def test_the_scene_gives_the_table(sc, state):
    _, props, info, H, B = run(state, radius=1, suppress=2, max_models=4)
    print("proposals (u, v, votes, index):", [(round(p["u"], 1), round(p["v"], 1), p["votes"], p["index"]) for p in props], info)
    assert [p["index"] for p in props] == TABLE_INDEX
    assert [(round(p["u"], 1), round(p["v"], 1), p["votes"]) for p in props] == TABLE
    for p, truth in zip(props[:2], (scene.V_BACKGROUND, scene.V_PATCH)):
        assert abs(p["u"] - truth[0]) <= STEP_PX_S and abs(p["v"] - truth[1]) <= STEP_PX_S, (p, truth)
    assert info["voted"] + info["unscored"] + info["off_lattice"] == len(sc["t"]) and H.sum() == info["voted"]
    assert [p["votes"] for p in props] == sorted((p["votes"] for p in props), reverse=True)
    assert all(B[divmod(p["index"], 36)] == p["votes"] and H[divmod(p["index"], 36)] == p["peak"] for p in props)


def test_alternation_from_the_first_two_proposals_meets_section_15s_bars(sc, state):
    models, _, _, _, _ = run(state, radius=1, suppress=2, max_models=2)
    models, gid, records = ar.alternate(sc, models, 3, RES, GUARD, MIN_EVENTS, HARD_CAP, rounds_per_fit=2, max_alternations=5)
    rec, pur = ar.recall_purity(sc, gid)
    flow = [r for r in records if r["flows"]][-1]["flows"][1]
    print("alternations %d, recall %.4f, purity %.4f, group 1's median flow (%.1f, %.1f), iterations %s" %
          (len(records), rec, pur, flow[0], flow[1], [r["iterations"] for r in records]))
    assert len(records) <= 5 and rec >= 0.99
    assert abs(flow[0] - scene.V_PATCH[0]) <= 5.0 and abs(flow[1] - scene.V_PATCH[1]) <= 5.0, flow


# ---- (c) mutations: each must change the result ----

def test_without_smoothing_a_background_neighbour_comes_second(state_fine):
    smooth = run(state_fine, radius=1, suppress=2, max_models=2)[1]
    raw = run(state_fine, radius=0, suppress=1, max_models=2)[1]
    near = lambda p, v: abs(p["u"] - v[0]) <= STEP_PX_S and abs(p["v"] - v[1]) <= STEP_PX_S
    print("step 0.02: r = 1 %s; r = 0 %s" % ([(round(p["u"], 1), round(p["v"], 1), p["votes"]) for p in smooth],
                                             [(round(p["u"], 1), round(p["v"], 1), p["votes"]) for p in raw]))
    assert near(smooth[0], scene.V_BACKGROUND) and near(smooth[1], scene.V_PATCH)
    assert near(raw[0], scene.V_BACKGROUND) and near(raw[1], scene.V_BACKGROUND) and not near(raw[1], scene.V_PATCH)


def hand(bins, n_x=6, n_y=7):
    """A state by hand on the lattice x = 0 .. n_x - 1, y = 0 .. n_y - 1 (step 1): bins {(i, j): votes} -> arrays, lattice."""
    bx, by = [], []
    for (i, j), c in bins.items():
        bx += [float(i)] * c
        by += [float(j)] * c
    xs, ys = gref.sweep_values(0.0, n_x, 1.0), gref.sweep_values(0.0, n_y, 1.0)
    return np.ones(len(bx)), np.array(bx), np.array(by), xs, ys


def test_ties_towards_the_higher_index_change_the_pick():
    st = hand({(1, 1): 5, (4, 5): 5})
    a = pr.propose(*st, radius=0, suppress=1, max_models=2)[1]
    b = pr.propose(*st, radius=0, suppress=1, max_models=2, mutate="ties_up")[1]
    assert [p["index"] for p in a] == [1 * 7 + 1, 4 * 7 + 5] and [p["index"] for p in b] == [4 * 7 + 5, 1 * 7 + 1]


def test_suppress_zero_returns_adjacent_bins(state):
    sup0 = run(state, radius=1, suppress=0, max_models=4)[1]
    sup2 = run(state, radius=1, suppress=2, max_models=4)[1]
    i0, j0 = divmod(sup0[0]["index"], 36)
    i1, j1 = divmod(sup0[1]["index"], 36)
    assert max(abs(i0 - i1), abs(j0 - j1)) == 1 and [p["index"] for p in sup0] != [p["index"] for p in sup2]


def test_counting_unscored_events_changes_the_votes():
    ms, bx, by, xs, ys = hand({(2, 3): 4, (0, 0): 3})
    ms[-3:] = 0.0   # the three events at (0, 0) were never scored: their best is the reset state's (0, 0)
    _, props, info, H, _ = pr.propose(ms, bx, by, xs, ys, radius=0, suppress=0, max_models=4)
    _, mprops, minfo, mH, _ = pr.propose(ms, bx, by, xs, ys, radius=0, suppress=0, max_models=4, mutate="count_unscored")
    assert (info["voted"], info["unscored"], H[0, 0]) == (4, 3, 0) and len(props) == 1
    assert (minfo["voted"], minfo["unscored"], mH[0, 0]) == (7, 0, 3) and len(mprops) == 2


# ---- (d) hand-made states ----

def test_a_peak_in_a_lattice_corner_is_padded_with_zeros():
    for corner in ((0, 0), (0, 6), (5, 0), (5, 6)):
        _, props, _, H, B = pr.propose(*hand({corner: 9}), radius=2, suppress=64, max_models=3)
        assert B.sum() == 9 * 9 and (B > 0).sum() == 9 and B[corner] == 9 and H[corner] == 9
        # B is 9 on the 3 x 3 points the lattice has within 2 steps of the corner: the pick is the one with the lowest index
        lowest = max(0, corner[0] - 2) * 7 + max(0, corner[1] - 2)
        assert [(p["index"], p["votes"]) for p in props] == [(lowest, 9)]


def test_two_equal_peaks_come_in_index_order():
    _, props, _, _, _ = pr.propose(*hand({(3, 2): 6, (0, 4): 6}), radius=0, suppress=0, max_models=8)
    assert [(p["index"], p["votes"]) for p in props] == [(4, 6), (23, 6)]


def test_a_best_off_the_lattice_does_not_vote():
    ms, bx, by, xs, ys = hand({(2, 2): 3, (1, 1): 2})
    bx[-1] = 1.5                        # between two lattice values
    by[-2] = np.nextafter(1.0, 2.0)     # one ulp off
    _, props, info, H, _ = pr.propose(ms, bx, by, xs, ys, radius=0, suppress=0, max_models=8)
    assert (info["voted"], info["off_lattice"], info["unscored"]) == (3, 2, 0) and H.sum() == 3 and len(props) == 1


def test_min_votes_cuts_the_list():
    st = hand({(0, 0): 9, (2, 3): 5, (5, 6): 2})
    assert [p["votes"] for p in pr.propose(*st, radius=0, suppress=0, max_models=8, min_votes=1)[1]] == [9, 5, 2]
    assert [p["votes"] for p in pr.propose(*st, radius=0, suppress=0, max_models=8, min_votes=5)[1]] == [9, 5]
    assert pr.propose(*st, radius=0, suppress=0, max_models=8, min_votes=10)[1] == []


def test_max_models_1_and_64():
    st = hand({(i, j): 1 + i + 6 * j for i in range(6) for j in range(7)})
    assert [p["index"] for p in pr.propose(*st, radius=0, suppress=0, max_models=1)[1]] == [5 * 7 + 6]
    props = pr.propose(*st, radius=0, suppress=0, max_models=64)[1]
    assert len(props) == 42 and [p["votes"] for p in props] == sorted((1 + i + 6 * j for i in range(6) for j in range(7)), reverse=True)


def test_everything_unscored_gives_no_proposal():
    ms, bx, by, xs, ys = hand({(1, 1): 4})
    models, props, info, H, B = pr.propose(np.zeros(4), bx, by, xs, ys)
    assert models == [] and props == [] and not H.any() and not B.any()
    assert info == dict(voted=0, unscored=4, off_lattice=0, n_x=6, n_y=7, proposals=0)


def test_the_model_compensates_the_proposed_flow():
    models, props, _, _, _ = pr.propose(*hand({(2, 3): 4}), radius=0, suppress=0, max_models=1)
    m = models[0]
    assert (m.total_dx, m.total_dy) == (-2.0, -3.0) and (m.cx, m.cy, m.dx, m.dy, m.rot, m.div, m.total_rot, m.total_div) == (0,) * 8
    assert (props[0]["u"], props[0]["v"]) == gref.compute_uv(2.0, 3.0)


# ---- (e) bf::ModelProposer::propose_from_best against the restatement ----

def build_program(out_dir, sanitize):
    exe = os.path.join(out_dir, "test_propose" + ("_san" if sanitize else ""))
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra"] + (SAN if sanitize else []) + [
        "-I" + os.path.join(ROOT, "better_flow_amd", "host"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_propose.cpp"), "-lm", "-o", exe])
    return exe


def program_case(exe, tmp, name, ms, bx, by, lattice, opts):
    """One run of the program; lattice (x_low, x_hi, x_step, y_low, y_hi, y_step, nz), opts (radius, suppress, K, min_votes)."""
    inp, prefix = os.path.join(tmp, name + ".bin"), os.path.join(tmp, name + "_")
    with open(inp, "wb") as f:
        f.write(np.array([len(ms)], dtype=np.int64).tobytes() + np.array(lattice, dtype=np.float64).tobytes() +
                np.array(list(opts) + [0] * 4, dtype=np.int32).tobytes())
        for a in (ms, bx, by):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([exe, inp, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode()[-3000:])
    assert r.stdout.decode().splitlines()[0] == "device entry absent"
    xs, ys = gref.sweep_values(lattice[0], lattice[1], lattice[2]), gref.sweep_values(lattice[3], lattice[4], lattice[5])
    models, props, info, H, B = pr.propose(ms, bx, by, xs, ys, lattice[6], *opts)
    read = lambda suffix: open(prefix + suffix, "rb").read()
    assert read("H.u32") == H.tobytes() and read("B.u32") == B.tobytes(), name
    assert read("proposals.bin") == pr.flat_proposals(props).tobytes(), name
    exp_info = np.array([info["n_x"], info["n_y"]], dtype=np.int64).tobytes() + \
        np.array([info[k] for k in ("voted", "unscored", "off_lattice", "proposals")], dtype=np.int32).tobytes()
    assert read("info.bin") == exp_info, name
    from better_flow_amd import accel
    raw, sz = read("models.bin"), ctypes.sizeof(accel.Model)
    assert len(raw) == sz * len(models)
    values = lambda m: np.array([getattr(m, k) for k, _ in type(models[0])._fields_ if not k.startswith("_")], dtype=np.float64).tobytes()
    for k, m in enumerate(models):
        assert values(accel.Model.from_buffer_copy(raw[k * sz:(k + 1) * sz])) == values(m), (name, k)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_model_proposer_host_path_equals_the_restatement(state, tmp_path, sanitize):
    exe = build_program(str(tmp_path), sanitize)
    g, _ = state
    lat = (-0.72, 0.72, 0.04, -0.72, 0.72, 0.04, 127.0)
    for name, opts in (("table", (1, 2, 4, 1)), ("r0", (0, 0, 64, 1)), ("r8", (8, 64, 64, 1)), ("cut", (1, 2, 8, 700))):
        program_case(exe, str(tmp_path), name, g.max_score, g.best_nx, g.best_ny, lat, opts)
    ms, bx, by, _, _ = hand({(0, 0): 9, (5, 6): 9, (2, 3): 1, (1, 1): 2})
    ms[-1] = 0.0
    bx[-2] = 0.25
    by[0] = float("nan")
    program_case(exe, str(tmp_path), "hand", ms, bx, by, (0.0, 6.0, 1.0, 0.0, 7.0, 1.0, 127.0), (2, 1, 8, 1))
    program_case(exe, str(tmp_path), "empty", np.zeros(0), np.zeros(0), np.zeros(0), lat, (1, 2, 8, 1))


# ---- (f) the command line on the oracle-backed build ----

@pytest.fixture(scope="module")
def oracle_cli():
    sys.path.insert(0, os.path.join(ROOT, "tests", "shim"))
    import build as shim_build
    return shim_build.build()


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    from better_flow_amd import synth
    d = tmp_path_factory.mktemp("objects_cli")
    txt = str(d / "ev.txt")
    synth.write_txt(txt, synth.make_slice(3000, 64, 64, 0.03, seed=5))
    return txt


def test_cli_help_lists_the_flags(oracle_cli, tmp_path):
    out = subprocess.run([oracle_cli, "--help"], cwd=str(tmp_path), stdout=subprocess.PIPE, timeout=60).stdout.decode()
    for flag in ("--objects=<K>", "--objects-range=", "--objects-step=", "--objects-radius=", "--objects-suppress=",
                 "--objects-min-votes=", "--objects-scale="):
        assert flag in out, flag


def test_cli_objects_on_a_library_without_the_entries_names_the_entry(oracle_cli, recording, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([oracle_cli, "--objects=2", "--quiet", "--img-prefix", str(out), recording], cwd=str(out),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"bf_propose_models" in r.stderr, (r.returncode, r.stderr[-500:])
    assert os.listdir(str(out)) == []


@pytest.mark.parametrize("args", (["--engine=stream", "--objects=2"], ["--objects=2", "second"], ["--objects=0"], ["--objects=65"],
                                  ["--objects=2", "--objects-scale=2"], ["--objects=2", "--objects-radius=9"],
                                  ["--objects=2", "--objects-step=0"]),
                         ids=("stream", "two_inputs", "zero", "too_many", "even_scale", "radius", "step"))
def test_cli_objects_refusals(oracle_cli, recording, tmp_path, args):
    out = tmp_path / "out"
    out.mkdir()
    args = [recording if a == "second" else a for a in args]
    r = subprocess.run([oracle_cli] + args + ["--quiet", "--img-prefix", str(out), recording], cwd=str(out),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 1 and b"--objects" in r.stderr, (r.returncode, r.stderr[-500:])
    assert os.listdir(str(out)) == []

"""Tracking objects across slices on the CPU: the restatement tests/track_ref.py on the three-slice scene
tests/track_scene.py, the match rule's cases, the warm path on the restatement, and the ABI of bf_track_keep / bf_track_overlap /
bf_track_drop.  No GPU: the device is held to the restatement by tests/test_gpu_track.py.

The scene's bars are conditions, worked out before the device existed: with the events carried back by dt a group puts at least
0.8 of its inside events on its own track's pixels and at most 0.05 on the other's; with dt ignored the patch puts less than 0.2
on its own, and match() does not give it its track."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import project_groups_ref as pr
import segment_scene as scene
import track_ref as tr
import track_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, GUARD, MIN_EVENTS, HARD_CAP = (scene.H, scene.W), (90, 120), 100, 20000


@pytest.fixture(scope="module")
def slices():
    sl, step = track_scene.make()
    assert step == 30_000_000 and len(sl) == 3
    for s in sl:
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return sl


def truth(sl):
    return sl["is_patch"].astype(np.int32), [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity(scene.V_PATCH)]


# ---- (a) ABI ----

def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    from better_flow_amd import accel
    mirrors = {"bf_track_opts": accel.TrackOpts, "bf_track_info": accel.TrackInfo}
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
    assert [ctypes.sizeof(m) for m in mirrors.values()] == [32, 32]


def test_symbols_exported_and_bound():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    for name in ("bf_track_keep", "bf_track_overlap", "bf_track_drop"):
        assert name in accel.EXPORTS and hasattr(lib, name), name
    for name in ("track_keep", "track_overlap", "track_drop", "tracks_held"):
        assert hasattr(accel.Accel, name), name
    out = (ctypes.c_int32 * 16)()
    assert lib.bf_abi_struct_sizes(out, 16) == 10   # (its ten entries stay)
    assert lib.bf_track_drop(None) == accel.BF_ERR_ARG and lib.bf_track_keep(None, None, None, 0, None, None) == accel.BF_ERR_ARG


# ---- (b) the scene: where a group's events land on the previous slice's owner plane ----

def shares(table, inside):
    return [[table[k, j] / max(int(inside[k]), 1) for j in range(table.shape[1])] for k in range(table.shape[0])]


@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("pair", [(0, 1), (1, 2)])
def test_with_dt_a_group_lands_on_its_own_track(slices, scale, pair):
    prev, new = slices[pair[0]], slices[pair[1]]
    ids_p, ms = truth(prev)
    ids_n, _ = truth(new)
    plane, _, Kp = tr.keep(prev, ids_p, ms, scale, RES)
    table, inside, info = tr.overlap(new, ids_n, ms, plane, Kp, track_scene.STEP_NS, scale, RES)
    print("scale %d, slices %d->%d: background %s, patch %s, info %s" % (scale, pair[0], pair[1], table[0].tolist(), table[1].tolist(), info))
    s = shares(table, inside)
    assert inside.tolist() == table.sum(axis=1).tolist() and inside.sum() + info["outside"] + info["unassigned"] == len(new["t"])
    for k in range(2):
        assert s[k][k] >= 0.8, (k, s[k])
        assert s[k][1 - k] <= 0.05, (k, s[k])
    assert tr.match(table, inside) == [0, 1]


def test_without_dt_the_patch_loses_its_track(slices):
    prev, new = slices[0], slices[1]
    ids_p, ms = truth(prev)
    ids_n, _ = truth(new)
    plane, _, Kp = tr.keep(prev, ids_p, ms, 3, RES)
    table, inside, _ = tr.overlap(new, ids_n, ms, plane, Kp, track_scene.STEP_NS, 3, RES, mutate="no_dt")
    zero, _, _ = tr.overlap(new, ids_n, ms, plane, Kp, 0, 3, RES)
    assert table.tobytes() == zero.tobytes()   # (the mutation is dt = 0)
    print("no dt: background %s, patch %s" % (table[0].tolist(), table[1].tolist()))
    assert table[1, 1] / inside[1] < 0.2
    assert tr.match(table, inside)[1] != 1


def test_swapped_groups_swap_the_rows_and_keep_the_track_ids(slices):
    prev, new = slices[0], slices[1]
    ids_p, ms = truth(prev)
    ids_n, _ = truth(new)
    plane, _, Kp = tr.keep(prev, ids_p, ms, 3, RES)
    table, inside, info = tr.overlap(new, ids_n, ms, plane, Kp, track_scene.STEP_NS, 3, RES)
    t2, i2, info2 = tr.overlap(new, 1 - ids_n, ms[::-1], plane, Kp, track_scene.STEP_NS, 3, RES)
    assert t2.tobytes() == table[::-1].tobytes() and i2.tolist() == inside[::-1].tolist() and info2 == info
    a, _, _ = tr.track_ids(tr.match(table, inside), [7, 9], 10)
    b, _, _ = tr.track_ids(tr.match(t2, i2), [7, 9], 10)
    assert a == [7, 9] and b == [9, 7]


# ---- (c) match(): the rule's cases (tests/cpp/test_track_match.cpp walks the same list on the host's function) ----

MATCH_CASES = [
    # (name, table [K][Kp + 1], inside or None for the rows' sums, num, den, expected)
    ("diagonal", [[90, 2, 8], [1, 95, 4]], None, 1, 2, [0, 1]),
    ("tie goes to the smallest k, then the smallest j", [[50, 50, 0], [50, 50, 0]], None, 1, 2, [0, 1]),
    ("just below the threshold", [[49, 0, 51]], None, 1, 2, [-1]),
    ("exactly at the threshold", [[50, 0, 50]], None, 1, 2, [0]),
    ("more groups than tracks", [[10, 0], [80, 20], [30, 0]], None, 1, 2, [-1, 0, -1]),
    ("more tracks than groups", [[5, 60, 20, 15]], None, 1, 2, [1]),
    ("an all-zero row", [[0, 0, 0], [0, 10, 0]], None, 1, 2, [-1, 1]),
    ("no kept group", [[12], [0]], None, 1, 2, [-1, -1]),
    ("the largest fails: nothing smaller is tried", [[40, 0, 60], [0, 30, 0]], None, 1, 2, [-1, -1]),
    ("a taken track is not given twice", [[90, 0, 10], [60, 30, 10]], None, 1, 2, [0, -1]),
    ("another threshold", [[30, 0, 70]], None, 3, 10, [0]),
]


@pytest.mark.parametrize("case", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_match_cases(case):
    _, table, inside, num, den, want = case
    table = np.array(table, dtype=np.int64)
    inside = table.sum(axis=1) if inside is None else np.array(inside)
    assert tr.match(table, inside, num, den) == want


def test_match_ties_up_is_a_different_rule():
    table = np.array([[50, 50, 0], [50, 50, 0], [50, 50, 0]])
    assert tr.match(table, table.sum(axis=1)) == [0, 1, -1]
    assert tr.match(table, table.sum(axis=1), mutate="ties_up") == [-1, 0, 1]


def test_track_ids_inherit_start_and_end():
    ids, ended, nxt = tr.track_ids([-1, 0, -1], [4], 5)
    assert (ids, ended, nxt) == ([5, 4, 6], [], 7)
    ids, ended, nxt = tr.track_ids([1], [4, 5, 6], 7)
    assert (ids, ended, nxt) == ([5], [4, 6], 7)


# ---- (d) the warm path on the restatement: slice N's fitted models are slice N + 1's candidates ----

_WARM = []


def warm_chain(slices):
    """assign_ref.alternate on every slice, slice 0 from the two true models, slice N + 1 from slice N's fitted models (no
    search); after every slice the overlap against the previous slice's kept plane and match().  Computed once."""
    if not _WARM:
        models = truth(slices[0])[1]
        out, kept, track, next_id = [], None, None, 0
        for s, sl in enumerate(slices):
            models, gid, _ = ar.alternate(sl, models, 3, RES, GUARD, MIN_EVENTS, HARD_CAP, rounds_per_fit=2, max_alternations=5)
            if kept is None:
                track, next_id = [0, 1], 2
                table = inside = None
            else:
                table, inside, _ = tr.overlap(sl, gid, models, kept[0], kept[1], track_scene.STEP_NS, 3, RES)
                track, _, next_id = tr.track_ids(tr.match(table, inside), track, next_id)
            plane, _, Kp = tr.keep(sl, gid, models, 3, RES)
            kept = (plane, Kp)
            res, _, _, u, v = gr.solve(sl, gid, 2, 3, RES, GUARD, MIN_EVENTS, warm=list(models), hard_cap=HARD_CAP)
            flows = [gr.median_flow(u, v, r.idx) if r.events else (0.0, 0.0) for r in res]
            out.append(dict(gid=gid, models=list(models), track=list(track), table=table, inside=inside, flows=flows,
                            recall=ar.recall_purity(sl, gid)))
        _WARM.append(out)
    return _WARM[0]


def test_warm_alternation_keeps_both_identities_over_three_slices(slices):
    chain = warm_chain(slices)
    for s, c in enumerate(chain):
        print("slice %d: tracks %s, recall (patch, background) %.4f %.4f, flows %s, table %s" %
              (s, c["track"], c["recall"][0], c["recall"][1], [tuple(round(x, 2) for x in f) for f in c["flows"]],
               None if c["table"] is None else c["table"].tolist()))
    assert [c["track"] for c in chain] == [[0, 1]] * 3
    # the identities are the objects', not only the indices': in every slice the group of track 1 holds the majority of the
    # patch's events and the group of track 0 the majority of the background's (a track IS the object it holds most of)
    for c in chain:
        assert c["recall"][0] > 0.5 and c["recall"][1] > 0.5, c["recall"]

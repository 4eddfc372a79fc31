"""The entries on the K models' vote planes share their scratch through one set of host helpers (csrc/bf_assign_abi.cpp,
bf_vote_planes.h): the vote and box planes, the staged warps, the projection's base pass and its result block serve
bf_assign_groups, bf_project_groups, bf_merge_scores, bf_track_keep, bf_track_overlap and bf_hold_groups alike.  So on ONE
context the calls are run in two different orders, and every output of every call -- planes, tables, scores, infos, the held
flow -- must equal in bytes the same call on a FRESH context that ran only that call (bf_track_overlap: after its bf_track_keep).
That covers the kept plane too: bf_project_groups and bf_merge_scores run between a keep and the overlap that reads it.

Bar.  Every output is integers after an event's pixel, or doubles computed per event from the event and its model alone: nothing
depends on what ran before, so every comparison is EQUALITY of bytes, no tolerance."""
import numpy as np
import pytest

from test_gpu_groups import to_accel
from test_gpu_track import random_slice, small_models

pytestmark = pytest.mark.gpu

RES, N, K = (33, 65), 3000, 3
DT = 2_000_000
SETTINGS = [(3, 2), (1, 0)]   # (scale, margin)
FIRST = ("keep", "project", "merge", "assign", "overlap", "hold", "project")
SECOND = ("hold", "project", "keep", "merge", "assign", "project", "overlap")


def make_acc(accel_mod):
    return accel_mod.Accel(device=0, max_events=N, max_rows=512, max_cols=1024)


def load(a, sl, ids):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    a.global_set_window(1, 5)   # (bf_hold_groups needs the search's window on the slice)
    a.set_groups(ids, K)


def arrays(*xs):
    return b"".join(x.tobytes() for x in xs)


def call(a, name, ms, scale, margin):
    """One entry's every output as bytes."""
    if name == "keep":
        plane, info = a.track_keep(ms, scale, RES, margin=margin)
        return plane.tobytes() + bytes(info)
    if name == "project":
        img, scores, info = a.project_groups(ms, scale, RES, margin=margin)
        return arrays(img["count"], img["label"], img["bgr"]) + b"".join(bytes(s) for s in scores) + bytes(info)
    if name == "merge":
        gain, inside, events, info = a.merge_scores(ms, scale, RES, margin=margin)
        return arrays(gain, inside, events) + bytes(info)
    if name == "assign":
        gid, score, counts, info = a.assign_groups(ms, scale, RES, margin=margin, install=False)
        return arrays(gid, score, counts) + bytes(info)
    if name == "overlap":
        table, inside, info = a.track_overlap(ms, DT, scale, RES, margin=margin)
        return arrays(table, inside) + bytes(info)
    assert name == "hold"
    a.hold_groups(ms)
    return arrays(*a.global_get_flow().values())


@pytest.fixture(scope="module")
def case(accel_mod):
    """The slice, its ids (some -1), the models, and per setting every call's bytes on a context of its own."""
    sl = random_slice(41, N, RES)
    ids = ((np.arange(N) * 7) % (K + 1) - 1).astype(np.int32)
    ms = to_accel(accel_mod, small_models(K))   # rotation and divergence
    alone = {}
    for scale, margin in SETTINGS:
        for name in sorted(set(FIRST)):
            a = make_acc(accel_mod)
            try:
                load(a, sl, ids)
                if name == "overlap":
                    a.track_keep(ms, scale, RES, margin=margin, want_plane=False)
                alone[scale, margin, name] = call(a, name, ms, scale, margin)
            finally:
                a.close()
    assert (ids == -1).any()
    for s in SETTINGS:   # (no two calls of a setting give the same bytes; the held flow alone does not depend on the setting)
        assert len({alone[s + (name,)] for name in set(FIRST)}) == len(set(FIRST))
    assert all(alone[SETTINGS[0] + (name,)] != alone[SETTINGS[1] + (name,)] for name in set(FIRST) - {"hold"})
    return sl, ids, ms, alone


@pytest.mark.parametrize("scale,margin", SETTINGS)
def test_every_call_in_two_orders_on_one_context_equals_the_call_alone(accel_mod, case, scale, margin):
    sl, ids, ms, alone = case
    a = make_acc(accel_mod)
    try:
        load(a, sl, ids)
        for order in (FIRST, SECOND):
            for step, name in enumerate(order):
                got = call(a, name, ms, scale, margin)
                assert got == alone[scale, margin, name], (order, step, name)
    finally:
        a.close()

"""bf_merge_scores on the MI355X (csrc/bf_merge.hip: k_merge_total, k_merge_vote, k_merge_gain; the base planes and the box sum of
bf_project.hip and bf_assign.hip) against tests/merge_ref.py, the numpy restatement.

Bar.  After an event's pixel the operator is integer counts and sums, and the pixel is bf_assign_groups' own
(tests/test_gpu_assign.py holds it to the restatement): every comparison is EQUALITY of the gains, the inside counts, the event
counts and the info, no tolerance.  The end-to-end case is teacher-forced -- the device's own ids and models go into the
restatement at every step of the loop -- and ends at the bars of tests/test_merge_cpu.py: two objects, recall >= 0.99, the
patch's flow within 5 px/s."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import merge_ref as mr
import project_groups_ref as pr
import segment_scene as scene
from test_gpu_groups import fields, seeded_models, to_accel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = scene.H, scene.W
GUARD, MIN_EVENTS, HARD_CAP = (90, 120), 100, 20000


@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def four(sc):
    """The four groups of DESIGN section 18's table: (models, ids) from the restatement, computed once."""
    import test_merge_cpu as cpu
    return cpu.four_groups_state(sc)


@pytest.fixture(scope="module")
def truth(sc):
    ids, ms = pr.scene_truth(sc)
    ids.setflags(write=False)
    return ids, ms


@pytest.fixture(scope="module")
def acc(accel_mod, sc):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    yield a
    a.close()


def upload(a, sl):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])


def info_dict(info):
    return {k: getattr(info, k) for k in mr.INFO_FIELDS}


def same(dev, ref, what):
    gain, inside, events, info = dev
    print("%s: info %s" % (what, info_dict(info)))
    assert info_dict(info) == ref["info"], (what, info_dict(info), ref["info"])
    assert events.dtype == np.int32 and events.tolist() == ref["events"].tolist(), (what, events.tolist(), ref["events"].tolist())
    assert inside.dtype == np.int32 and inside.shape == ref["inside"].shape
    bad = np.argwhere(inside != ref["inside"])
    assert bad.size == 0, (what, "inside", bad[:4].tolist(), [(int(inside[tuple(b)]), int(ref["inside"][tuple(b)])) for b in bad[:4]])
    assert gain.dtype == np.uint64 and gain.shape == ref["gain"].shape
    bad = np.argwhere(gain != ref["gain"])
    assert bad.size == 0, (what, "gain", len(bad), bad[:4].tolist(), [(int(gain[tuple(b)]), int(ref["gain"][tuple(b)])) for b in bad[:4]])
    assert gain.tobytes() == ref["gain"].tobytes() and inside.tobytes() == ref["inside"].tobytes(), what


def dev_bytes(r):
    return r[0].tobytes() + r[1].tobytes() + r[2].tobytes() + bytes(r[3])


_REF = {}


def ref_scores(sl, name, ids, models, scale, sensor_res=(H, W), margin=0, targets_per_pass=0):
    """The restatement of one call, computed once per name and never changed."""
    if name not in _REF:
        r = mr.scores(sl, ids, models, scale, sensor_res, margin, targets_per_pass)
        for k in ("gain", "inside", "events"):
            r[k].setflags(write=False)
        _REF[name] = r
    return _REF[name]


# ---- 1. the scene's four groups: scales, margins ----

@pytest.mark.parametrize("margin", [0, 6])
@pytest.mark.parametrize("scale", [1, 3, 5])
def test_scene_four_groups(accel_mod, sc, four, scale, margin):
    models, ids = four
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=scale * H + scale, max_cols=scale * W + scale)
    try:
        upload(a, sc)
        a.set_groups(ids, 4)
        r = ref_scores(sc, ("four", scale, margin), ids, models, scale, margin=margin)
        same(a.merge_scores(to_accel(accel_mod, models), scale, (H, W), margin=margin), r, "four groups")
        assert r["info"]["rows"] == scale * (H + 2 * margin) and r["info"]["unassigned"] == 13
        if (scale, margin) == (3, 0):   # the table of DESIGN section 18
            assert r["info"]["sum_sq"] == 5883271 and r["gain"][2].tolist() == [278340, 363002, 370624, 374892]
    finally:
        a.close()


# ---- 2. group counts, ids of -1, empty groups, outside ----

def test_one_group(accel_mod, sc, acc):
    upload(acc, sc)
    ids = np.zeros(len(sc["t"]), np.int32)
    ms = [ar.model_of_velocity(scene.V_BACKGROUND)]
    acc.set_groups(ids, 1)
    r = ref_scores(sc, "one", ids, ms, 3)
    dev = acc.merge_scores(to_accel(accel_mod, ms), 3, (H, W))
    same(dev, r, "K = 1")
    assert dev[0].tolist() == [[3135808]] == [[dev[3].sum_sq]]   # gain == [[S]] (DESIGN section 17's table)


def random_slice(n, rows, cols, seed, duration_ns=30_000_000):
    rng = np.random.default_rng(seed)
    return dict(fr_x=rng.integers(0, rows, n).astype(np.int32), fr_y=rng.integers(0, cols, n).astype(np.int32),
                t=np.sort(rng.integers(0, duration_ns, n)).astype(np.int64))


def ids64(n):
    """Ids -1 .. 63 spread over the slice, groups 5 and 40 empty."""
    ids = ((np.arange(n) * 7) % 65 - 1).astype(np.int32)
    ids[(ids == 5) | (ids == 40)] = -1
    return ids


def test_sixty_four_groups_with_rotation_and_divergence_on_33_by_65(accel_mod):
    n = 4000
    sl = random_slice(n, 33, 65, seed=3)
    ids, ms = ids64(n), seeded_models(64)
    a = accel_mod.Accel(device=0, max_events=n, max_rows=512, max_cols=512)
    try:
        upload(a, sl)
        a.set_groups(ids, 64)
        r = mr.scores(sl, ids, ms, 3, (33, 65))
        assert r["info"]["unassigned"] > 0 and r["events"][5] == 0 == r["events"][40] and r["info"]["passes"] == 1
        assert not r["gain"][5].any() and not r["gain"][40].any() and not r["inside"][5].any()   # two empty groups
        assert (r["inside"] < r["events"][:, None]).any() and len(np.unique(r["gain"])) > 500
        same(a.merge_scores(to_accel(accel_mod, ms), 3, (33, 65)), r, "K = 64")
    finally:
        a.close()


@pytest.mark.parametrize("scale", [1, 9])
def test_a_sensor_of_one_pixel(accel_mod, scale):
    sl = random_slice(2000, 1, 1, seed=3)
    ids = (np.arange(2000) % 4 - 1).astype(np.int32)
    ms = [gr.oracle.Model(), ar.model_of_velocity((150.0, -80.0)), ar.model_of_velocity((-90.0, 40.0))]
    a = accel_mod.Accel(device=0, max_events=2000, max_rows=512, max_cols=512)
    try:
        upload(a, sl)
        a.set_groups(ids, 3)
        for margin in (0, 1):
            r = mr.scores(sl, ids, ms, scale, (1, 1), margin)
            # (a sensor of one pixel has wsx = 0: without a margin the window test rejects every event)
            assert (r["info"]["sum"] > 0) == (margin > 0) and r["events"].tolist() == [500, 500, 500]
            same(a.merge_scores(to_accel(accel_mod, ms), scale, (1, 1), margin=margin), r, "1 x 1 at scale %d, margin %d" % (scale, margin))
    finally:
        a.close()


def test_a_model_that_sends_three_quarters_of_a_group_outside(accel_mod, sc, truth, acc):
    upload(acc, sc)
    ids = truth[0]
    ms = [ar.model_of_velocity((5400.0, -4050.0)), ar.model_of_velocity(scene.V_PATCH)]
    acc.set_groups(ids, 2)
    r = ref_scores(sc, "far", ids, ms, 3)
    e, ins = r["events"], r["inside"]
    assert 0.2 * e[0] <= ins[0, 0] <= 0.25 * e[0] and ins[0, 1] > 0.9 * e[0] and ins[1, 0] < ins[1, 1], (e.tolist(), ins.tolist())
    same(acc.merge_scores(to_accel(accel_mod, ms), 3, (H, W)), r, "far model")


# ---- 3. contention, gains beyond 32 bits, many groups on one row ----

def test_70000_events_of_two_groups_on_one_pixel(accel_mod):
    n = 70000
    sl = dict(fr_x=np.full(n, 7, np.int32), fr_y=np.full(n, 9, np.int32), t=(np.arange(n) * 400).astype(np.int64))
    ids = (np.arange(n) % 2).astype(np.int32)
    ms = [gr.oracle.Model()] * 2
    a = accel_mod.Accel(device=0, max_events=n, max_rows=64, max_cols=64)
    try:
        upload(a, sl)
        a.set_groups(ids, 2)
        for scale in (1, 3):
            r = mr.scores(sl, ids, ms, scale, (12, 16))
            half = n // 2
            assert r["info"]["sum_sq"] == scale * scale * n * n > 1 << 32 and int(r["gain"][0, 1]) == scale * scale * 3 * half * half
            assert scale == 1 or int(r["gain"].min()) > 1 << 32   # (3 x 35000^2 = 3.7e9 at scale 1, nine times that at scale 3)
            same(a.merge_scores(to_accel(accel_mod, ms), scale, (12, 16)), r, "pile at scale %d" % scale)
    finally:
        a.close()


def test_3000_events_of_64_groups_on_one_pixel_row(accel_mod):
    n = 3000
    rng = np.random.default_rng(9)
    sl = dict(fr_x=np.full(n, 5, np.int32), fr_y=rng.integers(0, 40, n).astype(np.int32), t=np.sort(rng.integers(0, 1000, n)).astype(np.int64))
    ids = rng.integers(0, 64, n).astype(np.int32)
    ms = [gr.oracle.Model()] * 64   # (t < 1 us: no model moves an event; every group lands on the row)
    a = accel_mod.Accel(device=0, max_events=n, max_rows=64, max_cols=128)
    try:
        upload(a, sl)
        a.set_groups(ids, 64)
        for scale in (1, 3):
            r = mr.scores(sl, ids, ms, scale, (12, 40))
            assert (r["gain"] == r["gain"][:, :1]).all() and r["gain"].all()   # one model: every column is the diagonal
            same(a.merge_scores(to_accel(accel_mod, ms), scale, (12, 40)), r, "one row at scale %d" % scale)
    finally:
        a.close()


# ---- 4. passes, storage order, repeatability, the other entries' buffers, state ----

def ids8(n):
    ids = ((np.arange(n) * 11) % 9 - 1).astype(np.int32)
    return ids


def test_targets_per_pass_changes_the_passes_and_no_byte(accel_mod, sc, acc):
    upload(acc, sc)
    ids, ms = ids8(len(sc["t"])), seeded_models(8)
    acc.set_groups(ids, 8)
    ms8 = to_accel(accel_mod, ms)
    out = {}
    for tpp, passes in ((0, 1), (1, 8), (3, 3)):
        r = ref_scores(sc, ("k8", tpp), ids, ms, 3, targets_per_pass=tpp)
        dev = acc.merge_scores(ms8, 3, (H, W), targets_per_pass=tpp)
        same(dev, r, "targets_per_pass %d" % tpp)
        assert dev[3].passes == passes
        out[tpp] = dev[0].tobytes() + dev[1].tobytes() + dev[2].tobytes()
    assert out[0] == out[1] == out[3]


def test_three_storage_orders_give_the_same_bytes_and_two_runs_agree(accel_mod, sc, four, acc):
    models, ids = four
    ms4, ms64, i64 = to_accel(accel_mod, models), to_accel(accel_mod, seeded_models(64)), ids64(len(sc["t"]))

    def calls():
        acc.set_groups(ids, 4)
        out = [acc.merge_scores(ms4, 3, (H, W)), acc.merge_scores(ms4, 3, (H, W)), acc.merge_scores(ms4, 1, (H, W), margin=6)]
        acc.set_groups(i64, 64)
        out.append(acc.merge_scores(ms64, 1, (H, W), targets_per_pass=24))
        return [dev_bytes(r) for r in out]

    upload(acc, sc)
    plain = calls()
    assert plain[0] == plain[1], "two runs of one call"
    upload(acc, sc)
    acc.run_tiles(4, 4, 3, (H, W), (30, 40), MIN_EVENTS)   # (the events are now stored sorted by tile, with a permutation)
    assert calls() == plain
    upload(acc, sc)
    acc.set_groups(gr.scene_groups(sc), 4)
    acc.run_groups(4, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)   # (... sorted by group)
    assert calls() == plain
    acc.set_groups(ids, 4)
    same(acc.merge_scores(ms4, 3, (H, W)), ref_scores(sc, ("four", 3, 0), ids, models, 3), "sorted storage")


def test_alternating_with_assign_and_project_on_one_context(accel_mod, sc, truth, acc):
    ids, ms = truth
    ms2 = to_accel(accel_mod, ms)
    assign_bytes = lambda r: r[0].tobytes() + r[1].tobytes() + r[2].tobytes() + bytes(r[3])
    project_bytes = lambda r: r[0]["count"].tobytes() + r[0]["label"].tobytes() + r[0]["bgr"].tobytes() + b"".join(bytes(s) for s in r[1]) + bytes(r[2])
    alone = []
    for call, to_bytes in ((lambda s: acc.merge_scores(ms2, s, (H, W)), dev_bytes),
                           (lambda s: acc.assign_groups(ms2, s, (H, W), use_prior=True, install=False), assign_bytes),
                           (lambda s: acc.project_groups(ms2, s, (H, W)), project_bytes)):
        upload(acc, sc)
        acc.set_groups(ids, 2)
        alone.append([to_bytes(call(s)) for s in (3, 1)])
    upload(acc, sc)
    acc.set_groups(ids, 2)
    for _ in range(2):
        for i, s in enumerate((3, 1)):
            assert assign_bytes(acc.assign_groups(ms2, s, (H, W), use_prior=True, install=False)) == alone[1][i]
            assert dev_bytes(acc.merge_scores(ms2, s, (H, W))) == alone[0][i]
            assert project_bytes(acc.project_groups(ms2, s, (H, W))) == alone[2][i]


def test_the_slices_state_is_untouched(accel_mod, sc, truth, acc):
    ids, ms = truth
    lattice = accel_mod.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)

    def sequence(merge):
        upload(acc, sc)
        acc.set_cloud(scene.SCALE, H, W)
        nx, ny = scene.flow_of(scene.V_BACKGROUND)
        acc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
        acc.segment(**scene.OPTS)
        acc.set_groups(gr.scene_groups(sc), 4)
        acc.global_set_window(1, 5)
        acc.global_search(lattice, want_surface=False)
        acc.global_hold_best()

        def state():
            lab, comps, cl = acc.segment_get()
            return lab.tobytes() + comps.tobytes() + cl.tobytes() + b"".join(x.tobytes() for x in acc.writeout_events()) + \
                b"".join(v.tobytes() for v in acc.global_get_events().values()) + \
                b"".join(v.tobytes() for v in acc.global_get_flow().values()) + b"".join(x.tobytes() for x in acc.get_time_img())

        before = state()
        if merge:
            four_models = to_accel(accel_mod, [ms[1], ms[0], ms[0], ms[0]])
            acc.merge_scores(four_models, 3, (H, W), margin=6)
            acc.merge_scores(four_models, 1, (H, W), targets_per_pass=2)
            assert state() == before
        # the held grouping: the grouped solve gives what it gives without the merge scores
        m, i, q = acc.run_groups(4, 3, (H, W), (30, 40), MIN_EVENTS, hard_iter_cap=HARD_CAP)
        return before + b"".join(fields(x) for x in m) + b"".join(fields(x) for x in i) + b"".join(fields(x) for x in q)

    assert sequence(True) == sequence(False)


# ---- 5. errors, zero events ----

def test_every_error_code(accel_mod, sc, truth):
    A = accel_mod
    ids, ms = truth
    a = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    ms = to_accel(A, ms)

    def code(fn):
        with pytest.raises(A.BfError) as e:
            fn()
        return e.value.code

    try:
        assert code(lambda: a.merge_scores(ms, 3, (H, W))) == A.BF_ERR_STATE                     # before an upload
        upload(a, sc)
        assert code(lambda: a.merge_scores(ms, 3, (H, W))) == A.BF_ERR_STATE                     # no grouping held
        a.set_groups(ids, 2)
        for kw in (dict(scale=2), dict(scale=11), dict(margin=-1), dict(margin=65537), dict(targets_per_pass=-1), dict(sensor_res=(0, W)),
                   dict(sensor_res=(H, 65537))):
            args = dict(scale=3, sensor_res=(H, W))
            args.update(kw)
            assert code(lambda: a.merge_scores(ms, **args)) == A.BF_ERR_ARG, kw
        assert code(lambda: a.merge_scores([], 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.merge_scores([ms[0]] * 65, 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.merge_scores([ms[0]] * 3, 3, (H, W))) == A.BF_ERR_ARG              # the grouping has K = 2
        o = A.MergeOpts(3, H, W, 0, 0)
        assert a.L.bf_merge_scores(a.h, ctypes.byref(o), None, 2, None, None, None, None) == A.BF_ERR_ARG   # NULL models
        assert a.L.bf_merge_scores(a.h, None, (A.Model * 2)(*ms), 2, None, None, None, None) == A.BF_ERR_ARG   # NULL opts
        assert a.L.bf_merge_scores(None, None, None, 0, None, None, None, None) == A.BF_ERR_ARG
        a.set_groups(np.zeros(len(sc["t"]), np.int32), 64)
        assert code(lambda: a.merge_scores([ms[0]] * 64, 9, (1000, 1000))) == A.BF_ERR_CAPACITY   # 64 x 9000 x 9000 words
        # every output NULL is a valid call
        a.set_groups(ids, 2)
        assert a.L.bf_merge_scores(a.h, ctypes.byref(o), (A.Model * 2)(*ms), 2, None, None, None, None) == A.BF_OK
        a.upload_events(sc["fr_x"], sc["fr_y"], sc["t"], noise=np.zeros(len(sc["t"]), np.uint8))
        a.set_groups(ids, 2)
        assert code(lambda: a.merge_scores(ms, 3, (H, W))) == A.BF_ERR_ARG                       # a noise mask
    finally:
        a.close()


def test_zero_events(accel_mod, truth):
    a = accel_mod.Accel(device=0, max_events=16, max_rows=64, max_cols=64)
    try:
        a.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        a.set_groups(np.zeros(0, np.int32), 2)
        dev = a.merge_scores(to_accel(accel_mod, truth[1]), 3, (12, 16))
        empty = dict(fr_x=np.zeros(0, np.int32), fr_y=np.zeros(0, np.int32), t=np.zeros(0, np.int64))
        same(dev, mr.scores(empty, np.zeros(0, np.int32), truth[1], 3, (12, 16)), "zero events")
        assert not dev[0].any() and not dev[1].any() and not dev[2].any() and not any(info_dict(dev[3]).values())
    finally:
        a.close()


# ---- 6. the identity against the device's own projection ----

def test_gain_is_the_change_of_the_devices_own_objective(accel_mod, sc, four, acc):
    """For all pairs at K = 4: S - gain[b][b] + gain[b][a] is bf_project_groups' sum_sq with models[b] replaced by models[a]."""
    models, ids = four
    ms = to_accel(accel_mod, models)
    upload(acc, sc)
    acc.set_groups(ids, 4)
    gain, _, _, info = acc.merge_scores(ms, 3, (H, W))
    S = info.sum_sq
    assert acc.project_groups(ms, 3, (H, W), want=())[2].sum_sq == S
    for b in range(4):
        for a in range(4):
            swapped = list(ms)
            swapped[b] = ms[a]
            after = acc.project_groups(swapped, 3, (H, W), want=())[2].sum_sq
            assert S - int(gain[b, b]) + int(gain[b, a]) == after, (b, a)


# ---- 7. end to end: search, proposals, alternation, the merge-down loop ----

@pytest.fixture(scope="module")
def device_reduction(accel_mod, sc, acc):
    """search + propose_models(max_models=4) + the alternation of DESIGN section 15 + merge_ref.reduce driven by the device:
    every assignment and every score teacher-forced against the restatement.  -> (models, ids, steps, last scores)."""
    from test_gpu_assign import refit
    from test_gpu_assign import same as same_assign
    A = accel_mod
    helper = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        upload(acc, sc)
        acc.global_set_window(1, 5)
        o = A.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)
        acc.global_search(o, want_surface=False)
        models, _, _ = acc.propose_models(o, max_models=4)
        assert len(models) == 4
        upload(acc, sc)
        prior = None
        for alt in range(5):
            changed = None
            for _ in range(2):
                dev = acc.assign_groups(models, 3, (H, W), use_prior=prior is not None)
                changed = dev[3].changed if changed is None else changed
                prior = dev[0]
            if alt > 0 and changed == 0:
                break
            models, _, _ = refit(A, acc, helper, sc, prior, models)
        print("after the alternation: counts %s" % np.bincount(prior[prior >= 0], minlength=4).tolist())

        def alternation(ms, ids):
            ms = to_accel(A, list(ms))
            upload(acc, sc)
            acc.set_groups(ids, len(ms))
            for _ in range(2):
                dev = acc.assign_groups(ms, 3, (H, W), use_prior=True)
                same_assign(dev, ar.assign(sc, ms, 3, (H, W), prior=ids), "the loop's assignment")   # teacher-forced
                ids = dev[0]
            ms, _, _ = refit(A, acc, helper, sc, ids, ms)
            return ms, ids

        def score(ids, ms):
            upload(acc, sc)
            acc.set_groups(ids, len(ms))
            dev = acc.merge_scores(to_accel(A, list(ms)), 3, (H, W))
            ref = mr.scores(sc, ids, ms, 3, (H, W))
            same(dev, ref, "the loop's scores at K = %d" % len(ms))   # teacher-forced
            print(np.round(mr.ratios(ref["gain"]), 4))
            return ref

        return mr.reduce(sc, models, prior, 3, (H, W), GUARD, MIN_EVENTS, HARD_CAP, 9, 10, dissolve_below=MIN_EVENTS,
                         alternation=alternation, score=score)
    finally:
        helper.close()


def test_end_to_end_reduces_four_proposals_to_two_objects(accel_mod, sc, acc, device_reduction):
    from test_gpu_assign import refit
    models, ids, steps, last = device_reduction
    print(steps, last["info"])
    assert len(models) == 2 and last["info"]["models"] == 2 and steps and steps[-1]["K_after"] == 2
    assert any(s["kind"] == "merge" for s in steps)
    rec, _ = ar.recall_purity(sc, ids)
    helper = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        upload(acc, sc)
        acc.set_groups(ids, 2)
        _, _, flows = refit(accel_mod, acc, helper, sc, ids, to_accel(accel_mod, list(models)))
    finally:
        helper.close()
    print("recall %.4f, flows %s" % (rec, flows))
    assert rec >= 0.99
    assert abs(flows[1][0] - scene.V_PATCH[0]) <= 5.0 and abs(flows[1][1] - scene.V_PATCH[1]) <= 5.0, flows
    p = mr.pick(last["gain"], last["events"], 9, 10)
    assert p is not None and not p[2]


# ---- 8. bf::ObjectMerger, bf::ObjectFinder and the command line ----

def build_program(tmp_path):
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_object_merge")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_object_merge.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_object_merger_and_finder_on_the_device(accel_mod, sc, four, device_reduction, tmp_path):
    """tests/cpp/test_object_merge.cpp linked against the product library: scores() takes bf_merge_scores and leaves the
    restatement's bytes; bf::ObjectFinder with merge_num = 9 takes the same steps and leaves the same ids and models as the loop
    through Accel above."""
    import test_merge_cpu as cpu
    exe = build_program(tmp_path)
    models, ids = four
    cpu.program_case(exe, tmp_path, "scene", sc, ids, models, 3, (H, W), margin=6, expect_path="device")
    empty = dict(fr_x=np.zeros(0, np.int32), fr_y=np.zeros(0, np.int32), t=np.zeros(0, np.int64))
    cpu.program_case(exe, tmp_path, "zero", empty, np.zeros(0, np.int32), models[:2], 3, (12, 16), expect_path="device")
    ev, prefix = str(tmp_path / "events.txt"), str(tmp_path / "find_")
    with open(ev, "w") as f:
        for a, b, c in zip(sc["fr_x"].tolist(), sc["fr_y"].tolist(), sc["t"].tolist()):
            f.write("%d %d %d\n" % (a, b, c))
    r = subprocess.run([exe, "find", ev, "4", str(H), str(W), str(GUARD[0]), str(GUARD[1]), str(MIN_EVENTS), str(HARD_CAP), "9", "10",
                        str(MIN_EVENTS), prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    dmodels, dids, steps, last = device_reduction
    lines = open(prefix + "steps.txt").read().splitlines()
    print("\n".join(lines))
    want = ["%s %d %d %d %d %d %d" % (s["kind"], s["b"], s["a"], s["gain_ba"], s["gain_bb"], s["events_b"], s["K_after"]) for s in steps]
    assert lines == want + ["info %d %d" % (len(dmodels), last["info"]["sum_sq"])]
    assert np.fromfile(prefix + "gid.i32", dtype=np.int32).tobytes() == np.asarray(dids, np.int32).tobytes()
    counts = np.fromfile(prefix + "counts.i32", dtype=np.int32)
    assert counts.tolist() == last["events"].tolist() + [last["info"]["unassigned"]]
    raw = open(prefix + "models.bin", "rb").read()
    sz = ctypes.sizeof(accel_mod.Model)
    assert len(raw) == len(dmodels) * sz
    for k, m in enumerate(to_accel(accel_mod, list(dmodels))):
        assert fields(accel_mod.Model.from_buffer_copy(raw[k * sz:(k + 1) * sz])) == fields(m), k
    assert np.fromfile(prefix + "origin.i32", dtype=np.int32).tolist() == [0, 1]


def test_cli_objects_merge_on_the_scene(sc, tmp_path):
    """bf_motion_compensator --objects=4 --objects-merge on the scene written as an event file: two groups and the unassigned
    count in objects_0.txt, an objects_0.merge.txt consistent with it, and --objects-img projects the reduced grouping.  Without
    the flag the four proposed groups stay."""
    from better_flow_amd import synth
    exe = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")
    txt = str(tmp_path / "scene.txt")
    synth.write_txt(txt, sc)

    def run(name, extra):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([exe, "--objects=4"] + extra + ["--res-x=%d" % H, "--res-y=%d" % W, "--quiet", "--img-prefix", str(out), txt],
                           cwd=str(out), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return out

    plain, merged = run("plain", []), run("merged", ["--objects-merge", "--objects-img"])
    assert sorted(os.listdir(str(plain))) == ["objects_0.txt"]
    assert sorted(os.listdir(str(merged))) == ["objects_0.merge.txt", "objects_0.pgm", "objects_0.ppm", "objects_0.score.txt", "objects_0.txt"]
    assert len(open(str(plain / "objects_0.txt")).read().splitlines()) == 5
    lines = open(str(merged / "objects_0.txt")).read().splitlines()
    print("\n".join(lines))
    assert len(lines) == 3 and lines[2].split()[0] == "unassigned"
    groups = [ln.split() for ln in lines[:2]]
    assert [g[0] for g in groups] == ["0", "1"] and all(len(g) == 16 for g in groups)
    assert sum(int(g[1]) for g in groups) + int(lines[2].split()[1]) == len(sc["t"])
    patch = min(groups, key=lambda g: abs(float(g[2]) - scene.V_PATCH[0]) + abs(float(g[3]) - scene.V_PATCH[1]))
    assert abs(float(patch[2]) - scene.V_PATCH[0]) <= 5.0 and abs(float(patch[3]) - scene.V_PATCH[1]) <= 5.0, patch
    steps = [ln.split() for ln in open(str(merged / "objects_0.merge.txt")).read().splitlines()]
    print(steps)
    assert steps[-1][0] == "info" and int(steps[-1][1]) == 2 and all(len(s) == 7 and s[0] in ("merge", "dissolve") for s in steps[:-1])
    assert [int(s[6]) for s in steps[:-1]] == [3, 2]   # four proposals, two steps, K after each
    score = [ln.split() for ln in open(str(merged / "objects_0.score.txt")).read().splitlines()]
    info = dict(zip(pr.INFO_FIELDS, (int(v) for v in score[-1][1:])))
    # the projection's objective of the reduced grouping is the merger's final S
    assert info["models"] == 2 and info["sum_sq"] == int(steps[-1][2]) and info["unassigned"] == int(lines[2].split()[1])
    assert [int(s[1]) for s in score[:2]] == [int(g[1]) for g in groups]

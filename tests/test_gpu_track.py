"""bf_track_keep / bf_track_overlap / bf_track_drop on the MI355X (csrc/bf_track.hip: k_track_overlap; the keep drives the
projection's kernels) against tests/track_ref.py, the numpy restatement.

Bar.  After an event's pixel both entries are integer counts and smallest indices, and the pixel is bf_assign_groups' own with
one time operand changed: every comparison is EQUALITY of the kept plane, the overlap table, the inside counts and the info, no
tolerance.  The kept plane is also held to the bytes of bf_project_groups' label on the same context."""
import ctypes

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import project_groups_ref as pr
import segment_scene as scene
import track_ref as tr
import track_scene
from test_gpu_groups import fields, seeded_models, to_accel

pytestmark = pytest.mark.gpu

H, W = scene.H, scene.W
STEP = track_scene.STEP_NS
GUARD, MIN_EVENTS, HARD_CAP = (90, 120), 100, 20000


@pytest.fixture(scope="module")
def slices():
    sl, _ = track_scene.make()
    for s in sl:
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return sl


def truth(sl):
    return sl["is_patch"].astype(np.int32), [ar.model_of_velocity(scene.V_BACKGROUND), ar.model_of_velocity(scene.V_PATCH)]


def make_acc(accel_mod, n, rows=3 * H + 3, cols=3 * W + 3):
    return accel_mod.Accel(device=0, max_events=max(n, 16), max_rows=rows, max_cols=cols)


@pytest.fixture(scope="module")
def acc(accel_mod, slices):
    a = make_acc(accel_mod, max(len(s["t"]) for s in slices))
    yield a
    a.close()


def upload(a, sl):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])


def info_dict(info):
    return {k: getattr(info, k) for k in tr.INFO_FIELDS}


def random_slice(seed, n, res, t_max=30_000_000):
    rng = np.random.default_rng(seed)
    return dict(fr_x=rng.integers(0, res[0], n).astype(np.int32), fr_y=rng.integers(0, res[1], n).astype(np.int32),
                t=np.sort(rng.integers(0, t_max, n)).astype(np.int64))


def empty_slice():
    return dict(fr_x=np.zeros(0, np.int32), fr_y=np.zeros(0, np.int32), t=np.zeros(0, np.int64))


def keep_same(accel_mod, a, sl, ids, ms, scale, res, margin=0, what="keep", against_projection=True):
    """upload + set_groups + track_keep on `a`, held to the restatement and to bf_project_groups' label; -> (plane, Kp) of the
    restatement."""
    upload(a, sl)
    a.set_groups(ids, len(ms))
    dms = to_accel(accel_mod, ms)
    plane, info = a.track_keep(dms, scale, res, margin=margin)
    ref_plane, ref_info, Kp = tr.keep(sl, ids, ms, scale, res, margin)
    print("%s: info %s" % (what, info_dict(info)))
    assert info_dict(info) == ref_info, (what, info_dict(info), ref_info)
    assert plane.dtype == np.int32 and plane.shape == ref_plane.shape and plane.tobytes() == ref_plane.tobytes(), what
    assert a.tracks_held == Kp
    if against_projection:
        img, _, _ = a.project_groups(dms, scale, res, margin=margin, want=("label",))
        assert img["label"].tobytes() == plane.tobytes(), what
    return ref_plane, Kp


def overlap_same(accel_mod, a, sl, ids, ms, kept, dt, scale, res, margin=0, what="overlap", loaded=False):
    """upload + set_groups (unless loaded) + track_overlap on `a`, held to the restatement; -> the device's result."""
    if not loaded:
        upload(a, sl)
        a.set_groups(ids, len(ms))
    dev = a.track_overlap(to_accel(accel_mod, ms), dt, scale, res, margin=margin)
    table, inside, info = tr.overlap(sl, ids, ms, kept[0], kept[1], dt, scale, res, margin)
    print("%s: info %s, rows %s" % (what, info_dict(dev[2]), dev[0][:4].tolist()))
    assert info_dict(dev[2]) == info, (what, info_dict(dev[2]), info)
    assert dev[0].dtype == np.int32 and dev[0].shape == table.shape and dev[0].tobytes() == table.tobytes(), \
        (what, np.argwhere(dev[0] != table)[:4].tolist())
    assert dev[1].tobytes() == inside.tobytes(), what
    return dev


def dev_bytes(r):
    return r[0].tobytes() + r[1].tobytes() + bytes(r[2])


# ---- 1. the scene's pairs of consecutive slices ----

@pytest.mark.parametrize("margin", [0, 6])
@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("pair", [(0, 1), (1, 2)])
def test_scene_pairs(accel_mod, slices, acc, pair, scale, margin):
    prev, new = slices[pair[0]], slices[pair[1]]
    ids_p, ms = truth(prev)
    kept = keep_same(accel_mod, acc, prev, ids_p, ms, scale, (H, W), margin)
    dev = overlap_same(accel_mod, acc, new, truth(new)[0], ms, kept, STEP, scale, (H, W), margin)
    table, inside = dev[0].astype(np.int64), dev[1].astype(np.int64)
    for k in range(2):   # the bars of tests/test_track_cpu.py
        assert table[k, k] >= 0.8 * inside[k] and table[k, 1 - k] <= 0.05 * inside[k]


def test_negative_dt(accel_mod, slices, acc):
    ids1, ms = truth(slices[1])
    kept = keep_same(accel_mod, acc, slices[1], ids1, ms, 3, (H, W))
    dev = overlap_same(accel_mod, acc, slices[0], truth(slices[0])[0], ms, kept, -STEP, 3, (H, W))
    assert dev[0][0, 0] >= 0.8 * dev[1][0] and dev[0][1, 1] >= 0.8 * dev[1][1]


def test_dt_zero_on_the_kept_slice_is_the_projections_own_pixel(accel_mod, slices, acc):
    sl = slices[0]
    ids, ms = truth(sl)
    kept = keep_same(accel_mod, acc, sl, ids, ms, 1, (H, W))
    dev = overlap_same(accel_mod, acc, sl, ids, ms, kept, 0, 1, (H, W), loaded=True)
    assert (dev[0][:, kept[1]] == 0).all()   # at scale 1 an event's own pixel has an owner
    _, scores, pinfo = acc.project_groups(to_accel(accel_mod, ms), 1, (H, W), want=())
    assert dev[1].tolist() == [s.inside for s in scores] and dev[2].outside == pinfo.outside


# ---- 2. many groups, ids of -1, empty groups, K != Kp ----

def ids64(n):
    """Ids -1 .. 63 spread over the slice, groups 5 and 40 empty."""
    ids = ((np.arange(n) * 7) % 65 - 1).astype(np.int32)
    ids[(ids == 5) | (ids == 40)] = -1
    return ids


def small_models(K):
    """seeded_models with the centres inside a 33 x 65 sensor."""
    ms = seeded_models(K)
    for i, m in enumerate(ms[1:]):
        m.cx, m.cy = 4.0 + (7 * i) % 25, 3.0 + (11 * i) % 60
    return ms


def test_sixty_four_groups_with_rotation_and_divergence(accel_mod):
    res, n = (33, 65), 3000
    prev, new = random_slice(31, n, res), random_slice(32, n, res)
    ms = small_models(64)
    a = make_acc(accel_mod, n, 512, 1024)
    try:
        for scale, margin in ((3, 2), (1, 0)):
            kept = keep_same(accel_mod, a, prev, ids64(n), ms, scale, res, margin)
            dev = overlap_same(accel_mod, a, new, ids64(n)[::-1].copy(), ms, kept, 5_000_000, scale, res, margin)
            assert dev[2].unassigned > 0 and dev[1][5] == 0 == dev[1][40] and (dev[1] > 0).sum() == 62
    finally:
        a.close()


def test_kept_groups_and_new_groups_differ_in_number(accel_mod):
    res, n = (33, 65), 3000
    prev, new = random_slice(33, n, res), random_slice(34, n, res)
    ms64, ms3 = small_models(64), small_models(3)
    ids3 = (np.arange(n) % 4 - 1).astype(np.int32)
    ids2 = (np.arange(n) % 2).astype(np.int32)
    a = make_acc(accel_mod, n, 512, 1024)
    try:
        kept = keep_same(accel_mod, a, prev, ids64(n), ms64, 3, res)
        dev = overlap_same(accel_mod, a, new, ids3, ms3, kept, 2_000_000, 3, res, what="Kp = 64, K = 3")
        assert dev[0].shape == (3, 65)
        kept = keep_same(accel_mod, a, prev, ids2, ms3[:2], 3, res)
        dev = overlap_same(accel_mod, a, new, ids64(n), ms64, kept, 2_000_000, 3, res, what="Kp = 2, K = 64")
        assert dev[0].shape == (64, 3)
    finally:
        a.close()


@pytest.mark.parametrize("scale", [1, 9])
def test_a_sensor_of_one_pixel(accel_mod, scale):
    res, n = (1, 1), 2000
    prev, new = random_slice(35, n, res), random_slice(36, n, res)
    ids = (np.arange(n) % 4 - 1).astype(np.int32)
    ms = [gr.oracle.Model(), ar.model_of_velocity((150.0, -80.0)), ar.model_of_velocity((-90.0, 40.0))]
    a = make_acc(accel_mod, n, 512, 512)
    try:
        for margin in (0, 1):   # (a sensor of one pixel has wsx = 0: without a margin the window test rejects every event)
            kept = keep_same(accel_mod, a, prev, ids, ms, scale, res, margin)
            dev = overlap_same(accel_mod, a, new, ids, ms, kept, 1_000_000, scale, res, margin)
            assert (dev[1].sum() > 0) == (margin > 0) and dev[2].outside > 0
    finally:
        a.close()


def test_zero_events_in_either_slice(accel_mod):
    res = (12, 16)
    sl = random_slice(37, 500, res)
    ids = (np.arange(500) % 2).astype(np.int32)
    ms = [gr.oracle.Model(), ar.model_of_velocity((150.0, -80.0))]
    a = make_acc(accel_mod, 500, 64, 64)
    try:
        kept = keep_same(accel_mod, a, empty_slice(), np.zeros(0, np.int32), ms, 3, res)   # a kept plane of all -1
        assert (kept[0] == -1).all() and kept[0].shape == (36, 48) and a.tracks_held == 2
        dev = overlap_same(accel_mod, a, sl, ids, ms, kept, 1000, 3, res)
        assert (dev[0][:, :2] == 0).all() and dev[0][:, 2].sum() == dev[1].sum() > 0
        kept = keep_same(accel_mod, a, sl, ids, ms, 3, res)
        dev = overlap_same(accel_mod, a, empty_slice(), np.zeros(0, np.int32), ms, kept, 1000, 3, res)
        assert not dev[0].any() and not dev[1].any() and not any(info_dict(dev[2]).values())
    finally:
        a.close()


# ---- 3. the time operand: the f32 nearest to the 64-bit t + dt ----

def test_times_of_two_e8_ns_with_dt_beyond_two_to_the_33(accel_mod):
    """t up to 2e8 ns, dt = 2^33 + 1: the sum needs 34 bits and the f32's last place is 1024 ns.  For these seeds the rounding
    decides a pixel AND a word of the table: the restatement with the time operand rounded toward zero gives another table."""
    res, scale, margin, dt, K, n = (48, 64), 9, 40, (1 << 33) + 1, 8, 4000
    rng = np.random.default_rng(21)
    ms = [ar.model_of_velocity((float(p), float(q))) for p, q in rng.uniform(-4, 4, (K, 2))]
    prev, new = random_slice(7, n, res, 200_000_000), random_slice(164, n, res, 200_000_000)
    ids_p, ids_n = (np.arange(n) * 3 % K).astype(np.int32), (np.arange(n) % K).astype(np.int32)
    a = make_acc(accel_mod, n, 1200, 1300)
    try:
        kept = keep_same(accel_mod, a, prev, ids_p, ms, scale, res, margin, against_projection=False)
        dev = overlap_same(accel_mod, a, new, ids_n, ms, kept, dt, scale, res, margin)
        wrong = tr.overlap(new, ids_n, ms, kept[0], kept[1], dt, scale, res, margin, mutate="trunc_time")[0]
        assert (wrong != dev[0]).any() and dev[1].sum() == n   # (the rounding is visible, and every event is inside)
    finally:
        a.close()


# ---- 4. contention: one hot LDS word, a wave of 64 distinct keys ----

def test_70000_events_of_two_groups_on_one_pixel(accel_mod):
    n = 70000
    sl = dict(fr_x=np.full(n, 7, np.int32), fr_y=np.full(n, 9, np.int32), t=(np.arange(n) * 400).astype(np.int64))
    ids = (np.arange(n) % 3 != 0).astype(np.int32)
    ms = [gr.oracle.Model()] * 2
    a = make_acc(accel_mod, n, 64, 64)
    try:
        kept = keep_same(accel_mod, a, sl, ids, ms, 1, (12, 16))
        dev = overlap_same(accel_mod, a, sl, ids, ms, kept, 0, 1, (12, 16), loaded=True)
        assert dev[0].tolist() == [[0, int((ids == 0).sum()), 0], [0, int((ids == 1).sum()), 0]]   # the pixel is group 1's
    finally:
        a.close()


def test_3000_events_of_64_groups_on_one_pixel_row(accel_mod):
    n = 3000
    rng = np.random.default_rng(9)
    sl = dict(fr_x=np.full(n, 5, np.int32), fr_y=rng.integers(0, 40, n).astype(np.int32), t=np.sort(rng.integers(0, 1000, n)).astype(np.int64))
    ids = rng.integers(0, 64, n).astype(np.int32)
    ms = [gr.oracle.Model()] * 64   # (t < 1 us: no model moves an event; a wave holds up to 64 distinct (k, j))
    a = make_acc(accel_mod, n, 64, 128)
    try:
        for scale in (1, 3):
            kept = keep_same(accel_mod, a, sl, ids, ms, scale, (12, 40))
            dev = overlap_same(accel_mod, a, sl, ids, ms, kept, 500, scale, (12, 40), loaded=True)
            print("distinct (k, j):", int((dev[0] > 0).sum()))
            assert (dev[0] > 0).sum() > 640 and dev[1].sum() + dev[2].outside == n   # (more than ten keys per group)
    finally:
        a.close()


# ---- 5. storage order; what the kept plane survives; a second context ----

def test_upload_order_and_sorted_storage_give_the_same_bytes(accel_mod, slices, acc):
    ids0, ms = truth(slices[0])
    ids1 = truth(slices[1])[0]
    dms = to_accel(accel_mod, ms)
    kept = keep_same(accel_mod, acc, slices[0], ids0, ms, 3, (H, W))
    plain = overlap_same(accel_mod, acc, slices[1], ids1, ms, kept, STEP, 3, (H, W))
    upload(acc, slices[1])
    acc.set_groups(ids1, 2)
    acc.run_groups(2, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)   # (the events are now stored sorted by group)
    again = acc.track_overlap(dms, STEP, 3, (H, W))
    assert dev_bytes(again) == dev_bytes(plain)
    upload(acc, slices[1])
    acc.run_tiles(4, 4, 3, (H, W), (30, 40), MIN_EVENTS)   # (... sorted by tile)
    acc.set_groups(ids1, 2)
    assert dev_bytes(acc.track_overlap(dms, STEP, 3, (H, W))) == dev_bytes(plain)
    # the keep on sorted storage keeps the same plane
    upload(acc, slices[0])
    acc.set_groups(ids0, 2)
    acc.run_groups(2, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)
    plane, _ = acc.track_keep(dms, 3, (H, W))
    assert plane.tobytes() == kept[0].tobytes()


def test_the_kept_plane_survives_what_drops_slice_state(accel_mod, slices, acc):
    ids0, ms = truth(slices[0])
    ids1 = truth(slices[1])[0]
    dms = to_accel(accel_mod, ms)
    kept = keep_same(accel_mod, acc, slices[0], ids0, ms, 3, (H, W))
    want = dev_bytes(overlap_same(accel_mod, acc, slices[1], ids1, ms, kept, STEP, 3, (H, W)))
    # an upload, bf_set_cloud, bf_run, bf_global_set_window, bf_segment, bf_set_groups, bf_assign_groups with install,
    # bf_project_groups and bf_merge_scores (they clear the shared vote planes)
    upload(acc, slices[2])
    acc.set_cloud(3, H, W)
    acc.run()
    acc.global_set_window(1, 5)
    upload(acc, slices[2])
    acc.set_cloud(scene.SCALE, H, W)
    nx, ny = scene.flow_of(scene.V_BACKGROUND)
    acc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
    acc.segment(**scene.OPTS)
    acc.set_groups(truth(slices[2])[0], 2)
    acc.assign_groups(dms, 3, (H, W), install=True)
    acc.project_groups(dms, 3, (H, W), want=())
    acc.merge_scores(dms, 3, (H, W))
    assert acc.tracks_held == 2
    upload(acc, slices[1])
    acc.set_groups(ids1, 2)
    assert dev_bytes(acc.track_overlap(dms, STEP, 3, (H, W))) == want


def test_a_second_contexts_plane_is_independent(accel_mod, slices, acc):
    ids0, ms = truth(slices[0])
    ids1 = truth(slices[1])[0]
    dms = to_accel(accel_mod, ms)
    other = make_acc(accel_mod, len(slices[1]["t"]))
    try:
        kept = keep_same(accel_mod, acc, slices[0], ids0, ms, 3, (H, W))
        assert other.tracks_held == -1
        swapped = keep_same(accel_mod, other, slices[0], 1 - ids0, ms[::-1], 3, (H, W))   # the same plane with the labels swapped
        assert acc.tracks_held == 2 and (swapped[0] != kept[0]).any()
        a = overlap_same(accel_mod, acc, slices[1], ids1, ms, kept, STEP, 3, (H, W))
        b = overlap_same(accel_mod, other, slices[1], ids1, ms, swapped, STEP, 3, (H, W))
        assert a[0][:, :2].tobytes() == b[0][:, 1::-1].tobytes()
        other.track_drop()
        assert other.tracks_held == -1 and acc.tracks_held == 2
        assert dev_bytes(acc.track_overlap(dms, STEP, 3, (H, W))) == dev_bytes(a)
    finally:
        other.close()


# ---- 6. state ----

def test_the_slices_state_is_untouched_by_both_entries(accel_mod, slices, acc):
    sc = slices[0]
    ids, ms = truth(sc)
    lattice = accel_mod.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)

    def sequence(track):
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
        if track:
            four = to_accel(accel_mod, [ms[1], ms[0], ms[0], ms[0]])
            acc.track_keep(four, 3, (H, W), margin=6)
            acc.track_overlap(four, STEP, 3, (H, W), margin=6)
            acc.track_keep(four, 1, (H, W), want_plane=False)
            acc.track_overlap(four, -STEP, 1, (H, W))
            assert state() == before
        # the held grouping: the grouped solve gives what it gives without the two entries
        m, i, q = acc.run_groups(4, 3, (H, W), (30, 40), MIN_EVENTS, hard_iter_cap=HARD_CAP)
        return before + b"".join(fields(x) for x in m) + b"".join(fields(x) for x in i) + b"".join(fields(x) for x in q)

    assert sequence(True) == sequence(False)


def test_tracks_held_through_keep_replace_drop_and_upload(accel_mod):
    res = (12, 16)
    sl = random_slice(38, 400, res)
    a = make_acc(accel_mod, 400, 64, 64)
    try:
        assert a.tracks_held == -1
        a.track_drop()   # (nothing kept: a valid call)
        upload(a, sl)
        a.set_groups(np.arange(400, dtype=np.int32) % 3, 3)
        a.track_keep(to_accel(accel_mod, small_models(3)), 3, res, want_plane=False)
        assert a.tracks_held == 3
        upload(a, sl)
        assert a.tracks_held == 3 and a.get_stat("groups_held") == -1
        a.set_groups(np.arange(400, dtype=np.int32) % 5, 5)
        a.track_keep(to_accel(accel_mod, small_models(5)), 1, res, margin=2, want_plane=False)
        assert a.tracks_held == 5
        a.track_drop()
        assert a.tracks_held == -1
        a.track_drop()
    finally:
        a.close()


# ---- 7. errors ----

def test_every_error_code_and_a_refused_keep_leaves_the_plane(accel_mod, slices):
    A = accel_mod
    sc = slices[0]
    ids, ms_ref = truth(sc)
    a = make_acc(A, len(sc["t"]))
    ms = to_accel(A, ms_ref)

    def code(fn):
        with pytest.raises(A.BfError) as e:
            fn()
        return e.value.code

    try:
        assert code(lambda: a.track_keep(ms, 3, (H, W))) == A.BF_ERR_STATE                          # before an upload
        assert code(lambda: a.track_overlap(ms, 0, 3, (H, W))) == A.BF_ERR_STATE
        upload(a, sc)
        assert code(lambda: a.track_keep(ms, 3, (H, W))) == A.BF_ERR_STATE                          # no grouping held
        assert code(lambda: a.track_overlap(ms, 0, 3, (H, W))) == A.BF_ERR_STATE
        a.set_groups(ids, 2)
        assert code(lambda: a.track_overlap(ms, 0, 3, (H, W))) == A.BF_ERR_STATE                    # no plane kept
        kept = keep_same(A, a, sc, ids, ms_ref, 3, (H, W))
        good = dev_bytes(a.track_overlap(ms, 0, 3, (H, W)))
        # a refused keep, every way: the previous plane stays
        for kw in (dict(scale=2), dict(scale=11), dict(margin=-1), dict(margin=65537), dict(sensor_res=(0, W)), dict(sensor_res=(H, 65537))):
            args = dict(scale=3, sensor_res=(H, W), want_plane=False)
            args.update(kw)
            assert code(lambda: a.track_keep(ms, **args)) == A.BF_ERR_ARG, kw
        assert code(lambda: a.track_keep([], 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.track_keep([ms[0]] * 65, 3, (H, W), want_plane=False)) == A.BF_ERR_ARG
        assert code(lambda: a.track_keep([ms[0]] * 3, 3, (H, W))) == A.BF_ERR_ARG                   # the grouping has K = 2
        o = A.TrackOpts(3, H, W, 0)
        two = (A.Model * 2)(*ms)
        assert a.L.bf_track_keep(a.h, ctypes.byref(o), None, 2, None, None) == A.BF_ERR_ARG          # NULL models
        assert a.L.bf_track_keep(a.h, None, two, 2, None, None) == A.BF_ERR_ARG                      # NULL opts
        assert a.L.bf_track_keep(None, None, None, 0, None, None) == A.BF_ERR_ARG
        a.set_groups(np.zeros(len(sc["t"]), np.int32), 64)
        assert code(lambda: a.track_keep([ms[0]] * 64, 9, (1000, 1000), want_plane=False)) == A.BF_ERR_CAPACITY
        a.set_groups(ids, 2)
        assert a.tracks_held == 2 and dev_bytes(a.track_overlap(ms, 0, 3, (H, W))) == good
        # the overlap's own
        for kw in (dict(scale=1), dict(margin=1), dict(sensor_res=(H, W + 1)), dict(sensor_res=(H + 1, W)), dict(scale=2)):
            args = dict(scale=3, sensor_res=(H, W))
            args.update(kw)
            assert code(lambda: a.track_overlap(ms, 0, **args)) == A.BF_ERR_ARG, kw                 # not the kept window
        assert code(lambda: a.track_overlap(ms, (1 << 40) + 1, 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.track_overlap(ms, -(1 << 40) - 1, 3, (H, W))) == A.BF_ERR_ARG
        a.track_overlap(ms, 1 << 40, 3, (H, W))
        a.track_overlap(ms, -(1 << 40), 3, (H, W))
        assert code(lambda: a.track_overlap([], 0, 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.track_overlap([ms[0]] * 65, 0, 3, (H, W))) == A.BF_ERR_ARG
        assert code(lambda: a.track_overlap([ms[0]] * 3, 0, 3, (H, W))) == A.BF_ERR_ARG             # the grouping has K = 2
        assert a.L.bf_track_overlap(a.h, ctypes.byref(o), None, 2, 0, None, None, None) == A.BF_ERR_ARG
        assert a.L.bf_track_overlap(a.h, None, two, 2, 0, None, None, None) == A.BF_ERR_ARG
        assert a.L.bf_track_overlap(None, None, None, 0, 0, None, None, None) == A.BF_ERR_ARG
        assert a.L.bf_track_drop(None) == A.BF_ERR_ARG
        # every output NULL is a valid call
        assert a.L.bf_track_overlap(a.h, ctypes.byref(o), two, 2, 0, None, None, None) == A.BF_OK
        assert a.L.bf_track_keep(a.h, ctypes.byref(o), two, 2, None, None) == A.BF_OK
        a.upload_events(sc["fr_x"], sc["fr_y"], sc["t"], noise=np.zeros(len(sc["t"]), np.uint8))
        a.set_groups(ids, 2)
        assert code(lambda: a.track_keep(ms, 3, (H, W))) == A.BF_ERR_ARG                            # a noise mask
        assert code(lambda: a.track_overlap(ms, 0, 3, (H, W))) == A.BF_ERR_ARG
        upload(a, sc)
        a.set_groups(ids, 2)
        assert dev_bytes(a.track_overlap(ms, 0, 3, (H, W))) == good and kept[1] == 2
        a.track_drop()
        assert code(lambda: a.track_overlap(ms, 0, 3, (H, W))) == A.BF_ERR_STATE                    # dropped
    finally:
        a.close()

"""bf_hold_groups and bf_group_flow_medians on the MI355X (csrc/bf_hold_groups.hip: k_hold_groups, k_median_count,
k_median_pick) against tests/hold_groups_ref.py, the numpy restatement, and through every reader of the held flow as
tests/test_gpu_global_flow.py checks the other modes.

Bit for bit: (nx, ny), the positions, the owner planes, the field against the device's own held (u, v), the colour coding of the
device's own field, every frame payload, the -o rows, the medians against the restatement applied to the device's own (u, v).
Bounded: the held (u, v) against the host's compute_uv (global_flow_ref.UV_REL, derived there), and the medians against the
host-libm restatement by the same bound times the group's largest |u_i|: an order statistic moves by at most the largest
perturbation of its inputs, and the mean of two such by no more."""
import ctypes as C

import numpy as np
import pytest

import assign_ref as ar
import flowimg_ref as FI
import global_cells_ref as GC
import global_flow_ref as R
import groups_ref as gr
import hold_groups_ref as hg
import project_groups_ref as pr
import segment_scene as scene
from test_gpu_global_flow import _consumers, check_get_flow, check_renders
from test_gpu_groups import fields, seeded_models, to_accel
from test_gpu_project_groups import device_objects, ids64, random_slice   # noqa: F401  (device_objects: a fixture)

pytestmark = pytest.mark.gpu

H, W = scene.H, scene.W
GUARD, MIN_EVENTS, HARD_CAP = (90, 120), 100, 20000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def truth(sc):
    ids, ms = pr.scene_truth(sc)
    ids.setflags(write=False)
    return ids, ms


@pytest.fixture(scope="module")
def held_ref(sc, truth):
    """The restatement of the scene's hold, computed once and never changed."""
    h = hg.hold(sc, *truth)
    for v in h.values():
        v.setflags(write=False)
    return h


@pytest.fixture(scope="module")
def acc(accel_mod, sc):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    yield a
    a.close()


def ev_of(sl):
    return sl["fr_x"], sl["fr_y"], sl["t"]


def upload(a, sl):
    a.upload_events(*ev_of(sl))


def hold(accel_mod, a, sl, ids, ms, K=None, window=(1, 5)):
    """upload, window, grouping, hold."""
    upload(a, sl)
    a.global_set_window(*window)
    a.set_groups(ids, len(ms) if K is None else K)
    a.hold_groups(to_accel(accel_mod, ms))


def reader_bytes(a, res):
    """Every synchronous reader's output as one byte string."""
    out = b"".join(v.tobytes() for v in a.global_get_flow().values())
    for rule in (FI.LAST_UPLOADED, FI.FIRST_UPLOADED):
        out += b"".join(x.tobytes() for x in a.global_flow_field(*res, rule))
        out += b"".join(x.tobytes() for x in a.global_color_flow_img(*res, rule, want_hs=True))
        out += b"".join(x.tobytes() for x in a.global_render_flow_frame(*res, rule))
    out += b"".join(x.tobytes() for x in a.group_flow_medians())
    return out


# ---- 1. the hold against the restatement ----

def test_scene_with_truth_ids_and_the_two_true_models(accel_mod, sc, truth, held_ref, acc):
    hold(accel_mod, acc, sc, *truth)
    dev = check_get_flow(acc, held_ref, "scene")
    check_renders(acc, dev, ev_of(sc), (H, W), "scene")
    # every patch event carries the patch's flow, not the background's
    p = sc["is_patch"]
    assert np.abs(dev["u"][p] - scene.V_PATCH[0]).max() < 1e-9 and np.abs(dev["v"][~p] - scene.V_BACKGROUND[1]).max() < 1e-9


def test_sixty_four_groups_with_rotation_and_divergence_on_33x65(accel_mod):
    sl = random_slice(3000, 33, 65, seed=3)
    ids, ms = ids64(3000), seeded_models(64)
    assert (ids == -1).any() and not (ids == 5).any() and not (ids == 40).any()
    a = accel_mod.Accel(device=0, max_events=3000, max_rows=128, max_cols=256)
    try:
        hold(accel_mod, a, sl, ids, ms)
        dev = check_get_flow(a, hg.hold(sl, ids, ms), "K = 64")
        none = ids < 0
        assert not dev["u"][none].any() and not dev["v"][none].any()
        assert np.array_equal(dev["pr_x"][none], sl["fr_x"][none].astype(np.float64))
        check_renders(a, dev, ev_of(sl), (33, 65), "K = 64")
        um, vm, counts = a.group_flow_medians()
        rum, rvm, rcounts = hg.medians(dev["u"], dev["v"], ids, 64)
        assert np.array_equal(counts, rcounts) and counts[5] == 0 == counts[40] and um[5] == 0.0 == vm[40]
        assert np.array_equal(_bits(um), _bits(rum)) and np.array_equal(_bits(vm), _bits(rvm))
    finally:
        a.close()


def test_one_event_on_a_one_pixel_sensor(accel_mod):
    sl = dict(fr_x=np.zeros(1, np.int32), fr_y=np.zeros(1, np.int32), t=np.zeros(1, np.int64))
    ms = [ar.model_of_velocity((150.0, -80.0))]
    a = accel_mod.Accel(device=0, max_events=1, max_rows=16, max_cols=16)
    try:
        hold(accel_mod, a, sl, np.zeros(1, np.int32), ms)
        dev = check_get_flow(a, hg.hold(sl, np.zeros(1, np.int32), ms), "1 x 1")
        for rule in (FI.LAST_UPLOADED, FI.FIRST_UPLOADED):
            owner, U, V = a.global_flow_field(1, 1, rule)
            assert owner.tolist() == [[0]] and _bits(U)[0, 0] == _bits(dev["u"])[0] and _bits(V)[0, 0] == _bits(dev["v"])[0]
        um, vm, counts = a.group_flow_medians()
        assert _bits(um)[0] == _bits(dev["u"])[0] and _bits(vm)[0] == _bits(dev["v"])[0] and counts.tolist() == [1, 0]
    finally:
        a.close()


def test_zero_events(accel_mod, truth):
    a = accel_mod.Accel(device=0, max_events=16, max_rows=64, max_cols=96)
    em = accel_mod.Emit(a, 64, 20, 30, 64)
    try:
        a.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        a.global_set_window(3, 5)
        a.set_groups(np.zeros(0, np.int32), 2)
        a.hold_groups(to_accel(accel_mod, truth[1]))
        keep = np.full(4, -7.0)
        assert a.L.bf_global_get_flow(a.h, *[keep.ctypes.data_as(C.c_void_p)] * 6) == 0 and (keep == -7.0).all()
        owner, U, V = a.global_flow_field(20, 30)
        assert (owner == -1).all() and not U.any() and not V.any()
        assert (a.global_color_flow_img(20, 30) == 255).all()
        p, _, f = a.global_render_flow_frame(20, 30)
        assert (p[:, 30:60] == 255).all() and not p[:, :30].any() and (f == np.float32(1e9)).all()
        assert em.slice(0, 0, 0, held=True) == (-1, None)
        um, vm, counts = a.group_flow_medians()
        assert not um.any() and not vm.any() and counts.tolist() == [0, 0, 0]
    finally:
        em.close()
        a.close()


def test_times_up_to_2e8_ns_where_float_of_t_rounds(accel_mod):
    sl = random_slice(3000, 33, 65, seed=7, duration_ns=200_000_000)
    assert (sl["t"].astype(np.float32).astype(np.int64) != sl["t"]).any()                 # float(t) does round
    ids = (np.arange(3000) % 4 - 1).astype(np.int32)
    ms = [ar.model_of_velocity((15.0, -8.0)), seeded_models(3)[1], ar.model_of_velocity((-9.0, 4.0))]
    a = accel_mod.Accel(device=0, max_events=3000, max_rows=128, max_cols=256)
    try:
        hold(accel_mod, a, sl, ids, ms)
        dev = check_get_flow(a, hg.hold(sl, ids, ms), "2e8 ns")
        check_renders(a, dev, ev_of(sl), (33, 65), "2e8 ns")
    finally:
        a.close()


# ---- 2. the hold against the device itself ----

def test_one_group_is_set_model_and_writeout_on_a_second_context(accel_mod, sc, acc):
    m = seeded_models(3)[2]                                                               # rotation and divergence
    assert m.total_rot != 0 and m.total_div != 0
    hold(accel_mod, acc, sc, np.zeros(len(sc["t"]), np.int32), [m])
    got = acc.global_get_flow()
    b = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        upload(b, sc)
        b.set_cloud(3, H, W)
        b.set_model(to_accel(accel_mod, m))
        _, _, nx, ny = b.writeout_events()
        u, v = b.compute_uv()
    finally:
        b.close()
    assert nx.any() and len(np.unique(nx)) > 100
    for k, ref in (("nx", nx), ("ny", ny), ("u", u), ("v", v)):
        assert np.array_equal(_bits(got[k]), _bits(ref)), k


# ---- 3. storage order ----

def test_storage_orders_and_later_resorts_leave_every_readers_bytes(accel_mod, sc, truth, acc):
    ids, ms = truth
    ms2 = to_accel(accel_mod, ms)
    hold(accel_mod, acc, sc, ids, ms)
    plain = reader_bytes(acc, (H, W))
    # the events sorted by group before the hold
    upload(acc, sc)
    acc.set_groups(gr.scene_groups(sc), 4)
    acc.run_groups(4, 3, (H, W), GUARD, MIN_EVENTS, hard_iter_cap=HARD_CAP)
    acc.global_set_window(1, 5)
    acc.set_groups(ids, 2)
    acc.hold_groups(ms2)
    assert reader_bytes(acc, (H, W)) == plain
    # ... and sorted again, the grouping replaced twice, AFTER the hold: the hold keeps its own slot order
    flow_only = lambda: b"".join(v.tobytes() for v in acc.global_get_flow().values()) + \
        b"".join(x.tobytes() for x in acc.global_render_flow_frame(H, W))
    before = flow_only()
    acc.run_groups(2, 3, (H, W), (30, 40), MIN_EVENTS, hard_iter_cap=HARD_CAP)
    assert flow_only() == before
    acc.assign_groups(ms2, 3, (H, W), install=True)
    assert flow_only() == before
    acc.set_groups(gr.scene_groups(sc), 4)
    assert flow_only() == before
    acc.global_set_cells(H, W, 16, 16)                                                    # (drops a grid hold, not this one)
    assert flow_only() == before
    acc.set_groups(ids, 2)
    assert reader_bytes(acc, (H, W)) == plain


# ---- 4. the -o rows ----

def test_emit_rows_carry_the_groups_flow(accel_mod):
    ts, row, col = R.emit_stream()
    slices = R.emit_slices(ts)
    Hh, Ww = R.EMIT_SENSOR
    cap = 2 * len(ts)
    ms = to_accel(accel_mod, seeded_models(3))
    a = accel_mod.Accel(device=0, max_events=len(ts), max_rows=3 * Hh + 3, max_cols=3 * Ww + 3)
    em = accel_mod.Emit(a, cap, Hh, Ww, 2 * len(ts))
    try:
        for k, (first, n, start, lead) in enumerate(slices):
            s = slice(first, first + n)
            t_loc = ts[s].astype(np.int64) - start
            a.upload_events(row[s].astype(np.int32), col[s].astype(np.int32), t_loc.astype(np.int32))
            a.global_set_window(3, 15)
            a.set_groups(((np.arange(n) * 5 + k) % 4 - 1).astype(np.int32), 3)
            a.hold_groups(ms)
            flow = a.global_get_flow(keys=("u", "v"))
            assert flow["u"].any() and (flow["u"] == 0).any()
            ld = (int(ts[first - 1]), int(row[first - 1]), int(col[first - 1])) if lead else None
            ticket, rows = em.slice(n, first, start, lead=ld, held=True)
            assert ticket == k
            want = R.emit_rows(ts, row, col, slices, k, (flow["u"], flow["v"]), cap)
            assert len(want["t"]) > 0
            for key in ("t", "row", "col"):
                assert np.array_equal(rows[key], want[key]), (k, key)
            for key in ("u", "v"):
                assert np.array_equal(_bits(rows[key]), _bits(want[key])), (k, key)
    finally:
        em.close()
        a.close()


# ---- 5. state and errors ----

def test_every_error_code_and_a_refused_hold_keeps_the_flow(accel_mod):
    A = accel_mod
    ev = GC.tie_slice(False)
    n = len(ev[0])
    ids = (np.arange(n) % 3 - 1).astype(np.int32)
    ms = to_accel(A, seeded_models(2))
    arr = (A.Model * 2)(*ms)
    a = A.Accel(device=0, max_events=n, max_rows=128, max_cols=128)
    em = A.Emit(a, 4 * n, 24, 24, 4 * n)
    fr = C.c_void_p()
    assert a.L.bf_flow_frame_create(a.h, 24, 24, 1, A.BF_FRAME_PPM, C.byref(fr)) == 0
    L = a.L

    def all_refuse(what):
        for name, call in _consumers(A, a, em, fr, n).items():
            assert call() == A.BF_ERR_STATE, (what, name)
        assert L.bf_group_flow_medians(a.h, None, None, None) == A.BF_ERR_STATE, what

    try:
        assert L.bf_hold_groups(None, arr, 2) == A.BF_ERR_ARG
        assert L.bf_group_flow_medians(None, None, None, None) == A.BF_ERR_ARG
        assert L.bf_hold_groups(a.h, arr, 2) == A.BF_ERR_STATE                            # before an upload
        a.upload_events(*ev)
        assert L.bf_hold_groups(a.h, arr, 2) == A.BF_ERR_STATE                            # no global window
        a.set_groups(ids, 2)
        assert L.bf_hold_groups(a.h, arr, 2) == A.BF_ERR_STATE                            # ... a grouping does not replace it
        a.upload_events(*ev)
        a.global_set_window(3, 15)
        assert L.bf_hold_groups(a.h, arr, 2) == A.BF_ERR_STATE                            # no grouping
        all_refuse("window, no hold")
        a.global_hold_best()
        assert L.bf_group_flow_medians(a.h, None, None, None) == A.BF_ERR_STATE           # a held flow, no grouping
        a.set_groups(ids, 2)
        assert L.bf_group_flow_medians(a.h, None, None, None) == A.BF_OK                  # ANY mode's flow; every output NULL
        a.hold_groups(ms)
        good = a.global_get_flow()
        assert good["u"].any()
        for call in (lambda: L.bf_hold_groups(a.h, None, 2), lambda: L.bf_hold_groups(a.h, arr, 0),
                     lambda: L.bf_hold_groups(a.h, (A.Model * 65)(*([ms[0]] * 65)), 65), lambda: L.bf_hold_groups(a.h, arr, 1),
                     lambda: L.bf_hold_groups(a.h, (A.Model * 3)(*([ms[0]] * 3)), 3)):
            assert call() == A.BF_ERR_ARG
            flow = a.global_get_flow()
            assert all(flow[k].tobytes() == good[k].tobytes() for k in R.KEYS)              # refused: the flow is as it was
        a.set_groups(np.zeros(n, np.int32), 65)
        assert L.bf_group_flow_medians(a.h, None, None, None) == A.BF_ERR_CAPACITY
        assert L.bf_global_get_flow(a.h, None, None, None, None, None, None) == A.BF_OK
        a.global_set_window(3, 15)                                                        # drops the hold
        all_refuse("set_window")
        a.set_groups(ids, 2)
        a.hold_groups(ms)
        a.upload_events(*ev)                                                              # invalidates it
        all_refuse("upload")
        a.upload_events(*ev, noise=np.zeros(n, np.uint8))
        a.global_set_window(3, 15)
        a.set_groups(ids, 2)
        assert L.bf_hold_groups(a.h, arr, 2) == A.BF_ERR_ARG                              # a noise mask
    finally:
        L.bf_flow_frame_destroy(fr)
        em.close()
        a.close()


def test_groups_held_statistic(accel_mod):
    """bf_get_stat "groups_held": -1 without a grouping, K with one, -1 again after an upload."""
    ev = GC.tie_slice(False)
    n = len(ev[0])
    a = accel_mod.Accel(device=0, max_events=n, max_rows=128, max_cols=128)
    try:
        assert a.get_stat("groups_held") == -1
        a.upload_events(*ev)
        assert a.get_stat("groups_held") == -1
        a.set_groups(np.zeros(n, np.int32), 5)
        assert a.get_stat("groups_held") == 5
        a.set_groups(np.full(n, -1, np.int32), 0)
        assert a.get_stat("groups_held") == 0
        a.assign_groups(to_accel(accel_mod, seeded_models(3)), 3, (24, 24), install=True)
        assert a.get_stat("groups_held") == 3
        a.upload_events(*ev)
        assert a.get_stat("groups_held") == -1
    finally:
        a.close()


def test_the_slices_state_is_untouched(accel_mod, sc, truth, acc):
    ids, ms = truth
    lattice = accel_mod.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)
    four = to_accel(accel_mod, [ms[1], ms[0], ms[0], ms[0]])

    def sequence(with_hold):
        upload(acc, sc)
        acc.set_cloud(scene.SCALE, H, W)
        nx, ny = scene.flow_of(scene.V_BACKGROUND)
        acc.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
        acc.segment(**scene.OPTS)
        acc.set_groups(gr.scene_groups(sc), 4)
        acc.global_set_window(1, 5)
        acc.global_search(lattice, want_surface=False)

        def state():
            lab, comps, cl = acc.segment_get()
            return lab.tobytes() + comps.tobytes() + cl.tobytes() + b"".join(x.tobytes() for x in acc.writeout_events()) + \
                b"".join(v.tobytes() for v in acc.global_get_events().values()) + b"".join(x.tobytes() for x in acc.get_time_img())

        before = state()
        if with_hold:
            acc.hold_groups(four)
            acc.group_flow_medians()
            acc.global_flow_field(H, W)
            assert state() == before
        # the held grouping and the vote planes' users give what they give without the hold
        g = acc.assign_groups(four, 3, (H, W), use_prior=True, install=False)
        m, i, q = acc.run_groups(4, 3, (H, W), (30, 40), MIN_EVENTS, hard_iter_cap=HARD_CAP)
        return before + g[0].tobytes() + g[1].tobytes() + g[2].tobytes() + b"".join(fields(x) for x in m) + \
            b"".join(fields(x) for x in i) + b"".join(fields(x) for x in q)

    assert sequence(True) == sequence(False)


# ---- 6. the medians as bits: flows crafted through bf_global_hold_field on cells of one pixel ----

MED_RES = (72, 64)


def median_case():
    """(nx, ny, ids) of 4608 events, one per pixel of a 72 x 64 sensor: groups of 1, 2, 3, 64, 65 and 4097 random values, several
    groups whose two middles are neighbouring doubles, equal middles, zeros of both signs, all negative, all equal; the other
    ids up to 63 empty; the rest -1 with values far outside."""
    rng = np.random.default_rng(17)
    parts = []
    for c in (1, 2, 3, 64, 65, 4097):
        parts.append((rng.uniform(-0.3, 0.3, c), rng.uniform(-0.3, 0.3, c)))
    for base in (0.0371, 0.1113, -0.0717, 0.2049):                                        # groups 6 .. 9
        nb = np.nextafter(base, 1.0)
        parts.append((np.array([base - 0.01, base, nb, base + 0.01]), np.array([0.0, 0.0, 0.0, 0.0])))
    parts.append((np.array([0.01, 0.05, 0.05, 0.09]), np.array([-0.02, -0.02, 0.03, -0.02])))     # 10: equal middles
    parts.append((np.array([-0.0, 0.0, -0.0]), np.array([0.01, 0.01, 0.01])))                   # 11: u = -0, +0, -0
    parts.append((np.array([-0.0, 0.0]), np.array([0.02, 0.02])))                               # 12: an even count of zeros
    parts.append((-rng.uniform(0.01, 0.3, 6), -rng.uniform(0.01, 0.3, 6)))                      # 13: all negative
    parts.append((np.full(10, 0.123), np.full(10, -0.0456)))                                    # 14: all equal
    nx = np.concatenate([p[0] for p in parts])
    ny = np.concatenate([p[1] for p in parts])
    ids = np.concatenate([np.full(len(p[0]), k, np.int32) for k, p in enumerate(parts)])
    rest = MED_RES[0] * MED_RES[1] - len(nx)
    assert rest > 100
    nx = np.concatenate([nx, np.full(rest, 0.9)])
    ny = np.concatenate([ny, np.full(rest, -0.9)])
    ids = np.concatenate([ids, np.full(rest, -1, np.int32)])
    return nx, ny, ids


def run_median_case(accel_mod, a, nx, ny, ids, order):
    """Event i sits on pixel i and carries (nx, ny, ids)[order[i]]: the device's medians, counts and own (u, v)."""
    n = MED_RES[0] * MED_RES[1]
    px = np.arange(n)
    a.upload_events((px // MED_RES[1]).astype(np.int32), (px % MED_RES[1]).astype(np.int32), np.zeros(n, np.int32))
    a.global_set_window(1, 5)
    a.global_set_cells(*MED_RES, 1, 1)
    a.global_hold_field(nx[order].reshape(MED_RES), ny[order].reshape(MED_RES), mode=R.CELLS)
    a.set_groups(ids[order], 64)
    flow = a.global_get_flow(keys=("u", "v"))
    return a.group_flow_medians(), flow


def test_medians_as_bits_in_two_storage_orders(accel_mod):
    nx, ny, ids = median_case()
    n = len(ids)
    rng = np.random.default_rng(23)
    a = accel_mod.Accel(device=0, max_events=n, max_rows=3 * MED_RES[0] + 3, max_cols=3 * MED_RES[1] + 3)
    try:
        results = []
        for order in (rng.permutation(n), np.arange(n)[::-1].copy()):
            (um, vm, counts), flow = run_median_case(accel_mod, a, nx, ny, ids, order)
            rum, rvm, rcounts = hg.medians(flow["u"], flow["v"], ids[order], 64)
            assert np.array_equal(counts, rcounts), (counts.tolist(), rcounts.tolist())
            bad = np.nonzero((_bits(um) != _bits(rum)) | (_bits(vm) != _bits(rvm)))[0]
            assert bad.size == 0, [(int(k), um[k], rum[k], vm[k], rvm[k]) for k in bad[:6]]
            results.append((um, vm, counts))
            u = flow["u"]
            of = lambda k: u[ids[order] == k]
            # what the cases are there for, checked on the device's own values
            assert counts[:6].tolist() == [1, 2, 3, 64, 65, 4097] and not counts[15:64].any() and counts[64] == n - counts[:64].sum()
            last_pass_only = 0
            for k in (6, 7, 8, 9):
                s = np.sort(hg.key(of(k)))
                last_pass_only += int(s[1] != s[2] and (int(s[1]) ^ int(s[2])) < 256)
            assert last_pass_only >= 1                                                    # two middles only the last digit separates
            assert _bits(um)[11] == _bits(-0.0)[0] and _bits(um)[12] == _bits(0.0)[0]
            assert (of(13) < 0).all() and len(np.unique(_bits(of(14)))) == 1 and _bits(um)[14] == _bits(of(14))[0]
        # the same multiset in two storage orders: the same bits
        assert all(x.tobytes() == y.tobytes() for x, y in zip(*results))
    finally:
        a.close()


def test_medians_on_the_scene(accel_mod, sc, truth, held_ref, acc):
    ids, ms = truth
    some = ids.copy()
    some[::11] = -1
    hold(accel_mod, acc, sc, some, ms)
    flow = acc.global_get_flow(keys=("u", "v"))
    um, vm, counts = acc.group_flow_medians()
    rum, rvm, rcounts = hg.medians(flow["u"], flow["v"], some, 2)                         # the device's own (u, v): bits
    assert np.array_equal(counts, rcounts) and counts[2] == int((some < 0).sum())
    assert np.array_equal(_bits(um), _bits(rum)) and np.array_equal(_bits(vm), _bits(rvm))
    host = hg.hold(sc, some, ms)
    hum, hvm, _ = hg.medians(host["u"], host["v"], some, 2)                               # libm's hypot: bounded
    for k in range(2):
        for dev, ref, arr in ((um[k], hum[k], host["u"]), (vm[k], hvm[k], host["v"])):
            bound = R.UV_REL * np.abs(arr[some == k]).max()
            print("group %d: median %.17g, host %.17g, bound %.3g" % (k, dev, ref, bound))
            assert abs(dev - ref) <= bound
    # only some outputs asked for
    only = np.zeros(2)
    assert acc.L.bf_group_flow_medians(acc.h, None, only.ctypes.data_as(C.c_void_p), None) == 0 and np.array_equal(_bits(only), _bits(vm))


# ---- 7. end to end through Accel: search, proposals, alternation, hold, medians ----

def test_end_to_end_flow_of_the_found_objects(accel_mod, sc, acc, device_objects):
    models, gid = device_objects
    upload(acc, sc)
    acc.global_set_window(1, 5)
    acc.set_groups(gid, 2)
    acc.hold_groups(models)
    um, vm, counts = acc.group_flow_medians()
    print("found objects: medians %s / %s, counts %s" % (um.tolist(), vm.tolist(), counts.tolist()))
    patch = int(np.argmin(np.hypot(um - scene.V_PATCH[0], vm - scene.V_PATCH[1])))
    assert np.hypot(um[patch] - scene.V_PATCH[0], vm[patch] - scene.V_PATCH[1]) <= 5.0
    recall, _ = ar.recall_purity(sc, gid, patch_group=patch, background_group=1 - patch)
    assert recall >= 0.99, recall
    flow = acc.global_get_flow(keys=("u", "v"))
    on_patch = sc["is_patch"] & (gid == patch)
    assert np.hypot(flow["u"][on_patch] - scene.V_PATCH[0], flow["v"][on_patch] - scene.V_PATCH[1]).max() <= 5.0

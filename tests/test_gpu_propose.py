"""bf_propose_models on the MI355X (csrc/bf_propose.hip: k_propose_vote in its two forms, k_propose_box, k_propose_pick) against
tests/propose_ref.py, the numpy restatement.

Bar.  After the index match the operator is integer counts, maxima and lowest indices, and the per-event best state it reads is
brought back from the device (bf_global_get_events) and handed to the restatement: every comparison is EQUALITY of proposals,
models, info, H and B, no tolerance.  What the search itself leaves in that state is held to the numpy search by
tests/test_gpu_global*.py; the scene's first case also pins the proposals to the table of DESIGN section 16, which the numpy
search gave.  The alternation from the proposals is teacher-forced as in tests/test_gpu_assign.py and ends on its semantic bars
(recall >= 0.99, group 1's median flow within 5 px/s of the patch's velocity, within five alternations)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import assign_ref as ar
import groups_ref as gr
import propose_ref as pr
import segment_scene as scene
from test_gpu_groups import fields, to_accel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = scene.H, scene.W
GUARD, MIN_EVENTS, HARD_CAP = (90, 120), 100, 20000
INFO_KEYS = ("n_x", "n_y", "voted", "unscored", "off_lattice", "proposals")
LDS_FORM, GLOBAL_FORM = 1, 2
# the scene's proposals at r = 1, suppress = 2 after the scale-1 search over the 36 x 36 lattice
TABLE = [(597, 3878), (1124, 1621), (1231, 746), (1234, 617)]


@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def acc(accel_mod, sc):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    yield a
    a.close()


def upload(a, sl):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])


def lattice36(A):
    return A.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04)


def info_dict(info):
    return {k: getattr(info, k) for k in INFO_KEYS}


def dev_bytes(r):
    models, props, info, Hd, Bd = r
    return b"".join(fields(m) for m in models) + b"".join(bytes(p) for p in props) + bytes(info) + Hd.tobytes() + Bd.tobytes()


def check(a, opts, what, form=LDS_FORM, **kw):
    """One call against the restatement of the state the device holds; returns the device's result."""
    ev = a.global_get_events()
    xs, ys, nz = pr.lattice_values(opts)
    rm, rp, rinfo, rH, rB = pr.propose(ev["max_score"], ev["best_nx"], ev["best_ny"], xs, ys, nz, **kw)
    dev = a.propose_models(opts, want_planes=True, **kw)
    models, props, info, Hd, Bd = dev
    print("%s: info %s, first proposals %s" % (what, info_dict(info), [(p.index, p.votes, p.peak) for p in props[:4]]))
    assert info_dict(info) == rinfo, (what, info_dict(info), rinfo)
    assert Hd.dtype == np.uint32 and Hd.shape == rH.shape and Hd.tobytes() == rH.tobytes(), what
    assert Bd.tobytes() == rB.tobytes(), what
    got = np.frombuffer(b"".join(bytes(p) for p in props), dtype=pr.flat_proposals([]).dtype)
    assert got.tobytes() == pr.flat_proposals(rp).tobytes(), (what, got, rp)
    assert [fields(m) for m in models] == [fields(m) for m in to_accel(sys.modules[type(a).__module__], rm)], what
    assert info.voted + info.unscored + info.off_lattice == a.n
    assert a.get_stat("propose_form") == (form if a.n else 0), what
    votes = [p.votes for p in props]
    assert votes == sorted(votes, reverse=True)
    return dev


# ---- 1. the scene ----

@pytest.fixture(scope="module")
def scene_state(accel_mod, sc, acc):
    """The scene searched at scale 1 over the 36 x 36 lattice; the tests below that use it leave the state as it is."""
    upload(acc, sc)
    acc.global_set_window(1, 5)
    acc.global_search(lattice36(accel_mod), want_surface=False)
    return lattice36(accel_mod)


def test_scene_at_scale_1_gives_the_table(sc, acc, scene_state):
    _, props, info, _, _ = check(acc, scene_state, "scene, scale 1", radius=1, suppress=2, max_models=4)
    assert [(p.index, p.votes) for p in props] == TABLE
    step = 0.04 / 1.27e-3   # one lattice step in px / s
    for p, truth in zip(props[:2], (scene.V_BACKGROUND, scene.V_PATCH)):
        assert abs(p.u - truth[0]) <= step and abs(p.v - truth[1]) <= step, (p.u, p.v, truth)


@pytest.mark.parametrize("radius", [0, 1, 8])
@pytest.mark.parametrize("suppress", [0, 2, 64])
@pytest.mark.parametrize("max_models", [1, 64])
def test_scene_options(acc, scene_state, radius, suppress, max_models):
    check(acc, scene_state, "r %d sup %d K %d" % (radius, suppress, max_models), radius=radius, suppress=suppress,
          max_models=max_models)


def test_min_votes_cuts_the_list(acc, scene_state):
    _, props, _, _, _ = check(acc, scene_state, "min_votes 700", radius=1, suppress=2, max_models=8, min_votes=700)
    assert [p.index for p in props] == [k for k, v in TABLE if v >= 700] and len(props) == 3


def test_a_repeated_call_gives_the_same_bytes(acc, scene_state):
    a = dev_bytes(acc.propose_models(scene_state, want_planes=True))
    assert a == dev_bytes(acc.propose_models(scene_state, want_planes=True))


def test_scene_at_scale_3(accel_mod, sc):
    a = accel_mod.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        upload(a, sc)
        a.global_set_window(3, 5)
        o = lattice36(accel_mod)
        a.global_search(o, want_surface=False)
        _, props, _, _, _ = check(a, o, "scene, scale 3", radius=1, suppress=2, max_models=4)
        step = 0.04 / 1.27e-3
        for p, truth in zip(props[:2], (scene.V_BACKGROUND, scene.V_PATCH)):
            assert abs(p.u - truth[0]) <= step and abs(p.v - truth[1]) <= step, (p.u, p.v, truth)
    finally:
        a.close()


# ---- 2. lattices: the default one barely searched, and one beyond the LDS ----

def test_default_lattice_after_a_pyramid_search(accel_mod, sc, acc):
    upload(acc, sc)
    acc.global_set_window(1, 5)
    acc.global_set_cells(H, W, 45, 60)
    o = accel_mod.Accel.global_search_opts()
    _, _, evaluated, _, _ = acc.global_search_cells_pyramid(o, levels=3, factor=4, radius=1)
    _, _, info, Hd, _ = check(acc, o, "default lattice, pyramid", radius=1, suppress=2, max_models=8)
    assert (info.n_x, info.n_y) == (180, 80) and len(evaluated) < 180 * 80 // 4
    mask = np.ones(180 * 80, dtype=bool)
    mask[evaluated] = False
    assert not Hd.ravel()[mask].any(), "a bin nobody evaluated holds votes"


def test_large_lattice_takes_the_global_atomic_form(accel_mod, sc):
    sl = {k: v[:2000] for k, v in sc.items()}
    a = accel_mod.Accel(device=0, max_events=2000, max_rows=H + 8, max_cols=W + 8)
    try:
        upload(a, sl)
        a.global_set_window(1, 5)
        a.global_set_cells(H, W, 45, 60)
        o = accel_mod.Accel.global_search_opts(x_low=-0.64, x_hi=0.64, x_step=0.005, y_low=-0.64, y_hi=0.64, y_step=0.005)
        a.global_search_cells_pyramid(o, levels=4, factor=4, radius=1)
        _, _, info, _, _ = check(a, o, "256 x 256 lattice", form=GLOBAL_FORM, radius=1, suppress=2, max_models=8)
        assert info.n_x >= 256 and info.n_y >= 256 and info.voted > 0
        check(a, o, "256 x 256 lattice, r 8", form=GLOBAL_FORM, radius=8, suppress=64, max_models=64)
    finally:
        a.close()


# ---- 3. a pile, a thin spread, the corners ----

def random_slice(n, rows, cols, seed, duration_ns=30_000_000):
    rng = np.random.default_rng(seed)
    return dict(fr_x=rng.integers(0, rows, n).astype(np.int32), fr_y=rng.integers(0, cols, n).astype(np.int32),
                t=np.sort(rng.integers(0, duration_ns, n)).astype(np.int64))


def test_a_pile_beyond_sixteen_bits(accel_mod):
    n = 70000
    sl = random_slice(n, 64, 64, 3)
    a = accel_mod.Accel(device=0, max_events=n, max_rows=72, max_cols=72)
    try:
        upload(a, sl)
        a.global_set_window(1, 5)
        o = lattice36(accel_mod)
        xs, ys, _ = pr.lattice_values(o)
        # every event the candidate keeps inside the window, (63 / 64)^2 of them, takes this one candidate
        a.global_project_all(xs[18], ys[19], want_img=False, want_scores=False)
        _, props, info, Hd, _ = check(a, o, "pile", radius=1, suppress=2, max_models=8)
        assert info.voted > 65535 and Hd[18, 19] == info.voted and len(props) == 1
        # B is the same over the 3 x 3 points around the pile: the pick is the one with the lowest index
        assert (props[0].index, props[0].votes, props[0].peak) == (17 * 36 + 18, info.voted, 0)
    finally:
        a.close()


def test_a_state_spread_thin(accel_mod):
    n = 3000
    sl = random_slice(n, 200, 200, 4)
    a = accel_mod.Accel(device=0, max_events=n, max_rows=208, max_cols=208)
    try:
        upload(a, sl)
        a.global_set_window(1, 3)
        o = accel_mod.Accel.global_search_opts(x_low=-1.6, x_hi=1.6, x_step=0.1, y_low=-1.6, y_hi=1.6, y_step=0.1)
        a.global_search(o, want_surface=False)
        _, _, info, Hd, _ = check(a, o, "thin", radius=0, suppress=0, max_models=64)
        print("thin: %d voters over %d bins, largest bin %d" % (info.voted, int((Hd > 0).sum()), int(Hd.max())))
        assert (Hd > 0).sum() > 64, "the votes must fall on more distinct bins than a wave has lanes"
    finally:
        a.close()


@pytest.mark.parametrize("corner", [(0, 0), (0, 35), (35, 0), (35, 35)])
def test_a_peak_in_a_lattice_corner(accel_mod, sc, acc, corner):
    upload(acc, sc)
    acc.global_set_window(1, 5)
    o = lattice36(accel_mod)
    xs, ys, _ = pr.lattice_values(o)
    acc.global_project_all(xs[corner[0]], ys[corner[1]], want_img=False, want_scores=False)
    for r in (1, 8):
        _, props, info, Hd, Bd = check(acc, o, "corner %s r %d" % (corner, r), radius=r, suppress=2, max_models=4)
        assert Hd[corner] == info.voted > 0 and Bd[corner] == info.voted
        # zero padding: B is the vote count on the (r + 1)^2 points the lattice has within r of the corner, zero elsewhere; the
        # pick is the one of them with the lowest index
        assert (Bd > 0).sum() == (r + 1) ** 2 and Bd.sum() == info.voted * (r + 1) ** 2
        assert props[0].index == max(0, corner[0] - r) * 36 + max(0, corner[1] - r) and props[0].votes == info.voted


# ---- 4. a state off the lattice, no events, errors ----

def test_a_state_continued_off_the_lattice(accel_mod, sc, acc):
    upload(acc, sc)
    acc.global_set_window(1, 5)
    o = lattice36(accel_mod)
    acc.global_search(o, want_surface=False)
    acc.global_project_all(*scene.flow_of(scene.V_BACKGROUND), want_img=False, want_scores=False)
    _, _, info, _, _ = check(acc, o, "off the lattice", radius=1, suppress=2, max_models=4)
    assert info.off_lattice > 0 and info.voted > 0


def test_zero_events(accel_mod):
    a = accel_mod.Accel(device=0, max_events=16, max_rows=64, max_cols=64)
    try:
        a.upload_events(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        a.global_set_window(1, 5)
        o = lattice36(accel_mod)
        models, props, info, Hd, Bd = a.propose_models(o, want_planes=True)
        assert models == [] and props == [] and not Hd.any() and not Bd.any() and Hd.shape == (36, 36)
        assert info_dict(info) == dict(n_x=36, n_y=36, voted=0, unscored=0, off_lattice=0, proposals=0)
        assert a.get_stat("propose_form") == 0
    finally:
        a.close()


def test_every_error_code(accel_mod, sc):
    A = accel_mod
    a = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    o = lattice36(A)

    def code(fn):
        with pytest.raises(A.BfError) as e:
            fn()
        return e.value.code

    def raw(lat=o, po=None, models=False, props=False, cap=8, hist=False, box=False, planes_cap=36 * 36):
        po = po if po is not None else A.AccelProposeOpts(1, 2, 8, 1)
        m, p = (A.Model * 64)(), (A.Proposal * 64)()
        h, b = np.zeros(36 * 36, np.uint32), np.zeros(36 * 36, np.uint32)
        return a.L.bf_propose_models(a.h, ctypes.byref(lat), ctypes.byref(po), m if models else None, p if props else None, cap,
                                     h.ctypes.data_as(ctypes.c_void_p) if hist else None,
                                     b.ctypes.data_as(ctypes.c_void_p) if box else None, planes_cap, None)

    try:
        upload(a, sc)
        assert code(lambda: a.propose_models(o)) == A.BF_ERR_ARG                                   # no window
        a.global_set_window(1, 5)
        for kw in (dict(radius=-1), dict(radius=9), dict(suppress=-1), dict(suppress=65), dict(max_models=0), dict(max_models=65),
                   dict(min_votes=0)):
            assert code(lambda: a.propose_models(o, **kw)) == A.BF_ERR_ARG, kw
        bad = A.Accel.global_search_opts(x_low=0.5, x_hi=-0.5)
        assert raw(lat=bad) == A.BF_ERR_ARG                                                         # the lattice's own range
        assert raw(models=True, cap=7) == A.BF_ERR_ARG and raw(props=True, cap=7) == A.BF_ERR_ARG   # cap < max_models
        assert raw(cap=0) == A.BF_OK                                                                # ... matters only with an output
        assert raw(hist=True, planes_cap=36 * 36 - 1) == A.BF_ERR_ARG and raw(box=True, planes_cap=0) == A.BF_ERR_ARG
        assert raw(planes_cap=0) == A.BF_OK
        nz = A.Accel.global_search_opts(x_low=-0.72, x_hi=0.72, x_step=0.04, y_low=-0.72, y_hi=0.72, y_step=0.04, nz=100.0)
        assert raw(lat=nz, models=True) == A.BF_ERR_ARG and raw(lat=nz, props=True) == A.BF_OK       # models need nz 127
        big = A.Accel.global_search_opts(x_low=0.0, x_hi=2049.0, x_step=1.0, y_low=0.0, y_hi=2048.0, y_step=1.0)
        assert raw(lat=big) == A.BF_ERR_CAPACITY                                                    # 2049 x 2048 > 2^22
        assert a.L.bf_propose_models(None, None, None, None, None, 0, None, None, 0, None) == A.BF_ERR_ARG
        assert a.L.bf_propose_models(a.h, None, None, None, None, 0, None, None, 0, None) == A.BF_OK   # NULL: the defaults
        upload(a, sc)
        assert code(lambda: a.propose_models(o)) == A.BF_ERR_STATE                                 # an upload since the window
    finally:
        a.close()


# ---- 5. storage order, state ----

def test_sorted_storage_gives_the_same_bytes(accel_mod, sc, acc):
    o = lattice36(accel_mod)

    def run():
        acc.global_set_window(1, 5)
        acc.global_search(o, want_surface=False)
        return dev_bytes(acc.propose_models(o, want_planes=True))

    upload(acc, sc)
    plain = run()
    upload(acc, sc)
    acc.run_tiles(4, 4, 3, (H, W), (30, 40), MIN_EVENTS)   # (the events are now stored sorted, with a permutation)
    assert run() == plain


def test_the_state_is_untouched(accel_mod, sc, acc):
    o = lattice36(accel_mod)
    gid = gr.scene_groups(sc)

    def sequence(propose):
        upload(acc, sc)
        acc.set_cloud(3, H, W)
        acc.set_groups(gid, 4)
        acc.global_set_window(1, 5)
        acc.global_search(o, want_surface=False)
        acc.global_hold_best()

        def state():
            return b"".join(v.tobytes() for v in acc.global_get_events().values()) + \
                b"".join(v.tobytes() for v in acc.global_get_flow().values()) + b"".join(x.tobytes() for x in acc.get_time_img())

        before = state()
        if propose:
            acc.propose_models(o, want_planes=True)
            acc.propose_models(o, radius=8, suppress=0, max_models=64)
            assert state() == before
        m, i, q = acc.run_groups(4, 3, (H, W), (30, 40), MIN_EVENTS, hard_iter_cap=HARD_CAP)
        return before + b"".join(fields(x) for x in m) + b"".join(fields(x) for x in i) + b"".join(fields(x) for x in q)

    assert sequence(True) == sequence(False)


# ---- 6. end to end: search, proposals, alternation ----

@pytest.fixture(scope="module")
def device_objects(accel_mod, sc, acc):
    """search + propose_models(max_models=2) + the alternation of DESIGN section 15 from the proposed models, every assignment
    teacher-forced against the restatement: (proposals, models, gid, records [changed, counts, iterations], last flows)."""
    from test_gpu_assign import refit, same
    A = accel_mod
    helper = A.Accel(device=0, max_events=len(sc["t"]), max_rows=3 * H + 3, max_cols=3 * W + 3)
    try:
        upload(acc, sc)
        acc.global_set_window(1, 5)
        o = lattice36(A)
        acc.global_search(o, want_surface=False)
        models, props, _ = acc.propose_models(o, max_models=2)
        assert len(models) == 2
        upload(acc, sc)
        prior, flows, records = None, None, []
        for alt in range(5):
            changed = None
            for _ in range(2):
                dev = acc.assign_groups(models, 3, (H, W), use_prior=prior is not None)
                same(dev, ar.assign(sc, models, 3, (H, W), prior=prior), "alternation %d" % alt)   # teacher-forced
                changed = dev[3].changed if changed is None else changed
                prior = dev[0]
            if alt > 0 and changed == 0:
                records.append([changed] + dev[2].tolist() + [-1, -1])
                break
            models, its, flows = refit(A, acc, helper, sc, prior, models)
            records.append([changed] + dev[2].tolist() + its)
            rec, pur = ar.recall_purity(sc, prior)
            print("alternation %d: recall %.4f purity %.4f iterations %s flows %s" % (alt + 1, rec, pur, its, flows))
        return props, models, prior, records, flows
    finally:
        helper.close()


def test_alternation_from_the_proposed_models(sc, device_objects):
    props, _, gid, records, flows = device_objects
    assert [(p.index, p.votes) for p in props] == TABLE[:2]
    rec, pur = ar.recall_purity(sc, gid)
    print("recall %.4f, purity %.4f, %d alternations" % (rec, pur, len(records)))
    assert len(records) <= 5 and rec >= 0.99
    assert abs(flows[1][0] - scene.V_PATCH[0]) <= 5.0 and abs(flows[1][1] - scene.V_PATCH[1]) <= 5.0, flows


def test_object_finder_gives_the_same_objects(accel_mod, sc, device_objects, tmp_path):
    """tests/cpp/test_object_finder.cpp linked against the product library: bf::ObjectFinder's proposals, ids, models and
    records equal the run through Accel above; its flows meet the same bar."""
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_object_finder")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_object_finder.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ev, prefix = str(tmp_path / "events.txt"), str(tmp_path / "out_")
    with open(ev, "w") as f:
        for a, b, c in zip(sc["fr_x"].tolist(), sc["fr_y"].tolist(), sc["t"].tolist()):
            f.write("%d %d %d\n" % (a, b, c))
    r = subprocess.run([exe, ev, "2", str(H), str(W), str(GUARD[0]), str(GUARD[1]), str(MIN_EVENTS), str(HARD_CAP), prefix],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    props, models, gid, records, _ = device_objects
    assert open(prefix + "proposals.bin", "rb").read() == b"".join(bytes(p) for p in props)
    assert np.fromfile(prefix + "records.i32", dtype=np.int32).reshape(-1, 6).tolist() == records
    assert np.fromfile(prefix + "gid.i32", dtype=np.int32).tobytes() == gid.tobytes()
    raw = open(prefix + "models.bin", "rb").read()
    sz = ctypes.sizeof(accel_mod.Model)
    assert len(raw) == 2 * sz
    for k in range(2):
        assert fields(accel_mod.Model.from_buffer_copy(raw[k * sz:(k + 1) * sz])) == fields(models[k]), k
    flows = np.fromfile(prefix + "flows.f64", dtype=np.float64).reshape(2, 2)
    print("bf::ObjectFinder: median flows per group (u, v):", flows[:, 0].tolist(), flows[:, 1].tolist())
    assert abs(flows[0, 1] - scene.V_PATCH[0]) <= 5.0 and abs(flows[1, 1] - scene.V_PATCH[1]) <= 5.0, flows


def test_cli_objects_on_the_scene(sc, tmp_path):
    """bf_motion_compensator --objects=2 on the scene written as an event file: one slice, two groups, and the patch's group
    moves with the patch's velocity to within 5 px/s."""
    from better_flow_amd import synth
    exe = os.path.join(ROOT, "better_flow_amd", "host", "bf_motion_compensator")
    txt, out = str(tmp_path / "scene.txt"), tmp_path / "out"
    out.mkdir()
    synth.write_txt(txt, sc)
    r = subprocess.run([exe, "--objects=2", "--res-x=%d" % H, "--res-y=%d" % W, "--quiet", "--img-prefix",
                        str(out), txt], cwd=str(out), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert sorted(os.listdir(str(out))) == ["objects_0.txt"]
    lines = open(str(out / "objects_0.txt")).read().splitlines()
    print("\n".join(lines))
    assert len(lines) == 3 and lines[2].split()[0] == "unassigned"
    groups = [ln.split() for ln in lines[:2]]
    assert [g[0] for g in groups] == ["0", "1"] and all(len(g) == 16 for g in groups)
    assert sum(int(g[1]) for g in groups) + int(lines[2].split()[1]) == len(sc["t"])
    patch = min(groups, key=lambda g: abs(float(g[2]) - scene.V_PATCH[0]) + abs(float(g[3]) - scene.V_PATCH[1]))
    assert abs(float(patch[2]) - scene.V_PATCH[0]) <= 5.0 and abs(float(patch[3]) - scene.V_PATCH[1]) <= 5.0, patch
    assert int(patch[1]) >= 0.99 * int(sc["is_patch"].sum())

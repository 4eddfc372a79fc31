"""bf_set_groups / bf_set_groups_from_segments / bf_run_groups on the MI355X (csrc/bf_tiles.hip: the keyed counting sort, the
group boxes, k_group_optimizer) against the tile grid's bytes and against tests/groups_ref.py, the restatement on the CPU
oracle.

Bars.  Where two device computations must be the same function of a group's event set (tile ids as groups, permuted
numbering, other groups dropped, ids from the device's own segmentation or from the host, two runs of one call): equal bytes.
Against the oracle: the first bar of test_gpu_config4.agrees only -- iteration count within +-1, per-event flow within
max(1e-4 relative, 0.02 px/s), widened by the oracle's own last step when the counts differ; tests/test_groups_cpu.py shows
the scene's groups are order-stable in the oracle, so no permutation fallback.  set_model's warp alone: 1 ulp of nx, ny."""
import os
import subprocess

import numpy as np
import pytest

import groups_ref as gr
import segment_scene as scene
from better_flow_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W = scene.H, scene.W
GUARD = (90, 120)
HARD_CAP = 20000


def fields(s):
    """A ctypes struct's fields as bytes (no padding; NaN-safe)."""
    return np.array([getattr(s, k) for k, _ in s._fields_ if not k.startswith("_")], dtype=np.float64).tobytes()


def make_acc(accel_mod, n, scale=3):
    return accel_mod.Accel(device=0, max_events=max(n, 1), max_rows=scale * H + scale, max_cols=scale * W + scale)


def upload(acc, sl):
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])


@pytest.fixture(scope="module")
def sc():
    return scene.make()


@pytest.fixture(scope="module")
def scene_acc(accel_mod, sc):
    a = make_acc(accel_mod, len(sc["t"]))
    yield a
    a.close()


def seeded_models(K):
    """Model 0 the background's; the others seeded non-zero totals about a centre inside the sensor."""
    rng = np.random.default_rng(5)
    out = [gr.background_model()]
    for _ in range(1, K):
        m = gr.oracle.Model()
        m.cx, m.cy = rng.uniform(20, 70), rng.uniform(20, 100)
        m.total_dx, m.total_dy = rng.uniform(-0.3, 0.3, 2)
        m.total_rot, m.total_div = rng.uniform(-2e-3, 2e-3, 2)
        out.append(m)
    return out


def to_accel(accel_mod, warm):
    if warm is None:
        return None
    one = lambda m: accel_mod.Model(**{k: getattr(m, k) for k, _ in gr.oracle.Model._fields_})
    return [one(m) for m in warm] if isinstance(warm, list) else one(warm)


def check_against_ref(sl, gid, K, scale, min_events, warm, infos, u, v, what, groups=None, guard=GUARD):
    """The first bar of test_gpu_config4.agrees for every group of one run_groups call."""
    res, _, _, ou, ov = gr.solve(sl, gid, K, scale, (H, W), guard, min_events, warm=warm, hard_cap=HARD_CAP)
    worst = 0.0
    for g, r in enumerate(res):
        idx = r.idx
        git = infos[g].iterations
        print("%s group %d: %d events, rc %d / %d, iterations %d / %d" % (what, g, r.events, infos[g].rc, r.rc, git, r.iterations))
        assert infos[g].rc == r.rc, (what, g)
        if groups is not None:
            q = groups[g]
            assert (q.events, q.row_min, q.row_max, q.col_min, q.col_max, q.rows, q.cols) == r.box, (what, g)
        if r.rc != 0:
            continue
        assert abs(git - r.iterations) <= 1, (what, g, git, r.iterations)
        tol_u, tol_v = np.maximum(1e-4 * np.abs(ou[idx]), 0.02), np.maximum(1e-4 * np.abs(ov[idx]), 0.02)
        if git != r.iterations and r.iterations >= 3:   # max_iter = K runs K + 1 iterations
            one = np.where(gid == g, 0, -1)
            w1 = warm[g] if isinstance(warm, list) else warm
            r1, _, _, u1, v1 = gr.solve(sl, one, 1, scale, (H, W), guard, min_events, warm=w1, hard_cap=HARD_CAP,
                                        max_iter=r.iterations - 2)
            assert r1[0].iterations == r.iterations - 1
            tol_u, tol_v = tol_u + np.abs(ou[idx] - u1[idx]).max(), tol_v + np.abs(ov[idx] - v1[idx]).max()
        du, dv = np.abs(u[idx] - ou[idx]), np.abs(v[idx] - ov[idx])
        print("   flow deviation %.3e / %.3e px/s" % (du.max(), dv.max()))
        worst = max(worst, du.max(), dv.max())
        assert np.all(du <= tol_u) and np.all(dv <= tol_v), (what, g, du.max(), dv.max())
    rest = np.flatnonzero(np.asarray(gid) < 0)
    assert not u[rest].any() and not v[rest].any(), what
    return res, worst


# ---- 1. the same bits as the tile grid ----

def test_tile_ids_as_groups_are_the_tile_grids_bytes(accel_mod):
    GR, GC, S, ME = 6, 8, 3, 256
    sl = synth.make_slice(60000, H, W, 0.030, seed=1)
    n = len(sl["t"])
    tid = (np.minimum(sl["fr_x"].astype(np.int64) * GR // H, GR - 1) * GC +
           np.minimum(sl["fr_y"].astype(np.int64) * GC // W, GC - 1)).astype(np.int32)
    K = GR * GC
    guard = (H // GR, W // GC)
    a = make_acc(accel_mod, n)
    upload(a, sl)
    tm, ti = a.run_tiles(GR, GC, S, (H, W), guard, min_events=ME, hard_iter_cap=HARD_CAP)
    tu, tv = a.compute_uv()
    assert sum(1 for i in ti if i.rc == 0) >= K // 2, "most tiles must run"

    def groups(gid):
        upload(a, sl)
        a.set_groups(gid, K)
        m, i, q = a.run_groups(K, S, (H, W), guard, ME, hard_iter_cap=HARD_CAP)
        u, v = a.compute_uv()
        return m, i, q, u, v

    m, i, q, u, v = groups(tid)
    for k in range(K):
        assert fields(m[k]) == fields(tm[k]) and fields(i[k]) == fields(ti[k]), k
        assert q[k].events == int((tid == k).sum())
    assert u.tobytes() == tu.tobytes() and v.tobytes() == tv.tobytes()
    # another numbering: the results permute, the bytes stay
    perm = np.random.default_rng(3).permutation(K).astype(np.int32)
    m2, i2, _, u2, v2 = groups(perm[tid])
    for k in range(K):
        assert fields(m2[perm[k]]) == fields(tm[k]) and fields(i2[perm[k]]) == fields(ti[k]), k
    assert u2.tobytes() == tu.tobytes() and v2.tobytes() == tv.tobytes()
    # half of the tiles in no group: the others keep their bytes, the dropped events read (0, 0)
    drop = (tid % 2) == 1
    m3, i3, q3, u3, v3 = groups(np.where(drop, -1, tid))
    for k in range(0, K, 2):
        assert fields(m3[k]) == fields(tm[k]) and fields(i3[k]) == fields(ti[k]), k
    for k in range(1, K, 2):
        assert q3[k].events == 0 and i3[k].rc == accel_mod.BF_SKIPPED and i3[k].iterations == 0
    assert u3[~drop].tobytes() == tu[~drop].tobytes() and v3[~drop].tobytes() == tv[~drop].tobytes()
    assert not u3[drop].any() and not v3[drop].any()
    a.close()


# ---- 2. the scene's four groups against the restatement ----

@pytest.fixture(scope="module")
def scene_runs(accel_mod, sc, scene_acc):
    """cold / one shared warm model / K warm models on the scene's four groups at scale 3: {name: (warm, models, infos,
    groups, u, v, nx, ny)}, computed once."""
    gid = gr.scene_groups(sc)
    a = scene_acc
    upload(a, sc)
    a.set_groups(gid, 4)
    out = {}
    for name, warm in (("cold", None), ("shared", gr.background_model()), ("each", seeded_models(4))):
        m, i, q = a.run_groups(4, 3, (H, W), GUARD, 100, warm=to_accel(accel_mod, warm), hard_iter_cap=HARD_CAP)
        u, v = a.compute_uv()
        _, _, nx, ny = a.writeout_events()
        out[name] = (warm, m, i, q, u, v, nx, ny)
    return gid, out


@pytest.mark.parametrize("name", ["cold", "shared", "each"])
def test_scene_groups_against_the_restatement(sc, scene_runs, name):
    gid, runs = scene_runs
    warm, m, i, q, u, v = runs[name][:6]
    res, worst = check_against_ref(sc, gid, 4, 3, 100, warm, i, u, v, name, groups=q)
    assert all(r.rc == 0 for r in res)
    print("%s: worst flow deviation %.3e px/s" % (name, worst))
    if name == "cold":
        mu = gr.median_flow(u, v, res[0].idx)
        assert abs(mu[0] - 400.0) < 1.0 and abs(mu[1] + 300.0) < 1.0, mu


# ---- 3. capacity and guards in one call ----

@pytest.mark.parametrize("name", ["cold", "shared"])
def test_capacity_and_guards_in_one_call(accel_mod, sc, scene_acc, scene_runs, name):
    _, runs = scene_runs
    warm, m4, i4, _, u4, v4 = runs[name][:6]
    bg = np.flatnonzero(~sc["is_patch"])
    gid = np.where(sc["is_patch"], 0, 1).astype(np.int32)
    gid[bg[:50]] = 2
    a = scene_acc
    upload(a, sc)
    a.set_groups(gid, 3)
    m, i, q = a.run_groups(3, 3, (H, W), GUARD, 100, warm=to_accel(accel_mod, warm), hard_iter_cap=HARD_CAP)   # BF_OK
    u, v = a.compute_uv()
    _, _, nx, ny = a.writeout_events()
    assert q[1].rows * q[1].cols * 16 > 156 * 1024 and q[1].events == len(bg) - 50
    assert i[1].rc == accel_mod.BF_ERR_CAPACITY and i[1].iterations == 0
    assert i[2].rc == accel_mod.BF_SKIPPED and i[2].iterations == 0 and q[2].events == 50
    # the patch: the same event set as group 0 of the four-group call, so the same bytes
    p = sc["is_patch"]
    assert i[0].rc == 0 and fields(m[0]) == fields(m4[0]) and fields(i[0]) == fields(i4[0])
    assert u[p].tobytes() == u4[p].tobytes() and v[p].tobytes() == v4[p].tobytes()
    if warm is None:
        assert not nx[~p].any() and not ny[~p].any() and not u[~p].any() and not v[~p].any()
    else:   # what set_model left, for the group that did not fit and for the one the guard skipped
        _, onx, ony, _, _ = gr.solve(sc, gid, 3, 3, (H, W), GUARD, 100, warm=warm, no_run=(0, 1, 2))
        for got, want in ((nx, onx), (ny, ony)):
            assert np.all(np.abs(got[~p] - want[~p]) <= np.spacing(np.abs(want[~p]))), np.abs(got[~p] - want[~p]).max()
        assert np.abs(onx[~p]).min() > 0.0
        assert fields(m[1]) == fields(to_accel(accel_mod, warm))   # the model set_model installed


# ---- 4. groups from the device's own segmentation ----

def test_groups_from_the_segmentation(accel_mod, sc, scene_acc):
    a = scene_acc
    upload(a, sc)
    a.set_cloud(scene.SCALE, H, W)
    nx, ny = scene.flow_of(scene.V_BACKGROUND)
    a.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
    a.segment(**scene.OPTS)
    _, _, cl = a.segment_get()
    assert a.set_groups_from_segments() == 1
    b = make_acc(accel_mod, len(sc["t"]))
    upload(b, sc)
    b.set_groups(cl, 1)
    first = True
    for warm in (None, gr.background_model()):
        w = to_accel(accel_mod, warm)
        ra = a.run_groups(1, scene.SCALE, (H, W), GUARD, 100, warm=w, hard_iter_cap=HARD_CAP)
        ua, va = a.compute_uv()
        rb = b.run_groups(1, scene.SCALE, (H, W), GUARD, 100, warm=w, hard_iter_cap=HARD_CAP)
        ub, vb = b.compute_uv()
        for x, y in zip(ra, rb):
            assert fields(x[0]) == fields(y[0])
        assert ua.tobytes() == ub.tobytes() and va.tobytes() == vb.tobytes()
        check_against_ref(sc, cl, 1, scene.SCALE, 100, warm, ra[1], ua, va, "segments " + ("warm" if warm else "cold"), groups=ra[2])
        if first:
            first = False
            keep = (fields(ra[0][0]), fields(ra[1][0]), ua.tobytes(), va.tobytes())
            assert ra[1][0].iterations == 1 and not ua.any() and not va.any()   # (the finding of DESIGN section 14)
    # a warp invalidates the segmentation, not the grouping
    upload(a, sc)
    a.set_cloud(scene.SCALE, H, W)
    a.project_4param_reinit(nx, ny, 0.0, 0.0, 0.0, 0.0)
    a.segment(**scene.OPTS)
    assert a.set_groups_from_segments() == 1
    a.project_4param_reinit(0.1, 0.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(accel_mod.BfError) as e:
        a.segment_get()
    assert e.value.code == accel_mod.BF_ERR_STATE
    with pytest.raises(accel_mod.BfError) as e:
        a.set_groups_from_segments()
    assert e.value.code == accel_mod.BF_ERR_STATE
    ra = a.run_groups(1, scene.SCALE, (H, W), GUARD, 100, hard_iter_cap=HARD_CAP)
    ua, va = a.compute_uv()
    assert (fields(ra[0][0]), fields(ra[1][0]), ua.tobytes(), va.tobytes()) == keep
    b.close()


# ---- 5. edges ----

def test_edges_states_and_arguments(accel_mod):
    sl = synth.make_slice(3000, H, W, 0.030, seed=2)
    n = len(sl["t"])
    a = make_acc(accel_mod, n)

    def raises(code, f, *args, **kw):
        with pytest.raises(accel_mod.BfError) as e:
            f(*args, **kw)
        assert e.value.code == code, (e.value.code, code)

    run = lambda K, **kw: a.run_groups(K, 1, (H, W), GUARD, 100, hard_iter_cap=HARD_CAP, **kw)   # (scale 1: half a sensor fits the LDS)
    raises(accel_mod.BF_ERR_STATE, a.set_groups, np.zeros(n, dtype=np.int32), 1)       # before an upload
    raises(accel_mod.BF_ERR_STATE, run, 1)
    upload(a, sl)
    raises(accel_mod.BF_ERR_STATE, run, 1)                                              # no grouping yet
    raises(accel_mod.BF_ERR_STATE, a.set_groups_from_segments)                          # no segmentation held
    # K = 0
    a.set_groups(np.full(n, -1, dtype=np.int32), 0)
    m, i, q = run(0)
    u, v = a.compute_uv()
    assert m == [] and i == [] and not u.any() and not v.any()
    # every id -1 with K = 2; an empty group in the middle; a group of one event
    a.set_groups(np.full(n, -1, dtype=np.int32), 2)
    m, i, q = run(2)
    assert [x.rc for x in i] == [accel_mod.BF_SKIPPED] * 2 and [x.events for x in q] == [0, 0] and not a.compute_uv()[0].any()
    gid = np.where(sl["fr_x"] < 45, 0, 2).astype(np.int32)
    gid[7] = 3
    a.set_groups(gid, 4)
    m, i, q = run(4)
    u, v = a.compute_uv()
    assert [x.events for x in q] == [int((gid == g).sum()) for g in range(4)] and q[1].events == 0 and q[3].events == 1
    assert i[1].rc == accel_mod.BF_SKIPPED and i[3].rc == accel_mod.BF_SKIPPED and u[7] == 0.0 and v[7] == 0.0
    check_against_ref(sl, gid, 4, 1, 100, None, i, u, v, "edges", groups=q)
    assert i[0].rc == 0 and i[2].rc == 0
    # the same call twice: the same bytes
    m2, i2, _ = run(4)
    u2, v2 = a.compute_uv()
    assert all(fields(x) == fields(y) for x, y in zip(m + i, m2 + i2)) and u2.tobytes() == u.tobytes() and v2.tobytes() == v.tobytes()
    # arguments
    bad = gid.copy()
    bad[11] = 4
    raises(accel_mod.BF_ERR_ARG, a.set_groups, bad, 4)                                  # id = K
    bad[11] = -2
    raises(accel_mod.BF_ERR_ARG, a.set_groups, bad, 4)
    raises(accel_mod.BF_ERR_CAPACITY, a.set_groups, gid, 16384)                         # K + 1 buckets
    a.set_groups(gid, 4)
    raises(accel_mod.BF_ERR_ARG, run, 4, warm=[accel_mod.Model()] * 2)                  # 2 warm models for 4 groups
    # a fresh upload ends the grouping
    upload(a, sl)
    raises(accel_mod.BF_ERR_STATE, run, 4)
    # a noise mask
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"], noise=np.zeros(n, dtype=np.uint8))
    a.set_groups(gid, 4)
    raises(accel_mod.BF_ERR_ARG, run, 4)
    # fewer events than one work-group has threads
    near = np.flatnonzero((sl["fr_x"] < 30) & (sl["fr_y"] < 35))[:100]
    assert len(near) == 100
    few = {k: sl[k][near] for k in ("fr_x", "fr_y", "t")}
    upload(a, few)
    g = np.zeros(100, dtype=np.int32)
    a.set_groups(g, 1)
    m, i, q = a.run_groups(1, 3, (H, W), (15, 15), 20, hard_iter_cap=HARD_CAP)
    u, v = a.compute_uv()
    check_against_ref(few, g, 1, 3, 20, None, i, u, v, "100 events", groups=q, guard=(15, 15))
    assert i[0].rc == 0
    a.close()


# ---- 6. bf::ObjectTasks: the device path ----

@pytest.mark.parametrize("name", ["cold", "each"])
def test_object_tasks_device_path_equals_run_groups(accel_mod, sc, scene_runs, tmp_path, name):
    """tests/cpp/test_object_tasks.cpp linked against the product library: the models, return codes, iteration counts and (nx, ny)
    of Accel.run_groups on the scene's four groups (tests/test_groups_cpu.py holds the host path to the restatement)."""
    import test_groups_cpu as cpu
    gid, runs = scene_runs
    warm, m, i, _, _, _, nx, ny = runs[name]
    host = os.path.join(ROOT, "better_flow_amd", "host")
    exe = str(tmp_path / "test_object_tasks")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-pthread", "-ffp-contract=off", "-I" + host, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_object_tasks.cpp"), "-L" + os.path.join(ROOT, "better_flow_amd"),
                           "-lbf_accel", "-Wl,-rpath," + os.path.join(ROOT, "better_flow_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ev = str(tmp_path / "events.txt")
    cpu.write_events(ev, sc, gid)
    arg = "-"
    if warm is not None:
        arg = str(tmp_path / "warm.bin")
        cpu.write_models(arg, warm)
    prefix = str(tmp_path / "out_")
    r = subprocess.run([exe, ev, "4", "3", str(H), str(W), str(GUARD[0]), str(GUARD[1]), "100", str(HARD_CAP), arg, prefix],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout.decode().splitlines()[0] == "path device"
    models, infos, onx, ony = cpu.read_outputs(prefix, 4, len(gid))
    for k in range(4):
        assert fields(models[k]) == fields(m[k]), k
        assert (int(infos[k, 0]), int(infos[k, 1])) == (i[k].rc, i[k].iterations), k
    assert onx.tobytes() == nx.tobytes() and ony.tobytes() == ny.tobytes()

"""The held flow of a grouping and its per-group medians on the CPU: the symbols and their binding, the restatement
(tests/hold_groups_ref.py) on the two-motion scene with project_groups_ref.scene_truth, the median's rules on hand-made cases,
its agreement with bf::ObjectFinder::group_flows' formula, and mutations of the restatement's rules, each of which changes a
result."""
import ctypes

import numpy as np
import pytest

import global_flow_ref as R
import hold_groups_ref as hg
import project_groups_ref as pr
import segment_scene as scene


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
def held(sc, truth):
    h = hg.hold(sc, *truth)
    for v in h.values():
        v.setflags(write=False)
    return h


def test_symbols_exported_and_bound():
    from better_flow_amd import accel
    lib = ctypes.CDLL(accel.LIB_PATH)
    for name in ("bf_hold_groups", "bf_group_flow_medians"):
        assert name in accel.EXPORTS and hasattr(lib, name), name
    assert callable(accel.Accel.hold_groups) and callable(accel.Accel.group_flow_medians)


def test_scene_medians_are_the_truth_flows(sc, truth, held):
    ids = truth[0]
    um, vm, counts = hg.medians(held["u"], held["v"], ids, 2)
    print("medians: background (%.6f, %.6f), patch (%.6f, %.6f); counts %s" % (um[0], vm[0], um[1], vm[1], counts.tolist()))
    assert counts.tolist() == [int((ids == 0).sum()), int((ids == 1).sum()), 0]
    assert np.hypot(um[1] - scene.V_PATCH[0], vm[1] - scene.V_PATCH[1]) <= 5.0          # the bar of DESIGN section 15
    assert np.hypot(um[0] - scene.V_BACKGROUND[0], vm[0] - scene.V_BACKGROUND[1]) <= 5.0
    assert np.array_equal(ids == 1, sc["is_patch"])


def test_a_pure_translation_group_has_one_flow(truth, held):
    ids = truth[0]
    for k in range(2):
        for key in ("nx", "ny", "u", "v"):
            assert len(np.unique(_bits(held[key][ids == k]))) == 1, (k, key)
    assert _bits(held["u"][ids == 0][0]) != _bits(held["u"][ids == 1][0])
    # the positions still differ per event: pr = fr - (k * t) / 10000
    assert len(np.unique(held["pr_x"][ids == 1])) > 1


def test_ids_of_minus_one_are_zero_flow_at_their_own_pixel(sc, truth):
    ids = truth[0].copy()
    ids[::7] = -1
    h = hg.hold(sc, ids, truth[1])
    none = ids < 0
    for key in ("nx", "ny", "u", "v"):
        assert not h[key][none].any(), key
    assert np.array_equal(h["pr_x"][none], sc["fr_x"][none].astype(np.float64))
    assert np.array_equal(h["pr_y"][none], sc["fr_y"][none].astype(np.float64))
    assert h["u"][~none].all()
    _, _, counts = hg.medians(h["u"], h["v"], ids, 2)
    assert counts[2] == int(none.sum()) and counts.sum() == len(ids)


def test_median_rules():
    assert hg.median([]) == 0.0 and _bits(hg.median([]))[0] == 0
    assert hg.median([7.5]) == 7.5
    assert hg.median([3.0, 1.0, 2.0]) == 2.0                                  # odd: element c / 2
    assert hg.median([4.0, 1.0, 3.0, 2.0]) == 2.5                             # even: the mean of the two middles
    assert hg.median([5.0, 1.0, 5.0, 9.0]) == 5.0                             # equal middles
    a = np.nextafter(1.0, 2.0)
    assert _bits(hg.median([0.0, 1.0, a, 2.0]))[0] == _bits(0.5 * (1.0 + a))[0]
    # the key order puts -0.0 below +0.0: an odd count whose middle is a zero names WHICH zero
    assert _bits(hg.median([-0.0, 0.0, 0.0]))[0] == _bits(0.0)[0]
    assert _bits(hg.median([-0.0, -0.0, 0.0]))[0] == _bits(-0.0)[0]
    assert _bits(hg.median([0.0, -1.0, -0.0]))[0] == _bits(-0.0)[0]
    assert _bits(hg.median([-0.0, 0.0]))[0] == _bits(0.0)[0]                  # 0.5 * (-0 + +0) = +0
    assert hg.median([-3.0, -1.0, -2.0, -7.0]) == -2.5                        # all negative: reversed bit order
    k = hg.key(np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf]))
    assert (np.diff(k.astype(object)) > 0).all()
    x = np.random.default_rng(3).normal(size=101)
    assert np.array_equal(_bits(hg.unkey(hg.key(x))), _bits(x))
    for c in (100, 101):
        assert _bits(hg.median(x[:c]))[0] == _bits(np.median(x[:c]))[0]


def test_median_is_the_object_finders_formula(sc, truth, held):
    """bf::ObjectFinder::group_flows: std::sort and the mean of the two middles, on the same host (u, v)."""
    ids = truth[0]
    rng = np.random.default_rng(5)
    for u in (held["u"], held["v"], rng.normal(size=len(ids)) * 300.0):
        for k in range(2):
            vals = u[ids == k]
            for c in (len(vals), len(vals) - 1):
                assert _bits(hg.median(vals[:c]))[0] == _bits(hg.finder_median(vals[:c]))[0], (k, c)


def test_mutations_each_change_a_result(sc, truth, held):
    ids, ms = truth
    assert not np.array_equal(hg.hold(sc, ids, ms, mutate="model0")["u"], held["u"])
    four = np.array([1.0, 2.0, 4.0, 8.0])
    assert hg.median(four, mutate="upper") == 4.0 != hg.median(four)
    some = ids.copy()
    some[::3] = -1
    h = hg.hold(sc, some, ms)
    plain = hg.medians(h["u"], h["v"], some, 2)
    mutant_h = hg.hold(sc, some, ms, mutate="minus_one_in_0")
    assert not np.array_equal(mutant_h["u"], h["u"])                          # the -1 events took group 0's flow
    mutant = hg.medians(h["u"], h["v"], some, 2, mutate="minus_one_in_0")
    assert mutant[2].tolist() != plain[2].tolist()
    # with -1 in the majority their zero flow becomes group 0's median
    most = ids.copy()
    most[sc["is_patch"] == 0] = -1
    most[np.nonzero(ids == 0)[0][:100]] = 0
    h = hg.hold(sc, most, ms)
    assert hg.medians(h["u"], h["v"], most, 2)[0][0] != 0.0 == hg.medians(h["u"], h["v"], most, 2, mutate="minus_one_in_0")[0][0]


def test_uv_is_the_host_compute_uv_of_n(held):
    u, v = R.event_uv(held["nx"][:50], held["ny"][:50], hg.NZ)
    assert np.array_equal(_bits(u), _bits(held["u"][:50])) and np.array_equal(_bits(v), _bits(held["v"][:50]))

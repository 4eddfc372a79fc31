"""The coarse-to-fine / seeded per-cell search, restated (tests/global_pyramid_ref.py): the level schedule on hand-made
cell bests, the evaluation order, and on small slices the pyramid's S(k, cell) against the exhaustive restatement
(tests/global_cells_ref.py).  No GPU."""
import numpy as np
import pytest

import global_cells_ref as GC
import global_pyramid_ref as P
import global_ref as G
from better_flow_amd import synth


def test_strides_and_strided_level():
    assert P.strides(1, 2) == [1] and P.strides(3, 4) == [16, 4, 1] and P.strides(2, 3) == [3, 1]
    # 7 x 5 lattice, stride 3 (neither size a multiple): i in {0, 3, 6}, j in {0, 3}
    assert P.strided_level(7, 5, 3) == [0, 3, 15, 18, 30, 33]
    assert P.strided_level(7, 5, 1) == list(range(35))                     # levels = 1: the lattice in sweep order


def test_centres_rule():
    events = np.array([5, 0, 5, 5, 5, 5])
    best_sum = np.array([9, 9, 0, 0, 0, 7])
    best_k = np.array([12, 12, 3, 3, 3, 20])
    # no seeds: a cell with events and S > 0 only
    assert P.centres(events, best_sum, best_k, None) == [12, None, None, None, None, 20]
    # seeds: the running best wins where S > 0, an empty cell stays out, -1 is no seed
    seeds = np.array([1, 1, 8, -1, 0, -1])
    assert P.centres(events, best_sum, best_k, seeds) == [12, None, 8, None, 0, 20]


def test_window_clipped_at_all_four_edges():
    n_x, n_y = 6, 5

    def win(i, j, s, r, done=()):
        return P.window_level(n_x, n_y, s, r, [i * n_y + j], set(done))

    assert win(0, 0, 1, 1) == [0, 1, 5, 6]                                  # top-left corner
    assert win(5, 4, 1, 1) == [23, 24, 28, 29]                              # bottom-right corner
    assert win(0, 2, 2, 1) == [0, 2, 4, 10, 12, 14]                         # top edge, stride 2
    assert win(3, 4, 2, 1) == [7, 9, 17, 19, 27, 29]                        # right edge: j = 2, 4; i = 1, 3, 5
    assert win(2, 2, 1, 1) == [6, 7, 8, 11, 12, 13, 16, 17, 18]             # interior: the full 3 x 3
    assert len(win(2, 2, 1, 3)) == 30                                       # radius beyond every edge: the whole lattice
    assert win(2, 2, 1, 1, done=[12, 6]) == [7, 8, 11, 13, 16, 17, 18]      # minus what was evaluated


def test_overlapping_windows_have_no_duplicates_and_ascend():
    n_x, n_y = 8, 8
    a, b = 3 * 8 + 3, 3 * 8 + 4                                             # neighbours: 6 of 9 points shared
    ks = P.window_level(n_x, n_y, 1, 1, [a, None, b, a], set())
    assert ks == sorted(set(ks)) and len(ks) == 12
    assert P.window_level(n_x, n_y, 1, 1, [None, None], set()) == []


class _FakeCells:
    """hand-made S(k, cell): a peak per cell on a 9 x 7 lattice, no events needed"""

    def __init__(self, events, peaks, n_y):
        self.events = np.asarray(events, dtype=np.int64)
        self.n_cells, self.n_cell_x, self.n_cell_y = len(events), 1, len(events)
        self.peaks, self.n_y = peaks, n_y

    def score(self, k):
        i, j = divmod(k, self.n_y)
        out = np.zeros(self.n_cells, dtype=np.int64)
        for c, p in enumerate(self.peaks):
            if p is not None and self.events[c]:
                out[c] = max(0, 100 - 10 * (abs(i - p[0]) + abs(j - p[1])))
        return out


def test_schedule_on_hand_made_bests():
    xs, ys = list(range(9)), list(range(7))
    # cell 0 peaks at (8, 6), the far corner; cell 1 at (3, 3); cell 2 has no events; cell 3 scores 0 everywhere
    fake = _FakeCells([4, 4, 0, 4], [(8, 6), (3, 3), (1, 1), None], 7)
    out = P.search_pyramid(fake, xs, ys, 3, 2, 1, score=fake.score)
    ev = out["evaluated"]
    lc = out["level_count"]
    assert lc[0] == 3 * 2 and sum(lc) == len(ev) == len(set(ev))            # stride 4: i in {0, 4, 8}, j in {0, 4}
    at = 0
    for n in lc:                                                            # ascending inside every level
        assert ev[at:at + n] == sorted(ev[at:at + n])
        at += n
    # level 1 (stride 2): windows around cell 0's (8, 4) -- clipped at the bottom edge -- and cell 1's (4, 4); cells 2 and 3
    # contribute nothing
    l1 = ev[lc[0]:lc[0] + lc[1]]
    want = {i * 7 + j for i in (6, 8) for j in (2, 4, 6)} | {i * 7 + j for i in (2, 4, 6) for j in (2, 4, 6)}
    assert set(l1) == want - set(ev[:lc[0]])
    assert list(out["cells"]["best_index"].ravel()[:2]) == [8 * 7 + 6, 3 * 7 + 3]
    # an empty cell and an all-zero cell answer with the lowest evaluated k
    assert list(out["cells"]["best_index"].ravel()[2:]) == [0, 0] and not out["cells"]["best_sum"].ravel()[2:].any()
    # seeded: no strided pass; a seed of -1 and an empty cell contribute nothing
    out = P.search_pyramid(fake, xs, ys, 1, 2, 1, seeds=[8 * 7 + 6, -1, 10, -1], score=fake.score)
    assert out["evaluated"] == [7 * 7 + 5, 7 * 7 + 6, 8 * 7 + 5, 8 * 7 + 6] and out["level_count"] == [4]
    assert list(out["cells"]["best_index"].ravel()) == [8 * 7 + 6, 7 * 7 + 5, 7 * 7 + 5, 7 * 7 + 5]
    # a zero-scoring cell keeps its seed as the centre on every level
    out = P.search_pyramid(fake, xs, ys, 2, 2, 1, seeds=[-1, -1, -1, 3 * 7 + 3], score=fake.score)
    lvl0 = {i * 7 + j for i in (1, 3, 5) for j in (1, 3, 5)}                # stride 2 around the one seed
    assert set(out["evaluated"][:9]) == lvl0
    # level 1: cell 0's best of level 0 is (5, 5), cell 1's is (3, 3), cell 3 (all zero) stays on its seed (3, 3)
    lvl1 = {i * 7 + j for i in (4, 5, 6) for j in (4, 5, 6)} | {i * 7 + j for i in (2, 3, 4) for j in (2, 3, 4)}
    assert set(out["evaluated"][9:]) == lvl1 - lvl0 and out["level_count"] == [9, 15]
    with pytest.raises(AssertionError):
        P.search_pyramid(fake, xs, ys, 1, 2, 1, seeds=[-1, -1, 5, -1], score=fake.score)   # nothing to evaluate


def test_answer_rule_does_not_depend_on_level_order():
    assert P.answer([5, 3, 9], [7, 7, 2]) == 1                              # equal values: the lowest k
    assert P.answer([5, 3, 9], [0, 0, 0]) == 1
    run = P.Running(2)
    for k, S in ((9, [4, 0]), (2, [4, 0]), (5, [3, 0])):
        run.fold(k, np.array(S))
    assert list(run.best_k) == [2, 2] and list(run.best_sum) == [4, 0]


def _small_slice():
    sl = synth.make_slice(1500, 24, 32, 0.05, seed=4, velocity=(30.0, -20.0))
    return sl["fr_x"].astype(np.int64), sl["fr_y"].astype(np.int64), sl["t"].astype(np.int64)


def test_pyramid_values_are_entries_of_the_exhaustive_surface():
    ev = _small_slice()
    xs, ys = G.sweep_values(-0.006, 0.0065, 0.001), G.sweep_values(-0.004, 0.0045, 0.001)   # 13 x 9
    full = GC.GlobalCells(*ev, 24, 32, 12, 16, scale=3, metric_wsize=15)
    fsurf, fcells, fbest = full.search_cells(xs, ys)
    flat = fsurf.reshape(full.n_cells, -1)
    # levels = 1: the whole lattice in sweep order, every output of the exhaustive restatement
    ref = GC.GlobalCells(*ev, 24, 32, 12, 16, scale=3, metric_wsize=15)
    one = P.search_pyramid(ref, xs, ys, 1, 2, 1)
    assert one["evaluated"] == list(range(len(xs) * len(ys))) and np.array_equal(one["surface"], flat)
    for k in GC.CELL_FIELDS:
        assert np.array_equal(one["cells"][k], fcells[k]), k
    assert one["slice"] == fbest
    for k in ("max_score", "best_nx", "best_ny", "best_pr_x", "best_pr_y"):
        assert np.array_equal(getattr(ref, k), getattr(full, k)), k
    for levels, factor, radius in ((2, 2, 1), (3, 2, 1), (2, 4, 2)):
        ref = GC.GlobalCells(*ev, 24, 32, 12, 16, scale=3, metric_wsize=15)
        out = P.search_pyramid(ref, xs, ys, levels, factor, radius)
        e = out["evaluated"]
        assert len(e) == len(set(e)) < len(xs) * len(ys)
        assert np.array_equal(out["surface"], flat[:, e])                   # bit for bit the exhaustive entries
        bs = out["cells"]["best_sum"].ravel()
        assert (bs <= fcells["best_sum"].ravel()).all()
        # the exhaustive rule restricted to the evaluated set: largest value, lowest k among equals
        sub = flat[:, sorted(e)]
        assert np.array_equal(out["cells"]["best_index"].ravel(), np.array(sorted(e))[np.argmax(sub, axis=1)])
        assert np.array_equal(bs, sub.max(axis=1))


# The cheapest of the settings tried on the two-motion slice of DESIGN.md's "OptimizerGlobal" section for which all eight
# cells answer within 2 grid steps of the truth (scratch search over levels 2..3, factor 2..8, radius 1..4; the table is in
# DESIGN.md).
RECOVERY_SETTING = dict(levels=3, factor=4, radius=2)


def recovery_case():
    """(events, xs, ys, grid arguments, window) of the recovery test, shared with the GPU test"""
    xs, ys = G.default_grid()
    return GC.two_motion_slice(), xs, ys, (64, 128, 32, 32), (3, 15)


def check_recovery(cells):
    tol = 2 * GC.GRID_STEP
    assert cells["best_u"].shape == (2, 4)
    for cx in range(2):
        for cy in range(4):
            tu, tv = GC.TWO_MOTION_TRUTH["left" if cy < 2 else "right"]
            u, v = cells["best_u"][cx, cy], cells["best_v"][cx, cy]
            print("cell %d: (%.2f, %.2f) px/s, truth (%g, %g)" % (cx * 4 + cy, u, v, tu, tv))
            assert abs(u - tu) <= tol and abs(v - tv) <= tol, (cx, cy, u, v)


_recovery_cache = {}


def recovery_reference():
    """the restatement's run of the committed setting, computed once per session"""
    if not _recovery_cache:
        ev, xs, ys, grid, (scale, mw) = recovery_case()
        ref = GC.GlobalCells(*ev, *grid, scale=scale, metric_wsize=mw)
        _recovery_cache["out"] = P.search_pyramid(ref, xs, ys, **RECOVERY_SETTING)
        _recovery_cache["ref"] = ref
    return _recovery_cache["ref"], _recovery_cache["out"]


def test_two_motions_recovered_by_the_committed_setting():
    _, out = recovery_reference()
    print("evaluated %d of 14400, per level %s" % (len(out["evaluated"]), out["level_count"]))
    assert len(out["evaluated"]) < 14400 // 10
    check_recovery(out["cells"])

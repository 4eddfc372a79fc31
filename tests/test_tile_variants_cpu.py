"""The rows of tests/tile_rows.py on the reference alone (no GPU): each row fits the tile kernels' LDS, gives the oracle enough
tiles to optimise, finite flow in all of them, and -- what lets tests/test_gpu_tile_variants.py hold EVERY tile to the oracle --
no tile whose oracle run depends on the order of its events beyond the project's flow bar (the reference's f32 running time sums
are order dependent, accel_lib.h:162; tests/test_gpu_config4.py meets tiles where a long loop amplifies that into other iteration
counts).  The local rows give every window more than the minimum of evaluations, and l7a has tiles on both sides of the window
kernel's register file.

Measured (tiles the oracle optimised / skipped, iterations, worst forward-vs-reversed flow deviation in px/s):
s1 62 / 2, max 2527, 2.2e-3; s5 62 / 2, max 315, 1.5e-5; s7 42 / 22, max 260, 2.9e-5; s9 40 / 24, max 196, 1.8e-2 (under the
0.02 px/s bar); stream 64 / 0, 19..31, 4.3e-5; g1600 1437 / 163, all 6, 1.6e-5; g16384 14935 / 1449, 2..4, 1.05e-2.  No tile
disagrees with its reversed run in any row.
"""
import numpy as np
import pytest

import tile_rows as tr


@pytest.mark.parametrize("rid", sorted(tr.ROLLING))
def test_rolling_row_qualifies_on_the_oracle(oracle_lib, rid):
    row = tr.Row(rid)
    assert row.max_px() * 16 <= tr.LDS_PLANE_BYTES, (rid, row.max_px())
    ran = skipped = disagree = 0
    worst = 0.0
    its, per_tile = [], []
    for k in range(row.nt):
        sel = row.sel(k)
        per_tile.append(len(sel))
        fwd = row.oracle(oracle_lib, sel)
        rc, it, u, v, _ = fwd
        assert rc in (0, 1), (rid, k, rc)
        if rc == 1:
            skipped += 1
            continue
        ran += 1
        its.append(it)
        assert np.isfinite(u).all() and np.isfinite(v).all(), (rid, k)
        agree, du, dv = tr.order_deviation(fwd, row.oracle(oracle_lib, sel[::-1]))
        disagree += not agree
        worst = max(worst, du, dv)
    print("%s: max_px %d, events per tile %d..%d; oracle ran %d tiles, skipped %d; iterations %d..%d; worst forward-vs-reversed "
          "deviation %.3e px/s; %d tiles disagree" % (rid, row.max_px(), min(per_tile), max(per_tile), ran, skipped, min(its), max(its),
                                                      worst, disagree))
    assert ran == tr.MIN_RAN[rid] if rid == "stream" else ran >= tr.MIN_RAN[rid], (rid, ran, skipped)
    assert disagree == 0, (rid, disagree)
    # what the row is in the table for
    if rid == "s5":
        assert row.max_px() == 9900
    if rid == "s7":
        assert min(per_tile) == 0                                  # tiles without events
    if rid == "stream":
        assert min(per_tile) < tr.TILE_REGISTER_EVENTS < max(per_tile) and max(its) == row.max_iter + 1   # (warps of streamed events)
    if rid == "g1600":
        assert row.nt == 1600
    if rid == "g16384":
        assert row.nt == 16384


def test_refused_row_is_over_the_lds_limit():
    """Row s9's scale on row s1's sensor and grid: the refusal tests/test_gpu_tile_variants.py asks of the library."""
    n, H, W, s, gr, gc = tr.ROLLING["s1"][:6]
    assert tr.max_px(H, W, tr.ROLLING["s9"][3], gr, gc) == 32076 and 32076 * 16 > tr.LDS_PLANE_BYTES


@pytest.mark.parametrize("rid", sorted(tr.LOCAL))
def test_local_row_qualifies_on_the_oracle(oracle_lib, rid):
    n, H, W, s, gr, gc, wsz, seed = tr.LOCAL[rid]
    assert s == 7
    sl = tr.local_slice(rid)
    order, bounds = tr.tile_order(sl, H, W, gr, gc)
    evals, per_tile = [], []
    for k in range(gr * gc):
        sel = order[bounds[k]:bounds[k + 1]]
        per_tile.append(len(sel))
        rc, st = tr.local_oracle(oracle_lib, rid, sl, sel, k)
        assert rc == 0 and st.evaluations > 19, (rid, k, rc, st.evaluations)
        evals.append(st.evaluations)
    print("%s: events per tile %d..%d, evaluations %d..%d" % (rid, min(per_tile), max(per_tile), min(evals), max(evals)))
    if rid == "l7a":
        assert min(per_tile) < tr.LOCAL_REGISTER_EVENTS < max(per_tile), (min(per_tile), max(per_tile))
        assert (s * wsz + s) ** 2 * 6 + 16 == 129670               # the window's LDS (bf_local.hip)
    if rid == "l7b":
        assert (H % gr != 0 or W % gc != 0) and gr != gc

"""Every compiled instantiation of the tile-grid optimizers (BASELINE config 4) and every path of the tile sort, each run once
against the oracle: what tests/test_gpu_variants.py is for the two-kernel loop.  The rows are tests/tile_rows.py's;
tests/test_tile_variants_cpu.py shows on the reference alone what each of them reaches.

bf_run_tiles, EVERY tile against its own oracle run.  Return code equal; a skipped tile's events have zero flow; iteration count
within +-1, and EQUAL where max_iter caps the run; per-event flow under test_gpu_config4.agrees' bar (1e-4 relative / 0.02 px/s,
widened by the oracle's own last step when the counts differ by one), widened further by the tile's own forward-vs-reversed
deviation of the ORACLE (tile_rows.order_deviation: how much of the answer the reference's order-dependent f32 time sums decide).
A tile that still fails may be matched by the oracle on the reversed order or one of 120 seeded permutations of its events, as in
test_config4_full_size_every_tile_against_its_oracle; the number of such tiles is printed and capped at ran // 50.

After two updates (max_iter = 1) the scale rows' tile models are held to the oracle's at the bars of test_gpu_variants.py /
test_gpu_borders.py (cnt equal, six fields within 3e-4 x max(1, |value|)): box sum, Scharr and moments per HS before a loop has
amplified anything.  bf_run_tiles_many must be the bytes of bf_run_tiles; two rows are run twice for repeatability; the scale-7
window grids must EQUAL the oracle; bad scales and a window beyond the LDS are refused on the host.
"""
import numpy as np
import pytest

import tile_rows as tr

pytestmark = pytest.mark.gpu

MODEL_FIELDS = ("cx", "cy", "dx", "dy", "rot", "div")


def make_acc(accel_mod, row, n=None, scale=None):
    s = row.scale if scale is None else scale
    return accel_mod.Accel(max_events=n or len(row.sl["t"]), max_rows=s * row.H + s, max_cols=s * row.W + s)


def run_row(acc, row, max_iter=None):
    sl = row.sl
    acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    models, infos = acc.run_tiles(row.gr, row.gc, row.scale, (row.H, row.W), row.guard, min_events=row.min_events,
                                  max_iter=row.max_iter if max_iter is None else max_iter, hard_iter_cap=row.hard_cap)
    u, v = acc.compute_uv()
    return models, infos, u, v


def canon(models, infos):
    """test_gpu_config4's: return code, iteration count, dividers and the model's bytes of every tile."""
    return [(i.rc, i.iterations, i.x_divider, i.y_divider, i.rot_divider, i.div_divider,
             tuple(np.float64(getattr(m, f)).tobytes() for f, _ in m._fields_ if f != "_pad")) for m, i in zip(models, infos)]


_SINGLE = {}


def single(accel_mod, rid, seed_offset=0):
    """bf_run_tiles on a row's slice alone in a fresh context, once per module: (row, canon, u bytes, v bytes)."""
    if (rid, seed_offset) not in _SINGLE:
        row = tr.Row(rid, seed_offset)
        acc = make_acc(accel_mod, row)
        try:
            models, infos, u, v = run_row(acc, row)
        finally:
            acc.close()
        _SINGLE[(rid, seed_offset)] = (row, canon(models, infos), u.tobytes(), v.tobytes())
    return _SINGLE[(rid, seed_offset)]


@pytest.mark.parametrize("rid", sorted(tr.ROLLING))
def test_tile_row_every_tile_against_its_oracle(oracle_lib, accel_mod, rid):
    row = tr.Row(rid)
    acc = make_acc(accel_mod, row)
    try:
        models, infos, u, v = run_row(acc, row)
        again = run_row(acc, row) if rid in ("stream", "g1600") else None   # (held to the first run below)
    finally:
        acc.close()
    cap = row.max_iter + 1 if row.max_iter >= 0 else None
    ran = skipped = second_bar = off_by_one = capped = 0
    worst = 0.0
    for k in range(row.nt):
        sel = row.sel(k)
        fwd = row.oracle(oracle_lib, sel)
        orc, oit = fwd[0], fwd[1]
        orc = accel_mod.BF_ERR_NOCONV if orc < 0 else orc
        assert infos[k].rc == orc, (rid, k, infos[k].rc, orc, len(sel))
        if orc == 1:
            skipped += 1
            assert infos[k].iterations == 0 and not u[sel].any() and not v[sel].any(), (rid, k)
            continue
        assert orc == 0, (rid, k, orc)   # (tile_variants_cpu: every tile of every row runs or is skipped)
        ran += 1
        git = infos[k].iterations
        if cap is not None and (oit == cap or git == cap):
            capped += 1
            assert git == oit, (rid, k, git, oit)
        off_by_one += git != oit
        _, du, dv = tr.order_deviation(fwd, row.oracle(oracle_lib, sel[::-1]))
        ok, _, dev = tr.agrees(oracle_lib, row, sel, u[sel], v[sel], git, widen=(du, dv), fwd=fwd)
        if ok:
            worst = max(worst, dev)
            continue
        rng = np.random.default_rng(1000 + k)
        hit = None
        for trial in range(121):
            perm = np.arange(len(sel))[::-1].copy() if trial == 0 else rng.permutation(len(sel))
            if tr.agrees(oracle_lib, row, sel[perm], u[sel][perm], v[sel][perm], git)[0]:
                hit = trial
                break
        assert hit is not None, \
            "%s tile %d: GPU %d iterations, oracle %d (upload order), flow off by %.3e px/s (the oracle's own orders differ by %.3e) " \
            "-- and no permutation of the tile's events makes the oracle agree" % (rid, k, git, oit, dev, max(du, dv))
        second_bar += 1
    print("tile row %s (scale %d, %d x %d tiles): %d tiles ran / %d skipped; %d off by one iteration, %d at the iteration cap; worst "
          "flow deviation under the first bar %.3e px/s; %d tiles needed the permutation bar (cap %d)"
          % (rid, row.scale, row.gr, row.gc, ran, skipped, off_by_one, capped, worst, second_bar, ran // 50))
    assert ran == tr.MIN_RAN[rid] if rid == "stream" else ran >= tr.MIN_RAN[rid], (rid, ran, skipped)
    assert second_bar <= ran // 50, (rid, second_bar)
    if again is not None:   # repeatable bit for bit on the same context (integer accumulators, fixed reduction order)
        models2, infos2, u2, v2 = again
        assert canon(models, infos) == canon(models2, infos2), rid
        assert u.tobytes() == u2.tobytes() and v.tobytes() == v2.tobytes(), rid


@pytest.mark.parametrize("rid", tr.SCALE_ROWS)
def test_tile_models_after_two_updates(oracle_lib, accel_mod, rid):
    row = tr.Row(rid)
    acc = make_acc(accel_mod, row)
    try:
        models, infos, _, _ = run_row(acc, row, max_iter=1)
    finally:
        acc.close()
    ran = 0
    worst = 0.0
    for k in range(row.nt):
        orc, oit, _, _, om = row.oracle(oracle_lib, row.sel(k), max_iter=1)
        assert infos[k].rc == orc, (rid, k, infos[k].rc, orc)
        if orc != 0:
            continue
        ran += 1
        gm = models[k]
        assert infos[k].iterations == oit, (rid, k, infos[k].iterations, oit)
        assert gm.cnt == om.cnt, (rid, k, gm.cnt, om.cnt)
        for f in MODEL_FIELDS:
            a, b = getattr(om, f), getattr(gm, f)
            worst = max(worst, abs(a - b) / max(1.0, abs(a)))
            assert abs(a - b) <= 3e-4 * max(1.0, abs(a)), (rid, k, f, a, b)
    print("tile row %s after two updates: %d tiles, valid-pixel counts equal, worst model field deviation %.3e x max(1, |value|)"
          % (rid, ran, worst))
    assert ran >= tr.MIN_RAN[rid], (rid, ran)


@pytest.mark.parametrize("rid", tr.SCALE_ROWS)
def test_tiles_many_same_bits_as_tiles(accel_mod, rid):
    """K = 2 contexts -- the row's slice and the same row at seed + 1 -- in one bf_run_tiles_many launch, twice in a row."""
    singles = [single(accel_mod, rid, off) for off in (0, 1)]
    rows = [s[0] for s in singles]
    nmax = max(len(r.sl["t"]) for r in rows)
    accs = [make_acc(accel_mod, r, n=nmax) for r in rows]
    try:
        for rnd in range(2):
            for a, r in zip(accs, rows):
                a.upload_events(r.sl["fr_x"], r.sl["fr_y"], r.sl["t"])
            r0 = rows[0]
            out = accel_mod.run_tiles_many(accs, r0.gr, r0.gc, r0.scale, (r0.H, r0.W), r0.guard, min_events=r0.min_events,
                                           max_iter=r0.max_iter, hard_iter_cap=r0.hard_cap)
            for k, (a, (_, ref, ru, rv)) in enumerate(zip(accs, singles)):
                assert canon(*out[k]) == ref, (rid, rnd, k)
                u, v = a.compute_uv()
                assert u.tobytes() == ru and v.tobytes() == rv, (rid, rnd, k)
    finally:
        for a in accs:
            a.close()
    print("tile row %s: bf_run_tiles_many of 2 slices, twice: every tile the bytes of bf_run_tiles (%d + %d tiles ran)"
          % (rid, sum(c[0] == 0 for c in singles[0][1]), sum(c[0] == 0 for c in singles[1][1])))


@pytest.mark.parametrize("rid", sorted(tr.LOCAL))
def test_local_scale7_every_window_equals_its_oracle_run(oracle_lib, accel_mod, rid):
    n, H, W, s, gr, gc, wsz, seed = tr.LOCAL[rid]
    sl = tr.local_slice(rid)
    acc = accel_mod.Accel(max_events=len(sl["t"]), max_rows=s * H + s, max_cols=s * W + s)
    try:
        acc.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
        guard = (max(1, H // gr), max(1, W // gc))
        states, rcs = acc.local_run_tiles(gr, gc, s, wsz, (H, W), guard, max_evaluations=tr.LOCAL_MAX_EVALUATIONS)
    finally:
        acc.close()
    order, bounds = tr.tile_order(sl, H, W, gr, gc)
    evals = []
    for k in range(gr * gc):
        sel = order[bounds[k]:bounds[k + 1]]
        orc, ost = tr.local_oracle(oracle_lib, rid, sl, sel, k)
        orc = accel_mod.BF_ERR_NOCONV if orc < 0 else orc
        assert rcs[k] == orc, (rid, k, rcs[k], orc)
        for f in ("nx", "ny", "last_score", "dnx", "dny", "dn_th", "evaluations"):
            assert getattr(states[k], f) == getattr(ost, f), (rid, k, f, getattr(states[k], f), getattr(ost, f), len(sel))
        evals.append(states[k].evaluations)
    print("local row %s (scale %d, %d x %d windows of %d): every window equals its oracle run; evaluations %d..%d"
          % (rid, s, gr, gc, wsz, min(evals), max(evals)))
    assert min(evals) > 19


def test_tile_grid_refusals_leave_the_context_usable(accel_mod):
    """Even scales and scales above 9 are BF_ERR_ARG; a tile window beyond the LDS is BF_ERR_CAPACITY before anything is launched
    (row s9's scale on row s1's sensor and grid: max_px 32076) -- and the context then solves row s1 as a fresh one does."""
    row, ref, ru, rv = single(accel_mod, "s1")
    big = tr.ROLLING["s9"][3]
    acc = make_acc(accel_mod, row, scale=big)
    try:
        acc.upload_events(row.sl["fr_x"], row.sl["fr_y"], row.sl["t"])
        for scale, code in ((2, accel_mod.BF_ERR_ARG), (11, accel_mod.BF_ERR_ARG), (big, accel_mod.BF_ERR_CAPACITY)):
            with pytest.raises(accel_mod.BfError) as e:
                acc.run_tiles(row.gr, row.gc, scale, (row.H, row.W), row.guard, min_events=row.min_events, hard_iter_cap=row.hard_cap)
            assert e.value.code == code, (scale, e.value.code, str(e.value))
        models, infos, u, v = run_row(acc, row)
    finally:
        acc.close()
    assert canon(models, infos) == ref and u.tobytes() == ru and v.tobytes() == rv
    print("tile grid refusals: scale 2 and 11 BF_ERR_ARG, max_px 32076 BF_ERR_CAPACITY; row s1 afterwards the bytes of a fresh context")

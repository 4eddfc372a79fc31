"""The stencil kernel of the two-kernel loop (K3, bf_stencil.hip) takes its tiles in launch order (2-D launch) or, for the slab
formats of contexts that share the GPU (co_schedule: the update in K3's tail or in its own kernel), maps a 1-D launch id to a
tile (bf_rules::tile_of_block: work-groups b, b + 8, ... take one band of tile rows); event lists and the update at the scatter
head keep the launch order.  Here both orders are run on the smallest grids where an error in the map shows -- one tile,
fewer than 8 tiles, exactly 8, 8 k + 1 and 8 k + 7, one column, one row, ragged in both directions -- at scales 1, 3 and 5, with
the three scatter formats forced (dense slabs, event lists, own pixels + margin plane) and the update in each of its three
homes (the head of the scatter kernel, the last work-group of K3 under co_schedule, a kernel of its own), and held BIT FOR BIT
to the global-atomics loop on the same slice (binned = 0, fused = 0: no bins, no slabs, k_stencil<SRC> on a 2-D grid in launch
order), as tests/test_gpu_variants.py holds the compiled variants.

What is compared, over a cold run capped at 3 iterations: the return code, the iteration count, every trace record and the
returned model (bytes), the time and count image after the run, and the per-event flow.  The C-ABI does not hand out K3's time
tile, its Scharr gates or the fifteen words of the moment accumulators; they are held through the records: `cnt` of a record IS
the number of pixels that passed the gate in that iteration, cx / cy / dx / dy / rot / div are computed from the accumulator words
by the one update all loops share, and those words are exact integer sums (order-free), so a tile taken twice, a tile left out
or a tile read at the wrong place changes the bytes of the first record.  Every slice puts events -- and pixels that pass the
gate: solid 5 x 5 blocks on a lattice finer than a tile -- into every tile, and the reference run is asserted to have valid
pixels wherever the image is large enough to have a 3 x 3 neighbourhood.

Which form ran: bf_get_stat names the scatter format, K3's mode and whether the update sat at the scatter head.  Under co_schedule
no statistic tells the update in K3's tail from the update as its own kernel (the launch count of a run follows the polling
too); that home is held by the option being accepted -- bf_set_option fails on an unknown key or value -- as
tests/test_gpu_exact.py holds its unobservable forms.

Each slice has at most a few thousand events; a case takes milliseconds on the GPU."""
import numpy as np
import pytest

from test_gpu_variants import packed

ITER = 3
TRACE_CAP = ITER + 3

# name -> (sensor rows, sensor columns, scale, uniform events); the tile grid is ceil(scale rows / 16) x ceil(scale columns / 64)
SLICES = {
    "1x1_one_tile":        (1, 1, 1, 64),
    "2x5_one_tile":        (2, 5, 1, 200),
    "3x2_six_tiles":       (40, 100, 1, 2000),
    "4x2_eight_tiles":     (50, 70, 1, 2000),
    "3x3_nine_tiles_s3":   (16, 60, 3, 2000),
    "5x3_fifteen_tiles_s5": (15, 30, 5, 1500),
    "5x5_25_tiles_s3":     (25, 100, 3, 3000),
    "7x1_one_column_s3":   (37, 21, 3, 2000),
    "10x1_one_column":     (150, 40, 1, 2000),
    "1x10_one_row":        (12, 600, 1, 2000),
    "1x3_one_row_s5":      (3, 30, 5, 400),
}
GRIDS = {"1x1_one_tile": (1, 1), "2x5_one_tile": (1, 1), "3x2_six_tiles": (3, 2), "4x2_eight_tiles": (4, 2), "3x3_nine_tiles_s3": (3, 3),
         "5x3_fifteen_tiles_s5": (5, 3), "5x5_25_tiles_s3": (5, 5), "7x1_one_column_s3": (7, 1), "10x1_one_column": (10, 1),
         "1x10_one_row": (1, 10), "1x3_one_row_s5": (1, 3)}
# what the cases are there for (asserted below, on the tile counts)
assert {gy * gx for gy, gx in GRIDS.values()} >= {1, 6, 8, 9, 15, 25}   # one tile, < 8, == 8, 8 k + 1 (k = 1, 3), 8 k + 7
assert {SLICES[k][2] for k in SLICES} == {1, 3, 5}

FORMATS = {"dense": (0, 0, dict(bin_compact=0, bin_split=0)), "lists": (2, 1, dict(bin_compact=2, bin_split=0)),
           "own_pixels": (3, 2, dict(bin_compact=0, bin_split=2))}   # name -> (scatter_format, k3_mode, options)
HOMES = {"head": dict(co_schedule=0), "tail": dict(co_schedule=1, sep_update=0), "own_kernel": dict(co_schedule=1, sep_update=2)}


def tile_slice(name):
    """Events on an h x w sensor whose bounding box is the whole sensor: solid 5 x 5 blocks (two events per pixel) centred every
    10 rows and 20 columns and against the last row and column -- every 16 x 64 tile at scale 1 holds a whole block, so it has
    pixels that pass the 3 x 3 gate --, `n` events uniformly over the sensor, and the four corners.  Times rise along both axes
    (a gradient for the moments) with a jitter; sorted by time."""
    h, w, s, n = SLICES[name]
    rng = np.random.default_rng(4000 + 17 * h + 3 * w + s)
    T = 0.03
    cr = sorted(set(list(range(2, h, 10)) + [max(h - 3, 0)]))
    cc = sorted(set(list(range(2, w, 20)) + [max(w - 3, 0)]))
    blocks = np.array([(r + dr, c + dc) for r in cr for c in cc for dr in range(-2, 3) for dc in range(-2, 3)
                       if 0 <= r + dr < h and 0 <= c + dc < w], np.int64)
    br, bc = np.tile(blocks[:, 0], 2), np.tile(blocks[:, 1], 2)
    rows = np.concatenate([br, rng.integers(0, h, n), [0, 0, h - 1, h - 1]])
    cols = np.concatenate([bc, rng.integers(0, w, n), [0, w - 1, 0, w - 1]])
    assert len(rows) <= 6000, (name, len(rows))
    t = T * (0.1 + 0.35 * rows / max(h, 2) + 0.35 * cols / max(w, 2) + 0.15 * rng.random(len(rows)))
    order = np.argsort(t, kind="stable")
    return dict(fr_x=rows[order].astype(np.int32), fr_y=cols[order].astype(np.int32), t=np.floor(t[order] * 1e9).astype(np.int32))


def solve(a, sl, name):
    h, w, s, _ = SLICES[name]
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    gw = a.set_cloud(s, h, w)
    assert (gw.scale_img_x, gw.scale_img_y) == (s * h, s * w), (name, gw.scale_img_x, gw.scale_img_y)
    assert (-(-gw.scale_img_x // 16), -(-gw.scale_img_y // 64)) == GRIDS[name], name
    o = a.default_opts()
    o.res_x, o.res_y, o.want_uv, o.trace_cap, o.max_iter, o.min_events = h, w, 1, TRACE_CAP, ITER, 10
    rc, m, info = a.run(o)
    trace = a.get_trace(TRACE_CAP)
    u, v = a.compute_uv()
    timg = a.get_time_img()
    got = dict(rc=rc, it=info.iterations, model=packed(m), trace=[packed(t) for t in trace], flow=(u.tobytes(), v.tobytes()),
               timg=tuple(np.ascontiguousarray(x).tobytes() for x in timg))
    return got, trace, info


def capacity(name):
    h, w, s, _ = SLICES[name]
    return dict(max_events=8192, max_rows=s * h + s, max_cols=s * w + s)


@pytest.fixture(scope="module")
def references(accel_mod):
    """Per slice, computed once: the slice and the global-atomics loop's result on it."""
    from helpers import make_accel
    cache = {}

    def get(name):
        if name not in cache:
            sl = tile_slice(name)
            a = make_accel(accel_mod, dict(binned=0, fused=0), **capacity(name))
            try:
                ref, tr, info = solve(a, sl, name)
                assert a.get_stat("k1_threads") == -1 and a.get_stat("k3_mode") == -1 and a.get_stat("bins") == 0
            finally:
                a.close()
            h, w, s, _ = SLICES[name]
            print("%s: reference rc %d, %d iterations, valid pixels per record %s" % (name, ref["rc"], ref["it"], [t.model.cnt for t in tr]))
            assert len(tr) >= 1, (name, ref["rc"], ref["it"])
            if s * h >= 3 and s * w >= 3:   # (an image with a 3 x 3 neighbourhood: the gate passes somewhere, the moments are not all 0)
                assert tr[0].model.cnt > 0, name
                assert ref["it"] >= ITER and len(tr) >= ITER, (name, ref["rc"], ref["it"], len(tr))
            cache[name] = (sl, ref)
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("home", sorted(HOMES))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", sorted(SLICES))
def test_tile_order_same_bits_as_global_atomics(accel_mod, references, name, fmt, home):
    from helpers import make_accel
    sl, ref = references(name)
    scatter_format, k3_mode, fopts = FORMATS[fmt]
    opts = dict(binned=2, fused=0)
    opts.update(fopts)
    opts.update(HOMES[home])
    a = make_accel(accel_mod, opts, **capacity(name))
    try:
        got, _, info = solve(a, sl, name)
        stat = {k: a.get_stat(k) for k in ("scatter_format", "k1_head", "k3_half_scale", "k3_mode", "k3_capped", "bins")}
    finally:
        a.close()
    print("%s, %s, update at %s: ran %s, %d launches" % (name, fmt, home, stat, info.launches))
    # the two-kernel loop ran, in the asked format, with the update where it was asked for; the plain build (a few tiles)
    assert stat["scatter_format"] == scatter_format and stat["k3_mode"] == k3_mode and stat["bins"] >= 1, stat
    assert stat["k1_head"] == (1 if home == "head" else 0) and stat["k3_half_scale"] == SLICES[name][2] // 2 and stat["k3_capped"] == 0, stat
    for field in ("rc", "it", "model", "flow", "timg"):
        assert got[field] == ref[field], (name, fmt, home, field)
    assert len(got["trace"]) == len(ref["trace"])
    for k, (g_, r_) in enumerate(zip(got["trace"], ref["trace"])):
        assert g_ == r_, (name, fmt, home, "trace record", k)

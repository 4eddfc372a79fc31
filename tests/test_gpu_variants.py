"""Every compiled variant of the two-kernel tile-binned loop's kernels, run once and compared bit for bit.

The scatter kernel (bf_scatter.hip) is compiled per (update home, work-group size, events per thread, slab format) and with /
without the warp, the stencil kernel (bf_stencil.hip) per (HS = scale / 2, MODE, plain / capped-scalar-register build).  Which of
them runs is no option: the plan derives it from the event count, the scaled image size and the CU count
(better_flow_amd/csrc/bf_plan_rules.h).  tests/cpp/test_plan.cpp sweeps those rules on the host and holds the set of scatter
tuples they can return to tests/variants_reachable.txt; here ROWS has, for every tuple of that table and for each of the 30
stencil combinations, a slice that lands on it on the MI355X's 256 CUs -- the smallest one found with the rules (`test_plan rows`
prints the variant of a slice; tests/test_plan_cpu.py re-checks every row without a GPU).

Each row: a cold run of 12 iterations (the first scatter pass is the no-warp instantiation, the later ones the warp one); the
stats of bf_get_stat ("k1_*", "k3_*", "bin_*") must name exactly the row's variant -- a mismatch fails, nothing is skipped; the
return code, iteration count, every trace record, the final model, the per-event flow and the time image must be the BYTES of the
global-atomics loop on the same slice (binned = 0, fused = 0: no bins, no slabs, another stencil kernel), which in turn must
match the CPU oracle over the first two updates at test_gpu_borders.py's bars (valid-pixel count equal, the six model fields
within 3e-4 x max(1, |value|)).

The slices are not uniform: synth.make_slice's moving scene, plus a hot region (the fullest bin holds at least twice the
average, so that the scatter kernel's second pass runs -- the plan sizes a pass by the average), an empty corner (bins without
events), and events within two pixels of the bin boundaries and of the image borders (test_gpu_borders.border_slice)."""
import os
import struct

import numpy as np
import pytest

from better_flow_amd import synth

K = 12
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "variants_reachable.txt")

# (H, W, scale, n) -> (rows, columns) of a bin in scaled pixels, as the plan's cost model shapes them on 256 CUs
SLICES = {
    (65, 67, 1, 20000): (32, 16),
    (65, 67, 1, 30000): (32, 16),
    (65, 67, 1, 50000): (32, 16),
    (65, 67, 1, 80000): (32, 16),
    (65, 67, 3, 20000): (32, 16),
    (65, 67, 5, 120000): (32, 16),
    (65, 67, 7, 20000): (48, 32),
    (65, 67, 9, 20000): (48, 64),
    # >= 2048 stencil tiles of 16 x 64 scaled pixels: the capped build
    (141, 190, 9, 200000): (80, 64),
    (180, 240, 7, 200000): (80, 64),
    (250, 333, 5, 200000): (80, 64),
    (420, 560, 3, 200000): (80, 64),
    (1200, 1800, 1, 200000): (80, 64),
    # event lists over >= 1024 bins of < 1024 events: 256-thread work-groups (4 per thread needs > 724 events per bin)
    (325, 433, 3, 1200000): (32, 32),
    (650, 870, 3, 50000): (80, 64),
    (650, 870, 3, 300000): (80, 64),
}

# (slice, head, format, (threads, events per thread), (HS, MODE, capped))
ROWS = [
    ((65, 67, 1, 20000), 0, 0, (512, 4), (0, 0, 0)),
    ((65, 67, 1, 20000), 0, 2, (512, 2), (0, 1, 0)),
    ((65, 67, 1, 20000), 0, 3, (512, 4), (0, 2, 0)),
    ((65, 67, 1, 20000), 1, 0, (512, 4), (0, 0, 0)),
    ((65, 67, 1, 20000), 1, 2, (512, 2), (0, 1, 0)),
    ((65, 67, 1, 20000), 1, 3, (512, 4), (0, 2, 0)),
    ((65, 67, 1, 30000), 0, 0, (512, 8), (0, 0, 0)),
    ((65, 67, 1, 30000), 0, 2, (512, 4), (0, 1, 0)),
    ((65, 67, 1, 30000), 0, 3, (512, 8), (0, 2, 0)),
    ((65, 67, 1, 30000), 1, 0, (1024, 2), (0, 0, 0)),
    ((65, 67, 1, 30000), 1, 2, (512, 4), (0, 1, 0)),
    ((65, 67, 1, 30000), 1, 3, (1024, 2), (0, 2, 0)),
    ((65, 67, 1, 50000), 0, 0, (512, 10), (0, 0, 0)),
    ((65, 67, 1, 50000), 0, 2, (512, 8), (0, 1, 0)),
    ((65, 67, 1, 50000), 1, 0, (1024, 4), (0, 0, 0)),
    ((65, 67, 1, 50000), 1, 2, (512, 8), (0, 1, 0)),
    ((65, 67, 1, 50000), 1, 3, (1024, 4), (0, 2, 0)),
    ((65, 67, 1, 80000), 0, 0, (512, 12), (0, 0, 0)),
    ((65, 67, 1, 80000), 1, 0, (1024, 8), (0, 0, 0)),
    ((65, 67, 1, 80000), 1, 3, (1024, 8), (0, 2, 0)),
    ((65, 67, 3, 20000), 0, 0, (512, 1), (1, 0, 0)),
    ((65, 67, 3, 20000), 0, 2, (512, 1), (1, 1, 0)),
    ((65, 67, 3, 20000), 0, 3, (512, 1), (1, 2, 0)),
    ((65, 67, 3, 20000), 1, 0, (512, 1), (1, 0, 0)),
    ((65, 67, 3, 20000), 1, 2, (512, 1), (1, 1, 0)),
    ((65, 67, 3, 20000), 1, 3, (512, 1), (1, 2, 0)),
    ((65, 67, 5, 120000), 0, 0, (512, 2), (2, 0, 0)),
    ((65, 67, 5, 120000), 0, 2, (512, 2), (2, 1, 0)),
    ((65, 67, 5, 120000), 0, 3, (512, 2), (2, 2, 0)),
    ((65, 67, 5, 120000), 1, 0, (512, 2), (2, 0, 0)),
    ((65, 67, 5, 120000), 1, 3, (512, 2), (2, 2, 0)),
    ((65, 67, 7, 20000), 0, 0, (512, 1), (3, 0, 0)),
    ((65, 67, 7, 20000), 0, 2, (512, 1), (3, 1, 0)),
    ((65, 67, 7, 20000), 0, 3, (512, 1), (3, 2, 0)),
    ((65, 67, 9, 20000), 0, 0, (512, 1), (4, 0, 0)),
    ((65, 67, 9, 20000), 0, 2, (512, 1), (4, 1, 0)),
    ((65, 67, 9, 20000), 0, 3, (512, 1), (4, 2, 0)),
    ((141, 190, 9, 200000), 0, 0, (512, 1), (4, 0, 1)),
    ((141, 190, 9, 200000), 1, 2, (512, 1), (4, 1, 1)),
    ((141, 190, 9, 200000), 0, 3, (512, 1), (4, 2, 1)),
    ((180, 240, 7, 200000), 1, 0, (512, 1), (3, 0, 1)),
    ((180, 240, 7, 200000), 0, 2, (512, 1), (3, 1, 1)),
    ((180, 240, 7, 200000), 1, 3, (512, 1), (3, 2, 1)),
    ((250, 333, 5, 200000), 0, 0, (512, 1), (2, 0, 1)),
    ((250, 333, 5, 200000), 1, 2, (512, 1), (2, 1, 1)),
    ((250, 333, 5, 200000), 0, 3, (512, 1), (2, 2, 1)),
    ((325, 433, 3, 1200000), 0, 2, (256, 4), (1, 1, 0)),
    ((325, 433, 3, 1200000), 1, 2, (256, 4), (1, 1, 0)),
    ((420, 560, 3, 200000), 1, 0, (512, 1), (1, 0, 1)),
    ((420, 560, 3, 200000), 0, 3, (512, 1), (1, 2, 1)),
    ((650, 870, 3, 50000), 0, 2, (256, 1), (1, 1, 1)),
    ((650, 870, 3, 50000), 1, 2, (256, 1), (1, 1, 1)),
    ((650, 870, 3, 300000), 0, 2, (256, 2), (1, 1, 1)),
    ((650, 870, 3, 300000), 1, 2, (256, 2), (1, 1, 1)),
    ((1200, 1800, 1, 200000), 0, 0, (512, 1), (0, 0, 1)),
    ((1200, 1800, 1, 200000), 0, 2, (512, 1), (0, 1, 1)),
    ((1200, 1800, 1, 200000), 1, 3, (512, 1), (0, 2, 1)),
]


def reachable_table():
    with open(TABLE) as f:
        return {tuple(int(x) for x in ln.split()) for ln in f if ln.strip() and not ln.startswith("#")}


def row_id(row):
    (H, W, s, n), head, fmt, k1, k3 = row
    return "%dx%d_s%d_n%d-%s%dx%d_f%d-hs%d_m%d_%s" % ((W, H, s, n, "head" if head else "lean") + k1 + (fmt,) + k3[:2] +
                                                     ("capped" if k3[2] else "plain",))


def variant_slice(key):
    """Exactly n events on an H x W sensor whose bounding box is the whole sensor: 5/8 moving scene, 1/4 hot region, 1/8 within two
    pixels of an image border or of a bin boundary; nothing in the bottom-right corner (rows >= 3/4 H and columns >= 3/4 W)."""
    from test_gpu_borders import border_slice
    H, W, s, n = key
    tsr, ts = SLICES[key]
    seed = 1000 + (H * 31 + W * 7 + s * 3 + n) % 9973
    rng = np.random.default_rng(seed)
    # (above a million events a shorter slice: count and time sum of a pixel still pack into one 64-bit word, as in every other row)
    T = 0.03 if n <= 1000000 else 0.012
    n_hot, n_edge = n // 4, n // 8
    n_base = n - n_hot - n_edge
    in_corner = lambda r, c: (r >= (3 * H) // 4) & (c >= (3 * W) // 4)

    def take(r, c, t, m):   # m of the events outside the corner, evenly over the slice
        keep = ~in_corner(r, c)
        r, c, t = r[keep], c[keep], t[keep]
        assert len(r) >= m, (key, len(r), m)
        pick = np.linspace(0, len(r) - 1, m).astype(np.int64)
        return r[pick].astype(np.int32), c[pick].astype(np.int32), t[pick].astype(np.int64)

    base = synth.make_slice(2 * n_base + 64, H, W, T, seed=seed)
    parts = [take(base["fr_x"], base["fr_y"], base["t"], n_base)]
    # the hot region: a sixteenth of the sensor, up and left of the centre, with a quarter of the events
    # (... or less, so that it holds at least four events per sensor pixel: at scale 1 the Scharr gate wants all nine pixels of
    # a 3 x 3 neighbourhood valid, and a slice without one such neighbourhood ends after its first iteration)
    shrink = min(1.0, (n_hot / 4.0 / ((H // 4) * (W // 4))) ** 0.5)
    hh, hw = max(int(H // 4 * shrink), 2), max(int(W // 4 * shrink), 2)
    t_hot = np.sort(rng.uniform(0, T, n_hot))
    r_hot = np.floor(H // 4 + rng.uniform(0, hh, n_hot) + 30.0 * (H / 180.0) * t_hot)
    c_hot = np.floor(W // 5 + rng.uniform(0, hw, n_hot) - 40.0 * (H / 180.0) * t_hot)
    parts.append(take(np.clip(r_hot, 0, H - 1), np.clip(c_hot, 0, W - 1), (t_hot * 1e9), n_hot))
    # the image borders and corners (half), and the bin boundaries: sensor rows / columns around every multiple of the bin size
    n_img = n_edge // 2
    bs = border_slice(H, W, 2 * n_img + 64, seed)
    parts.append(take(bs["fr_x"], bs["fr_y"], np.floor(bs["t"] * (T / 0.03)), n_img))   # (border_slice lasts 0.03 s)
    m = 2 * (n_edge - n_img) + 64
    t_b = np.sort(rng.uniform(0, T, m))
    on_rows = rng.random(m) < 0.5
    r_b = np.where(on_rows, rng.integers(1, max(2, -(-s * H // tsr)), m) * tsr // s + rng.integers(-2, 3, m), rng.integers(0, H, m))
    c_b = np.where(on_rows, rng.integers(0, W, m), rng.integers(1, max(2, -(-s * W // ts)), m) * ts // s + rng.integers(-2, 3, m))
    parts.append(take(np.clip(r_b, 0, H - 1), np.clip(c_b, 0, W - 1), (t_b * 1e9), n_edge - n_img))
    fr_x, fr_y, t = (np.concatenate([p[i] for p in parts]) for i in range(3))
    order = np.argsort(t, kind="stable")
    sl = dict(fr_x=fr_x[order], fr_y=fr_y[order], t=t[order].astype(np.int32))
    assert len(sl["t"]) == n
    assert sl["fr_x"].min() == 0 and sl["fr_x"].max() == H - 1 and sl["fr_y"].min() == 0 and sl["fr_y"].max() == W - 1, key
    # what the slice is for: the fullest bin at least twice the average, and bins without events
    nbc = -(-s * W // ts)
    per_bin = np.bincount((s * sl["fr_x"].astype(np.int64) // tsr) * nbc + s * sl["fr_y"].astype(np.int64) // ts,
                          minlength=-(-s * H // tsr) * nbc)
    assert per_bin.max() >= 2.0 * per_bin.mean() and per_bin.min() == 0, (key, per_bin.max(), per_bin.mean(), per_bin.min())
    return sl


def packed(rec):
    """The bytes of a ctypes record's fields, padding left out."""
    out = b""
    for name, typ in rec._fields_:
        if name.startswith("_pad"):
            continue
        v = getattr(rec, name)
        out += packed(v) if hasattr(v, "_fields_") else struct.pack({"d": "<d", "f": "<f", "i": "<i", "I": "<I"}[typ._type_], v)
    return out


def solve(a, sl, H, W, s):
    a.upload_events(sl["fr_x"], sl["fr_y"], sl["t"])
    a.set_cloud(s, H, W)
    o = a.default_opts()
    o.res_x, o.res_y, o.want_uv, o.trace_cap, o.max_iter, o.min_events = H, W, 1, K + 2, K, 10
    rc, m, info = a.run(o)
    trace = a.get_trace(K + 2)
    u, v = a.compute_uv()
    timg = a.get_time_img()
    return dict(rc=rc, it=info.iterations, model=packed(m), trace=[packed(t) for t in trace], flow=(u.tobytes(), v.tobytes()),
                timg=tuple(np.ascontiguousarray(x).tobytes() for x in timg)), trace


@pytest.fixture(scope="module")
def references(accel_mod, oracle_lib):
    """Per distinct slice, computed once: the slice, and the global-atomics loop's result on it, itself held to the oracle."""
    from helpers import make_accel
    cache = {}

    def get(key):
        if key not in cache:
            H, W, s, n = key
            sl = variant_slice(key)
            a = make_accel(accel_mod, dict(binned=0, fused=0), max_events=n, max_rows=s * H + s, max_cols=s * W + s)
            try:
                ref, gtr = solve(a, sl, H, W, s)
                assert a.get_stat("k1_threads") == -1 and a.get_stat("k3_mode") == -1 and a.get_stat("bins") == 0
            finally:
                a.close()
            assert ref["it"] >= 2 and len(gtr) >= 2, (key, ref["rc"], ref["it"])
            o = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
            w_ = o.set_cloud(s, H, W)
            rc_, lp_, otr = o.run(w_, oracle_lib.Model(), max_iter=K, res_x=H, res_y=W, trace_cap=K + 2, min_events=10)
            for k in range(2):
                om, gm = otr[k].model, gtr[k].model
                assert om.cnt == gm.cnt, (key, k, om.cnt, gm.cnt)
                for f in ("cx", "cy", "dx", "dy", "rot", "div"):
                    a_, b_ = getattr(om, f), getattr(gm, f)
                    assert abs(a_ - b_) <= 3e-4 * max(1.0, abs(a_)), (key, k, f, a_, b_)
            cache[key] = (sl, ref)
        return cache[key]
    return get


HIT = {}   # row id -> the variant the run reported


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_variant_same_bits_as_global_atomics(accel_mod, references, row):
    from helpers import make_accel
    key, head, fmt, k1, k3 = row
    H, W, s, n = key
    sl, ref = references(key)
    opts = dict(binned=2, fused=0, bin_compact=2 if fmt == 2 else 0, bin_split=2 if fmt == 3 else 0, co_schedule=0 if head else 1)
    a = make_accel(accel_mod, opts, max_events=n, max_rows=s * H + s, max_cols=s * W + s)
    try:
        got, _ = solve(a, sl, H, W, s)
        stat = {k: a.get_stat(k) for k in ("scatter_format", "k1_head", "k1_threads", "k1_events_per_thread", "k3_half_scale",
                                           "k3_mode", "k3_capped", "bin_rows", "bin_cols", "bin_margin", "bins")}
    finally:
        a.close()
    print("%s: ran %s" % (row_id(row), stat))
    assert (stat["k1_head"], stat["k1_threads"], stat["k1_events_per_thread"], stat["scatter_format"]) == (head,) + k1 + (fmt,), stat
    assert (stat["k3_half_scale"], stat["k3_mode"], stat["k3_capped"]) == k3, stat
    assert (stat["bin_rows"], stat["bin_cols"]) == SLICES[key] and stat["bin_margin"] == 8, stat
    assert stat["bins"] == -(-s * H // stat["bin_rows"]) * -(-s * W // stat["bin_cols"]), stat
    HIT[row_id(row)] = ((head,) + k1 + (fmt,), k3)
    for field in ("rc", "it", "model", "flow", "timg"):
        assert got[field] == ref[field], (row_id(row), field)
    assert len(got["trace"]) == len(ref["trace"])
    for k, (g_, r_) in enumerate(zip(got["trace"], ref["trace"])):
        assert g_ == r_, (row_id(row), "trace record", k)


@pytest.mark.gpu
def test_rows_hit_every_reachable_variant():
    """The union of what the rows above RAN is the committed table of reachable scatter variants, and all 30 stencil
    combinations: a variant added to the plan without a row fails here."""
    assert len(HIT) == len(ROWS), "rows that did not report a variant: %s" % sorted(set(map(row_id, ROWS)) - set(HIT))
    assert {v[0] for v in HIT.values()} == reachable_table()
    assert {v[1] for v in HIT.values()} == {(hs, mode, capped) for hs in range(5) for mode in range(3) for capped in range(2)}

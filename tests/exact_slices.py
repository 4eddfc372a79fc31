"""The slices of the exact-reference tests (tests/test_exact_ref_cpu.py, tests/test_gpu_exact.py) -- TEST INFRASTRUCTURE ONLY.

Seeded numpy, 5 000 - 8 000 events; sensor coordinates 0 .. 24 x 0 .. 40, i.e. 75 x 123 scaled pixels at scale 3 -- several
16 x 64 stencil tiles, ragged in both directions --, and 0 .. 70 x 0 .. 90 for scale 1:
    small   t in [0, 4000) ns: every box sum below 2^22 ns, where one nanosecond more or less changes the f32 bits of the pixel
            (30 ms slices, sums around 1e8 ns, hide such an error in many of the pixels)
    piles   pixels with exactly 1, 2, 254, 255, 256, 257, 300 and 1000 events, a scale or more apart (the device's reciprocal
            table ends at 256 events), and an adjacent pair of 255 + 1 events whose boxes overlap under the moderate warp: 255
            next to 256
    signed  t in [-15 ms, +15 ms] (tmin < 0: the cnt * tmin re-bias), a pixel whose times sum to exactly 0 ns (cnt > 0, mean 0:
            invalid for Scharr) and pixels with means of exactly 999, 1000, 1001 ns (1000 ns = 1e-6f is invalid, 1001 ns valid)
    wide    t up to 2^31 - 1: the widest time field that still packs with the count into 64 bits
"""
import numpy as np

import exact_ref as X

SENSORS = {3: (24, 40), 1: (70, 90)}          # largest row / column a slice uses: scaled image 3 * 24 + 3 = 75 x 123, 71 x 91
KINDS = ("small", "piles", "signed", "wide")
PILE_KS = (1, 2, 254, 255, 256, 257, 300, 1000)
# reserved pixels, 9 apart (the largest scale) in both directions
SPOTS = [(r, c) for r in (3, 12, 21) for c in (4, 13, 22, 31)]
PAIR_A = SPOTS[8]                             # 255 events; PAIR_B = the pixel one column on, 1 event
SPECIAL = {"zero": SPOTS[9], "m999": SPOTS[10], "m1000": SPOTS[11], "m1001": SPOTS[0]}   # (signed slice)
ODD_SCALES, EVEN_SCALES = (1, 3, 5, 7, 9), (2, 4, 8)

_cache = {}


def make_slice(kind, H, W):
    """The slice `kind` on rows 0 .. H, columns 0 .. W (both corners hold an event).  Returns a dict with fr_x, fr_y (int32),
    t (int64), H, W, t_abs (largest |t|) and, where they exist, the reserved pixels."""
    key = (kind, H, W)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng({"small": 11, "piles": 12, "signed": 13, "wide": 14}[kind] * 1000 + H)
    reserved = set()
    extra = []                                # (row, column, times)
    if kind == "piles":
        for k, spot in zip(PILE_KS, SPOTS):
            extra.append(spot + (rng.integers(0, 30000000, k),))
        # the pair: A stays (times below 1 us), B's one event is the latest of the slice and moves half a pixel towards A
        extra.append(PAIR_A + (rng.integers(0, 1000, 255),))
        extra.append((PAIR_A[0], PAIR_A[1] + 1, np.array([29999999])))
    if kind == "signed":
        extra.append(SPECIAL["zero"] + (np.array([-5000, 5000, -7, 7]),))
        for name, mean in (("m999", 999), ("m1000", 1000), ("m1001", 1001)):
            extra.append(SPECIAL[name] + (np.array([mean - 300, mean + 300]),))
    for r, c, _ in extra:
        reserved.add((r, c))
    free = np.array([(r, c) for r in range(H + 1) for c in range(W + 1) if (r, c) not in reserved], np.int64)
    n_bg = 5000
    pick = free[rng.integers(0, len(free), n_bg)]
    pick[0], pick[1] = (0, 0), (H, W)         # the bounding box is the whole extent
    if kind == "small":
        t = rng.integers(0, 4000, n_bg)
    elif kind == "piles":
        t = rng.integers(0, 30000000, n_bg)
    elif kind == "signed":
        t = rng.integers(-15000000, 15000001, n_bg)
        t[2], t[3] = -15000000, 15000000
    else:
        t = rng.integers(0, 1 << 31, n_bg)
        t[2], t[3] = 0, (1 << 31) - 1
    rows = [pick[:, 0]] + [np.full(len(e[2]), e[0]) for e in extra]
    cols = [pick[:, 1]] + [np.full(len(e[2]), e[1]) for e in extra]
    ts = [t] + [np.asarray(e[2]) for e in extra]
    fr_x, fr_y, t = np.concatenate(rows), np.concatenate(cols), np.concatenate(ts).astype(np.int64)
    order = rng.permutation(len(t))           # container order must not matter
    sl = dict(kind=kind, H=H, W=W, fr_x=fr_x[order].astype(np.int32), fr_y=fr_y[order].astype(np.int32), t=t[order],
              t_abs=int(np.abs(t).max()))
    assert 5000 <= len(sl["t"]) <= 40000
    assert sl["fr_x"].min() == 0 and sl["fr_x"].max() == H and sl["fr_y"].min() == 0 and sl["fr_y"].max() == W
    if kind == "signed":
        assert sl["t"].min() < 0
    if kind == "wide":                        # large tbits, still packed: count << tbits | sum(t - tmin) fits 64 bits
        span = int((sl["t"] - sl["t"].min()).sum())
        assert sl["t"].max() == (1 << 31) - 1 and 40 <= span.bit_length() and span.bit_length() + len(sl["t"]).bit_length() <= 64
    _cache[key] = sl
    return sl


def warps(sl):
    """(name, parameters of project_4param_reinit) x 3: the identity; a moderate warp (the latest event moves half a pixel along
    the columns and a quarter along the rows, plus a little divergence and rotation about the middle); one strong enough that
    events leave the window (a dozen pixels).  An event moves by n / 127 * t / 1e4 pixels, so the parameters scale with the
    slice's largest |t|."""
    unit = 1.27e6 / sl["t_abs"]               # n that moves the latest event by one pixel
    cx, cy = sl["H"] / 2.0 + 0.25, sl["W"] / 2.0 - 0.5
    return (("identity", (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
            ("moderate", (-0.25 * unit, 0.5 * unit, cx, cy, 2.0e-3 * unit, -1.5e-3 * unit)),
            ("strong", (9.0 * unit, -12.0 * unit, cx, cy, -0.05 * unit, 0.04 * unit)))


def window_of(sl, scale):
    """The window bf_set_cloud / np_ref.window give for the slice (its bounding box is rows 0 .. H, columns 0 .. W)."""
    import np_ref
    return np_ref.window(sl["fr_x"], sl["fr_y"], scale, sl["H"] + 1, sl["W"] + 1)


def reference_images(sl, w, scale, pr_x, pr_y, noise=None):
    cnt, S = X.planes(pr_x, pr_y, sl["t"], w, scale, noise)
    return cnt, S, X.time_from_planes(cnt, S)

"""tests/exact_ref.py proven on the CPU, before any GPU test relies on it (no GPU needed).

Against the oracle (oracle/bf_oracle.c) and the independent numpy restatement (tests/np_ref.py), on the small slices of
tests/exact_slices.py and on one moving-scene slice:
* the count image is the oracle's; the time image is the oracle's BITS where one event hit the pixel and within 1e-6 relative
  elsewhere -- the bar the GPU is held to against the oracle today, so the exact reference sits inside it (where times of both
  signs cancel in a pixel the oracle's own f32 sum cannot meet a relative bar; there it is 1e-6 of sum|t|: within_order_noise);
* every value of time_from_planes is within 2^-23 relative of the exact rational S / (1e9 cnt) (two f32 roundings of 2^-24 each
  plus the f64 ones);
* scharr has the bits of np_ref.scharr and of the oracle's sobel;
* moments agrees with the oracle's fast_model: cnt, cx, cy equal, dx, dy, rot, div within exact_ref.moment_bound -- the oracle
  is one particular summation order, so it must lie inside a bound that holds for every order;
* mutations: on the small-times slice one nanosecond added to any one event changes the bits of every pixel its splat covers,
  and a dropped event changes the count -- because every box sum of that slice is below 2^22 ns, which is asserted.
"""
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as X
import np_ref
from better_flow_amd import synth
from exact_slices import KINDS, SENSORS, make_slice, warps, window_of


def moving_slice():
    mv = synth.make_slice(20000, 60, 80, 0.03)
    return dict(kind="moving", H=59, W=79, fr_x=mv["fr_x"], fr_y=mv["fr_y"], t=mv["t"], t_abs=int(np.abs(mv["t"]).max()))


def cases():
    out = [(k, s) for k in KINDS for s in (1, 3)]
    return out + [("moving", 3)]


def get_slice(kind, scale):
    return moving_slice() if kind == "moving" else make_slice(kind, *SENSORS[1 if scale == 1 else 3])


def within_order_noise(time, otime, cnt, S, mag, t):
    """The 1e-6 bar against the oracle.  The oracle adds f32 terms one by one, so its error is relative to the sum of the terms'
    MAGNITUDES: |time - otime| <= 1e-6 sum|t| / (1e9 cnt), asserted on every pixel.  Wherever all events of a pixel share one
    sign (|S| == sum|t|) that IS the plain relative bar `rtol = 1e-6`, and it is asserted as such there: on every pixel of a slice
    without negative times, and on the one-signed pixels of the signed slice.  Only where times of both signs meet can the sum
    cancel -- down to exactly 0 ns, a pixel the signed slice holds on purpose, where the oracle's own f32 sum is a rounding
    residue of 1e-13 s -- and there no bar relative to the result can hold for the oracle itself."""
    scale_ = mag.astype(np.float64) / (1e9 * np.maximum(cnt, 1))
    assert np.all(np.abs(time.astype(np.float64) - otime.astype(np.float64)) <= 1e-6 * scale_)
    one_sign = np.abs(S) == mag
    if t.min() >= 0:
        assert one_sign.all()
    else:
        assert (one_sign & (cnt > 1)).any() and not one_sign.all()
    np.testing.assert_allclose(time[one_sign], otime[one_sign], rtol=1e-6, atol=0)


@pytest.fixture(scope="module")
def staged(oracle_lib):
    """Per (slice, scale, warp), computed once: the oracle's cloud after the warp, its images, and the exact reference's."""
    cache = {}

    def get(kind, scale, warp):
        key = (kind, scale, warp)
        if key not in cache:
            sl = get_slice(kind, scale)
            oc = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
            ow = oc.set_cloud(scale, sl["H"] + 1, sl["W"] + 1)
            oc.project_4param_reinit(*dict(warps(sl))[warp])
            otime, ocnt = oc.get_time_img(ow)
            cnt, S = X.planes(oc.pr_x, oc.pr_y, sl["t"], ow, scale)
            _, mag = X.planes(oc.pr_x, oc.pr_y, np.abs(sl["t"]), ow, scale)
            cache[key] = dict(sl=sl, oc=oc, ow=ow, otime=otime, ocnt=ocnt, cnt=cnt, S=S, mag=mag, time=X.time_from_planes(cnt, S))
        return cache[key]
    return get


@pytest.mark.parametrize("kind,scale", cases())
@pytest.mark.parametrize("warp", ("identity", "moderate", "strong"))
def test_planes_and_time_image_against_oracle(staged, kind, scale, warp):
    z = staged(kind, scale, warp)
    w = window_of(z["sl"], scale)
    assert X.as_window(z["ow"]) == {k: w[k] for k in ("wsx", "wsy", "R", "C", "x_shift", "y_shift")}
    assert np.array_equal(z["cnt"], z["ocnt"].astype(np.int64))
    assert z["time"].dtype == np.float32
    one = z["cnt"] == 1
    assert one.any() and np.array_equal(X.bits(z["time"])[one], X.bits(z["otime"])[one])
    within_order_noise(z["time"], z["otime"], z["cnt"], z["S"], z["mag"], z["sl"]["t"])
    assert np.array_equal(z["time"][z["cnt"] == 0], np.zeros((z["cnt"] == 0).sum(), np.float32))
    if warp == "strong":
        assert z["cnt"].sum() < scale * scale * len(z["sl"]["t"])


def test_planes_noise_mask_and_np_ref(oracle_lib):
    """The noise skip, against the oracle and against np_ref.time_img (event by event) on a cut of the signed slice."""
    sl = make_slice("signed", *SENSORS[3])
    noise = (np.arange(len(sl["t"])) % 3 == 0).astype(np.uint8)
    oc = oracle_lib.Cloud(sl["fr_x"], sl["fr_y"], sl["t"])
    oc.noise[:] = noise
    ow = oc.set_cloud(3, sl["H"] + 1, sl["W"] + 1)
    oc.project_4param_reinit(*warps(sl)[1][1])
    otime, ocnt = oc.get_time_img(ow)
    cnt, S = X.planes(oc.pr_x, oc.pr_y, sl["t"], ow, 3, noise)
    assert np.array_equal(cnt, ocnt.astype(np.int64)) and cnt.sum() < 9 * (len(noise) - noise.sum()) + 1
    _, mag = X.planes(oc.pr_x, oc.pr_y, np.abs(sl["t"]), ow, 3, noise)
    within_order_noise(X.time_from_planes(cnt, S), otime, cnt, S, mag, sl["t"])
    k = 1500
    w = window_of(sl, 3)
    ntime, ncnt = np_ref.time_img(oc.pr_x[:k], oc.pr_y[:k], sl["t"][:k], w, 3, noise[:k])
    cnt, S = X.planes(oc.pr_x[:k], oc.pr_y[:k], sl["t"][:k], w, 3, noise[:k])
    assert np.array_equal(cnt, ncnt.astype(np.int64))
    _, mag = X.planes(oc.pr_x[:k], oc.pr_y[:k], np.abs(sl["t"][:k]), w, 3, noise[:k])
    within_order_noise(X.time_from_planes(cnt, S), ntime, cnt, S, mag, sl["t"])


@pytest.mark.parametrize("kind,scale", cases())
def test_time_from_planes_against_the_exact_rational(staged, kind, scale):
    """|RN32(RN32(RN64(S) / 1e9) / RN32(cnt)) - S / (1e9 cnt)| <= 2^-23 |S / (1e9 cnt)| on every pixel with events, in exact
    rational arithmetic (Fraction of a float is the float's exact value)."""
    z = staged(kind, scale, "moderate")
    ii, jj = np.nonzero(z["cnt"] > 0)
    tol = Fraction(1, 1 << 23)
    worst = Fraction(0)
    for c, s, v in zip(z["cnt"][ii, jj].tolist(), z["S"][ii, jj].tolist(), z["time"][ii, jj].tolist()):
        exact = Fraction(s, 1000000000 * c)
        err = abs(Fraction(v) - exact)
        assert err <= tol * abs(exact), (c, s, v)
        if exact:
            worst = max(worst, err / abs(exact))
    print("%s, scale %d: %d pixels, worst relative error %.3e (2^-23 = %.3e)" % (kind, scale, len(ii), float(worst), 2.0 ** -23))


def test_valid_is_the_f32_comparison():
    f = np.float32(1e-6)
    assert float(f) < 1e-6 and float(np.nextafter(f, np.float32(1))) > 1e-6   # 1e-6f is the largest float below 1e-6
    v = np.array([f, np.nextafter(f, np.float32(1)), 0, -1, 1.001e-6, 0.999e-6], np.float32)
    assert X.valid(v).tolist() == [False, True, False, False, True, False]
    assert X.valid(v).tolist() == (v > f).tolist()
    # one event at 1000 ns is exactly 1e-6f (invalid), at 1001 ns it is valid
    assert X.bits(X.time_from_planes(np.array([1, 1, 2]), np.array([1000, 1001, 2000]))).tolist() == \
        X.bits(np.array([f, np.float32(1.001e-6), f])).tolist()


def test_scharr_bits(oracle_lib, staged):
    """A 40 x 70 image (np_ref is slow): a cut of a time image, a dense random image, one with holes and threshold values."""
    rng = np.random.default_rng(3)
    dense = rng.uniform(2e-6, 0.05, size=(40, 70)).astype(np.float32)
    holes = dense.copy()
    holes[rng.uniform(size=holes.shape) < 0.1] = 0.0
    holes[5, 5] = 1e-6
    holes[6, 9] = np.float32(1.0000001e-6)
    holes[20, 30] = -0.01
    cut = np.ascontiguousarray(staged("moving", 3, "moderate")["time"][60:100, 100:170])
    for img in (cut, dense, holes):
        gx, gy = X.scharr(img)
        assert gx.dtype == np.float32 and np.abs(gx).sum() > 0
        ngx, ngy = np_ref.scharr(img)
        ogx, ogy = oracle_lib.sobel(img)
        for a, b in ((gx, ngx), (gy, ngy), (gx, ogx), (gy, ogy)):
            assert np.array_equal(X.bits(a), X.bits(b))
    for img in (np.zeros((3, 3), np.float32), dense[:2, :5], dense[:1, :1], dense[:3, :3]):
        gx, gy = X.scharr(img)
        ogx, ogy = oracle_lib.sobel(img)
        assert np.array_equal(X.bits(gx), X.bits(ogx)) and np.array_equal(X.bits(gy), X.bits(ogy))


@pytest.mark.parametrize("kind,scale", cases())
@pytest.mark.parametrize("warp", ("identity", "moderate"))
def test_moments_against_oracle(oracle_lib, staged, kind, scale, warp):
    img = staged(kind, scale, warp)["time"]
    ref = X.moments(img)
    om = oracle_lib.fast_model(img)
    bound = X.moment_bound(ref)
    assert om.cnt == ref["cnt"] and ref["cnt"] > 100
    assert om.cx == ref["cx"] and om.cy == ref["cy"]
    for k in ("dx", "dy", "rot", "div"):
        o, r = getattr(om, k), ref[k]
        print("%s, scale %d, %s: %s oracle %.17g exact %.17g, off by %.3e, bound %.3e" % (kind, scale, warp, k, o, r, abs(o - r), bound[k]))
        assert abs(o - r) <= bound[k], (k, o, r, abs(o - r), bound[k])
    # the bound is tight enough to mean something: (N + 8) 2^-53, 1e-12 of the magnitude sums at a few thousand valid pixels
    n = ref["cnt"]
    assert 0 <= bound["dx"] <= 1.2e-16 * (n + 8) * ref["a"]["gx"] / n


def test_moments_small_known_answer():
    """A 5 x 7 ramp: every interior gradient known in closed form, so the sums are too."""
    i, j = np.mgrid[0:5, 0:7]
    img = (0.001 + 0.0005 * i + 0.00025 * j).astype(np.float32)
    m = X.moments(img)
    assert m["cnt"] == 35 and m["cx"] == 2.0 and m["cy"] == 3.0 and m["cxc"] == 0.0 and m["cyc"] == 0.0
    gx, gy = X.scharr(img)
    # sharr_x varies with the inner index l, the ROW offset, sharr_y with the column offset: -32 d/drow, -32 d/dcolumn
    assert np.allclose(gx[1:-1, 1:-1], -32 * 0.0005, rtol=1e-5) and np.allclose(gy[1:-1, 1:-1], -32 * 0.00025, rtol=1e-5)
    assert abs(m["dx"] - 15 * -32 * 0.0005 / 35) < 1e-9 and abs(m["dy"] - 15 * -32 * 0.00025 / 35) < 1e-9
    b = X.moment_bound(m)
    assert 0 < b["dx"] < 1e-15 and 0 < b["rot"] < 1e-14


def test_a_nanosecond_or_an_event_changes_the_reference():
    """Why the small-times slice exists.  Largest box sum below 2^22 ns (asserted), so: one nanosecond added to any one event
    changes the f32 bits of EVERY pixel its splat covers; one event dropped changes the count there.  200 seeded picks per
    scale.  (On the piles slice, 30 ms long, the same nanosecond leaves over a quarter of the pixels' bits unchanged: the last
    assertion holds that.)"""
    rng = np.random.default_rng(2024)
    for scale in (1, 3, 9):
        sl = make_slice("small", *SENSORS[1 if scale == 1 else 3])
        w = window_of(sl, scale)
        hs = scale // 2
        px, py = sl["fr_x"].astype(np.float64), sl["fr_y"].astype(np.float64)
        x, y, keep = X.targets(px, py, w, scale)
        assert keep.sum() > 4500   # (the events of the last row and column fall outside the window: accel_lib.h:157)
        cnt, S = X.planes(px, py, sl["t"], w, scale)
        assert 0 <= int(S.min()) and int(S.max()) < (1 << 22)
        base = X.bits(X.time_from_planes(cnt, S))
        for e in rng.choice(np.nonzero(keep)[0], 200).tolist():
            box = (slice(x[e] - hs, x[e] + hs + 1), slice(y[e] - hs, y[e] + hs + 1))
            t2 = sl["t"].copy()
            t2[e] += 1
            c2, S2 = X.planes(px, py, t2, w, scale)
            assert np.array_equal(c2, cnt) and (S2 - S).sum() == scale * scale and (S2 - S)[box].sum() == scale * scale
            changed = X.bits(X.time_from_planes(c2, S2)) != base
            assert changed[box].all() and changed.sum() == scale * scale, (scale, e)
            drop = np.ones(len(sl["t"]), bool)
            drop[e] = False
            c3, _ = X.planes(px[drop], py[drop], sl["t"][drop], w, scale)
            assert ((cnt - c3)[box] == 1).all() and (cnt - c3).sum() == scale * scale, (scale, e)
    # the same mutation on the piles slice (sums around 1e8 ns): invisible in over a quarter of the pixels with events
    sl = make_slice("piles", *SENSORS[3])
    w = window_of(sl, 3)
    px, py = sl["fr_x"].astype(np.float64), sl["fr_y"].astype(np.float64)
    cnt, S = X.planes(px, py, sl["t"], w, 3)
    same = X.bits(X.time_from_planes(cnt, S + 1)) == X.bits(X.time_from_planes(cnt, S))
    assert same[cnt > 0].mean() > 0.25, same[cnt > 0].mean()

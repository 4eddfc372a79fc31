"""An order-free reference of the time image and the moments -- TEST INFRASTRUCTURE ONLY.

The oracle (oracle/bf_oracle.c) and tests/np_ref.py add a pixel's times in f32 in container order, as the reference does
(accel_lib.h:162): their time image moves with the event order, and the device can be held to them only to 1e-6.  The
device keeps a count and an integer nanosecond sum per pixel and turns them into f32 with ONE documented sequence
(time_from_sums, better_flow_amd/csrc/bf_device_fns.h), so its time image has one right answer per pixel, bit for bit.
This module states that answer with integer planes and plain IEEE operations:

    planes            cnt and S = sum of t (ns) per pixel, int64, after the s x s splat (accel_lib.h:154-165)
    time_from_planes  RN32( RN32( RN64(S) / 1e9 ) / RN32(cnt) ) where cnt > 0, else 0 -- one formula for every count
                      (that the device's reciprocal table below 256 events gives the same bits is proven elsewhere,
                      tests/exhaustive_div.c; nothing here knows of the table)
    scharr            accel_lib.h:513-615 over whole arrays, every product and every add a separate f32 operation
    moments           object_model.cpp:4-39,103-126 from correctly rounded sums (math.fsum), in the centred form the
                      device uses (model_update_wave), with the sums of absolute values a bound needs
    moment_bound      how far a correct f64 evaluation in ANY summation order may be from `moments` (derived below)

Vectorised numpy and Python integers; no loop per event or per pixel except math.fsum's own.
tests/test_exact_ref_cpu.py proves it against the oracle and np_ref.py before a GPU test relies on it.
"""
import math

import numpy as np

F32 = np.float32
INT_MIN = -(1 << 31)
U = 2.0 ** -53   # unit roundoff of f64


def as_window(w):
    """The window as np_ref.window's dict, from that dict or from a Window record of the oracle / the library."""
    if isinstance(w, dict):
        return w
    return dict(wsx=w.metric_wsizex, wsy=w.metric_wsizey, R=w.scale_img_x, C=w.scale_img_y,
                x_shift=w.x_shift, y_shift=w.y_shift)


def trunc_x86(v):
    """double -> int as cvttsd2si converts: toward zero; NaN and everything outside int32 give INT_MIN."""
    v = np.asarray(v, dtype=np.float64)
    ok = np.isfinite(v) & (np.abs(v) < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), float(INT_MIN)).astype(np.int64)


def targets(pr_x, pr_y, w, scale, noise=None):
    """(x, y, keep): the scaled pixel of every event and whether it is scattered (accel_lib.h:152-158)."""
    w = as_window(w)
    hs = scale // 2
    x = trunc_x86(np.asarray(pr_x, np.float64) * float(scale) + float(int(w["x_shift"])))
    y = trunc_x86(np.asarray(pr_y, np.float64) * float(scale) + float(int(w["y_shift"])))
    keep = ~((x >= w["wsx"] + hs) | (x < hs) | (y >= w["wsy"] + hs) | (y < hs))
    if noise is not None:
        keep &= ~np.asarray(noise).astype(bool)
    return x, y, keep


def box_sum(a, hs):
    """a[i, j] summed over the (2 hs + 1)^2 box around every pixel that lies inside the array (integers: exact)."""
    R, C = a.shape
    p = np.zeros((R + 2 * hs, C + 2 * hs), dtype=a.dtype)
    p[hs:hs + R, hs:hs + C] = a
    rows = sum(p[k:k + R, :] for k in range(2 * hs + 1))
    return sum(rows[:, k:k + C] for k in range(2 * hs + 1))


def planes(pr_x, pr_y, t, window, scale, noise=None):
    """(cnt, S): int64 event count and sum of t in ns per pixel after the s x s splat."""
    w = as_window(window)
    R, C = w["R"], w["C"]
    x, y, keep = targets(pr_x, pr_y, w, scale, noise)
    flat = x[keep] * C + y[keep]
    cnt0 = np.zeros(R * C, np.int64)
    s0 = np.zeros(R * C, np.int64)
    np.add.at(cnt0, flat, 1)
    np.add.at(s0, flat, np.asarray(t, np.int64)[keep])
    # (the window test keeps every splat inside the image: hs <= x < wsx + hs and R = wsx + scale)
    return box_sum(cnt0.reshape(R, C), scale // 2), box_sum(s0.reshape(R, C), scale // 2)


def time_from_planes(cnt, S):
    """The device's documented arithmetic (time_from_sums): the integer sum rounded to f64, divided by 1e9, rounded to f32,
    divided in f32 by the count.  0 where cnt == 0."""
    cnt = np.asarray(cnt, np.int64)
    S = np.asarray(S, np.int64)
    sum_s = (S.astype(np.float64) / np.float64(1e9)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = sum_s / cnt.astype(F32)
    return np.where(cnt > 0, q, F32(0)).astype(F32)


def valid(img):
    """`p[j] > 0.000001`: a float against a double literal (object_model.cpp:22,108; accel_lib.h:534,599).  1e-6f, the float
    nearest to 1e-6, is the largest float BELOW it, so this is also `img > 1e-6f` in f32."""
    return np.asarray(img, F32).astype(np.float64) > 0.000001


SX = (3, 0, -3, 10, 0, -10, 3, 0, -3)
SY = (3, 10, 3, 0, 0, 0, -3, -10, -3)


def scharr(img):
    """accel_lib.h:513-615: the nine taps of np_ref.scharr in its order (column offset outer, row offset inner), every
    product and every add rounded to f32; zero unless the centre and all nine neighbours are valid; borders zero."""
    img = np.ascontiguousarray(img, F32)
    R, C = img.shape
    gx = np.zeros((R, C), F32)
    gy = np.zeros((R, C), F32)
    if R < 3 or C < 3:
        return gx, gy
    ok = valid(img)
    ax = np.zeros((R - 2, C - 2), F32)
    ay = np.zeros((R - 2, C - 2), F32)
    all_ok = np.ones((R - 2, C - 2), bool)
    idx = 0
    for k in range(3):
        for l in range(3):
            val = img[l:l + R - 2, k:k + C - 2]
            all_ok &= ok[l:l + R - 2, k:k + C - 2]
            ax = (ax + (val * F32(SX[idx])).astype(F32)).astype(F32)
            ay = (ay + (val * F32(SY[idx])).astype(F32)).astype(F32)
            idx += 1
    gx[1:-1, 1:-1] = np.where(all_ok, ax, F32(0))
    gy[1:-1, 1:-1] = np.where(all_ok, ay, F32(0))
    return gx, gy


def moments(img):
    """The model of an image (ObjectModel::update) from correctly rounded sums.

    valid = img > 1e-6f, n their number, ci = i - R // 2, cj = j - C // 2.  The six sums sum gx, sum gy, sum ci gx, sum ci gy,
    sum cj gx, sum cj gy run over the valid pixels with math.fsum over the f64 products; a product of a 16-bit integer and an
    f32 is exact in f64, so every sum is the real sum rounded once.  From them, as model_update_wave forms them:
        cx = RN64((sum ci + n (R // 2)) / n) (exact integer numerator), cy alike;  cxc = RN64(sum ci / n), cyc alike;
        dx = RN64(sgx / n), dy alike;
        rot = (sigy / n - cxc dy) - (sjgx / n - cyc dx),  div = (sigx / n - cxc dx) + (sjgy / n - cyc dy).
    Returns a dict with these, `cnt`, the sums (`s`) and the sums of absolute values (`a`), both keyed gx, gy, igx, igy,
    jgx, jgy."""
    img = np.ascontiguousarray(img, F32)
    R, C = img.shape
    gx, gy = scharr(img)
    ii, jj = np.nonzero(valid(img))
    n = int(len(ii))
    ci = (ii - R // 2).astype(np.float64)
    cj = (jj - C // 2).astype(np.float64)
    g0 = gx[ii, jj].astype(np.float64)
    g1 = gy[ii, jj].astype(np.float64)
    terms = dict(gx=g0, gy=g1, igx=ci * g0, igy=ci * g1, jgx=cj * g0, jgy=cj * g1)
    s = {k: math.fsum(v.tolist()) for k, v in terms.items()}
    a = {k: math.fsum(np.abs(v).tolist()) for k, v in terms.items()}
    sci = int((ii - R // 2).sum())
    scj = int((jj - C // 2).sum())
    out = dict(cnt=n, s=s, a=a, sci=sci, scj=scj, R=R, C=C)
    if n == 0:   # 0 / 0: NaN, as in the reference (its assert is compiled out)
        out.update(cx=math.nan, cy=math.nan, cxc=math.nan, cyc=math.nan, dx=math.nan, dy=math.nan, rot=math.nan, div=math.nan)
        return out
    dn = float(n)
    cx = float(sci + n * (R // 2)) / dn
    cy = float(scj + n * (C // 2)) / dn
    cxc, cyc = float(sci) / dn, float(scj) / dn
    dx, dy = s["gx"] / dn, s["gy"] / dn
    rot = (s["igy"] / dn - cxc * dy) - (s["jgx"] / dn - cyc * dx)
    div = (s["igx"] / dn - cxc * dx) + (s["jgy"] / dn - cyc * dy)
    out.update(cx=cx, cy=cy, cxc=cxc, cyc=cyc, dx=dx, dy=dy, rot=rot, div=div)
    return out


def moment_bound(m):
    """How far dx, dy, rot, div of a correct f64 evaluation may be from moments(img) -- derived, not measured.

    N = number of valid pixels, u = 2^-53.
    * A sum of N f64 terms x_k added in ANY order (any tree, any split into work-group partials) differs from the real sum by
      at most (N - 1) u sum|x_k| (each of the N - 1 additions rounds a partial sum no larger than sum|x_k|; second-order
      terms are below N^2 u^2, 1e-25 at N of a few thousand).  The terms themselves are exact (see moments).
    * The device adds its work-group partials as fixed point (MomentAcc): each partial is truncated below 2^-64, at most 2^10
      partials, so at most 1024 x 2^-64 absolute per sum; joining the two fixed-point words and converting them to f64 rounds
      twice more.
    * A division, a product and a subtraction add one rounding each, on either side; the reference side rounds its sum once.
    dx = sgx / n:  (N - 1) for the sum, 2 for the join, 1 for the division on the device; 1 + 1 in the reference:
        |dx - dx_ref| <= (N + 8) u sum|gx| / n            (dy alike)
    rot = (sigy / n - cxc dy) - (sjgx / n - cyc dx): each quotient as above; cxc is one rounding of an exact quotient, the
    product one more, each of the three subtractions one on a value no larger than the magnitude sum:
        |rot - rot_ref| <= (N + 8) u (sum|ci gy| + |cxc| sum|gy| + sum|cj gx| + |cyc| sum|gx|) / n + 1024 x 2^-64 / n
    div = (sigx / n - cxc dx) + (sjgy / n - cyc dy) alike with sum|ci gx|, |cxc| sum|gx|, sum|cj gy|, |cyc| sum|gy|.
    Nothing here depends on the order in which a kernel adds, so the bound survives retuning."""
    n, a = m["cnt"], m["a"]
    k = (n + 8) * U
    floor_ = 1024.0 * 2.0 ** -64 / n
    cxc, cyc = abs(m["cxc"]), abs(m["cyc"])
    return dict(dx=k * a["gx"] / n, dy=k * a["gy"] / n,
                rot=k * (a["igy"] + cxc * a["gy"] + a["jgx"] + cyc * a["gx"]) / n + floor_,
                div=k * (a["igx"] + cxc * a["gx"] + a["jgy"] + cyc * a["gy"]) / n + floor_)


def bits(a):
    """The bit patterns of an f32 array."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ulp_distance64(a, b):
    """Number of f64 values between two finite doubles of the same sign (0: the same bits)."""
    ia = np.array([a], np.float64).view(np.int64)[0]
    ib = np.array([b], np.float64).view(np.int64)[0]
    return abs(int(ia) - int(ib))


def first_mismatch(got_t, got_c, want_t, cnt, S, what):
    """None when the device's time image and count image are the reference's, bit for bit; else a message with everything
    one run needs: the pixel, its cnt and S, the bit patterns got and wanted, the number of pixels off, and `what` (the
    options of the case)."""
    gb, wb = bits(got_t), bits(want_t)
    bad = (gb != wb) | (np.asarray(got_c, np.int64) != cnt)
    if not bad.any():
        return None
    i, j = np.argwhere(bad)[0]
    return ("%s: %d of %d pixels differ; first at (%d, %d): cnt got %d want %d, S = %d ns, time bits got 0x%08x (%.9g) "
            "want 0x%08x (%.9g)" % (what, int(bad.sum()), bad.size, i, j, int(got_c[i, j]), int(cnt[i, j]), int(S[i, j]),
                                   int(gb[i, j]), float(got_t[i, j]), int(wb[i, j]), float(want_t[i, j])))

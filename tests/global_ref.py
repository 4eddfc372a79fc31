"""numpy restatement of the reference's OptimizerGlobal (optimizer_global.cpp:4-101,104-150,187-205;
optimizer_global.h:27-41) with this build's two stated definitions ("OptimizerGlobal"):

  * the per-event result is the winning candidate (best_nx, best_ny); best_u / best_v are Event::compute_uv of it
    (event.h:135-142), not the stale u / v the reference copies;
  * the slice objective of candidate k is S(k) = sum over accepted events of floor(score * 2^32), an exact integer,
    and the slice's best candidate is the first in sweep order with the largest S.

The blur is this build's stated 8-bit Gaussian (include/bf_accel.h): binomial taps, BORDER_REFLECT_101, exact integer
sum, one rounding.  Images are indexed (row, col) = (x, y) like the reference's cv::Mat::at<>(x, y).
"""
import math

import numpy as np

NZ = 127.0
TAPS = {0: [1], 1: [1, 2, 1], 2: [1, 4, 6, 4, 1], 3: [2, 7, 14, 18, 14, 7, 2]}


def window(fr_x, fr_y, scale=5, metric_wsize=None):
    """update_fields (optimizer_global.cpp:187-205); metric_wsize None: 5 * scale, as OptimizerGlobal(events, sc)
    (the default constructor is scale 5 with window 21, optimizer_global.h:27-29).
    An empty cloud gets the box x, y in [0, -1] (no pixels); the reference leaves it undefined."""
    if metric_wsize is None:
        metric_wsize = 5 * scale
    assert scale % 2 == 1 and metric_wsize % 2 == 1
    if len(fr_x):
        x_min, x_max = int(np.min(fr_x)), int(np.max(fr_x))
        y_min, y_max = int(np.min(fr_y)), int(np.max(fr_y))
    else:
        x_min, x_max, y_min, y_max = 0, -1, 0, -1
    sx = (x_max - x_min + 1) * scale
    sy = (y_max - y_min + 1) * scale
    return dict(scale=scale, metric_wsize=metric_wsize, x_min=x_min, y_min=y_min, x_max=x_max, y_max=y_max,
                scale_img_x=sx, scale_img_y=sy, scale_bordered_img_x=sx + metric_wsize,
                scale_bordered_img_y=sy + metric_wsize)


def sweep_values(lo, hi, step):
    """The reference's `for (v = lo; v < hi; v += step)` -- repeated double addition."""
    out = []
    v = float(lo)
    while v < hi:
        out.append(v)
        v += step
    return out


def default_grid():
    return sweep_values(-0.09, 0.09, 0.001), sweep_values(-0.04, 0.04, 0.001)


def project(fr_x, fr_y, t, nx, ny, nz=NZ):
    """Event::project -> apply_project (event.h:65-70,164-168): float kx = float(nx) / nz; pr = float(fr) - kx * float(t) / 10000.0"""
    kx = np.float32(np.float64(np.float32(nx)) / nz)
    ky = np.float32(np.float64(np.float32(ny)) / nz)
    ft = np.asarray(t).astype(np.float32)
    px = (kx * ft).astype(np.float32).astype(np.float64)
    py = (ky * ft).astype(np.float32).astype(np.float64)
    pr_x = np.asarray(fr_x).astype(np.float32).astype(np.float64) - px / 10000.0
    pr_y = np.asarray(fr_y).astype(np.float32).astype(np.float64) - py / 10000.0
    return pr_x, pr_y


def pixels(pr_x, pr_y, w):
    """optimizer_global.cpp:17-21: int x = pr_x * scale - x_min * scale (truncation), the acceptance test."""
    s = w["scale"]
    xf = np.trunc(pr_x * float(s) - float(w["x_min"] * s))
    yf = np.trunc(pr_y * float(s) - float(w["y_min"] * s))
    ok = (xf < w["scale_img_x"] - s) & (xf >= 0) & (yf < w["scale_img_y"] - s) & (yf >= 0)
    X = np.where(ok, xf, 0).astype(np.int64)
    Y = np.where(ok, yf, 0).astype(np.int64)
    return X, Y, ok


def _box(a, r0, r1):
    """sum of a over [i + r0, i + r1] x [j + r0, j + r1], zero outside."""
    R, C = a.shape
    pad = max(-r0, r1, 0)
    p = np.pad(a, pad)
    I = np.zeros((R + 2 * pad + 1, C + 2 * pad + 1), dtype=np.int64)
    I[1:, 1:] = p.cumsum(0).cumsum(1)
    a0, a1 = pad + r0, pad + r1 + 1
    return (I[a1:a1 + R, a1:a1 + C] - I[a0:a0 + R, a1:a1 + C] - I[a1:a1 + R, a0:a0 + C] + I[a0:a0 + R, a0:a0 + C])


def blur8(img, scale):
    """This build's 8-bit Gaussian, ksize = scale: binomial taps, BORDER_REFLECT_101, exact sum, one rounding."""
    h = scale // 2
    if h == 0:
        return img.astype(np.uint8)
    taps = np.array(TAPS[h], dtype=np.int64)
    n2 = int(taps.sum()) ** 2
    p = np.pad(img.astype(np.int64), h, mode="reflect")
    R, C = img.shape
    rows = sum(taps[k] * p[:, k:k + C] for k in range(2 * h + 1))
    acc = sum(taps[k] * rows[k:k + R, :] for k in range(2 * h + 1))
    return ((acc + n2 // 2) // n2).astype(np.uint8)


def project_img(fr_x, fr_y, t, w, nx, ny, nz=NZ):
    """The blurred bordered image of project_all (optimizer_global.cpp:13-37) and the accepted pixels."""
    pr_x, pr_y = project(fr_x, fr_y, t, nx, ny, nz)
    X, Y, ok = pixels(pr_x, pr_y, w)
    s, mw = w["scale"], w["metric_wsize"]
    off = s // 2 + mw // 2
    pts = np.zeros((w["scale_bordered_img_x"], w["scale_bordered_img_y"]), dtype=np.int64)
    np.add.at(pts, (X[ok] + off, Y[ok] + off), 1)
    h = s // 2
    cnt = np.minimum(_box(pts, -h, h), 255)          # each `if (< 255) ++` of :27-31: min(255, total)
    img = blur8(cnt, s) if s > 1 else cnt.astype(np.uint8)
    return img, pr_x, pr_y, X, Y, ok


def window_sums(img, w):
    """Per bordered pixel: non-zero sum and count of the metric_wsize^2 window centred there (get_event_score, :82-101)."""
    r = w["metric_wsize"] // 2
    v = img.astype(np.int64)
    return _box(v, -r, r), _box((v > 0).astype(np.int64), -r, r)


def score_fixed(nz_sum, nz_cnt):
    """floor(score * 2^32) of one event, exact: (sum << 32) // cnt (0 when the window has no non-zero pixel)."""
    nz_sum = np.asarray(nz_sum, dtype=np.int64)
    nz_cnt = np.asarray(nz_cnt, dtype=np.int64)
    return np.where(nz_cnt > 0, (nz_sum << 32) // np.maximum(nz_cnt, 1), 0)


class Global:
    """OptimizerGlobal over one cloud: per-event state that accumulates over project_all calls."""

    def __init__(self, fr_x, fr_y, t, scale=5, metric_wsize=None):
        self.fr_x = np.asarray(fr_x, dtype=np.int64)
        self.fr_y = np.asarray(fr_y, dtype=np.int64)
        self.t = np.asarray(t, dtype=np.int64)
        self.w = window(self.fr_x, self.fr_y, scale, metric_wsize)
        n = len(self.fr_x)
        self.max_score = np.zeros(n)
        self.best_nx = np.zeros(n)
        self.best_ny = np.zeros(n)
        self.best_nz = np.full(n, NZ)
        self.best_pr_x = self.fr_x.astype(np.float64)    # Event(x, y, t): best_pr = fr (event.h:31-35)
        self.best_pr_y = self.fr_y.astype(np.float64)

    def project_all(self, nx, ny, nz=NZ):
        """One project_all (optimizer_global.cpp:4-79).  Returns (blurred bordered image, current_scores, S)."""
        w = self.w
        img, pr_x, pr_y, X, Y, ok = project_img(self.fr_x, self.fr_y, self.t, w, nx, ny, nz)
        off = w["scale"] // 2 + w["metric_wsize"] // 2
        ssum, scnt = window_sums(img, w)
        es = ssum[X + off, Y + off]
        ec = scnt[X + off, Y + off]
        score = np.where(ec > 0, es / np.maximum(ec, 1), 0.0)          # get_event_score: a double
        f32 = score.astype(np.float32)                                  # current_scores is CV_32FC1
        cur = np.zeros((w["scale_img_x"], w["scale_img_y"]), dtype=np.float32)
        cur[X[ok], Y[ok]] = f32[ok]
        S = int(score_fixed(es[ok], ec[ok]).sum()) if ok.any() else 0
        # apply_score (event.h:113-121) on every accepted event, strict >
        up = ok & (f32.astype(np.float64) > self.max_score)
        self.max_score[up] = f32[up]
        self.best_nx[up] = nx
        self.best_ny[up] = ny
        self.best_nz[up] = nz
        self.best_pr_x[up] = pr_x[up]
        self.best_pr_y[up] = pr_y[up]
        return img, cur, S

    def search(self, xs, ys, nz=NZ):
        """compute_flow_bruteforce over the given candidate values (nx outer, ny inner).  Returns (surface, best)."""
        surf = np.zeros((len(xs), len(ys)), dtype=np.int64)
        for i, nx in enumerate(xs):
            for j, ny in enumerate(ys):
                surf[i, j] = self.project_all(nx, ny, nz)[2]
        k = int(np.argmax(surf)) if surf.size else 0      # first maximum in row-major (sweep) order
        return surf, (xs[k // len(ys)], ys[k % len(ys)], int(surf.flat[k]))

    def best_uv(self):
        """Event::compute_uv (event.h:135-142) of each event's winning candidate."""
        u = np.zeros(len(self.best_nx))
        v = np.zeros(len(self.best_nx))
        for i, (nx, ny, nz) in enumerate(zip(self.best_nx, self.best_ny, self.best_nz)):
            u[i], v[i] = compute_uv(nx, ny, nz)
        return u, v


def compute_uv(nx, ny, nz=NZ):
    xy_len = math.hypot(nx, ny)
    speed = xy_len / (nz / (1000000000 / (1 * 10000)))
    if xy_len == 0:
        return 0.0, 0.0
    return speed * nx / xy_len, speed * ny / xy_len

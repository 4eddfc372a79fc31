"""numpy restatement of the per-pixel flow rule stated in include/bf_accel.h ("per-pixel flow": bf_flow_field,
bf_color_flow_img; reference: EventFile::color_flow_img, event_file.h:318-350) -- TEST INFRASTRUCTURE ONLY.

Pixel of an event, ownership on the upload index, H / S with the x86 double -> uchar conversion, colour through the stated
HSV -> BGR float formula, the .flo layout and the flow-frame composition."""
import numpy as np

LAST_UPLOADED, FIRST_UPLOADED = 0, 1
INT_MIN = -2 ** 31
LOG_1025 = 0.024692612590371414          # log(1.025) as a double (0x1.949052e1d202ep-6)


def trunc_x86(v):
    """`int x = <double>` on x86-64 (cvttsd2si): truncation toward zero; NaN / out of the int32 range -> INT_MIN."""
    v = np.asarray(v, dtype=np.float64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)          # False for NaN
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), INT_MIN).astype(np.int64)


def to_uchar(v):
    """`uchar c = <double>`: the low byte of trunc_x86."""
    return (trunc_x86(v) & 0xff).astype(np.uint8)


def flow_field(pr_x, pr_y, u, v, noise, res_x, res_y, rule):
    """(owner, U, V), each (res_x, res_y): upload index of the owning event (-1: none) and its flow (0: none)."""
    n = len(pr_x)
    x, y = trunc_x86(pr_x), trunc_x86(pr_y)
    keep = (x >= 0) & (x < res_x) & (y >= 0) & (y < res_y)
    if noise is not None:
        keep &= np.asarray(noise) == 0
    idx = np.nonzero(keep)[0]
    pix = x[idx] * res_y + y[idx]
    if rule == FIRST_UPLOADED:
        owner = np.full(res_x * res_y, n, dtype=np.int64)
        np.minimum.at(owner, pix, idx)
        owner[owner == n] = -1
    else:
        owner = np.full(res_x * res_y, -1, dtype=np.int64)
        np.maximum.at(owner, pix, idx)
    has = owner >= 0
    U, V = np.zeros(res_x * res_y), np.zeros(res_x * res_y)
    U[has] = np.asarray(u, dtype=np.float64)[owner[has]]
    V[has] = np.asarray(v, dtype=np.float64)[owner[has]]
    return owner.astype(np.int32).reshape(res_x, res_y), U.reshape(res_x, res_y), V.reshape(res_x, res_y)


def hs_values(u, v):
    """(angle / 2, log_spd) as doubles: what the reference converts to the H and S bytes (event_file.h:330-338)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        speed = np.hypot(u, v)
        angle = np.where(speed != 0, (np.arctan2(v, u) + 3.1416) * 180 / 3.1416, 0.0)
        q = np.log(speed) / LOG_1025
        log_spd = np.where(q < 255.0, q, 255.0)              # std::min(255.0, q): 255 for a NaN q
    return angle / 2, log_spd


def near_integer(x, rel=1e-9):
    """Values within rel (relative) of an integer: where a last-place difference of atan2 / log / hypot may move a byte."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    r = np.where(fin, np.rint(np.where(fin, x, 0.0)), 0.0)
    return fin & (np.abs(x - r) <= rel * np.maximum(np.abs(x), 1.0))


def at_risk(u, v, rel=1e-9):
    """Where a last-place difference of atan2 / log / hypot between two math libraries may move the H or the S byte: angle / 2
    or log(speed) / log(1.025) within rel of an integer.  A quotient above 255 (1 + rel) is not at risk: std::min replaces it by
    the constant 255.0 whatever its last place says."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    a2, _ = hs_values(u, v)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.log(np.hypot(u, v)) / LOG_1025
    return near_integer(a2, rel) | (near_integer(q, rel) & (q <= 255.0 * (1.0 + rel)))


def hsv_to_bgr(H, S, V):
    """The HSV -> BGR convention stated in include/bf_accel.h (bf_color_time_img), vectorised in float32."""
    H, S, V = (np.asarray(a).astype(np.int64) for a in (H, S, V))
    h = H.astype(np.float32) * np.float32(6.0 / 180.0)
    sec = np.floor(h).astype(np.int64)
    f = h - sec.astype(np.float32)
    sec %= 6
    s = S.astype(np.float32) * np.float32(1.0 / 255.0)
    v = V.astype(np.float32) * np.float32(1.0 / 255.0)
    one = np.float32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))])
    m = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    out = np.empty(H.shape + (3,), dtype=np.uint8)
    idx = np.arange(H.size).reshape(H.shape)
    flat = tab.reshape(4, -1)
    for ch in range(3):
        x = flat[m[sec, ch].ravel(), idx.ravel()].reshape(H.shape) * np.float32(255.0)
        out[..., ch] = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    return out


def color_flow(owner, U, V):
    """(bgr, hs): the (res_x, res_y, 3) B, G, R image and the (res_x, res_y, 2) H, S bytes of a field."""
    has = owner >= 0
    a2, ls = hs_values(U, V)
    H = np.where(has, to_uchar(a2), 0).astype(np.uint8)
    S = np.where(has, to_uchar(ls), 0).astype(np.uint8)
    return hsv_to_bgr(H, S, np.full(H.shape, 255)), np.stack([H, S], axis=-1)


def flo_payload(owner, U, V):
    """(res_x, res_y, 2) float32: horizontal = v, vertical = u; 1e9 in both without an event."""
    out = np.stack([V.astype(np.float32), U.astype(np.float32)], axis=-1)
    out[owner < 0] = np.float32(1e9)
    return out


def flo_file(owner, U, V):
    p = flo_payload(owner, U, V)
    return np.float32(202021.25).astype("<f4").tobytes() + np.array([p.shape[1], p.shape[0]], "<i4").tobytes() + p.astype("<f4").tobytes()


def flow_frame(gray_comp, bgr, gray_raw):
    """compose_flow_frame (frame_writer.h): (res_x, 3 res_y, 3) B, G, R -- compensated grey | colour-coded flow | raw grey."""
    g = lambda a: np.repeat(np.asarray(a, dtype=np.uint8)[..., None], 3, axis=2)
    return np.concatenate([g(gray_comp), bgr, g(gray_raw)], axis=1)


def ppm_payload(frame_bgr):
    return np.ascontiguousarray(frame_bgr[..., ::-1])       # top-down R, G, B


def avi_payload(frame_bgr):
    rows, cols, _ = frame_bgr.shape
    stride = (cols * 3 + 3) & ~3
    out = np.zeros((rows, stride), dtype=np.uint8)
    out[:, :cols * 3] = frame_bgr[::-1].reshape(rows, cols * 3)   # bottom-up B, G, R, zero padding
    return out

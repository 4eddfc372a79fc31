"""The binary per-event flow file of `bf_motion_compensator --outfile-bin` (better_flow_amd/host/better_flow/event_reader.h).

Little endian: magic "BFFLSOA1", u64 n, then u64 t_ns[n], u16 row[n], u16 col[n], f64 u[n], f64 v[n] -- the columns of
the -o table ("t row col 1 v u" per text line).

And the per-pixel flow field of `--flow-field`, flow_N.flo: the Middlebury layout -- float32 202021.25, int32 width, int32
height, then per pixel, row-major, float32 horizontal and vertical flow.  Width = sensor columns (RES_Y), height = sensor rows
(RES_X); horizontal = best_v, vertical = best_u (the swap the -o table makes); 1e9 in both for a pixel without an event."""
import numpy as np

MAGIC = b"BFFLSOA1"
COLUMNS = (("t", "<u8"), ("row", "<u2"), ("col", "<u2"), ("u", "<f8"), ("v", "<f8"))


def read_flow_bin(path):
    """Return dict(t, row, col, u, v) of numpy arrays (uint64, uint16, uint16, float64, float64)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 16 or data[:8] != MAGIC:
        raise ValueError("%s: not a BFFLSOA1 flow file" % path)
    n = int(np.frombuffer(data, "<u8", 1, 8)[0])
    need = 16 + n * sum(np.dtype(d).itemsize for _, d in COLUMNS)
    if len(data) != need:
        raise ValueError("%s: %d bytes, a table of %d rows has %d" % (path, len(data), n, need))
    out, at = {}, 16
    for name, d in COLUMNS:
        out[name] = np.frombuffer(data, d, n, at).astype(np.dtype(d).newbyteorder("="))
        at += n * np.dtype(d).itemsize
    return out


def write_flow_bin(path, t, row, col, u, v):
    """The same file from five columns (for tests and tools)."""
    n = len(t)
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(np.uint64(n).astype("<u8").tobytes())
        for (name, d), col_ in zip(COLUMNS, (t, row, col, u, v)):
            a = np.asarray(col_)
            if len(a) != n:
                raise ValueError("column %s has %d rows, not %d" % (name, len(a), n))
            f.write(a.astype(d).tobytes())


FLO_TAG = 202021.25
FLO_NO_EVENT = 1e9


def read_flo(path):
    """Return (u, v, valid): (rows, cols) float32 row flow, column flow, and the mask of pixels that hold an event."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or np.frombuffer(data, "<f4", 1)[0] != np.float32(FLO_TAG):
        raise ValueError("%s: not a .flo file" % path)
    w, h = (int(x) for x in np.frombuffer(data, "<i4", 2, 4))
    if w < 0 or h < 0 or len(data) != 12 + 8 * w * h:
        raise ValueError("%s: %d bytes, a %d x %d field has %d" % (path, len(data), w, h, 12 + 8 * w * h))
    a = np.frombuffer(data, "<f4", 2 * w * h, 12).reshape(h, w, 2).astype(np.float32)
    valid = ~((a[..., 0] == np.float32(FLO_NO_EVENT)) & (a[..., 1] == np.float32(FLO_NO_EVENT)))
    return a[..., 1].copy(), a[..., 0].copy(), valid


def write_flo(path, u, v, valid=None):
    """The same file from a (rows, cols) row flow u and column flow v (for tests and tools)."""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    a = np.stack([v, u], axis=-1)
    if valid is not None:
        a[~np.asarray(valid, dtype=bool)] = np.float32(FLO_NO_EVENT)
    with open(path, "wb") as f:
        f.write(np.float32(FLO_TAG).astype("<f4").tobytes())
        f.write(np.array([u.shape[1], u.shape[0]], dtype="<i4").tobytes())
        f.write(a.astype("<f4").tobytes())

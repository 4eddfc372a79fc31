"""The binary per-event flow file of `bf_motion_compensator --outfile-bin` (better_flow_amd/host/better_flow/event_reader.h).

Little endian: magic "BFFLSOA1", u64 n, then u64 t_ns[n], u16 row[n], u16 col[n], f64 u[n], f64 v[n] -- the columns of
the -o table ("t row col 1 v u" per text line)."""
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

"""numpy restatement of bf_propose_models (include/bf_accel.h, "event groups: candidate models"): the votes
of the per-event best flow on the search's lattice, the box smoothing, the greedy pick with suppression, and the models.

Everything after the index match is an integer, so the device's results must EQUAL these."""
import numpy as np

import global_ref as gref
import groups_ref


def lattice_values(opts=None):
    """(x_vals, y_vals, nz) of a bf_global_search_opts-like object (attributes x_low .. nz) or dict; None: the defaults."""
    if opts is None:
        xs, ys = gref.default_grid()
        return xs, ys, gref.NZ
    g = (lambda k: opts[k]) if isinstance(opts, dict) else (lambda k: getattr(opts, k))
    return gref.sweep_values(g("x_low"), g("x_hi"), g("x_step")), gref.sweep_values(g("y_low"), g("y_hi"), g("y_step")), g("nz")


def index_of(vals, v):
    """Per element of v the index i with vals[i] == v (exact double equality; vals strictly increasing), or -1."""
    vals = np.asarray(vals, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    i = np.searchsorted(vals, v, side="left")
    ic = np.minimum(i, len(vals) - 1)
    return np.where((i < len(vals)) & (vals[ic] == v), ic, -1).astype(np.int64)


def votes(max_score, best_nx, best_ny, xs, ys, mutate=None):
    """-> (H uint32 [n_x, n_y], dict(voted, unscored, off_lattice))."""
    max_score = np.asarray(max_score, dtype=np.float64)
    scored = max_score > 0
    if mutate == "count_unscored":
        scored = np.ones(len(max_score), dtype=bool)
    i = index_of(xs, best_nx)
    j = index_of(ys, best_ny)
    on = (i >= 0) & (j >= 0)
    ok = scored & on
    H = np.zeros((len(xs), len(ys)), dtype=np.uint32)
    np.add.at(H, (i[ok], j[ok]), 1)
    return H, dict(voted=int(ok.sum()), unscored=int((~scored).sum()), off_lattice=int((scored & ~on).sum()))


def box(H, r):
    """B[i][j] = sum of H over |a|, |b| <= r, zero outside the lattice."""
    return gref._box(H.astype(np.int64), -r, r).astype(np.uint32)


def pick(H, B, suppress, max_models, min_votes, mutate=None):
    """The greedy pick -> [(index, votes, peak)] in pick order."""
    n_x, n_y = B.shape
    free = np.ones(B.shape, dtype=bool)
    out = []
    flat = B.astype(np.int64)
    for _ in range(max_models):
        if not free.any():
            break
        cand = np.where(free, flat, -1).ravel()
        if mutate == "ties_up":
            k = len(cand) - 1 - int(np.argmax(cand[::-1]))
        else:
            k = int(np.argmax(cand))            # the first of the largest: the lowest index
        if cand[k] < min_votes:
            break
        i, j = divmod(k, n_y)
        out.append((k, int(B[i, j]), int(H[i, j])))
        free[max(0, i - suppress):i + suppress + 1, max(0, j - suppress):j + suppress + 1] = False
    return out


def propose(max_score, best_nx, best_ny, xs, ys, nz=gref.NZ, radius=1, suppress=2, max_models=8, min_votes=1, mutate=None):
    """-> (models, proposals, info, H, B): models as groups_ref.warm_from_flow gives them, proposals a list of dicts (nx, ny,
    u, v, index, votes, peak), info a dict with the fields of bf_propose_info."""
    H, info = votes(max_score, best_nx, best_ny, xs, ys, mutate)
    B = box(H, radius)
    picks = pick(H, B, suppress, max_models, min_votes, mutate) if len(np.asarray(max_score)) else []
    props, models = [], []
    for k, v, p in picks:
        nx, ny = xs[k // len(ys)], ys[k % len(ys)]
        u, w = gref.compute_uv(nx, ny, nz)
        props.append(dict(nx=nx, ny=ny, u=u, v=w, index=k, votes=v, peak=p))
        models.append(groups_ref.warm_from_flow(nx, ny))
    info.update(n_x=len(xs), n_y=len(ys), proposals=len(props))
    return models, props, info, H, B


def flat_proposals(props):
    """The proposals as the bytes of a bf_proposal array."""
    dt = np.dtype([("nx", "<f8"), ("ny", "<f8"), ("u", "<f8"), ("v", "<f8"), ("index", "<i8"), ("votes", "<i4"), ("peak", "<i4")])
    a = np.zeros(len(props), dtype=dt)
    for i, p in enumerate(props):
        a[i] = tuple(p[k] for k in dt.names)
    return a

"""Two numpy-level restatements of the -o table's marking rule (DVS_flow::get_accumulated, dvs_flow.h:351-389).

host_rows: StreamEngine::get_accumulated (HostFlowAccumulator::table, flow_table.h) literally -- per-pixel prev / next
  chains over the whole history, a mark array per slice, an emitted event marking its later copies, same-pixel predecessors less than 0.1 ms before it and
  same-instant successors in every later slice.
device_rows: the form bf_emit.hip computes -- a covered byte per ring position read before the slice and written after
  it, the slice sorted by (pixel, arrival) and walked from each element (the pull form), and a per-pixel tail for marks
  beyond the slice's end.

A slice is (first, n, start_time, lead); both return the emitted arrival numbers in output order."""
import numpy as np

REACH = 100000


def host_rows(ts, pix, slices):
    ts = np.asarray(ts, dtype=np.uint64)
    N = len(ts)
    prev = [-1] * N
    nxt = [-1] * N
    last = {}
    for g in range(N):
        p = int(pix[g])
        if p in last:
            prev[g] = last[p]
            nxt[last[p]] = g
        last[p] = g
    K = len(slices)
    mark = []
    for (first, n, start, _lead) in slices:
        m = np.zeros(n, dtype=bool)
        for q in range(n):
            if int(ts[first + q]) >= start:
                break
            if int(ts[first + q]) + 1 == start:
                m[q] = True
        mark.append(m)
    out = []

    def mark_later(i, c):
        for j in range(i + 1, K):
            f, n = slices[j][0], slices[j][1]
            if f > c:
                break
            if c < f + n:
                mark[j][c - f] = True

    def emit(i, g):
        t = int(ts[g])
        if i + 1 < K:
            mark_later(i, g)
            c = prev[g]
            while c != -1 and ((t - int(ts[c])) & 0xFFFFFFFFFFFFFFFF) < REACH:
                mark_later(i, c)
                c = prev[c]
            c = nxt[g]
            while c != -1 and int(ts[c]) == t:
                mark_later(i, c)
                c = nxt[c]
        out.append(g)

    for i, (first, n, start, lead) in enumerate(slices):
        if lead:
            emit(i, first - 1)
        for q in range(n):
            if not mark[i][q]:
                emit(i, first + q)
    return out


def device_rows(ts, pix, slices, cap):
    ts = np.asarray(ts, dtype=np.uint64)
    plane = np.zeros(cap, dtype=bool)
    tail = {}                      # pixel -> (T, last arrival of the slice that set it)
    prev_end = 0
    out = []
    for (first, n, start, lead) in slices:
        els = ([first - 1] if lead else []) + list(range(first, first + n))
        if not els:
            continue
        t = [int(ts[g]) for g in els]
        p = [int(pix[g]) for g in els]
        emitted, before = [], []
        for k, g in enumerate(els):
            if lead and k == 0:
                emitted.append(True)
                before.append(False)
                continue
            cov = g < prev_end and bool(plane[g % cap])
            tl = tail.get(p[k])
            if tl is not None and g > tl[1] and t[k] == tl[0]:
                cov = True
            before.append(cov)
            emitted.append(not cov and t[k] - start != -1)
        order = sorted(range(len(els)), key=lambda k: (p[k], k))
        where = {k: s for s, k in enumerate(order)}
        t_new, last = t[-1], first + n - 1
        new_tail = dict(tail)
        for k in range(len(els)):
            if emitted[k] and t[k] == t_new and (p[k] not in tail or tail[p[k]][0] != t_new):
                new_tail[p[k]] = (t_new, last)
        cover = {}
        for k in range(1 if lead else 0, len(els)):
            cov = before[k] or emitted[k]
            s = where[k] + 1
            while not cov and s < len(order) and p[order[s]] == p[k] and t[order[s]] - t[k] < REACH:
                cov = emitted[order[s]]
                s += 1
            s = where[k] - 1
            while not cov and s >= 0 and p[order[s]] == p[k] and t[order[s]] == t[k]:
                cov = emitted[order[s]]
                s -= 1
            cover[els[k]] = cov
        for g, cov in cover.items():
            plane[g % cap] = cov
        tail = new_tail
        out.extend(g for g, e in zip(els, emitted) if e)
        prev_end = max(prev_end, first + n)
    return out

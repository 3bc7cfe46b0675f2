"""The cost-to-go field of tsl_nav_field.hip (include/taichislam_hip.h) restated twice, independently: `relax`, whole-grid
relaxation to the fixed point in numpy with int64, and `dijkstra`, a heap in plain Python; plus the parents and the path walk.  All integer: the
GPU's planes must equal these byte for byte."""
import heapq

import numpy as np

UNREACHED = 0xFFFFFFFF
MAXV = 0xFFFFFFFE
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))          # direction codes 0 .. 7: (di, dj), i the row
STEP = (5, 7, 5, 7, 5, 7, 5, 7)
_INF = 1 << 62


def planes(cost):
    c = np.asarray(cost, np.uint8)
    return c[None] if c.ndim == 2 else c


def seed_table(goals):
    """int64 [S, 4] = plane, row, col, value from [S, 3] (value 0) or [S, 4]; the value is read as uint32"""
    g = np.asarray(goals, np.int64).reshape(-1, np.shape(goals)[-1] if np.size(goals) else 4)
    if g.shape[1] == 3:
        g = np.concatenate([g, np.zeros((g.shape[0], 1), np.int64)], 1)
    g = g.copy()
    g[:, 3] &= 0xFFFFFFFF
    return g


def seed_plane(cost, goals, lethal):
    """(int64 [B, H, W] least seed value per cell, _INF where there is none; the number of bad seeds)"""
    c = planes(cost)
    B, H, W = c.shape
    s = np.full((B, H, W), _INF, np.int64)
    bad = 0
    for p, r, q, v in seed_table(goals).tolist():
        if not (0 <= p < B and 0 <= r < H and 0 <= q < W) or c[p, r, q] >= lethal:
            bad += 1
            continue
        s[p, r, q] = min(s[p, r, q], min(v, MAXV))
    return s, bad


def _shift(a, di, dj, fill):
    """b[i, j] = a[i + di, j + dj], `fill` outside"""
    H, W = a.shape[-2:]
    b = np.full_like(a, fill)
    i0, i1 = max(0, -di), min(H, H - di)
    j0, j1 = max(0, -dj), min(W, W - dj)
    if i0 < i1 and j0 < j1:
        b[..., i0:i1, j0:j1] = a[..., i0 + di:i1 + di, j0 + dj:j1 + dj]
    return b


def move_masks(cost, lethal, connectivity):
    """bool [8][B, H, W]: the move of code d out of the cell is allowed (the cell itself traversable)"""
    c = planes(cost)
    t = c < lethal
    nb = [_shift(t, di, dj, False) for di, dj in DIRS]
    out = []
    for d in range(8):
        ok = t & nb[d]
        if d & 1:
            ok = ok & nb[d - 1] & nb[(d + 1) & 7] if connectivity == 8 else np.zeros_like(t)
        out.append(ok)
    return out


def relax(cost, goals, neutral=50, lethal=253, connectivity=8, start=None):
    """whole-grid relaxation to the fixed point: (field uint32 [B, H, W], n_bad_seeds).  start: an int64 field to start from instead of the seeds"""
    c = planes(cost)
    s, bad = seed_plane(c, goals, lethal)
    f = s if start is None else np.where(np.asarray(start, np.int64).reshape(c.shape) == UNREACHED, _INF, np.asarray(start, np.int64).reshape(c.shape))
    ok = move_masks(c, lethal, connectivity)
    w = neutral + c.astype(np.int64)
    while True:
        g = f
        for d, (di, dj) in enumerate(DIRS):
            cand = np.where(ok[d], np.minimum(_shift(f, di, dj, _INF) + STEP[d] * w, MAXV), _INF)
            cand = np.where(_shift(f, di, dj, _INF) >= _INF, _INF, cand)
            g = np.minimum(g, cand)
        if np.array_equal(g, f):
            break
        f = g
    return np.where(f >= _INF, UNREACHED, f).astype(np.uint32), bad


def dijkstra(cost, goals, neutral=50, lethal=253, connectivity=8):
    """heap Dijkstra in plain Python: (field uint32 [B, H, W], n_bad_seeds)"""
    c = planes(cost)
    B, H, W = c.shape
    s, bad = seed_plane(c, goals, lethal)
    out = np.full((B, H, W), UNREACHED, np.uint32)
    for p in range(B):
        cs = c[p].tolist()
        dist = [[_INF] * W for _ in range(H)]
        heap = []
        for r, q in np.argwhere(s[p] < _INF).tolist():
            dist[r][q] = int(s[p, r, q])
            heap.append((dist[r][q], r, q))
        heapq.heapify(heap)
        while heap:
            dv, r, q = heapq.heappop(heap)
            if dv > dist[r][q]:
                continue
            # a move INTO (r, q) from a neighbour x costs s * (neutral + cost[x]): the cell that is left pays
            for d, (di, dj) in enumerate(DIRS):
                if (d & 1) and connectivity != 8:
                    continue
                xr, xq = r - di, q - dj
                if not (0 <= xr < H and 0 <= xq < W) or cs[xr][xq] >= lethal:
                    continue
                if (d & 1) and (cs[xr + di][xq] >= lethal or cs[xr][xq + dj] >= lethal):
                    continue
                nv = min(dv + STEP[d] * (neutral + cs[xr][xq]), MAXV)
                if nv < dist[xr][xq]:
                    dist[xr][xq] = nv
                    heapq.heappush(heap, (nv, xr, xq))
        d = np.array(dist, np.int64)
        out[p] = np.where(d >= _INF, UNREACHED, d).astype(np.uint32)
    return out, bad


def parents(cost, field, goals, neutral=50, lethal=253, connectivity=8):
    """u8 [B, H, W]: 255 unreached, 8 where the field equals a seed value placed on the cell, else the lowest code whose neighbour explains the field"""
    c = planes(cost)
    f = np.asarray(field, np.uint32).reshape(c.shape).astype(np.int64)
    s, _ = seed_plane(c, goals, lethal)
    ok = move_masks(c, lethal, connectivity)
    w = neutral + c.astype(np.int64)
    par = np.full(c.shape, 255, np.uint8)
    for d in range(7, -1, -1):
        di, dj = DIRS[d]
        fn = _shift(f, di, dj, UNREACHED)
        hit = ok[d] & (fn != UNREACHED) & (np.minimum(fn + STEP[d] * w, MAXV) == f)
        par[hit] = d
    par[s == f] = 8
    par[f == UNREACHED] = 255
    return par


def field_and_parent(cost, goals, neutral=50, lethal=253, connectivity=8, how=relax):
    f, bad = how(cost, goals, neutral, lethal, connectivity)
    return {"field": f, "parent": parents(cost, f, goals, neutral, lethal, connectivity), "n_bad_seeds": bad}


def follow(field, parent, starts, L):
    """the walk of tsl_tsdf_nav_field_paths: cells int16 [P, L, 2], length int32 [P], status u8 [P], cost uint32 [P]"""
    f = np.asarray(field, np.uint32)
    f = f[None] if f.ndim == 2 else f
    par = np.asarray(parent, np.uint8).reshape(f.shape)
    B, H, W = f.shape
    st = np.asarray(starts, np.int64).reshape(-1, 3)
    P = st.shape[0]
    cells = np.full((P, L, 2), -1, np.int16)
    length, status, cost = np.zeros(P, np.int32), np.zeros(P, np.uint8), np.full(P, UNREACHED, np.uint32)
    for n, (p, r, q) in enumerate(st.tolist()):
        if not (0 <= p < B and 0 <= r < H and 0 <= q < W):
            status[n] = 3
            continue
        cost[n] = f[p, r, q]
        if f[p, r, q] == UNREACHED or par[p, r, q] > 8:
            status[n] = 2
            continue
        status[n] = 1
        for t in range(L):
            cells[n, t] = (r, q)
            length[n] = t + 1
            d = int(par[p, r, q])
            if d == 8:
                status[n] = 0
                break
            if d > 8:
                status[n] = 2
                break
            r, q = r + DIRS[d][0], q + DIRS[d][1]
            if not (0 <= r < H and 0 <= q < W):
                status[n] = 2
                break
    return cells, length, status, cost


def check_path(cost, field, parent, goals, cells, length, neutral=50, lethal=253, connectivity=8, plane=0):
    """one finished path (status 0): follows `parent`, is a chain of allowed moves whose costs sum to the field at its start, and ends on a seed"""
    c = planes(cost)[plane].astype(np.int64)
    f = np.asarray(field, np.uint32).reshape(planes(cost).shape)[plane]
    par = np.asarray(parent, np.uint8).reshape(planes(cost).shape)[plane]
    n = int(length)
    pts = [tuple(int(v) for v in cells[t]) for t in range(n)]
    assert n >= 1 and all(v == -1 for v in np.asarray(cells[n:]).reshape(-1).tolist())
    total = 0
    for a, b in zip(pts[:-1], pts[1:]):
        d = (b[0] - a[0], b[1] - a[1])
        assert d in DIRS, (a, b)
        code = DIRS.index(d)
        assert par[a] == code, (a, b, par[a])
        assert c[a] < lethal and c[b] < lethal
        if code & 1:
            assert connectivity == 8 and c[a[0] + d[0], a[1]] < lethal and c[a[0], a[1] + d[1]] < lethal, (a, b)
        total += STEP[code] * (neutral + int(c[a]))
    end = pts[-1]
    assert par[end] == 8
    vals = [v for p, r, q, v in seed_table(goals).tolist() if (p, r, q) == (plane,) + end]
    assert vals and min(min(vals), MAXV) == int(f[end])
    assert min(total + int(f[end]), MAXV) == int(f[pts[0]]), (total, int(f[end]), int(f[pts[0]]))

"""The 3-D cost-to-go field of tsl_nav_field3.hip (include/taichislam_hip.h) restated twice, independently: `relax`, whole-volume
relaxation to the fixed point in numpy with int64 and 26 shifted copies, and `dijkstra`, a heap in plain Python; plus the parents and the path walk.  All
integer: the GPU's volumes must equal these byte for byte."""
import heapq

import numpy as np

UNREACHED = 0xFFFFFFFF
MAXV = 0xFFFFFFFE
SEED = 26
_D2 = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))           # nav_field's codes 0 .. 7: (di, dj)
# direction codes 0 .. 25: (dk, di, dj)
DIRS = tuple((0,) + d for d in _D2) + ((1, 0, 0),) + tuple((1,) + d for d in _D2) + ((-1, 0, 0),) + tuple((-1,) + d for d in _D2)
NZ = tuple(sum(1 for v in d if v) for d in DIRS)
STEP = tuple({1: 5, 2: 7, 3: 9}[n] for n in NZ)
MAXNZ = {6: 1, 18: 2, 26: 3}
_INF = 1 << 62


def seed_table(goals):
    """int64 [S, 4] = layer, row, col, value from [S, 3] (value 0) or [S, 4]; the value is read as uint32"""
    g = np.asarray(goals, np.int64).reshape(-1, np.shape(goals)[-1] if np.size(goals) else 4)
    if g.shape[1] == 3:
        g = np.concatenate([g, np.zeros((g.shape[0], 1), np.int64)], 1)
    g = g.copy()
    g[:, 3] &= 0xFFFFFFFF
    return g


def seed_volume(cost, goals, lethal):
    """(int64 [D, H, W] least seed value per cell, _INF where there is none; the number of bad seeds)"""
    c = np.asarray(cost, np.uint8)
    D, H, W = c.shape
    s = np.full((D, H, W), _INF, np.int64)
    bad = 0
    for k, r, q, v in seed_table(goals).tolist():
        if not (0 <= k < D and 0 <= r < H and 0 <= q < W) or c[k, r, q] >= lethal:
            bad += 1
            continue
        s[k, r, q] = min(s[k, r, q], min(v, MAXV))
    return s, bad


def _shift(a, d, fill):
    """b[k, i, j] = a[k + dk, i + di, j + dj], `fill` outside"""
    b = np.full_like(a, fill)
    src, dst = [], []
    for n, e in zip(a.shape, d):
        lo, hi = max(0, -e), min(n, n - e)
        if lo >= hi:
            return b
        dst.append(slice(lo, hi))
        src.append(slice(lo + e, hi + e))
    b[tuple(dst)] = a[tuple(src)]
    return b


def move_masks(cost, lethal, connectivity):
    """bool [26][D, H, W]: the move of code d out of the cell is allowed: every cell x + (a dk, b di, c dj), a, b, c in {0, 1}, is inside and traversable"""
    t = np.asarray(cost, np.uint8) < lethal
    out = []
    for d, (dk, di, dj) in enumerate(DIRS):
        if NZ[d] > MAXNZ[connectivity]:
            out.append(np.zeros_like(t))
            continue
        ok = t.copy()
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    ok &= _shift(t, (a * dk, b * di, c * dj), False)
        out.append(ok)
    return out


def relax(cost, goals, neutral=50, lethal=253, connectivity=26, start=None):
    """whole-volume relaxation to the fixed point: (field uint32 [D, H, W], n_bad_seeds).  start: a field to start from instead of the seeds"""
    c = np.asarray(cost, np.uint8)
    s, bad = seed_volume(c, goals, lethal)
    f = s if start is None else np.where(np.asarray(start, np.int64).reshape(c.shape) == UNREACHED, _INF, np.asarray(start, np.int64).reshape(c.shape))
    ok = move_masks(c, lethal, connectivity)
    live = [d for d in range(26) if ok[d].any()]
    w = neutral + c.astype(np.int64)
    while True:
        g = f
        for d in live:
            fn = _shift(f, DIRS[d], _INF)
            cand = np.where(ok[d] & (fn < _INF), np.minimum(fn + STEP[d] * w, MAXV), _INF)
            g = np.minimum(g, cand)
        if np.array_equal(g, f):
            break
        f = g
    return np.where(f >= _INF, UNREACHED, f).astype(np.uint32), bad


def dijkstra(cost, goals, neutral=50, lethal=253, connectivity=26):
    """heap Dijkstra in plain Python: (field uint32 [D, H, W], n_bad_seeds)"""
    c = np.asarray(cost, np.uint8)
    D, H, W = c.shape
    s, bad = seed_volume(c, goals, lethal)
    free = (c < lethal).tolist()
    cs = c.tolist()
    dist = np.full((D, H, W), _INF, np.int64).tolist()
    heap = []
    for k, r, q in np.argwhere(s < _INF).tolist():
        dist[k][r][q] = int(s[k, r, q])
        heap.append((dist[k][r][q], k, r, q))
    heapq.heapify(heap)
    moves = [(dk, di, dj, STEP[d]) for d, (dk, di, dj) in enumerate(DIRS) if NZ[d] <= MAXNZ[connectivity]]

    def inside_free(k, r, q):
        return 0 <= k < D and 0 <= r < H and 0 <= q < W and free[k][r][q]

    while heap:
        dv, k, r, q = heapq.heappop(heap)
        if dv > dist[k][r][q]:
            continue
        # a move INTO (k, r, q) from a neighbour x costs s * (neutral + cost[x]): the cell that is left pays
        for dk, di, dj, step in moves:
            xk, xr, xq = k - dk, r - di, q - dj
            if not inside_free(xk, xr, xq):
                continue
            if step > 5 and not all(inside_free(xk + a * dk, xr + b * di, xq + e * dj) for a in (0, 1) for b in (0, 1) for e in (0, 1)):
                continue
            nv = min(dv + step * (neutral + cs[xk][xr][xq]), MAXV)
            if nv < dist[xk][xr][xq]:
                dist[xk][xr][xq] = nv
                heapq.heappush(heap, (nv, xk, xr, xq))
    d = np.array(dist, np.int64)
    return np.where(d >= _INF, UNREACHED, d).astype(np.uint32), bad


def parents(cost, field, goals, neutral=50, lethal=253, connectivity=26):
    """u8 [D, H, W]: 255 unreached, 26 where the field equals a seed value placed on the cell, else the lowest code whose neighbour explains the field"""
    c = np.asarray(cost, np.uint8)
    f = np.asarray(field, np.uint32).reshape(c.shape).astype(np.int64)
    s, _ = seed_volume(c, goals, lethal)
    ok = move_masks(c, lethal, connectivity)
    w = neutral + c.astype(np.int64)
    par = np.full(c.shape, 255, np.uint8)
    for d in range(25, -1, -1):
        fn = _shift(f, DIRS[d], UNREACHED)
        hit = ok[d] & (fn != UNREACHED) & (np.minimum(fn + STEP[d] * w, MAXV) == f)
        par[hit] = d
    par[s == f] = SEED
    par[f == UNREACHED] = 255
    return par


def field_and_parent(cost, goals, neutral=50, lethal=253, connectivity=26, how=relax):
    f, bad = how(cost, goals, neutral, lethal, connectivity)
    return {"field": f, "parent": parents(cost, f, goals, neutral, lethal, connectivity), "n_bad_seeds": bad}


def walk(field, parent, starts, L):
    """the walk of tsl_tsdf_nav_field3_paths: cells int16 [P, L, 3], length int32 [P], status u8 [P], cost uint32 [P]"""
    f = np.asarray(field, np.uint32)
    par = np.asarray(parent, np.uint8).reshape(f.shape)
    D, H, W = f.shape
    st = np.asarray(starts, np.int64).reshape(-1, 3)
    P = st.shape[0]
    cells = np.full((P, L, 3), -1, np.int16)
    length, status, cost = np.zeros(P, np.int32), np.zeros(P, np.uint8), np.full(P, UNREACHED, np.uint32)
    for n, (k, r, q) in enumerate(st.tolist()):
        if not (0 <= k < D and 0 <= r < H and 0 <= q < W):
            status[n] = 3
            continue
        cost[n] = f[k, r, q]
        if f[k, r, q] == UNREACHED or par[k, r, q] > SEED:
            status[n] = 2
            continue
        status[n] = 1
        for t in range(L):
            cells[n, t] = (k, r, q)
            length[n] = t + 1
            d = int(par[k, r, q])
            if d == SEED:
                status[n] = 0
                break
            if d > SEED:
                status[n] = 2
                break
            k, r, q = k + DIRS[d][0], r + DIRS[d][1], q + DIRS[d][2]
            if not (0 <= k < D and 0 <= r < H and 0 <= q < W):
                status[n] = 2
                break
    return cells, length, status, cost


def check_path(cost, field, parent, goals, cells, length, neutral=50, lethal=253, connectivity=26):
    """one finished path (status 0): follows `parent`, is a chain of allowed moves whose costs sum to the field at its start, and ends on a seed"""
    c = np.asarray(cost, np.uint8).astype(np.int64)
    f = np.asarray(field, np.uint32).reshape(c.shape)
    par = np.asarray(parent, np.uint8).reshape(c.shape)
    n = int(length)
    pts = [tuple(int(v) for v in cells[t]) for t in range(n)]
    assert n >= 1 and all(v == -1 for v in np.asarray(cells[n:]).reshape(-1).tolist())
    total = 0
    for a, b in zip(pts[:-1], pts[1:]):
        d = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
        assert d in DIRS, (a, b)
        code = DIRS.index(d)
        assert par[a] == code and NZ[code] <= MAXNZ[connectivity], (a, b, par[a])
        for x in (0, 1):
            for y in (0, 1):
                for z in (0, 1):
                    assert c[a[0] + x * d[0], a[1] + y * d[1], a[2] + z * d[2]] < lethal, (a, b)
        total += STEP[code] * (neutral + int(c[a]))
    end = pts[-1]
    assert par[end] == SEED
    vals = [v for k, r, q, v in seed_table(goals).tolist() if (k, r, q) == end]
    assert vals and min(min(vals), MAXV) == int(f[end])
    assert min(total + int(f[end]), MAXV) == int(f[pts[0]]), (total, int(f[end]), int(f[pts[0]]))

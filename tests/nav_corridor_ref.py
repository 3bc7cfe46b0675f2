"""The free boxes and corridors of tsl_nav_corridor.hip (include/taichislam_hip.h) restated in plain numpy and Python.  The box is
restated twice, independently: `box_slices` tests every slab by slicing the free mask, `BoxTable` by eight lookups in a summed-volume table of the blocked
cells.  `chain` restates the walk along a path, `corridor` the whole entry point.  Nothing here knows about bits, words or waves."""
import numpy as np

BLOCKED, OUTSIDE = 1, 2
TAIL_LINK = 255                                                     # link of the rows past `count` (boxes and seed are -1 there)


def _ext3(ext):
    return tuple(int(e) for e in ext)


def box_slices(free, c, ext):
    """free: bool [D, H, W]; c = (k, i, j); ext = (e_k, e_i, e_j).  Returns ([k0, i0, j0, k1, i1, j1], flag)."""
    D, H, W = free.shape
    ck, ci, cj = (int(v) for v in c)
    ek, ei, ej = _ext3(ext)
    if not (0 <= ck < D and 0 <= ci < H and 0 <= cj < W):
        return [-1] * 6, OUTSIDE
    if not free[ck, ci, cj]:
        return [ck, ci, cj, ck, ci, cj], BLOCKED
    k0 = k1 = ck
    i0 = i1 = ci
    j0 = j1 = cj
    open_ = [True] * 6
    while any(open_):
        if open_[0]:
            n = j0 - 1
            if cj - n <= ej and n >= 0 and free[k0:k1 + 1, i0:i1 + 1, n].all():
                j0 = n
            else:
                open_[0] = False
        if open_[1]:
            n = j1 + 1
            if n - cj <= ej and n < W and free[k0:k1 + 1, i0:i1 + 1, n].all():
                j1 = n
            else:
                open_[1] = False
        if open_[2]:
            n = i0 - 1
            if ci - n <= ei and n >= 0 and free[k0:k1 + 1, n, j0:j1 + 1].all():
                i0 = n
            else:
                open_[2] = False
        if open_[3]:
            n = i1 + 1
            if n - ci <= ei and n < H and free[k0:k1 + 1, n, j0:j1 + 1].all():
                i1 = n
            else:
                open_[3] = False
        if open_[4]:
            n = k0 - 1
            if ck - n <= ek and n >= 0 and free[n, i0:i1 + 1, j0:j1 + 1].all():
                k0 = n
            else:
                open_[4] = False
        if open_[5]:
            n = k1 + 1
            if n - ck <= ek and n < D and free[n, i0:i1 + 1, j0:j1 + 1].all():
                k1 = n
            else:
                open_[5] = False
    return [k0, i0, j0, k1, i1, j1], 0


class BoxTable:
    """The second restatement: T[k, i, j] = the number of blocked cells in [0, k) x [0, i) x [0, j); a slab is free when its count is 0.  The faces are
    driven from a table (axis, sign) instead of six written-out branches."""
    FACES = ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))      # -j, +j, -i, +i, -k, +k

    def __init__(self, free):
        self.shape = free.shape
        self.free = free
        T = np.zeros(tuple(n + 1 for n in free.shape), np.int64)
        T[1:, 1:, 1:] = (~free).astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
        self.T = T

    def blocked_in(self, lo, hi):
        """blocked cells in the box lo .. hi, both inclusive"""
        T = self.T
        a0, b0, c0 = lo
        a1, b1, c1 = hi[0] + 1, hi[1] + 1, hi[2] + 1
        return int(T[a1, b1, c1] - T[a0, b1, c1] - T[a1, b0, c1] - T[a1, b1, c0] + T[a0, b0, c1] + T[a0, b1, c0] + T[a1, b0, c0] - T[a0, b0, c0])

    def box(self, c, ext):
        c = [int(v) for v in c]
        ext = _ext3(ext)
        if any(not (0 <= c[a] < self.shape[a]) for a in range(3)):
            return [-1] * 6, OUTSIDE
        if self.blocked_in(c, c):
            return c + c, BLOCKED
        lo, hi = list(c), list(c)
        live = list(range(6))
        while live:
            for f in list(live):
                axis, sign = self.FACES[f]
                n = (lo[axis] - 1) if sign < 0 else (hi[axis] + 1)
                good = abs(n - c[axis]) <= ext[axis] and 0 <= n < self.shape[axis]
                if good:
                    slo, shi = list(lo), list(hi)
                    slo[axis] = shi[axis] = n
                    good = self.blocked_in(slo, shi) == 0
                if good:
                    (lo if sign < 0 else hi)[axis] = n
                else:
                    live.remove(f)
        return lo + hi, 0


def tries(free, c, ext):
    """Every slab the inflation of c reads, in order, as the kernel divides it among lanes: (axis, sign, rows, words, moved).  A +-j try (axis 2) has
    one item per (k, i) of the box: rows = that count, words = 1.  A +-i or +-k try has one item per (row, 64-bit word of the run j0 .. j1): rows x words
    items.  A wave takes 64 items per pass.  Tries refused by ext or the volume's border read nothing and are left out."""
    c = [int(v) for v in c]
    ext = _ext3(ext)
    out = []
    if any(not (0 <= c[a] < free.shape[a]) for a in range(3)) or not free[tuple(c)]:
        return out
    lo, hi, live = list(c), list(c), list(BoxTable.FACES)
    while live:
        for f in list(live):
            axis, sign = f
            n = lo[axis] - 1 if sign < 0 else hi[axis] + 1
            good = abs(n - c[axis]) <= ext[axis] and 0 <= n < free.shape[axis]
            if good:
                sl = [slice(lo[x], hi[x] + 1) for x in range(3)]
                sl[axis] = n
                good = bool(free[tuple(sl)].all())
                span = [hi[x] - lo[x] + 1 for x in range(3)]
                if axis == 2:
                    out.append((axis, sign, span[0] * span[1], 1, good))
                else:
                    out.append((axis, sign, span[1 - axis], (hi[2] >> 6) - (lo[2] >> 6) + 1, good))
            if good:
                (lo if sign < 0 else hi)[axis] = n
            else:
                live.remove(f)
    return out


def boxes(cost, cells, free_below, ext, how="slices"):
    """tsl_tsdf_nav_boxes: boxes int16 [S, 6], flags u8 [S]"""
    free = np.asarray(cost) < int(free_below)
    cells = np.asarray(cells).reshape(-1, 3)
    table = BoxTable(free) if how == "table" else None
    out, fl = np.empty((len(cells), 6), np.int16), np.empty(len(cells), np.uint8)
    for s, c in enumerate(cells):
        b, f = table.box(c, ext) if table else box_slices(free, c, ext)
        out[s], fl[s] = b, f
    return out, fl


def inside(b, c):
    return all(b[a] <= c[a] <= b[a + 3] for a in range(3))


def meet(a, fa, b, fb):
    """whether two boxes share a cell; the box of a seed outside the volume has none"""
    return fa != OUTSIDE and fb != OUTSIDE and all(max(a[x], b[x]) <= min(a[x + 3], b[x + 3]) for x in range(3))


def chain(box_of, cells, length, Q):
    """The walk along one path.  box_of(c) -> (box, flag); cells [L, 3]; returns boxes [Q, 6], seed [Q], link [Q], count, status."""
    L = len(cells)
    bx, sd, lk = np.full((Q, 6), -1, np.int16), np.full(Q, -1, np.int32), np.full(Q, TAIL_LINK, np.uint8)
    n = min(int(length), L)
    if n <= 0:
        return bx, sd, lk, 0, 2
    s, q, status, prev = 0, 0, 1, None
    while q < Q:
        b, f = box_of(cells[s])
        bx[q], sd[q] = b, s
        lk[q] = (0 if prev is None else (1 if meet(prev[0], prev[1], b, f) else 2)) + (4 if f else 0)
        q += 1
        t = s
        if f == 0:
            while t + 1 < n and inside(b, [int(v) for v in cells[t + 1]]):
                t += 1
        if t == n - 1:
            status = 0
            break
        s = t if t > s else s + 1
        prev = (b, f)
    return bx, sd, lk, q, status


def corridor(cost, cells, length, free_below, ext, Q, how="slices"):
    """tsl_tsdf_nav_corridor: cells int16 [P, L, 3], length [P] -> dict of boxes [P, Q, 6], seed [P, Q], link [P, Q], count [P], status [P]"""
    free = np.asarray(cost) < int(free_below)
    table = BoxTable(free) if how == "table" else None
    memo = {}

    def box_of(c):
        key = tuple(int(v) for v in c)
        if key not in memo:
            memo[key] = table.box(key, ext) if table else box_slices(free, key, ext)
        return memo[key]
    cells = np.asarray(cells)
    P = cells.shape[0]
    out = {"boxes": np.empty((P, Q, 6), np.int16), "seed": np.empty((P, Q), np.int32), "link": np.empty((P, Q), np.uint8), "count": np.empty(P, np.int32),
           "status": np.empty(P, np.uint8)}
    for p in range(P):
        out["boxes"][p], out["seed"][p], out["link"][p], out["count"][p], out["status"][p] = chain(box_of, cells[p], length[p], Q)
    return out


def check_box(free, c, ext, b, f):
    """the properties of a box, from the definition's last line: free, contains its seed, within ext, and no face can move"""
    D, H, W = free.shape
    c = [int(v) for v in c]
    b = [int(v) for v in b]
    if any(not (0 <= c[a] < free.shape[a]) for a in range(3)):
        assert f == OUTSIDE and b == [-1] * 6
        return
    if not free[c[0], c[1], c[2]]:
        assert f == BLOCKED and b == c + c
        return
    assert f == 0
    assert all(0 <= b[a] <= c[a] <= b[a + 3] < free.shape[a] for a in range(3)), (c, b)
    assert all(c[a] - b[a] <= ext[a] and b[a + 3] - c[a] <= ext[a] for a in range(3)), (c, b, ext)
    assert free[b[0]:b[3] + 1, b[1]:b[4] + 1, b[2]:b[5] + 1].all(), (c, b)
    for a in range(3):
        for sign in (-1, 1):
            n = b[a] - 1 if sign < 0 else b[a + 3] + 1
            if abs(n - c[a]) > ext[a] or not (0 <= n < free.shape[a]):
                continue
            sl = [slice(b[x], b[x + 3] + 1) for x in range(3)]
            sl[a] = n
            assert not free[tuple(sl)].all(), f"the box {b} of {c} can grow on axis {a} towards {sign}"

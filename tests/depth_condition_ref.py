"""The depth conditioning of tsl_depth.hip (include/taichislam_hip.h "depth conditioning") restated twice, independently:
`condition_np`, whole planes shifted against each other in numpy int64, and `condition_loop`, one pixel at a time in plain Python integers, for small
images.  tests/test_depth_condition_cpu.py holds the two against each other; tests/test_depth_condition_gpu.py holds the kernels against condition_np byte for
byte.  Both take depth uint16 [n, h, w] (or [h, w]) and return {"depth", "status", "counts", "levels"} with a leading n (or without)."""
import numpy as np

KEPT, HOLE, RANGE, SPARSE, EDGE = range(5)
DEFAULTS = dict(d_min_mm=1, d_max_mm=65535, min_support=6, erode=1, radius=2, flags=0, levels=0, min_valid=2)


def rq_table(tol):
    return np.minimum(65535, (16 << 16) // np.asarray(tol, np.int64))


def _cfg(kw):
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise TypeError(k)
        c[k] = int(v)
    return c


def _shift(a, dy, dx, fill):
    """b[..., y, x] = a[..., y + dy, x + dx], `fill` where that lies outside the image"""
    h, w = a.shape[-2:]
    b = np.full_like(a, fill)
    ys, ye, xs, xe = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        b[..., ys:ye, xs:xe] = a[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return b


def halve_np(lv, tol, min_valid):
    tol = np.asarray(tol, np.int64)
    h2, w2 = lv.shape[-2] // 2, lv.shape[-1] // 2
    s = lv[..., :2 * h2, :2 * w2].astype(np.int64)
    b = np.stack([s[..., 0::2, 0::2], s[..., 0::2, 1::2], s[..., 1::2, 0::2], s[..., 1::2, 1::2]])
    valid = b > 0
    nv = valid.sum(0)
    ref = np.where(valid, b, 1 << 20).min(0)
    t = tol[np.minimum(ref, 65535) >> 8]
    member = valid & (b - ref <= t)
    m = member.sum(0)
    total = np.where(member, b, 0).sum(0)
    ok = nv >= min_valid
    return np.where(ok, (2 * total + m) // np.maximum(2 * m, 1), 0).astype(np.uint16)


def condition_np(depth, tol, ws, wr, **kw):
    c = _cfg(kw)
    depth = np.asarray(depth, np.uint16)
    single = depth.ndim == 2
    d = depth.reshape((-1,) + depth.shape[-2:]).astype(np.int64)
    tol, ws, wr = np.asarray(tol, np.int64), np.asarray(ws, np.int64), np.asarray(wr, np.int64)
    rq = rq_table(tol)
    hole = d == 0
    rng = ~hole & ((d < c["d_min_mm"]) | (d > c["d_max_mm"]))
    cand = ~hole & ~rng
    t = tol[d >> 8]
    cnt = np.zeros(d.shape, np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                cnt += _shift(cand, dy, dx, False) & (np.abs(_shift(d, dy, dx, 0) - d) <= t)
    sparse = cand & (cnt < c["min_support"])
    seed = sparse | hole if c["flags"] & 1 else sparse
    near = np.zeros(d.shape, bool)
    e = c["erode"]
    for dy in range(-e, e + 1):
        for dx in range(-e, e + 1):
            near |= _shift(seed, dy, dx, False)
    edge = cand & ~sparse & near & (e > 0)
    status = np.zeros(d.shape, np.uint8)
    status[hole], status[rng], status[sparse], status[edge] = HOLE, RANGE, SPARSE, EDGE
    kept = status == KEPT
    num, den = np.zeros(d.shape, np.int64), np.zeros(d.shape, np.int64)
    r = c["radius"]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            diff = _shift(d, dy, dx, 0) - d
            a = np.abs(diff)
            m = kept & _shift(kept, dy, dx, False) & (a <= t)
            qi = np.where(m, (a * rq[d >> 8]) >> 16, 0)
            assert qi.max() <= 16
            wgt = np.where(m, ws[abs(dy), abs(dx)] * wr[qi], 0)
            num += wgt * diff
            den += wgt
    assert (den[kept] > 0).all()
    off = (2 * num + den) // np.maximum(2 * den, 1)                # numpy's // on integers is the floor
    out = np.where(kept, np.clip(d + off, 1, 65535), 0).astype(np.uint16)
    counts = np.stack([(status == s).sum(axis=(1, 2)) for s in range(5)], axis=1).astype(np.int64)
    levels = []
    lv = out
    for _ in range(c["levels"]):
        lv = halve_np(lv, tol, c["min_valid"])
        levels.append(lv)
    if single:
        return {"depth": out[0], "status": status[0], "counts": counts[0], "levels": [l[0] for l in levels]}
    return {"depth": out, "status": status, "counts": counts, "levels": levels}


def _halve_loop(src, tol, min_valid):
    h2, w2 = len(src) // 2, len(src[0]) // 2
    dst = [[0] * w2 for _ in range(h2)]
    for y in range(h2):
        for x in range(w2):
            v = [p for p in (src[2 * y][2 * x], src[2 * y][2 * x + 1], src[2 * y + 1][2 * x], src[2 * y + 1][2 * x + 1]) if p != 0]
            if len(v) < min_valid:
                continue
            ref = min(v)
            mem = [p for p in v if p - ref <= tol[ref >> 8]]
            dst[y][x] = (2 * sum(mem) + len(mem)) // (2 * len(mem))
    return dst


def _frame_loop(D, tol, ws, wr, rq, c):
    h, w = len(D), len(D[0])
    inside = lambda y, x: 0 <= y < h and 0 <= x < w            # noqa: E731
    first = [[HOLE if D[y][x] == 0 else RANGE if (D[y][x] < c["d_min_mm"] or D[y][x] > c["d_max_mm"]) else KEPT for x in range(w)] for y in range(h)]
    st = [row[:] for row in first]
    for y in range(h):
        for x in range(w):
            if first[y][x] != KEPT:
                continue
            n = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if (dy or dx) and inside(yy, xx) and first[yy][xx] == KEPT and abs(D[yy][xx] - D[y][x]) <= tol[D[y][x] >> 8]:
                        n += 1
            if n < c["min_support"]:
                st[y][x] = SPARSE
    second = [row[:] for row in st]
    e = c["erode"]
    for y in range(h):
        for x in range(w):
            if second[y][x] != KEPT:
                continue
            for yy in range(y - e, y + e + 1):
                for xx in range(x - e, x + e + 1):
                    if inside(yy, xx) and (second[yy][xx] == SPARSE or (c["flags"] & 1 and second[yy][xx] == HOLE)):
                        st[y][x] = EDGE
    out = [[0] * w for _ in range(h)]
    r = c["radius"]
    for y in range(h):
        for x in range(w):
            if st[y][x] != KEPT:
                continue
            dp = D[y][x]
            num = den = 0
            for yy in range(y - r, y + r + 1):
                for xx in range(x - r, x + r + 1):
                    if not inside(yy, xx) or st[yy][xx] != KEPT:
                        continue
                    a = abs(D[yy][xx] - dp)
                    if a > tol[dp >> 8]:
                        continue
                    wgt = ws[abs(yy - y)][abs(xx - x)] * wr[(a * rq[dp >> 8]) >> 16]
                    num += wgt * (D[yy][xx] - dp)
                    den += wgt
            out[y][x] = min(max(dp + (2 * num + den) // (2 * den), 1), 65535)           # Python's // is the floor
    return out, st


def condition_loop(depth, tol, ws, wr, **kw):
    c = _cfg(kw)
    depth = np.asarray(depth, np.uint16)
    single = depth.ndim == 2
    frames = depth.reshape((-1,) + depth.shape[-2:])
    tol_l, ws_l, wr_l = [int(v) for v in tol], [[int(v) for v in row] for row in np.asarray(ws)], [int(v) for v in wr]
    rq = [min(65535, (16 << 16) // v) for v in tol_l]
    outs, sts, lvs = [], [], [[] for _ in range(c["levels"])]
    for f in frames:
        o, s = _frame_loop([[int(v) for v in row] for row in f], tol_l, ws_l, wr_l, rq, c)
        outs.append(o)
        sts.append(s)
        lv = o
        for l in range(c["levels"]):
            lv = _halve_loop(lv, tol_l, c["min_valid"])
            lvs[l].append(lv)
    out, status = np.array(outs, np.uint16).reshape(frames.shape), np.array(sts, np.uint8).reshape(frames.shape)
    counts = np.array([[int((s == k).sum()) for k in range(5)] for s in status], np.int64)
    h, w = frames.shape[1:]
    levels = [np.array(lvs[l], np.uint16).reshape(len(frames), h >> (l + 1), w >> (l + 1)) for l in range(c["levels"])]
    if single:
        return {"depth": out[0], "status": status[0], "counts": counts[0], "levels": [l[0] for l in levels]}
    return {"depth": out, "status": status, "counts": counts, "levels": levels}

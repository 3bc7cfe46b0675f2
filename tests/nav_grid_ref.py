"""numpy restatement of the navigation grids (include/taichislam_hip.h "navigation grids") over an export_sparse dictionary:
voxel classes, column counts and spans, cell classes, the distance transform by 2 R + 1 shifted minima per axis in int64, the cost lookup -- and
brute_d2, a second, independent distance (every cell against the list of obstacles) that the CPU tests hold the restatement against."""
import numpy as np

FREE, OCCUPIED, UNKNOWN = 0, 1, 2                # cell classes (TSL_NAV_*)
V_UNKNOWN, V_FREE, V_OCC = 0, 1, 2               # voxel classes
FLAG_UNKNOWN, FLAG_WALL = 1, 2
NO_LO, NO_HI = 32767, -32768


def surf_thres(voxel_scale):
    """the map's surface threshold as the library holds it: (float)(voxel_scale * 1.8)"""
    return np.float32(float(voxel_scale) * 1.8)


def voxel_classes(e, N, Nz, thres):
    """u8 [N, N, Nz]: a voxel the export does not hold is unknown, and so is an observed NaN"""
    c = np.full((N, N, Nz), V_UNKNOWN, np.uint8)
    idx = np.asarray(e["indices"]).astype(np.int64).reshape(-1, 3)
    t = np.asarray(e["TSDF"]).view(np.float16).astype(np.float32).reshape(-1)
    u = idx + np.array([N // 2, N // 2, Nz // 2])
    with np.errstate(invalid="ignore"):
        v = np.where(t < np.float32(thres), V_OCC, np.where(np.isnan(t), V_UNKNOWN, V_FREE)).astype(np.uint8)
    c[u[:, 0], u[:, 1], u[:, 2]] = v
    return c


def columns(vc, Nz, bands):
    """(counts uint16 [B, N, N, 3] = occupied, free, unknown; span int16 [B, N, N, 2] = lowest, highest occupied layer) of the bands [(k_min, k_max)]"""
    N = vc.shape[0]
    counts = np.zeros((len(bands), N, N, 3), np.uint16)
    span = np.zeros((len(bands), N, N, 2), np.int16)
    for b, (k0, k1) in enumerate(bands):
        assert -(Nz // 2) <= k0 <= k1 <= Nz // 2 - 1
        s = vc[:, :, k0 + Nz // 2:k1 + Nz // 2 + 1]
        occ = s == V_OCC
        counts[b, :, :, 0] = occ.sum(2)
        counts[b, :, :, 1] = (s == V_FREE).sum(2)
        counts[b, :, :, 2] = (s == V_UNKNOWN).sum(2)
        some = occ.any(2)
        span[b, :, :, 0] = np.where(some, k0 + occ.argmax(2), NO_LO)                       # the first / the last occupied layer of the band
        span[b, :, :, 1] = np.where(some, k1 - occ[:, :, ::-1].argmax(2), NO_HI)
    return counts, span


def cell_classes(counts, min_occ=1, min_free=1, max_unknown=None):
    n_occ, n_free, n_unk = (counts[..., a].astype(np.int64) for a in range(3))
    free = (n_free >= max(1, int(min_free))) & ((n_unk <= int(max_unknown)) if max_unknown is not None and max_unknown >= 0 else True)
    return np.where(n_occ >= max(1, int(min_occ)), OCCUPIED, np.where(free, FREE, UNKNOWN)).astype(np.uint8)


def _padded(obst, wall):
    """the obstacle mask with the ring of positions just outside the grid around it: obstacles with `wall`, nothing without (what lies beyond the ring
    holds no obstacle and is left out: a shift that reaches beyond the array offers nothing)"""
    n, m = obst.shape
    p = 1
    a = np.zeros((n + 2 * p, m + 2 * p), bool)
    if wall:
        a[:, :] = True
    a[p:p + n, p:p + m] = obst
    return a, p


def edt(obst, R, wall=False):
    """uint16 [n, m]: the squared distance to the nearest True cell of `obst` when it is <= R * R, else R * R + 1.  Along the second axis g = the distance
    to the nearest obstacle of the row capped at R + 1, by 2 R + 1 shifted minima; along the first d2 = min of di * di + g * g, again 2 R + 1 shifts."""
    R = int(R)
    a, p = _padded(np.asarray(obst, bool), wall)
    n, m = a.shape
    g = np.full((n, m), R + 1, np.int64)
    for dj in range(-R, R + 1):
        lo, hi = max(0, -dj), min(m, m - dj)                    # columns uj with 0 <= uj + dj < m
        if lo >= hi:
            continue
        hit = a[:, lo + dj:hi + dj]
        g[:, lo:hi] = np.where(hit, np.minimum(g[:, lo:hi], abs(dj)), g[:, lo:hi])
    g2 = g * g
    d2 = np.full((n, m), R * R + 1, np.int64)
    for di in range(-R, R + 1):
        lo, hi = max(0, -di), min(n, n - di)
        if lo >= hi:
            continue
        d2[lo:hi] = np.minimum(d2[lo:hi], di * di + g2[lo + di:hi + di])
    d2 = np.minimum(d2, R * R + 1)
    return d2[p:n - p, p:m - p].astype(np.uint16)


def brute_d2(obst, R, wall=False):
    """the same by pairwise distances from every cell to the list of obstacles (the wall's positions appended), clipped"""
    obst = np.asarray(obst, bool)
    n, m = obst.shape
    pts = [np.argwhere(obst).astype(np.int64)]
    if wall:
        i, j = np.arange(-1, n + 1), np.arange(-1, m + 1)
        pts += [np.stack([np.full(j.size, v), j], 1) for v in (-1, n)] + [np.stack([i, np.full(i.size, v)], 1) for v in (-1, m)]
    pts = np.concatenate(pts)
    far = int(R) * int(R) + 1
    if pts.shape[0] == 0:
        return np.full((n, m), far, np.uint16)
    ci, cj = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(m, dtype=np.int64), indexing="ij")
    d = (ci[..., None] - pts[:, 0]) ** 2 + (cj[..., None] - pts[:, 1]) ** 2
    return np.minimum(d.min(2), far).astype(np.uint16)


def obstacles(cls, flags):
    return (cls == OCCUPIED) | ((cls == UNKNOWN) if flags & FLAG_UNKNOWN else False)


def distances(cls, R, flags=0):
    """uint16 [B, N, N] from the cell classes"""
    return np.stack([edt(obstacles(c, flags), R, bool(flags & FLAG_WALL)) for c in cls])


def costs(cls, d2, lut, cost_unknown=255):
    lut = np.asarray(lut, np.uint8)
    return np.where(cls == UNKNOWN, np.uint8(cost_unknown), lut[d2.astype(np.int64)]).astype(np.uint8)


def nav_grid(e, N, Nz, voxel_scale, bands, R, free_thres=None, min_occ=1, min_free=1, max_unknown=None, flags=0, lut=None, cost_unknown=255):
    """The planes of tsl_tsdf_nav_grid for the map whose export_sparse dictionary is `e`: {cls, d2, counts, span[, cost]}.  bands: [(k_min, k_max)] voxel
    layers, R in voxels."""
    thres = surf_thres(voxel_scale) if free_thres is None else np.float32(free_thres)
    counts, span = columns(voxel_classes(e, N, Nz, thres), Nz, bands)
    cls = cell_classes(counts, min_occ, min_free, max_unknown)
    out = {"cls": cls, "counts": counts, "span": span, "d2": distances(cls, R, flags)}
    if lut is not None:
        assert np.asarray(lut).size == R * R + 2
        out["cost"] = costs(cls, out["d2"], lut, cost_unknown)
    return out


def assert_equal(got, want, what="", keys=None):
    """every plane both hold, byte for byte"""
    for k in keys or ("cls", "counts", "span", "d2", "cost"):
        if keys is None and (k not in want or k not in got):
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, f"{what}: {k} has shape {g.shape} / {g.dtype}, expected {w.shape} / {w.dtype}"
        bad = np.argwhere(g.view(w.dtype) != w)
        assert bad.shape[0] == 0, f"{what}: {k} differs in {bad.shape[0]} places, first at {bad[0].tolist()}: {g.view(w.dtype)[tuple(bad[0])]} != {w[tuple(bad[0])]}"

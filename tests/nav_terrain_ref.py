"""numpy restatement of the terrain layers (include/taichislam_hip.h "terrain layers for ground robots") over an export_sparse
dictionary, written straight from the definition: dense [N, N, Nz] voxel classes, standable layers and window statistics by plain loops over shifts, q in
float64, the Sobel sums in int64; d2 and cost are nav_grid_ref's transform of its own cls.  brute_column and brute_cell are a second, independent
statement -- one column, one cell at a time, Python loops, no helper shared with the first -- that the CPU tests hold the restatement against."""
import numpy as np

import nav_grid_ref as ng
from nav_grid_ref import FREE, OCCUPIED, UNKNOWN, V_FREE, V_OCC, surf_thres

NO_HEIGHT, NO_STAT, NO_SLOPE = 32767, 65535, 0xffffffff
COL_SUPPORT, COL_OBSTRUCTED, COL_EMPTY = 0, 1, 2
PLANES = ("height", "col", "step", "nsup", "slope2", "cls", "d2", "cost")


def dense(e, N, Nz, thres):
    """(voxel classes u8 [N, N, Nz], TSDF f16 [N, N, Nz], NaN where the export holds nothing)"""
    t = np.full((N, N, Nz), np.nan, np.float16)
    idx = np.asarray(e["indices"]).astype(np.int64).reshape(-1, 3)
    u = idx + np.array([N // 2, N // 2, Nz // 2])
    t[u[:, 0], u[:, 1], u[:, 2]] = np.asarray(e["TSDF"]).view(np.float16).reshape(-1)
    return ng.voxel_classes(e, N, Nz, thres), t


def standable(vc, clearance, free_run):
    """bool [N, N, Nz]: occupied, nothing occupied in the `clearance` layers above, the `free_run` layers above all free; a layer above the volume is
    unknown.  (The shifts run over the columns that hold an occupied voxel; no other column has a standable layer.)"""
    N, _, Nz = vc.shape
    assert 0 <= free_run <= clearance <= Nz
    sel = (vc == V_OCC).any(2)
    c = vc[sel]                                                  # [n, Nz]
    occ, fre = c == V_OCC, c == V_FREE
    ok = occ.copy()
    for d in range(1, clearance + 1):
        ok[:, :Nz - d] &= ~occ[:, d:]                            # (k + d outside the volume: unknown, not occupied)
    for d in range(1, free_run + 1):
        ok[:, :Nz - d] &= fre[:, d:]
        ok[:, Nz - d:] = False                                   # k + d outside the volume: unknown, not free
    out = np.zeros(vc.shape, bool)
    out[sel] = ok
    return out


def supports(vc, t, Nz, thres, bands, clearance, free_run, pick):
    """(height int16 [B, N, N], col u8 [B, N, N])"""
    N = vc.shape[0]
    st = standable(vc, clearance, free_run)
    th = np.float64(np.float32(thres))
    height = np.full((len(bands), N, N), NO_HEIGHT, np.int16)
    col = np.zeros((len(bands), N, N), np.uint8)
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    for b, (k0, k1) in enumerate(bands):
        assert -(Nz // 2) <= k0 <= k1 <= Nz // 2 - 1
        u0, u1 = k0 + Nz // 2, k1 + Nz // 2
        s = st[:, :, u0:u1 + 1]
        has = s.any(2)
        uk = np.where(pick == 0, u0 + s.argmax(2), u1 - s[:, :, ::-1].argmax(2))                # the first / the last standable layer of the band
        uk = np.where(has, uk, 0)
        up = np.minimum(uk + 1, Nz - 1)
        free_above = (uk + 1 < Nz) & (vc[ii, jj, up] == V_FREE)
        tk, tk1 = t[ii, jj, uk].astype(np.float64), t[ii, jj, up].astype(np.float64)
        with np.errstate(all="ignore"):
            r = np.float64(16.0) * (th - tk) / (tk1 - tk)
            q = np.where(r >= 15.0, 15.0, np.where(r >= 0.0, np.floor(r), 0.0)).astype(np.int64)      # (int)r of r >= 0 is its floor; a NaN fails both tests
        q = np.where(free_above, q, 0)
        height[b] = np.where(has, 16 * (uk - Nz // 2) + q, NO_HEIGHT).astype(np.int16)
        occ_any = (vc[:, :, u0:u1 + 1] == V_OCC).any(2)
        col[b] = np.where(has, COL_SUPPORT, np.where(occ_any, COL_OBSTRUCTED, COL_EMPTY))
    return height, col


def _shifted(a, di, dj, fill):
    """out[i, j] = a[i + di, j + dj], `fill` outside"""
    n, m = a.shape
    out = np.full((n, m), fill, a.dtype)
    i0, i1, j0, j1 = max(0, -di), min(n, n - di), max(0, -dj), min(m, m - dj)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out


def window_stats(height, w):
    """(step uint16, nsup uint16) [B, N, N]: (2 w + 1)^2 shifts of the heights"""
    h = height.astype(np.int64)
    step, nsup = np.zeros(h.shape, np.uint16), np.zeros(h.shape, np.uint16)
    for b in range(h.shape[0]):
        mx, mn, n = np.full(h[b].shape, -(1 << 40)), np.full(h[b].shape, 1 << 40), np.zeros(h[b].shape, np.int64)
        for di in range(-w, w + 1):
            for dj in range(-w, w + 1):
                v = _shifted(h[b], di, dj, NO_HEIGHT)
                ok = v != NO_HEIGHT
                mx, mn, n = np.where(ok, np.maximum(mx, v), mx), np.where(ok, np.minimum(mn, v), mn), n + ok
        own = h[b] != NO_HEIGHT
        step[b] = np.where(own, mx - mn, NO_STAT).astype(np.uint16)
        nsup[b] = np.where(own, n, NO_STAT).astype(np.uint16)
    return step, nsup


def sobel(height, s):
    """uint32 [B, N, N]"""
    h = height.astype(np.int64)
    out = np.zeros(h.shape, np.uint32)
    for b in range(h.shape[0]):
        H = {(di, dj): _shifted(h[b], di * s, dj * s, NO_HEIGHT) for di in (-1, 0, 1) for dj in (-1, 0, 1)}
        valid = np.ones(h[b].shape, bool)
        for v in H.values():
            valid &= v != NO_HEIGHT
        gx = H[1, -1] + 2 * H[1, 0] + H[1, 1] - H[-1, -1] - 2 * H[-1, 0] - H[-1, 1]
        gy = H[-1, 1] + 2 * H[0, 1] + H[1, 1] - H[-1, -1] - 2 * H[0, -1] - H[1, -1]
        out[b] = np.where(valid, np.minimum(gx * gx + gy * gy, NO_SLOPE - 1), NO_SLOPE).astype(np.uint32)
    return out


def classes(col, step, nsup, slope2, max_step, max_slope2, min_support):
    st, ns, sl = step.astype(np.int64), nsup.astype(np.int64), slope2.astype(np.int64)
    c = np.where(ns < int(min_support), UNKNOWN, FREE)
    c = np.where((sl != NO_SLOPE) & (sl > int(max_slope2)), OCCUPIED, c)
    c = np.where(st > int(max_step), OCCUPIED, c)
    c = np.where(col == COL_EMPTY, UNKNOWN, c)
    c = np.where(col == COL_OBSTRUCTED, OCCUPIED, c)
    return c.astype(np.uint8)


def nav_terrain(e, N, Nz, voxel_scale, bands, clearance, free_run=1, pick=0, window=1, slope_base=1, max_step=65534, max_slope2=NO_SLOPE, min_support=1, R=0,
                flags=0, lut=None, cost_unknown=255, free_thres=None):
    """The planes of tsl_tsdf_nav_terrain for the map whose export_sparse dictionary is `e`; every limit as the integer the library takes."""
    thres = surf_thres(voxel_scale) if free_thres is None else np.float32(free_thres)
    vc, t = dense(e, N, Nz, thres)
    height, col = supports(vc, t, Nz, thres, bands, clearance, free_run, pick)
    step, nsup = window_stats(height, window)
    slope2 = sobel(height, slope_base)
    cls = classes(col, step, nsup, slope2, max_step, max_slope2, min_support)
    out = {"height": height, "col": col, "step": step, "nsup": nsup, "slope2": slope2, "cls": cls, "d2": ng.distances(cls, R, flags)}
    if lut is not None:
        assert np.asarray(lut).size == R * R + 2
        out["cost"] = ng.costs(cls, out["d2"], lut, cost_unknown)
    return out


# ---- the second statement: one column, one cell at a time --------------------------------------------------------------------------------------
def brute_column(e_lookup, Nz, thres, i, j, k0, k1, clearance, free_run, pick):
    """(height, col) of column (i, j) for the band k0 .. k1.  e_lookup: {(i, j, k): f16 value} of the observed voxels (signed indices)."""
    th32 = np.float32(thres)

    def kind(k):                                                 # 'o', 'f' or 'u'
        if k < -(Nz // 2) or k > Nz // 2 - 1 or (i, j, k) not in e_lookup:
            return "u"
        v = np.float32(e_lookup[(i, j, k)])
        if v != v:
            return "u"
        return "o" if v < th32 else "f"
    found, any_occ = [], False
    for k in range(k0, k1 + 1):
        if kind(k) != "o":
            continue
        any_occ = True
        if any(kind(k + d) == "o" for d in range(1, clearance + 1)):
            continue
        if any(kind(k + d) != "f" for d in range(1, free_run + 1)):
            continue
        found.append(k)
    if not found:
        return NO_HEIGHT, (COL_OBSTRUCTED if any_occ else COL_EMPTY)
    k = found[0] if pick == 0 else found[-1]
    q = 0
    if kind(k + 1) == "f":
        a, b = float(np.float16(e_lookup[(i, j, k)])), float(np.float16(e_lookup[(i, j, k + 1)]))
        num, den = float(th32) - a, b - a
        with np.errstate(all="ignore"):
            r = float(np.float64(16.0) * np.float64(num) / np.float64(den))
        q = 15 if r >= 15.0 else (int(r) if r >= 0.0 else 0)
    return 16 * k + q, COL_SUPPORT


def brute_cell(height, col, ui, uj, w, s, max_step, max_slope2, min_support):
    """(step, nsup, slope2, cls) of cell (ui, uj) of one band's height and col planes"""
    N = height.shape[0]
    h = lambda a, b: int(height[a, b]) if 0 <= a < N and 0 <= b < N else NO_HEIGHT
    if col[ui, uj] != COL_SUPPORT:
        return NO_STAT, NO_STAT, NO_SLOPE, (OCCUPIED if col[ui, uj] == COL_OBSTRUCTED else UNKNOWN)
    vals = [h(ui + a, uj + b) for a in range(-w, w + 1) for b in range(-w, w + 1)]
    vals = [v for v in vals if v != NO_HEIGHT]
    step, nsup = max(vals) - min(vals), len(vals)
    nine = [h(ui + a * s, uj + b * s) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    slope2 = NO_SLOPE
    if NO_HEIGHT not in nine:
        gx = h(ui + s, uj - s) + 2 * h(ui + s, uj) + h(ui + s, uj + s) - h(ui - s, uj - s) - 2 * h(ui - s, uj) - h(ui - s, uj + s)
        gy = h(ui - s, uj + s) + 2 * h(ui, uj + s) + h(ui + s, uj + s) - h(ui - s, uj - s) - 2 * h(ui, uj - s) - h(ui + s, uj - s)
        slope2 = min(gx * gx + gy * gy, NO_SLOPE - 1)
    if step > max_step:
        cls = OCCUPIED
    elif slope2 != NO_SLOPE and slope2 > max_slope2:
        cls = OCCUPIED
    elif nsup < min_support:
        cls = UNKNOWN
    else:
        cls = FREE
    return step, nsup, slope2, cls


def lookup(e):
    idx = np.asarray(e["indices"]).astype(np.int64).reshape(-1, 3)
    t = np.asarray(e["TSDF"]).view(np.float16).reshape(-1)
    return {(int(a), int(b), int(c)): v for (a, b, c), v in zip(idx, t)}


def assert_equal(got, want, what="", keys=None):
    """every plane both hold, byte for byte"""
    for k in keys or PLANES:
        if keys is None and (k not in want or k not in got):
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, f"{what}: {k} has shape {g.shape} / {g.dtype}, expected {w.shape} / {w.dtype}"
        bad = np.argwhere(g.view(w.dtype) != w)
        assert bad.shape[0] == 0, f"{what}: {k} differs in {bad.shape[0]} places, first at {bad[0].tolist()}: {g.view(w.dtype)[tuple(bad[0])]} != {w[tuple(bad[0])]}"

"""numpy float32 restatement of the ESDF point queries (taichislam_amd/csrc/tsl_esdf_query.hip): the GPU results
must equal it bit for bit.  The map is given as a dense grid: val / known [N][N][Nz] indexed by voxel index - lo."""
import numpy as np

F32 = np.float32
CLAMP = F32(16777216.0)          # cell_floor: the cell index is clamped far outside any volume (NaN lands on the clamp)
HALF_DOWN = F32(0.49999997)      # rnd_i: round half away from zero in three instructions (tsl_common.hpp)


def lerp(a, b, t):
    return a + t * (b - a)


def trilinear(c, f, vs):
    """c f32 [n, 8] corner values, c[:, p << 2 | q << 1 | r] = V(b0 + p, b1 + q, b2 + r); f f32 [n, 3] cell fractions; vs the voxel size.
    Returns (dist f32 [n], grad f32 [n, 3]) in the kernel's order of evaluation.  (At f = 0 dist is c000 exactly -- for -0.0 it is +0.0.)"""
    c = np.asarray(c, F32)
    f0, f1, f2 = (np.asarray(f, F32)[:, a] for a in range(3))
    vs = F32(vs)
    c000, c001, c010, c011, c100, c101, c110, c111 = (c[:, k] for k in range(8))
    with np.errstate(invalid="ignore", over="ignore"):
        d = lerp(lerp(lerp(c000, c100, f0), lerp(c010, c110, f0), f1), lerp(lerp(c001, c101, f0), lerp(c011, c111, f0), f1), f2)
        g0 = lerp(lerp(c100 - c000, c110 - c010, f1), lerp(c101 - c001, c111 - c011, f1), f2) / vs
        g1 = lerp(lerp(c010 - c000, c110 - c100, f0), lerp(c011 - c001, c111 - c101, f0), f2) / vs
        g2 = lerp(lerp(c001 - c000, c101 - c100, f0), lerp(c011 - c010, c111 - c110, f0), f1) / vs
    return d.astype(F32), np.stack([g0, g1, g2], 1).astype(F32)


def grid_from_export(idx, val, N, Nz):
    """(val, known, lo) dense grids of a map N x N x Nz from an ESDF export: int16 indices [n, 3] and values [n]."""
    lo = np.array([-(N // 2), -(N // 2), -(Nz // 2)], np.int64)
    g = np.zeros((N, N, Nz), F32)
    k = np.zeros((N, N, Nz), bool)
    i = idx.astype(np.int64) - lo
    g[i[:, 0], i[:, 1], i[:, 2]] = val
    k[i[:, 0], i[:, 1], i[:, 2]] = True
    return g, k, lo


def query(xyz, mode, vs, val, known, lo, unknown=np.nan):
    """(dist f32 [n], grad f32 [n, 3] (zeros for mode 0), status u8 [n]) of tsl_esdf_query_points without the early-stop flag."""
    x = np.asarray(xyz, F32).reshape(-1, 3)
    n = x.shape[0]
    vs = F32(vs)
    shape = np.array(val.shape, np.int64)
    finite = np.isfinite(x).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        u = x / vs
        if mode == 0:
            r = u + np.copysign(HALF_DOWN, u)
            b = np.trunc(np.clip(np.nan_to_num(r, nan=0.0), -CLAMP, CLAMP)).astype(np.int64)
            hi = b
        else:
            fl = np.floor(u)
            fl = np.where(np.isnan(fl), CLAMP, np.clip(fl, -CLAMP, CLAMP)).astype(F32)
            b = fl.astype(np.int64)
            hi = b + 1
            f = (u - fl).astype(F32)
    ub, uh = b - lo, hi - lo
    inside = finite & (ub >= 0).all(1) & (uh < shape).all(1)
    dist = np.full(n, F32(unknown), F32)
    grad = np.zeros((n, 3), F32)
    status = np.full(n, 2, np.uint8)
    w = np.nonzero(inside)[0]
    ub = ub[w]
    if mode == 0:
        kn = known[ub[:, 0], ub[:, 1], ub[:, 2]]
        status[w] = np.where(kn, 0, 1)
        ok = w[kn]
        dist[ok] = val[ub[kn, 0], ub[kn, 1], ub[kn, 2]]
        return dist, grad, status
    c = np.empty((w.size, 8), F32)
    kn = np.ones(w.size, bool)
    for cc in range(8):
        o = ub + np.array([cc >> 2, (cc >> 1) & 1, cc & 1], np.int64)
        c[:, cc] = val[o[:, 0], o[:, 1], o[:, 2]]
        kn &= known[o[:, 0], o[:, 1], o[:, 2]]
    status[w] = np.where(kn, 0, 1)
    d, g = trilinear(c[kn], f[w[kn]], vs)
    dist[w[kn]] = d
    grad[w[kn]] = g
    return dist, grad, status

"""numpy restatement of the depth-and-colour alignment (taichislam_amd/csrc/tsl_align_rgbd.hip).  linearize: float32 in the
written order, the 66 integers of tsl_align_rgbd_sums (geo, then col), which the GPU must equal.  solve / track: float64 scalar code in the written
order, which the library's host functions must equal bit for bit.  Everything the colour term shares with the depth-only alignment is track_ref's:
the sampler, the robust weight, the fixed point, the system of one half, the retraction.  The map is a dense grid (val, known, lo, colour), colour f16
[N][N][Nz][3], as render_view_scenes.oracle_grid(o, colour=True) gives it."""
import math

import numpy as np

import render_view_ref as rv
import track_ref as tr

F32 = np.float32
N_SUMS = 2 * tr.N_SUMS                                   # geo = [0, 33), col = [33, 66)
GEO, COL = slice(0, tr.N_SUMS), slice(tr.N_SUMS, 2 * tr.N_SUMS)
DEFAULT_LEVELS = tr.DEFAULT_LEVELS


def voxel_luminance(col):
    """yv = ((77 r + 150 g) + 29 b) / 256 in f32 of f16 colours [..., 3]"""
    c = np.asarray(col).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (((F32(77.0) * c[..., 0] + F32(150.0) * c[..., 1]) + F32(29.0) * c[..., 2]) / F32(256.0)).astype(F32)


_LUMINANCE = []                                          # (colour grid, its luminance grid) of the last few maps: a track linearises over one map many times


def luminance_grid(colour):
    for c, y in _LUMINANCE:
        if c is colour:
            return y
    y = voxel_luminance(colour)
    _LUMINANCE.append((colour, y))
    del _LUMINANCE[:-3]
    return y


def image_luminance(rgb):
    """yi = (float)(77 R + 150 G + 29 B) / 65280 of uint8 pixels [..., 3]; the integer is exact"""
    c = np.asarray(rgb).astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]).astype(F32) / F32(65280.0)).astype(F32)


def linearize(depth, rgb, R, T, K, stride, vs, grid, d_min=0.3, d_max=5.0, r_max=0.4, g_max=4.0, huber=0.0, rc_max=1.0, gc_max=None, huber_c=0.0, order=None):
    """The 66 integers of one linearisation.  depth uint16 [h, w], rgb uint8 [h, w, 3]; grid = (val, known, lo, colour); the gates are the values after
    the defaults (gc_max None = 1 / vs, formed in f32); order: a permutation of the visited pixels (the sums do not depend on it)."""
    depth, rgb = np.asarray(depth), np.asarray(rgb)
    assert depth.dtype == np.uint16 and depth.ndim == 2 and rgb.dtype == np.uint8 and rgb.shape == depth.shape + (3,)
    val, known, lo, colour = grid
    h, w = depth.shape
    Rf = np.asarray(R, np.float64).reshape(3, 3).astype(F32)
    Tf = np.asarray(T, np.float64).reshape(3).astype(F32)
    Kf = np.asarray(K, np.float64).reshape(-1)
    fx, fy, cx, cy = (F32(Kf[i]) for i in (0, 4, 2, 5))
    vs = F32(vs)
    r_max, rc_max, huber_c = F32(r_max), F32(rc_max), F32(huber_c)
    gc_max = F32(1.0) / vs if gc_max is None else F32(gc_max)
    gcm2 = gc_max * gc_max
    out = np.zeros(N_SUMS, np.int64)
    out[GEO] = tr.linearize(depth, R, T, K, stride, vs, (val, known, lo), d_min=d_min, d_max=d_max, r_max=r_max, g_max=g_max, huber=huber, order=order)
    # the colour half: the same visited pixels, gate and back-projection
    thr_min, thr_max = F32(float(d_min) * 1000.0), F32(float(d_max) * 1000.0)
    jj, ii = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    i, j = ii.ravel(), jj.ravel()
    if order is not None:
        i, j = i[order], j[order]
    d = depth[j, i]
    df = d.astype(F32)
    gate = (d == 0) | (df > thr_max) | (df < thr_min)
    i, j, df = i[~gate], j[~gate], df[~gate]
    c = out[COL]
    c[tr.I_GATE] = gate.sum()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dep = df / F32(1000.0)
        px = (i.astype(F32) - cx) * dep / fx
        py = (j.astype(F32) - cy) * dep / fy
        pz = dep
        p = np.stack([((Rf[a, 0] * px + Rf[a, 1] * py) + Rf[a, 2] * pz) + Tf[a] for a in range(3)], 1).astype(F32)
        yi = image_luminance(rgb[j, i])
        s, kn, _ = rv.sample(p, vs, val, known, lo)
        Y, _, gY = rv.sample(p, vs, luminance_grid(colour), known, lo)          # the same corners and fractions
        c[tr.I_UNKNOWN] = (~kn).sum()
        p, s, Y, gY, yi = p[kn], s[kn], Y[kn], (gY[kn] / vs).astype(F32), yi[kn]
        rc = (Y - yi).astype(F32)
        far = ~(np.abs(s) <= r_max) | ~(np.abs(rc) <= rc_max)                    # off the surface, or a residual beyond the gate; a NaN is far
        c[tr.I_FAR] = far.sum()
        p, rc, gY = p[~far], rc[~far], gY[~far]
        gg = (gY[:, 0] * gY[:, 0] + gY[:, 1] * gY[:, 1]) + gY[:, 2] * gY[:, 2]
        bad = ~((gg > 0) & (gg <= gcm2))
        c[tr.I_GRAD] = bad.sum()
        p, rc, gY = p[~bad], rc[~bad], gY[~bad]
        c[tr.I_USED] = rc.size
        c0 = p[:, 1] * gY[:, 2] - p[:, 2] * gY[:, 1]
        c1 = p[:, 2] * gY[:, 0] - p[:, 0] * gY[:, 2]
        c2 = p[:, 0] * gY[:, 1] - p[:, 1] * gY[:, 0]
        J = [gY[:, 0], gY[:, 1], gY[:, 2], c0, c1, c2]
        wgt = tr.robust_weight(rc, huber_c)
        wJ = [wgt * x for x in J]
        q = [tr.fix(wJ[a] * J[b]) for a in range(6) for b in range(a, 6)] + [tr.fix(wJ[a] * rc) for a in range(6)] + [tr.fix((wgt * rc) * rc)]
        for k in range(28):
            c[k] = q[k].sum()
    return out


def auto_lambda(sums, balance=1.0):
    """balance * (Hg_00 + Hg_11 + Hg_22) / (Hc_00 + Hc_11 + Hc_22) of the integers as float64; 0 when the denominator is 0"""
    g, c = sums[GEO], sums[COL]
    num = (float(int(g[0])) + float(int(g[6]))) + float(int(g[11]))
    den = (float(int(c[0])) + float(int(c[6]))) + float(int(c[11]))
    return 0.0 if den == 0.0 else float(balance) * num / den


def solve(sums, lam, damping=0.0):
    """(xi, singular) of the combined step: Hd = Hg * 2^-20 + lam * (Hc * 2^-20), bd likewise, the diagonal damped, then track_ref's Cholesky"""
    Hg, bg = tr.system(sums[GEO])
    Hc, bc = tr.system(sums[COL])
    H = [[Hg[a][b] + lam * Hc[a][b] for b in range(6)] for a in range(6)]
    b = [bg[a] + lam * bc[a] for a in range(6)]
    for a in range(6):
        H[a][a] += damping * H[a][a]
    L = [[0.0] * 6 for _ in range(6)]
    zero = [0.0] * 6
    for j in range(6):
        d = H[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        if not (d > 0.0) or not math.isfinite(d):
            return zero, True
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            t = H[i][j]
            for k in range(j):
                t -= L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        t = -b[i]
        for k in range(i):
            t -= L[i][k] * y[k]
        y[i] = t / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t -= L[k][i] * x[k]
        x[i] = t / L[i][i]
    if not all(math.isfinite(v) for v in x):
        return zero, True
    return x, False


def track(depth, rgb, R, T, K, vs, grid, levels=DEFAULT_LEVELS, colour_weight=None, balance=1.0, min_step=1e-4, damping=0.0, min_used=6, **gates):
    """(R, T, info) of tsl_tsdf_track_rgbd; info = dict(status, iterations, lam, records), a record = dict(R, T, sums [66], xi, level).  colour_weight None:
    the automatic lambda of the first linearisation, held.  Lost when the GEOMETRIC n_used < min_used."""
    R = np.array(R, np.float64).reshape(3, 3)
    T = np.array(T, np.float64).reshape(3)
    Rl, Tl = R.copy(), T.copy()
    lam = None if colour_weight is None else float(colour_weight)
    records, status = [], 1

    def done(Ro, To, st):
        return Ro, To, dict(status=st, iterations=len(records), lam=0.0 if lam is None else lam, records=records)
    for lv, (stride, iters) in enumerate(levels):
        status = 1
        for _ in range(iters):
            sums = linearize(depth, rgb, R, T, K, stride, vs, grid, **gates)
            if lam is None:
                lam = auto_lambda(sums, balance)
            lost = int(sums[tr.I_USED]) < min_used
            xi, singular = ([0.0] * 6, False) if lost else solve(sums, lam, damping)
            records.append(dict(R=R.copy(), T=T.copy(), sums=sums, xi=np.array(xi, np.float64), level=lv))
            if lost or singular:
                return done(Rl, Tl, 2 if lost else 3)
            Rl, Tl = R.copy(), T.copy()
            R, T = tr.retract(xi, R, T)
            n2 = ((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + xi[3] * xi[3]) + xi[4] * xi[4]) + xi[5] * xi[5]
            if math.sqrt(n2) < min_step:
                status = 0
                break
    return done(R, T, status)

"""numpy restatement of the frame-to-model alignment (taichislam_amd/csrc/tsl_align.hip).  linearize: float32 in the written
order, the 33 integers of tsl_align_sums, which the GPU must equal.  solve / retract / track: float64 scalar code in the written order, which the
library's host functions must equal bit for bit.  points, robust_weight and iterate are what the registration (tests/register_ref.py) and the pose
search (tests/register_search_ref.py) share with it, as the kernels share tsl_align_common.hpp.  The map is a dense grid as in render_view_ref: val / known [N][N][Nz] indexed by voxel index - lo."""
import math

import numpy as np

import render_view_ref as rv

F32 = np.float32
SCALE = 2.0 ** 20
N_SUMS = 33                                              # H[21], b[6], e, n_used, n_gate, n_unknown, n_far, n_grad
I_E, I_USED, I_GATE, I_UNKNOWN, I_FAR, I_GRAD = 27, 28, 29, 30, 31, 32
DEFAULT_LEVELS = ((8, 4), (4, 4), (2, 6))


def visited(h, w, stride):
    return -(-h // stride) * -(-w // stride)


def fix(x):
    """Q(x) = (int64) rint((double)x * 2^20), round half to even.  x must be finite: the buckets keep a value that is not finite from every product
    (the conversion of a NaN to an integer is undefined)."""
    assert np.isfinite(x).all(), "a product that is not finite reached fix()"
    return np.rint(np.asarray(x, F32).astype(np.float64) * SCALE).astype(np.int64)


def robust_weight(r, huber):
    """wgt = huber > 0 && |r| > huber ? huber / |r| : 1 in f32"""
    a_r = np.abs(r)
    one = np.ones_like(r)
    return np.where((huber > 0) & (a_r > huber), huber / np.where(a_r > 0, a_r, one), one).astype(F32)


def points(p, t, vs, grid, r_max, g_max, huber, n_gate=0, addends=None):
    """What the alignment and the registration share: the 33 integers of the map-frame points p f32 [n, 3] against the target values t f32 [n] (zeros
    for the alignment): each point is unknown, far, grad or used, a used one adds its 28 products with the residual r = s - t.  n_gate: the
    caller's gate count, which it formed on the way to p.  addends: a list that receives the 28 int64 arrays [n_used] the sums are formed from."""
    val, known, lo = grid
    vs, r_max, g_max, huber = F32(vs), F32(r_max), F32(g_max), F32(huber)
    gm2 = g_max * g_max
    out = np.zeros(N_SUMS, np.int64)
    out[I_GATE] = n_gate
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s, kn, g = rv.sample(p, vs, val, known, lo)
        out[I_UNKNOWN] = (~kn).sum()
        p, s, t, g = p[kn], s[kn], t[kn], (g[kn] / vs).astype(F32)
        far = ~(np.abs(s) <= r_max)                       # a NaN interpolant is far
        out[I_FAR] = far.sum()
        p, s, t, g = p[~far], s[~far], t[~far], g[~far]
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        bad = ~((gg > 0) & (gg <= gm2))                   # a NaN gradient is grad
        out[I_GRAD] = bad.sum()
        p, s, t, g = p[~bad], s[~bad], t[~bad], g[~bad]
        out[I_USED] = s.size
        r = (s - t).astype(F32)
        c0 = p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1]
        c1 = p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2]
        c2 = p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]
        J = [g[:, 0], g[:, 1], g[:, 2], c0, c1, c2]
        wgt = robust_weight(r, huber)
        wJ = [wgt * x for x in J]
        q = [fix(wJ[a] * J[b]) for a in range(6) for b in range(a, 6)] + [fix(wJ[a] * r) for a in range(6)] + [fix((wgt * r) * r)]
        for k in range(28):
            out[k] = q[k].sum()
        if addends is not None:
            addends.extend(q)
    return out


def linearize(depth, R, T, K, stride, vs, grid, d_min=0.3, d_max=5.0, r_max=0.4, g_max=4.0, huber=0.0, order=None, addends=None):
    """The 33 integers of one linearisation.  depth uint16 [h, w]; R, T float64 (rounded to f32 once); K 9 values; grid = (val, known, lo);
    d_min / d_max / r_max / g_max / huber are the values after the defaults (r_max and g_max are rounded to f32 as the configuration holds them);
    order: a permutation of the visited pixels (the sums do not depend on it); addends: as in points."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 2
    h, w = depth.shape
    R = np.asarray(R, np.float64).reshape(3, 3).astype(F32)
    T = np.asarray(T, np.float64).reshape(3).astype(F32)
    K = np.asarray(K, np.float64).reshape(-1)
    fx, fy, cx, cy = (F32(K[i]) for i in (0, 4, 2, 5))
    vs = F32(vs)
    thr_min, thr_max = F32(float(d_min) * 1000.0), F32(float(d_max) * 1000.0)
    jj, ii = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    i, j = ii.ravel(), jj.ravel()
    if order is not None:
        i, j = i[order], j[order]
    d = depth[j, i]
    df = d.astype(F32)
    gate = (d == 0) | (df > thr_max) | (df < thr_min)
    i, j, df = i[~gate], j[~gate], df[~gate]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dep = df / F32(1000.0)
        px = (i.astype(F32) - cx) * dep / fx
        py = (j.astype(F32) - cy) * dep / fy
        pz = dep
        p = np.stack([((R[a, 0] * px + R[a, 1] * py) + R[a, 2] * pz) + T[a] for a in range(3)], 1).astype(F32)
    return points(p, np.zeros(p.shape[0], F32), vs, grid, r_max, g_max, huber, n_gate=gate.sum(), addends=addends)


def system(sums, damping=0.0):
    """(Hd 6 x 6 lists, bd) float64 of the 33 integers: H * 2^-20 mirrored, the diagonal damped"""
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for c in range(a, 6):
            x = float(int(sums[k])) * (1.0 / SCALE)
            H[a][c] = x
            H[c][a] = x
            k += 1
    b = [float(int(sums[21 + a])) * (1.0 / SCALE) for a in range(6)]
    for a in range(6):
        H[a][a] += damping * H[a][a]
    return H, b


def solve(sums, damping=0.0):
    """(xi = -Hd^-1 bd as 6 floats, singular) by Cholesky L L^T without pivoting, column by column"""
    H, b = system(sums, damping)
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


def retract(xi, R, T):
    """the Cayley map of omega = xi[3:]: (C R, C T + v) as float64 arrays"""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
    T = [float(v) for v in np.asarray(T, np.float64).reshape(-1)]
    xi = [float(v) for v in xi]
    a = [xi[3] * 0.5, xi[4] * 0.5, xi[5] * 0.5]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den = 1.0 + aa
    S = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    C = [[((((1.0 - aa) if i == j else 0.0) + (2.0 * a[i]) * a[j]) + 2.0 * S[i][j]) / den for j in range(3)] for i in range(3)]
    Rn = [(C[i][0] * R[j] + C[i][1] * R[3 + j]) + C[i][2] * R[6 + j] for i in range(3) for j in range(3)]
    Tn = [((C[i][0] * T[0] + C[i][1] * T[1]) + C[i][2] * T[2]) + xi[i] for i in range(3)]
    return np.array(Rn, np.float64).reshape(3, 3), np.array(Tn, np.float64)


def iterate(lin, R, T, levels, min_step, damping, min_used):
    """The iteration over the levels, shared by the alignment and the registration: lin(R, T, stride) gives the 33 integers at a float64 pose.
    Returns (R, T, info); info = dict(status, iterations, records), a record = dict(R, T, sums, xi, level)"""
    R = np.array(R, np.float64).reshape(3, 3)
    T = np.array(T, np.float64).reshape(3)
    Rl, Tl = R.copy(), T.copy()
    records, status = [], 1
    for lv, (stride, iters) in enumerate(levels):
        status = 1
        for _ in range(iters):
            sums = lin(R, T, stride)
            lost = int(sums[I_USED]) < min_used
            xi, singular = ([0.0] * 6, False) if lost else solve(sums, damping)
            records.append(dict(R=R.copy(), T=T.copy(), sums=sums, xi=np.array(xi, np.float64), level=lv))
            if lost or singular:
                return Rl, Tl, dict(status=2 if lost else 3, iterations=len(records), records=records)
            Rl, Tl = R.copy(), T.copy()
            R, T = retract(xi, R, T)
            n2 = ((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + xi[3] * xi[3]) + xi[4] * xi[4]) + xi[5] * xi[5]
            if math.sqrt(n2) < min_step:
                status = 0
                break
    return R, T, dict(status=status, iterations=len(records), records=records)


def track(depth, R, T, K, vs, grid, levels=DEFAULT_LEVELS, min_step=1e-4, damping=0.0, min_used=6, **gates):
    """(R, T, info) of tsl_tsdf_track_depth; info as iterate returns it"""
    return iterate(lambda R, T, stride: linearize(depth, R, T, K, stride, vs, grid, **gates), R, T, levels, min_step, damping, min_used)

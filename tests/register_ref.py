"""numpy restatement of the map-to-map registration (taichislam_amd/csrc/tsl_register.hip).  linearize: float32 in the written
order, the 33 integers of tsl_align_sums, which the GPU must equal.  The step, the retraction and the shape of the iteration are those of
tests/track_ref.py.  The source is a sparse export (int16 indices [n, 3], f16 TSDF [n], f16 W_TSDF [n]: the observed voxels of the submap), the
destination a dense grid as in render_view_ref: val / known [N][N][Nz] indexed by voxel index - lo."""
import math

import numpy as np

import render_view_ref as rv
import track_ref as tr

F32 = np.float32
DEFAULT_LEVELS = ((4, 4), (2, 4), (1, 6))
STRIDES = (1, 2, 4, 8, 16)


def source(export):
    """(indices int64 [n, 3], t f32 [n], w f32 [n]) of a sparse export"""
    return (np.asarray(export["indices"]).astype(np.int64), np.asarray(export["TSDF"]).view(np.float16).astype(F32),
            np.asarray(export["W_TSDF"]).view(np.float16).astype(F32))


def defaults(vs, internal_voxels, voxel_scale, w_min=0.0, band=0.0, r_max=0.0, g_max=0.0, huber=0.0):
    """the gates after the defaults, as the library forms them: band 0 = 2.0f * vs, r_max 0 = (float)(internal_voxels * voxel), g_max 0 = 4"""
    return dict(w_min=F32(w_min), band=F32(band) if band else F32(2.0) * F32(vs), r_max=F32(r_max) if r_max else F32(float(internal_voxels) * float(voxel_scale)),
                g_max=F32(g_max) if g_max else F32(4.0), huber=F32(huber))


def linearize(src, R, T, stride, vs, grid, w_min, band, r_max, g_max, huber=0.0, order=None):
    """The 33 integers of one linearisation.  src = source(export); R, T float64 (rounded to f32 once); grid = (val, known, lo) of the destination;
    w_min / band / r_max / g_max / huber are the values after the defaults; order: a permutation of the source's voxels (the sums do not depend on it)."""
    assert stride in STRIDES
    idx, t, w = src
    if order is not None:
        idx, t, w = idx[order], t[order], w[order]
    val, known, lo = grid
    R = np.asarray(R, np.float64).reshape(3, 3).astype(F32)
    T = np.asarray(T, np.float64).reshape(3).astype(F32)
    vs, w_min, band, r_max, g_max, huber = F32(vs), F32(w_min), F32(band), F32(r_max), F32(g_max), F32(huber)
    gm2 = g_max * g_max
    out = np.zeros(tr.N_SUMS, np.int64)
    lattice = ((idx % stride) == 0).all(1)
    idx, t, w = idx[lattice], t[lattice], w[lattice]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gate = ~(w >= w_min) | (np.abs(t) > band)
        out[tr.I_GATE] = gate.sum()
        idx, t = idx[~gate], t[~gate]
        q = idx.astype(F32) * vs
        p = np.stack([((R[a, 0] * q[:, 0] + R[a, 1] * q[:, 1]) + R[a, 2] * q[:, 2]) + T[a] for a in range(3)], 1).astype(F32)
        s, kn, g = rv.sample(p, vs, val, known, lo)
        out[tr.I_UNKNOWN] = (~kn).sum()
        p, s, t, g = p[kn], s[kn], t[kn], (g[kn] / vs).astype(F32)
        far = np.abs(s) > r_max
        out[tr.I_FAR] = far.sum()
        p, s, t, g = p[~far], s[~far], t[~far], g[~far]
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        bad = (gg == 0) | (gg > gm2)
        out[tr.I_GRAD] = bad.sum()
        p, s, t, g = p[~bad], s[~bad], t[~bad], g[~bad]
        out[tr.I_USED] = s.size
        r = (s - t).astype(F32)
        c0 = p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1]
        c1 = p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2]
        c2 = p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]
        J = [g[:, 0], g[:, 1], g[:, 2], c0, c1, c2]
        a_r = np.abs(r)
        one = np.ones_like(r)
        wgt = np.where((huber > 0) & (a_r > huber), huber / np.where(a_r > 0, a_r, one), one).astype(F32)
        wJ = [wgt * x for x in J]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                out[k] = tr.fix(wJ[a] * J[b]).sum()
                k += 1
        for a in range(6):
            out[21 + a] = tr.fix(wJ[a] * r).sum()
        out[tr.I_E] = tr.fix((wgt * r) * r).sum()
    return out


def visited(src, stride):
    """the observed voxels of the source on the lattice of `stride`"""
    return int(((src[0] % stride) == 0).all(1).sum())


def register(src, R, T, vs, grid, levels=DEFAULT_LEVELS, min_step=1e-4, damping=0.0, min_used=6, **gates):
    """(R, T, info) of tsl_tsdf_register_submap; info = dict(status, iterations, records), a record = dict(R, T, sums, xi, level)"""
    R = np.array(R, np.float64).reshape(3, 3)
    T = np.array(T, np.float64).reshape(3)
    Rl, Tl = R.copy(), T.copy()
    records, status = [], 1
    for lv, (stride, iters) in enumerate(levels):
        status = 1
        for _ in range(iters):
            sums = linearize(src, R, T, stride, vs, grid, **gates)
            lost = int(sums[tr.I_USED]) < min_used
            xi, singular = ([0.0] * 6, False) if lost else tr.solve(sums, damping)
            records.append(dict(R=R.copy(), T=T.copy(), sums=sums, xi=np.array(xi, np.float64), level=lv))
            if lost or singular:
                return Rl, Tl, dict(status=2 if lost else 3, iterations=len(records), records=records)
            Rl, Tl = R.copy(), T.copy()
            R, T = tr.retract(xi, R, T)
            n2 = ((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + xi[3] * xi[3]) + xi[4] * xi[4]) + xi[5] * xi[5]
            if math.sqrt(n2) < min_step:
                status = 0
                break
    return R, T, dict(status=status, iterations=len(records), records=records)

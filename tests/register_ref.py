"""numpy restatement of the map-to-map registration (taichislam_amd/csrc/tsl_register.hip).  linearize: float32 in the written
order, the 33 integers of tsl_align_sums, which the GPU must equal: the lattice, the gate and the transform here, the buckets and the sums by
track_ref.points.  The step, the retraction and the iteration are those of tests/track_ref.py.  The source is a sparse export (int16 indices [n, 3], f16 TSDF [n], f16 W_TSDF [n]: the observed voxels of the submap), the
destination a dense grid as in render_view_ref: val / known [N][N][Nz] indexed by voxel index - lo."""
import numpy as np

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


def linearize(src, R, T, stride, vs, grid, w_min, band, r_max, g_max, huber=0.0, order=None, addends=None):
    """The 33 integers of one linearisation.  src = source(export); R, T float64 (rounded to f32 once); grid = (val, known, lo) of the destination;
    w_min / band / r_max / g_max / huber are the values after the defaults; order: a permutation of the source's voxels (the sums do not depend on it);
    addends: as in track_ref.points."""
    assert stride in STRIDES
    idx, t, w = src
    if order is not None:
        idx, t, w = idx[order], t[order], w[order]
    R = np.asarray(R, np.float64).reshape(3, 3).astype(F32)
    T = np.asarray(T, np.float64).reshape(3).astype(F32)
    vs, w_min, band = F32(vs), F32(w_min), F32(band)
    lattice = ((idx % stride) == 0).all(1)
    idx, t, w = idx[lattice], t[lattice], w[lattice]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gate = ~((w >= w_min) & (np.abs(t) <= band))      # a NaN weight or value is gated
        idx, t = idx[~gate], t[~gate]
        q = idx.astype(F32) * vs
        p = np.stack([((R[a, 0] * q[:, 0] + R[a, 1] * q[:, 1]) + R[a, 2] * q[:, 2]) + T[a] for a in range(3)], 1).astype(F32)
    return tr.points(p, t, vs, grid, r_max, g_max, huber, n_gate=gate.sum(), addends=addends)


def visited(src, stride):
    """the observed voxels of the source on the lattice of `stride`"""
    return int(((src[0] % stride) == 0).all(1).sum())


def register(src, R, T, vs, grid, levels=DEFAULT_LEVELS, min_step=1e-4, damping=0.0, min_used=6, **gates):
    """(R, T, info) of tsl_tsdf_register_submap; info as track_ref.iterate returns it"""
    return tr.iterate(lambda R, T, stride: linearize(src, R, T, stride, vs, grid, **gates), R, T, levels, min_step, damping, min_used)

"""numpy restatement of the scan-to-model alignment (taichislam_amd/csrc/tsl_align_points.hip): the range gate and the
transform of a point cloud in float32 in the written order, then what the image form shares with it (track_ref.points, track_ref.iterate).
linearize_points also gives the per-point bucket and signed distance, which the GPU must equal bit for bit."""
import numpy as np

import render_view_ref as rv
import track_ref as tr

F32 = np.float32
USED, GATE, UNKNOWN, FAR, GRAD = 0, 1, 2, 3, 4            # the AL_* codes of tsl_align_common.hpp
DEFAULT_LEVELS = ((8, 4), (4, 4), (1, 6))


def visited(n, stride):
    return -(-n // stride)


def gate_and_transform(xyz, R, T, d_min, d_max):
    """(gate bool [m], p f32 [m, 3]) of the points xyz f32 [m, 3]: gate if a coordinate is not finite or l2 = (x x + y y) + z z is > d_max^2 or
    < d_min^2 (the squares formed in f32); p[a] = ((R[a][0] x + R[a][1] y) + R[a][2] z) + T[a] (meaningless where gated)"""
    R = np.asarray(R, np.float64).reshape(3, 3).astype(F32)
    T = np.asarray(T, np.float64).reshape(3).astype(F32)
    dmin2, dmax2 = F32(d_min) * F32(d_min), F32(d_max) * F32(d_max)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = (x * x + y * y) + z * z
        gate = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z)) | (l2 > dmax2) | (l2 < dmin2)
        p = np.stack([((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + T[a] for a in range(3)], 1).astype(F32)
    return gate, p


def classify(p, vs, grid, r_max, g_max):
    """(bucket uint8 [m], s f32 [m]) of the map-frame points p: the buckets of al_sample in its order; s is the interpolant for used, far and grad
    and +0 for unknown"""
    val, known, lo = grid
    vs, r_max, g_max = F32(vs), F32(r_max), F32(g_max)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s, kn, g = rv.sample(p, vs, val, known, lo)
        g = (g / vs).astype(F32)
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        far = ~(np.abs(s) <= r_max)
        bad = ~((gg > 0) & (gg <= g_max * g_max))
    bucket = np.where(~kn, UNKNOWN, np.where(far, FAR, np.where(bad, GRAD, USED))).astype(np.uint8)
    return bucket, np.where(kn, s, F32(0.0)).astype(F32)


def linearize_points(xyz, R, T, stride, vs, grid, d_min=0.3, d_max=5.0, r_max=0.4, g_max=4.0, huber=0.0, order=None, addends=None):
    """(the 33 integers, bucket uint8 [visited], s f32 [visited]) of one linearisation.  xyz f32 [n, 3] in the sensor frame; R, T float64 (rounded
    to f32 once); grid = (val, known, lo); the gates are the values after the defaults; order: a permutation of the visited points (the sums do not
    depend on it; bucket and s follow it); addends: as in track_ref.points."""
    xyz = np.ascontiguousarray(np.asarray(xyz, F32).reshape(-1, 3))[::stride]
    if order is not None:
        xyz = xyz[order]
    gate, p = gate_and_transform(xyz, R, T, d_min, d_max)
    bucket = np.full(xyz.shape[0], GATE, np.uint8)
    s = np.zeros(xyz.shape[0], F32)
    q = p[~gate]
    bucket[~gate], s[~gate] = classify(q, vs, grid, r_max, g_max)
    sums = tr.points(q, np.zeros(q.shape[0], F32), vs, grid, r_max, g_max, huber, n_gate=int(gate.sum()), addends=addends)
    assert [int((bucket == c).sum()) for c in (USED, GATE, UNKNOWN, FAR, GRAD)] == sums[tr.I_USED:].tolist()
    return sums, bucket, s


def track_points(xyz, R, T, vs, grid, levels=DEFAULT_LEVELS, min_step=1e-4, damping=0.0, min_used=6, **gates):
    """(R, T, info) of tsl_tsdf_track_points; info as track_ref.iterate returns it"""
    return tr.iterate(lambda R, T, stride: linearize_points(xyz, R, T, stride, vs, grid, **gates)[0], R, T, levels, min_step, damping, min_used)

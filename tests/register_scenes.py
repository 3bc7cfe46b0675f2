"""The registration scene shared by tests/test_register_cpu.py and tests/test_register_gpu.py: the box room of tests/track_scenes.py at SMALL (256^3,
0.04 m voxels, 320 x 240 frames).  The destination map holds frames 0..5.  The source submap holds frames 3..8 -- an overlapping but different set of
views -- integrated with poses pre-multiplied by D^-1, D a fixed displacement: the source grid is rotated and shifted against the destination's, and the
pose that takes source coordinates to destination coordinates is D."""
import functools

import numpy as np

import register_ref as rr
import render_view_scenes as rsc
import track_scenes as ts
from util import SMALL

F32 = np.float32
VS = ts.VS
SRC_FIRST, N_FRAMES = 3, 6
D_AXIS, D_DEG = (1.0, -2.0, 0.5), 3.0                          # a skew axis
D_T = np.array([0.05, -0.03, 0.017])                           # no component is a multiple of the voxel size
PERTURBATIONS = ts.PERTURBATIONS                               # 3 cm / 1.5 deg, 6 cm / 3 deg, 10 cm / 5 deg
HALF_VOXEL = 0.5 * SMALL["voxel_scale"]
# the gates after the defaults of SMALL: w_min 0, band 2 voxels, r_max = internal_voxels * voxel, g_max 4
GATES = rr.defaults(VS, SMALL["internal_voxels"], SMALL["voxel_scale"])
# Twice the largest final error tests/test_register_cpu.py::test_convergence measures with the restatement over the oracle's BATCHED maps (the margin of
# track_scenes.TRACK_BOUND_M).  Measured from 3 cm / 1.5 deg, 6 cm / 3 deg, 10 cm / 5 deg: all three converge (the basin reaches past 10 cm / 5 deg here).
MEASURED_M = (0.000807, 0.000807, 0.000807)
MEASURED_DEG = (0.013677, 0.013678, 0.013678)
MEASURED_ITERATIONS = (8, 8, 8)
MEASURED_STATUS = (0, 0, 0)
REGISTER_BOUND_M = 2 * max(MEASURED_M)
REGISTER_BOUND_DEG = 2 * max(MEASURED_DEG)


def displacement():
    """D = (R, T): source-submap coordinates to destination coordinates"""
    return ts.rotation(D_AXIS, D_DEG), D_T.copy()


def dst_frames():
    return ts.map_frames()


def src_frames():
    """[(R, T, depth)]: frames 3..8 seen from their true poses, with the poses the source submap integrates them at: D^-1 P"""
    Rd, Td = displacement()
    out = []
    for f in range(SRC_FIRST, SRC_FIRST + N_FRAMES):
        R, T = ts.pose(f)
        out.append((Rd.T @ R, Rd.T @ (T - Td), ts.box_depth(R, T)))
    return out


def perturbed_poses():
    """[(R, T)]: D moved by the three perturbations; per case a translation direction, then a rotation axis, from default_rng(13)"""
    Rd, Td = displacement()
    rng = np.random.default_rng(13)
    out = []
    for m, deg in PERTURBATIONS:
        tdir, axis = rng.standard_normal(3), rng.standard_normal(3)
        out.append((ts.rotation(axis, deg) @ Rd, Td + m * tdir / np.linalg.norm(tdir)))
    return out


def outside_pose():
    """D carried 20 m along x: every source voxel lands outside the destination's volume"""
    Rd, Td = displacement()
    return Rd, Td + np.array([20.0, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def dst_oracle():
    """the oracle's BATCHED map of frames 0..5 (the map of track_scenes)"""
    return ts.oracle_map()


@functools.lru_cache(maxsize=None)
def src_oracle():
    return rsc.room_oracle(ts.intrinsics(), src_frames(), SMALL)


@functools.lru_cache(maxsize=None)
def dst_grid():
    """(val, known, lo) of the destination for the restatement; shared and never written"""
    return ts.oracle_grid()


@functools.lru_cache(maxsize=None)
def src_export():
    return src_oracle().export_sparse()


@functools.lru_cache(maxsize=None)
def src_voxels():
    """register_ref.source of the source's export; shared and never written"""
    return rr.source(src_export())


@functools.lru_cache(maxsize=None)
def reference_runs():
    """[(R, T, info)] of register_ref.register from the three perturbed poses with the default levels; computed once"""
    return [rr.register(src_voxels(), R, T, VS, dst_grid(), **GATES) for R, T in perturbed_poses()]

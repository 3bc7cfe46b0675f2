"""The scenes of tests/test_track_points_cpu.py and tests/test_track_points_gpu.py: the box room and the six-frame map of tests/track_scenes.py, seen
by a spinning lidar at the true pose of the tracked frame, and the tracked depth image turned into the cloud the image kernel forms from it."""
import functools

import numpy as np

import track_points_ref as tpr
import track_scenes as ts

F32 = np.float32
RINGS, AZIMUTHS = 16, 360
# The rings span -25 .. +25 degrees about the sensor's horizontal plane: floor, ceiling and two walls of the observed corner are hit.  (At +-30 or
# +-35 degrees the undamped iteration ends in a cycle between two poses 1.5e-3 apart, as two dozen points on the rim of the observed space change
# between used and unknown; the final error is about a millimetre there too, but the last level never ends by min_step.)
ELEVATION_DEG = 25.0
VS = ts.VS
# the gates after the defaults of SMALL, as track_scenes.GATES: d_min / d_max are the range gate here
GATES = dict(ts.GATES)
# no point of the room is gated by these (test 2 of the issue: the depth-derived cloud against the image kernel)
WIDE = dict(d_min=1e-3, d_max=1e3)
# Twice the largest final error tests/test_track_points_cpu.py::test_convergence measures with the restatement over the oracle's BATCHED map on the
# spherical scan (the margin of track_scenes.TRACK_BOUND_*).  Measured from 3 cm / 1.5 deg, 6 cm / 3 deg, 10 cm / 5 deg: 0.001056 / 0.001070 /
# 0.001055 m and 0.05377 / 0.05342 / 0.05377 deg, after 11 / 8 / 10 linearisations, each with status 0.
TRACK_POINTS_BOUND_M = 2 * 0.001070
TRACK_POINTS_BOUND_DEG = 2 * 0.05377


def scan_directions():
    """float64 [RINGS * AZIMUTHS, 3]: unit directions in the sensor frame (optical convention: z forward, y down), ring by ring"""
    el = np.deg2rad(np.linspace(-ELEVATION_DEG, ELEVATION_DEG, RINGS))
    az = np.deg2rad(np.arange(AZIMUTHS, dtype=np.float64) * (360.0 / AZIMUTHS))
    e, a = np.meshgrid(el, az, indexing="ij")
    return np.stack([np.cos(e) * np.sin(a), -np.sin(e), np.cos(e) * np.cos(a)], -1).reshape(-1, 3)


def box_scan(R, T, dirs=None):
    """f32 [n, 3]: the points of the box's inside a sensor at the sensor-to-map pose (R, T) sees along `dirs`, in the sensor frame; ray / face
    intersection in float64 (the faces of track_scenes.box_depth), stored as f32"""
    ds = scan_directions() if dirs is None else np.asarray(dirs, np.float64)
    d = ds @ np.asarray(R, np.float64).reshape(3, 3).T
    T = np.asarray(T, np.float64).reshape(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (ts.BOX_HI - T) / d, np.where(d < 0, (ts.BOX_LO - T) / d, np.inf)).min(-1)
    return (ds * t[:, None]).astype(F32)


@functools.lru_cache(maxsize=None)
def scan():
    """the spherical scan from the true pose of track_scenes.tracked_frame(): 16 rings x 360 azimuths = 5760 points; shared and never written.  Most of
    the sphere looks at walls the six frames never saw, which fills n_unknown."""
    R, T, _ = ts.tracked_frame()
    out = box_scan(R, T)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wall_scan():
    """the points of the scan that lie on the wall the camera faces (the face y = BOX_HI[1] or x = BOX_HI[0], whichever holds more of them): a plane
    leaves three degrees of freedom open"""
    R, T, _ = ts.tracked_frame()
    q = scan().astype(np.float64) @ np.asarray(R, np.float64).T + T
    fwd = (scan()[:, 2] > 0)
    on = [fwd & (np.abs(q[:, a] - ts.BOX_HI[a]) < 1e-4) for a in (0, 1)]
    return np.ascontiguousarray(scan()[max(on, key=lambda m: m.sum())])


@functools.lru_cache(maxsize=None)
def singular_cloud():
    """Three points of wall_scan() that are used at the true pose.  The whole wall does not make a singular system: the reference's TSDF is
    projective, its gradient on a plane leans with the viewing rays, and the 656 used points of the wall give a positive definite H (eigenvalues
    4.5 .. 2624).  Three rows of J give a rank of at most three -- what an ideal plane leaves -- whatever the gradients are."""
    R, T, _ = ts.tracked_frame()
    _, bucket, _ = tpr.linearize_points(wall_scan(), R, T, 1, VS, ts.oracle_grid(), **GATES)
    used = wall_scan()[bucket == tpr.USED]
    return np.ascontiguousarray(used[:: used.shape[0] // 3][:3])


@functools.lru_cache(maxsize=None)
def depth_cloud():
    """f32 [m, 3]: the tracked depth image back-projected with the f32 expressions of k_align_linearize, for the pixels that pass the image gate, in
    row-major pixel order"""
    _, _, depth = ts.tracked_frame()
    K = np.asarray(ts.intrinsics(), np.float64).reshape(-1)
    fx, fy, cx, cy = (F32(K[i]) for i in (0, 4, 2, 5))
    thr_min, thr_max = F32(float(GATES["d_min"]) * 1000.0), F32(float(GATES["d_max"]) * 1000.0)
    jj, ii = np.meshgrid(np.arange(ts.H), np.arange(ts.W), indexing="ij")
    i, j, d = ii.ravel(), jj.ravel(), depth.ravel()
    df = d.astype(F32)
    ok = ~((d == 0) | (df > thr_max) | (df < thr_min))
    i, j, df = i[ok], j[ok], df[ok]
    dep = df / F32(1000.0)
    px = (i.astype(F32) - cx) * dep / fx
    py = (j.astype(F32) - cy) * dep / fy
    out = np.stack([px, py, dep], 1).astype(F32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_tracks():
    """[(R, T, info)] of track_points_ref.track_points from the three perturbed poses over the oracle's map on the spherical scan, with the default
    levels; computed once"""
    return [tpr.track_points(scan(), R, T, VS, ts.oracle_grid(), **GATES) for R, T in ts.perturbed_poses()]

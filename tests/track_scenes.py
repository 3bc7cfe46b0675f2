"""The tracking scene shared by tests/test_track_cpu.py and tests/test_track_gpu.py: a box room seen from inside (a sphere constrains rotation
weakly; a corner with floor and ceiling in view constrains all six degrees of freedom), its analytic depth, the frames that build the map, the
tracked frame and three fixed perturbations of its pose."""
import functools

import numpy as np

import render_view_ref as rv
import render_view_scenes as rsc
import track_ref as tr
from taichislam_amd.utils import synthetic as syn
from util import SMALL

F32 = np.float32
BOX_LO = np.array([-2.2, -2.0, -0.8])
BOX_HI = np.array([2.6, 2.4, 0.9])
H, W = 240, 320
START_DEG, DEG_PER_FRAME, N_FRAMES, TRACKED = 40.0, 3.0, 6, 2.5
PERTURBATIONS = ((0.03, 1.5), (0.06, 3.0), (0.10, 5.0))           # metres, degrees
VS = F32(SMALL["voxel_scale"])
# the gates after the defaults of SMALL: d_min / d_max = min / max_ray_length, r_max = internal_voxels * voxel, g_max = 4
GATES = dict(d_min=SMALL["min_ray_length"], d_max=SMALL["max_ray_length"], r_max=float(F32(SMALL["internal_voxels"] * SMALL["voxel_scale"])), g_max=4.0)
# Twice the largest final error tests/test_track_cpu.py::test_convergence measures with the restatement over the oracle's BATCHED map (the margin of
# render_view_scenes.ROUND_TRIP_BOUND).  Measured from 3 cm / 1.5 deg, 6 cm / 3 deg, 10 cm / 5 deg: 0.000513 / 0.000512 / 0.000512 m and
# 0.01826 / 0.01829 / 0.01826 deg.
TRACK_BOUND_M = 2 * 0.000513
TRACK_BOUND_DEG = 2 * 0.01829


def box_depth(R, T, h=H, w=W, K=None):
    """uint16 [h, w] millimetres: the optical-axis depth of the box's inside from the camera-to-map pose (R, T), by ray / face intersection in float64"""
    K = syn.scaled_intrinsics(h, w) if K is None else np.asarray(K, np.float64).reshape(-1)
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dc = np.stack([(ii - K[2]) / K[0], (jj - K[5]) / K[4], np.ones_like(ii)], -1)
    d = dc @ np.asarray(R, np.float64).reshape(3, 3).T
    T = np.asarray(T, np.float64).reshape(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (BOX_HI - T) / d, np.where(d < 0, (BOX_LO - T) / d, np.inf)).min(-1)
    return np.clip(np.rint(1000.0 * t), 0, 65535).astype(np.uint16)


def pose(f):
    return syn.camera_pose(f, start_deg=START_DEG, deg_per_frame=DEG_PER_FRAME)


def intrinsics():
    return syn.scaled_intrinsics(H, W)


def map_frames():
    """[(R, T, depth)] of the six 320 x 240 frames that build the map"""
    return [pose(f) + (box_depth(*pose(f)),) for f in range(N_FRAMES)]


def tracked_frame():
    """(R, T, depth): the true pose of the tracked frame -- a pose nobody integrated -- and its analytic image"""
    R, T = pose(TRACKED)
    return R, T, box_depth(R, T)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(th) * S + (1.0 - np.cos(th)) * (S @ S)


def perturbed_poses():
    """[(R, T)]: the true pose moved by 3 cm / 1.5 deg, 6 cm / 3 deg, 10 cm / 5 deg; per case a translation direction, then a rotation axis, from default_rng(7)"""
    R, T, _ = tracked_frame()
    rng = np.random.default_rng(7)
    out = []
    for m, deg in PERTURBATIONS:
        tdir, axis = rng.standard_normal(3), rng.standard_normal(3)
        out.append((rotation(axis, deg) @ R, T + m * tdir / np.linalg.norm(tdir)))
    return out


def away_pose():
    """the true pose turned by 180 degrees about the vertical: every back-projected point lies in space nobody observed"""
    R, T, _ = tracked_frame()
    return rotation([0.0, 0.0, 1.0], 180.0) @ R, T


def pose_error(R, T, Rt, Tt):
    """(metres, degrees) between two poses"""
    D = np.asarray(R, np.float64).reshape(3, 3) @ np.asarray(Rt, np.float64).reshape(3, 3).T
    return float(np.linalg.norm(np.asarray(T, np.float64).reshape(3) - Tt)), float(np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0))))


def shaped(depth, shape):
    """the image cropped or zero-padded (no depth) to `shape`, keeping pixel (0, 0) in place: the intrinsics stay those of the 320 x 240 image"""
    out = np.zeros(shape, np.uint16)
    h, w = min(shape[0], depth.shape[0]), min(shape[1], depth.shape[1])
    out[:h, :w] = depth[:h, :w]
    return out


@functools.lru_cache(maxsize=None)
def oracle_map():
    """the oracle's BATCHED map of the six frames"""
    return rsc.room_oracle(intrinsics(), map_frames(), SMALL)


@functools.lru_cache(maxsize=None)
def oracle_grid():
    """its dense grid (val, known, lo) for the restatement; shared and never written"""
    return rsc.oracle_grid(oracle_map())


@functools.lru_cache(maxsize=None)
def reference_tracks():
    """[(R, T, info)] of track_ref.track from the three perturbed poses over the oracle's map, with the default levels; computed once"""
    _, _, depth = tracked_frame()
    return [tr.track(depth, R, T, intrinsics(), VS, oracle_grid(), **GATES) for R, T in perturbed_poses()]

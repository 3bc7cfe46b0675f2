"""The scenes shared by tests/test_track_rgbd_cpu.py and tests/test_track_rgbd_gpu.py.

The wall: one textured plane seen head-on, hand-built through load_numpy.  Signed distance fixes one translation and two rotations of the camera and
says nothing about the other three degrees of freedom (sliding along the wall, turning about its normal); the texture fixes those.
The room: the box room of tests/track_scenes.py with an analytic texture on every wall, its six frames integrated with texture_enabled, the tracked
frame and the perturbations of track_scenes."""
import functools

import numpy as np

import render_view_ref as rv
import render_view_scenes as rsc
import track_ref as tr
import track_rgbd_ref as trc
import track_scenes as ts
from taichislam_amd.utils import synthetic as syn
from util import SMALL

F32 = np.float32
VS = ts.VS
TEXTURED = dict(SMALL, texture_enabled=True)
GATES = ts.GATES

# ---- the wall ---------------------------------------------------------------------------------------------------------------------------------
WALL_X = 1.5
WALL_I, WALL_JK = (25, 50), (-40, 40)                      # voxels i = 25 .. 50, j, k = -40 .. 40
WALL_H, WALL_W = 48, 64
WALL_K = np.array([64.0, 0.0, 31.5, 0.0, 64.0, 23.5, 0.0, 0.0, 1.0])
WALL_R = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])       # image z = map +x, image x = map -y, image y = map -z
WALL_T = np.zeros(3)
WALL_START = ((0.03, 2.0), (0.05, 3.0), (0.10, 4.0))       # metres, degrees off the true pose, mostly in the plane of the wall
WALL_TDIR = np.array([0.2, 0.8, -0.56])                    # the direction of the translation error: 20 % of it along the normal
WALL_AXIS = np.array([0.9, 0.3, -0.3])                     # the axis of the rotation error: mostly the normal
# Twice the largest final error tests/test_track_rgbd_cpu.py::test_convergence_on_the_wall measures with the restatement from the three starting guesses
# (the convention of track_scenes.TRACK_BOUND_*).  Measured: see that test's docstring.
WALL_BOUND_M = 2 * 0.000222
WALL_BOUND_DEG = 2 * 0.00112
# the same over the room (test_convergence_in_the_room)
ROOM_BOUND_M = 2 * 0.003287
ROOM_BOUND_DEG = 2 * 0.1986


def wall_colour(y, z):
    """f64 [..., 3] in [0.1, 0.9]: three channels of distinct sinusoids over the wall; luminance = 0.5 + 0.2008 sin(2 pi y / 0.64) + 0.1992 sin(2 pi z / 0.48 + 1)
    (wavelengths of 16 and 12 voxels)"""
    a, b = np.sin(2.0 * np.pi * y / 0.64), np.sin(2.0 * np.pi * z / 0.48 + 1.0)
    return np.stack([0.5 + 0.3 * a + 0.1 * b, 0.5 + 0.15 * a + 0.25 * b, 0.5 + 0.2 * a + 0.2 * b], -1)


@functools.lru_cache(maxsize=None)
def wall_voxels():
    """(indices int16 [n, 3], tsdf f16, weight f16, occupancy int8, colour f16 [n, 3]) of the wall: s = clip(1.5 - x, +-0.4) at weight 1"""
    i = np.arange(WALL_I[0], WALL_I[1] + 1, dtype=np.int16)
    jk = np.arange(WALL_JK[0], WALL_JK[1] + 1, dtype=np.int16)
    idx = np.stack(np.meshgrid(i, jk, jk, indexing="ij"), -1).reshape(-1, 3)
    p = idx.astype(np.float64) * float(VS)
    tsdf = np.clip(WALL_X - p[:, 0], -0.4, 0.4).astype(np.float16)
    n = idx.shape[0]
    return idx, tsdf, np.ones(n, np.float16), np.zeros(n, np.int8), wall_colour(p[:, 1], p[:, 2]).astype(np.float16)


def wall_grid(colour=None):
    """the dense grid (val, known, lo, colour) of the wall for the restatement; colour: other f16 colours [n, 3] in the order of wall_voxels"""
    idx, tsdf, _, _, col = wall_voxels()
    N = int(round(SMALL["map_scale"][0] / SMALL["voxel_scale"]))
    return rv.grid_from_export(idx, tsdf, N, N, np.ascontiguousarray(col if colour is None else colour).view(np.uint16))


@functools.lru_cache(maxsize=None)
def wall_grid_shared():
    return wall_grid()


def load_wall(g, colour=None):
    idx, tsdf, w, occ, col = wall_voxels()
    g.load_numpy(g.get_active_submap_id(), idx, tsdf, w, occ, col if colour is None else colour)


@functools.lru_cache(maxsize=None)
def wall_frame():
    """(depth uint16 [48, 64], rgb uint8 [48, 64, 3]): the analytic images of the wall from the true pose (WALL_R, WALL_T)"""
    jj, ii = np.meshgrid(np.arange(WALL_H, dtype=np.float64), np.arange(WALL_W, dtype=np.float64), indexing="ij")
    y, z = -WALL_X * (ii - WALL_K[2]) / WALL_K[0], -WALL_X * (jj - WALL_K[5]) / WALL_K[4]
    depth = np.full((WALL_H, WALL_W), int(round(1000.0 * WALL_X)), np.uint16)
    return depth, np.clip(np.rint(255.0 * wall_colour(y, z)), 0, 255).astype(np.uint8)


def wall_starts():
    """[(R, T)]: the true pose moved by 3 cm / 2 deg, 5 cm / 3 deg and 10 cm / 4 deg"""
    return [(ts.rotation(WALL_AXIS, deg) @ WALL_R, WALL_T + m * WALL_TDIR / np.linalg.norm(WALL_TDIR)) for m, deg in WALL_START]


def wall_away():
    """the true pose turned by 180 degrees: the camera looks at space nobody observed"""
    return ts.rotation([0.0, 0.0, 1.0], 180.0) @ WALL_R, WALL_T


def in_plane_error(R, T):
    """(metres along the wall, degrees about its normal) of a pose against the true one: the part of the error signed distance cannot see"""
    D = np.asarray(R, np.float64).reshape(3, 3) @ WALL_R.T
    d = np.asarray(T, np.float64).reshape(3) - WALL_T
    return float(np.hypot(d[1], d[2])), float(abs(np.degrees(np.arctan2(D[2, 1] - D[1, 2], D[1, 1] + D[2, 2]))))


@functools.lru_cache(maxsize=None)
def wall_tracks():
    """[(R, T, info)] of the restatement's colour track from the three starting guesses, automatic lambda; computed once"""
    depth, rgb = wall_frame()
    return [trc.track(depth, rgb, R, T, WALL_K, VS, wall_grid_shared(), **GATES) for R, T in wall_starts()]


# ---- the room ---------------------------------------------------------------------------------------------------------------------------------
def room_colour(p):
    """f64 [..., 3] in [0.1, 0.9]: an analytic texture over space; every wall of the box shows it varying in both of its directions"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([0.5 + 0.2 * np.sin(2.0 * np.pi * (x + y) / 0.9) + 0.2 * np.sin(2.0 * np.pi * z / 0.7),
                     0.5 + 0.2 * np.sin(2.0 * np.pi * (y - x) / 1.1 + 1.0) + 0.2 * np.sin(2.0 * np.pi * (z + x) / 0.8),
                     0.5 + 0.2 * np.sin(2.0 * np.pi * (x + z) / 1.0 + 2.0) + 0.2 * np.sin(2.0 * np.pi * y / 0.6)], -1)


def box_rgb(R, T, h=ts.H, w=ts.W, K=None):
    """uint8 [h, w, 3]: the colour of the box's inside at every pixel's hit point, by the ray / face intersection of track_scenes.box_depth"""
    K = syn.scaled_intrinsics(h, w) if K is None else np.asarray(K, np.float64).reshape(-1)
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dc = np.stack([(ii - K[2]) / K[0], (jj - K[5]) / K[4], np.ones_like(ii)], -1)
    d = dc @ np.asarray(R, np.float64).reshape(3, 3).T
    T = np.asarray(T, np.float64).reshape(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (ts.BOX_HI - T) / d, np.where(d < 0, (ts.BOX_LO - T) / d, np.inf)).min(-1)
    return np.clip(np.rint(255.0 * room_colour(T + t[..., None] * d)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def room_frames():
    """[(R, T, depth, rgb)] of the six frames of track_scenes that build the map"""
    return [(R, T, d, box_rgb(R, T)) for R, T, d in ts.map_frames()]


@functools.lru_cache(maxsize=None)
def room_tracked():
    """(R, T, depth, rgb): the tracked frame of track_scenes and its analytic colour image"""
    R, T, depth = ts.tracked_frame()
    return R, T, depth, box_rgb(R, T)


@functools.lru_cache(maxsize=None)
def room_oracle():
    """the oracle's BATCHED textured map of the six frames"""
    from oracle import BATCHED, OracleTSDF
    o = OracleTSDF(**TEXTURED)
    o.set_intrinsics(ts.intrinsics(), ts.intrinsics())
    for R, T, d, c in room_frames():
        o.integrate_depth(R, T, d, c, mode=BATCHED)
    return o


@functools.lru_cache(maxsize=None)
def room_grid():
    """its dense grid (val, known, lo, colour); shared and never written"""
    return rsc.oracle_grid(room_oracle(), colour=True)


@functools.lru_cache(maxsize=None)
def room_tracks():
    """[(R, T, info)] of the restatement's colour track from the three perturbed poses of track_scenes, automatic lambda; computed once"""
    _, _, depth, rgb = room_tracked()
    return [trc.track(depth, rgb, R, T, ts.intrinsics(), VS, room_grid(), **GATES) for R, T in ts.perturbed_poses()]

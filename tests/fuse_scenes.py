"""The smallest scenes that still reach every branch of the submap fusion (csrc/tsl_fuse.hip), shared by tests/test_fuse_window_cpu.py and
tests/test_fuse_poses_gpu.py.

Submap contents are index lists with seeded random voxel values, loaded with load_numpy / import_sparse into the HIP map and the oracle alike, so both
sides fuse the same bits without any integration.  The poses are what the rest of the suite never gives a fusion: rotations near a body diagonal of the
voxel lattice (which push corner splats out of the 15^3 LDS window), a general rotation, a scaled (non-orthonormal) matrix, and translations that put
half of the source outside each wall of the global volume."""
import numpy as np

from util import SMALL, tilt

VS = 0.04
SUB = dict(SMALL, map_scale=[2.56, 2.56], voxel_scale=VS, max_submap_num=4)               # N = Nz = 64: four bricks per axis
SUB_TEX = dict(SUB, texture_enabled=True)
GLOBALS = {
    "cube": dict(SUB, map_scale=[5.12, 5.12], is_global_map=True),                       # N = Nz = 128
    "flat": dict(SUB, map_scale=[5.12, 1.92], is_global_map=True),                       # N = 128, Nz = 48: the z walls cut a rotated source
}
SUB_DIMS = (64, 64)
GLOBAL_DIMS = {"cube": (128, 128), "flat": (128, 48)}


def rotation(axis, angle):
    """Rodrigues' formula, float64"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rotation_onto(src, dst):
    """the rotation about src x dst that turns src onto dst"""
    s = np.asarray(src, np.float64) / np.linalg.norm(src); d = np.asarray(dst, np.float64) / np.linalg.norm(dst)
    return rotation(np.cross(s, d), np.arccos(np.clip(s @ d, -1.0, 1.0)))


DIAG_X = rotation_onto((1, 1, 1), (1, 0, 0))
DIAG_Z = rotation_onto((1, 1, 1), (0, 0, 1))
GENERAL = rotation((0.3, -0.8, 0.5), 1.1)
YAW30 = rotation((0, 0, 1), np.deg2rad(30.0))

# name -> (R, T), float64.  The first group are controls (no miss expected), the second the miss poses
POSES = {
    "yaw30": (YAW30, np.array([0.013, -0.021, 0.007])),
    "tilt": (tilt(np.eye(3), 0.3, 0.2), np.array([0.011, -0.007, 0.003])),
    "diag_x": (DIAG_X, np.array([0.021, 0.002, 0.033])),
    "diag_x_t0": (DIAG_X, np.zeros(3)),
    "diag_z": (DIAG_Z, np.array([0.013, 0.027, -0.009])),
    "general": (GENERAL, np.array([0.5, -0.3, 0.2])),
    "scaled": (1.25 * DIAG_X, np.array([0.021, 0.002, 0.033])),                          # not a rigid pose: accepted unvalidated, the oracle defines the result
}
RIGID = [n for n in POSES if n != "scaled"]
# the six walls of the FLAT global map (x, y at +-2.56 m, z at +-0.96 m): the source's centre sits on the wall, off the lattice by a fraction of a voxel
_OFF = np.array([0.013, -0.009, 0.017])
WALL_POSES = {
    "wall_x_lo": (GENERAL, np.array([-2.56, 0.0, 0.0]) + _OFF), "wall_x_hi": (GENERAL, np.array([2.56, 0.0, 0.0]) + _OFF),
    "wall_y_lo": (GENERAL, np.array([0.0, -2.56, 0.0]) + _OFF), "wall_y_hi": (GENERAL, np.array([0.0, 2.56, 0.0]) + _OFF),
    "wall_z_lo": (GENERAL, np.array([0.0, 0.0, -0.96]) + _OFF), "wall_z_hi": (GENERAL, np.array([0.0, 0.0, 0.96]) + _OFF),
    "outside": (GENERAL, np.array([4.5, 0.3, 0.1])),                                      # every splat beyond the x wall: an empty map, no error
}
ALL_POSES = {**POSES, **WALL_POSES}


def _values(rng, n, textured):
    t = rng.uniform(-0.4, 0.4, n).astype(np.float16)
    w = rng.choice(np.array([1, 2, 5, 64], np.float16), n)
    occ = rng.choice(np.array([0, 1, 3], np.int8), n)
    col = rng.uniform(0.0, 255.0, (n, 3)).astype(np.float16) if textured else None
    return t, w, occ, col


def dense(textured=False):
    """DENSE: the 2 x 2 x 2 bricks at voxel indices -16..15, every voxel observed"""
    r = np.arange(-16, 16, dtype=np.int16)
    idx = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return (idx,) + _values(np.random.default_rng(20), len(idx), textured)


def shell(textured=False):
    """SHELL: a sphere shell of radius 0.7 m, two voxels thick -- sparse: some 8^3 blocks hold a few observed voxels, some none"""
    r = np.arange(-24, 24, dtype=np.int16)
    idx = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    d = np.linalg.norm(idx.astype(np.float64) * VS, axis=1)
    idx = idx[np.abs(d - 0.7) <= VS]
    return (idx,) + _values(np.random.default_rng(21), len(idx), textured)


def one_brick():
    """the one-brick source of the pool-exhaustion test"""
    r = np.arange(0, 16, dtype=np.int16)
    idx = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return (idx,) + _values(np.random.default_rng(22), len(idx), False)


# content -> list of (submap id, scene).  "both" holds DENSE in submap 0 and SHELL in submap 1, each fused with a pose of its own
CONTENTS = {"dense": [(0, dense)], "shell": [(0, shell)], "both": [(0, dense), (1, shell)]}
_NAMES = list(ALL_POSES)


def poses_of(content, pose):
    """the base pose of every submap of `content` for the case `pose`: submap 1 of "both" takes the pose two places further down the list"""
    out = [ALL_POSES[pose]]
    if len(CONTENTS[content]) == 2:
        out.append(ALL_POSES[_NAMES[(_NAMES.index(pose) + 2) % len(_NAMES)]])
    return out

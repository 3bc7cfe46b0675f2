"""Which corner splats of a submap fusion leave the 15^3 LDS window of k_fuse_splat_lds (csrc/tsl_fuse.hip), predicted without a GPU.

tests/fuse_window_ref.py restates the kernel's window arithmetic in numpy float32; this file pins what it predicts for the scenes of tests/fuse_scenes.py.
tests/test_fuse_poses_gpu.py then requires the kernel's own counter (option "fuse_window_misses") to equal these predictions, and the map to equal the
oracle's at the voxels the misses land on.

The window is NOT large enough for every rotation: an 8^3 block spans 7 voxels per edge, 7 * sqrt(3) = 12.12 along its body diagonal, which can straddle
14 floors; the far splat corner (+1) and org = min - 1 then give window index 15 = FW.  Yaw-like poses -- all the suite used before -- never get there."""
import numpy as np
import pytest

import fuse_scenes as S
import fuse_window_ref as W

# predicted misses of DENSE (32 768 observed voxels, 229 376 corner splats), per global map.  diag_x 48, diag_x_t0 12 and diag_z 40 on the cube are the
# figures of the float32 replay that found the gap; the others were computed the same way when this file was written
DENSE_MISSES = {
    "cube": {"yaw30": 0, "tilt": 0, "diag_x": 48, "diag_x_t0": 12, "diag_z": 40, "general": 12, "scaled": 14163,
             "wall_x_lo": 16, "wall_x_hi": 8, "wall_y_lo": 18, "wall_y_hi": 6, "wall_z_lo": 24, "wall_z_hi": 24, "outside": 0},
    "flat": {"yaw30": 0, "tilt": 0, "diag_x": 48, "diag_x_t0": 12, "diag_z": 40, "general": 12, "scaled": 13722,
             "wall_x_lo": 16, "wall_x_hi": 8, "wall_y_lo": 18, "wall_y_hi": 6, "wall_z_lo": 8, "wall_z_hi": 16, "outside": 0},
}
# SHELL (7 892 observed voxels) is sparse: fewer blocks lie on a diagonal
SHELL_MISSES = {
    "cube": {"yaw30": 0, "tilt": 0, "diag_x": 0, "diag_x_t0": 12, "diag_z": 0, "general": 0, "scaled": 4349,
             "wall_x_lo": 4, "wall_x_hi": 0, "wall_y_lo": 4, "wall_y_hi": 0, "wall_z_lo": 4, "wall_z_hi": 4, "outside": 0},
    "flat": {"yaw30": 0, "tilt": 0, "diag_x": 0, "diag_x_t0": 12, "diag_z": 0, "general": 0, "scaled": 4325,
             "wall_x_lo": 4, "wall_x_hi": 0, "wall_y_lo": 4, "wall_y_hi": 0, "wall_z_lo": 0, "wall_z_hi": 4, "outside": 0},
}
MISS_POSES = ("diag_x", "diag_x_t0", "diag_z", "general", "scaled")


def _count(scene, pose, gmap, fw=W.FW):
    R, T = S.ALL_POSES[pose]
    return W.window_misses(scene()[0], R, T, S.VS, S.SUB_DIMS, S.GLOBAL_DIMS[gmap], fw)


def test_scene_sizes():
    assert S.dense()[0].shape == (32768, 3) and S.shell()[0].shape == (7892, 3) and S.one_brick()[0].shape == (4096, 3)
    t = W.splat_table(S.dense()[0], *S.POSES["diag_x"], S.VS, S.SUB_DIMS, S.GLOBAL_DIMS["cube"])
    assert t["miss"].shape[0] == 229376                                      # 7 corners of every voxel, all inside the cubic global map
    for R in (S.DIAG_X, S.DIAG_Z, S.GENERAL, S.YAW30):
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
    assert np.allclose(S.DIAG_X @ (np.ones(3) / np.sqrt(3)), [1, 0, 0]) and np.allclose(S.DIAG_Z @ (np.ones(3) / np.sqrt(3)), [0, 0, 1])


@pytest.mark.parametrize("gmap", ["cube", "flat"])
@pytest.mark.parametrize("pose", list(S.ALL_POSES))
def test_predicted_misses_are_pinned(pose, gmap):
    for scene, table in ((S.dense, DENSE_MISSES), (S.shell, SHELL_MISSES)):
        n, vox = _count(scene, pose, gmap)
        assert n == table[gmap][pose], (scene.__name__, n)
        assert vox.shape[0] <= n and (n == 0) == (vox.shape[0] == 0)
        N, Nz = S.GLOBAL_DIMS[gmap]
        half = np.array([N // 2, N // 2, Nz // 2])
        assert (vox >= -half).all() and (vox < half).all()                   # misses are counted behind in_volume
    if pose in MISS_POSES:
        assert DENSE_MISSES[gmap][pose] > 0
    if pose in ("yaw30", "tilt", "outside"):
        assert DENSE_MISSES[gmap][pose] == 0 and SHELL_MISSES[gmap][pose] == 0


def test_the_largest_window_index_is_exactly_fw():
    """the pinned case: 48 of 229 376 splats leave the window, by one voxel: a window of 16 would hold them"""
    R, T = S.POSES["diag_x"]
    assert _count(S.dense, "diag_x", "cube")[0] == 48
    assert _count(S.dense, "diag_x", "cube", fw=16)[0] == 0


@pytest.mark.parametrize("gmap", ["cube", "flat"])
def test_a_window_of_16_holds_every_rigid_pose(gmap):
    rigid = S.RIGID + list(S.WALL_POSES)
    for scene in (S.dense, S.shell):
        for pose in rigid:
            assert _count(scene, pose, gmap, fw=16)[0] == 0, (scene.__name__, pose)
    assert _count(S.dense, "scaled", gmap, fw=16)[0] > 0                      # 1.25 x a rotation stretches a block's diagonal to 15.2 voxels: no rigid pose


def test_yaw_only_poses_of_the_streams_never_miss():
    """the base poses every earlier fusion test used: synthetic.camera_pose, a yaw about z times a fixed body-to-optical matrix"""
    from taichislam_amd.utils import synthetic as syn
    idx = S.dense()[0]
    for f in range(8):
        for start in (0.0, 22.5, 45.0, 120.0):
            R, T = syn.camera_pose(f, start_deg=start)
            assert W.window_misses(idx, R, T, S.VS, S.SUB_DIMS, S.GLOBAL_DIMS["cube"])[0] == 0, (f, start)


def test_bricks_that_only_blocks_with_misses_reach():
    """what the merge tests rely on: with DENSE at diag_x and SHELL at diag_z one global brick is reached only by blocks that have misses (so a wrong flush
    or miss branch loses it from the touched-brick mask); with the scaled pose one brick is reached by missed splats ALONE"""
    for pose, want_blocks, want_alone in (("diag_x", 1, 0), ("scaled", 58, 1)):
        tabs = [W.splat_table(sc()[0], R, T, S.VS, S.SUB_DIMS, S.GLOBAL_DIMS["cube"]) for (_, sc), (R, T) in zip(S.CONTENTS["both"], S.poses_of("both", pose))]
        via_blocks, alone = W.bricks_reached_only_with_misses(tabs, S.GLOBAL_DIMS["cube"])
        assert (len(via_blocks), len(alone)) == (want_blocks, want_alone), pose
        assert np.isin(alone, via_blocks).all()

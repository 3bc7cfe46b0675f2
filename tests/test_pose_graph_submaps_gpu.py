"""The pose graph end to end on the box room (tests/pose_graph_room.py): three overlapping submaps in a SubmapMapping, a drifted pose table, the three
registrations as constraints, optimize_poses(apply=True), and check_constraints on a fourth, deliberately wrong constraint."""
import numpy as np
import pytest

import pose_graph_room as room
import register_scenes as rs
import track_scenes as ts
from util import SMALL

pytestmark = pytest.mark.gpu


def _mapping():
    """the three submaps, integrated at the identity and opened on frames 0, 6 and 12; the pose table moved to room.start()"""
    from taichislam_amd.mapping import DenseTSDF, SubmapMapping
    opts = dict(SMALL, max_submap_num=4, max_bricks=12288)
    sm = SubmapMapping(DenseTSDF, keyframe_step=6, sub_opts=opts, global_opts=opts)
    sm.set_dep_camera_intrinsic(ts.intrinsics())
    body = (np.eye(3), np.zeros(3))
    for f, (R, T, d) in enumerate(rs.dst_frames() + rs.src_frames() + room.third_frames()):
        sm.recast_depth_to_map_by_frame(f, True, body, (R, T), d, np.array([], dtype=int))
    assert sm.submaps == {0: 0, 6: 1, 12: 2} and sorted(sm.opened) == [0, 6, 12]
    assert all(np.array_equal(sm.opened[f][0], np.eye(3)) and not sm.opened[f][1].any() for f in room.FRAMES)      # create_new_submap recorded the opening poses
    st = room.start()
    sm.set_frame_poses({f: st[f] for f in (6, 12)}, from_remote=True)
    return sm


def test_three_submaps_registered_and_optimised(hip_lib):
    from taichislam_amd.utils import pose_information
    sm = _mapping()
    for fa, fb in room.PAIRS:
        R, T, info = sm.register_submaps(fa, fb)
        assert info["status"] == 0
        sm.add_constraint(fa, fb, R, T, info["information"])
    assert len(sm.constraints) == 3
    g = sm.global_map
    table = (g.submaps_base_R_np.copy(), g.submaps_base_T_np.copy())
    sent = []
    sm.traj_send_handle = sent.append
    # apply=False moves nothing
    poses, report = sm.optimize_poses(odom_information=pose_information(*room.ODOM_SIGMA), **room.SOLVER)
    assert np.array_equal(table[0], g.submaps_base_R_np) and np.array_equal(table[1], g.submaps_base_T_np) and not sent
    assert report["status"] == 0 and report["n_odometry"] == 2 and report["edges"] == [(6, 0), (12, 6), (6, 0), (12, 0), (12, 6)]
    assert len(report["records"]) == report["iterations"] and report["cost"] < report["records"][0]["cost_before"]
    em, ed = room.errors(poses)
    before = room.errors(room.start())
    print(f"optimize_poses: status {report['status']}, {report['iterations']} iterations, cost {report['records'][0]['cost_before']:.4g} -> {report['cost']:.4g}, "
          f"error {before[0]:.6f} m {before[1]:.6f} deg -> {em:.6f} m {ed:.6f} deg (the restatement chain: {room.MEASURED_M} m {room.MEASURED_DEG} deg)")
    assert em <= room.ROOM_BOUND_M and ed <= room.ROOM_BOUND_DEG
    assert np.array_equal(poses[0][0], np.eye(3)) and not poses[0][1].any()      # the first own submap is the fixed one
    # apply=True: the same poses, now in the table, and told to the other agents
    poses2, _ = sm.optimize_poses(odom_information=pose_information(*room.ODOM_SIGMA), apply=True, **room.SOLVER)
    for f in room.FRAMES:
        sid = sm.submaps[f]
        assert np.array_equal(poses2[f][0], poses[f][0]) and np.array_equal(poses2[f][1], poses[f][1])
        assert np.array_equal(g.submaps_base_R_np[sid], poses[f][0]) and np.array_equal(g.submaps_base_T_np[sid], poses[f][1])
    assert len(sent) == 1 and sm.pgo_poses[12][0] is poses2[12][0]


def test_check_constraints_ranks_the_wrong_one_last(hip_lib):
    from taichislam_amd.utils import pose_information
    sm = _mapping()
    for fa, fb in room.PAIRS:
        R, T, info = sm.register_submaps(fa, fb)
        sm.add_constraint(fa, fb, R, T, info["information"])
    fa, fb, R, T = room.wrong_constraint()
    sm.add_constraint(fa, fb, R, T, sm.constraints[1][4])           # with the information of the sound constraint of the same pair
    g = sm.global_map
    table = (g.submaps_base_R_np.copy(), g.submaps_base_T_np.copy())
    out = sm.check_constraints(odom_information=pose_information(*room.ODOM_SIGMA), huber=3.0, **room.SOLVER)
    print("check_constraints: statuses", list(out["status"]), "leave-one-out", out["loo_cost"], "with every edge", out["full_cost"], "order", list(out["order"]))
    assert out["loo_cost"].shape == (4,) and out["order"][-1] == 3 and out["loo_cost"][3] > 10 * out["loo_cost"][:3].max()
    assert np.array_equal(table[0], g.submaps_base_R_np) and np.array_equal(table[1], g.submaps_base_T_np)      # nothing moved

"""Scan-to-model alignment without a GPU: the numpy restatement the GPU tests compare against (tests/track_points_ref.py) sorts every visited point
into one bucket, sums in an order-free way, agrees with the image restatement on the cloud an image back-projects to, and converges on the
spherical scan of the box room (tests/track_points_scenes.py) over the oracle's BATCHED map."""
import ctypes as C

import numpy as np

import track_points_ref as tpr
import track_points_scenes as tps
import track_ref as tr
import track_scenes as ts

F32 = np.float32


def test_buckets_partition_the_visited_points():
    Rt, Tt, _ = ts.tracked_frame()
    scan = tps.scan()
    for R, T in ((Rt, Tt), ts.perturbed_poses()[2], ts.away_pose()):
        for n in (1, 65, scan.shape[0]):
            for stride in (1, 7, n + 1):
                sums, bucket, s = tpr.linearize_points(scan[:n], R, T, stride, tps.VS, ts.oracle_grid(), **tps.GATES)
                v = tpr.visited(n, stride)
                assert sums[tr.I_USED:].sum() == v == bucket.size == s.size and (sums[tr.I_USED:] >= 0).all() and sums[tr.I_E] >= 0
                assert not s[(bucket == tpr.GATE) | (bucket == tpr.UNKNOWN)].view(np.uint32).any()        # +0.0, not -0.0
                if sums[tr.I_USED] == 0:
                    assert not sums[:tr.I_USED].any()
    # an empty cloud; a cloud of bad points is all gate
    sums, bucket, s = tpr.linearize_points(np.zeros((0, 3), F32), Rt, Tt, 1, tps.VS, ts.oracle_grid(), **tps.GATES)
    assert not sums.any() and bucket.size == 0 and s.size == 0
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 1], [1, 0, -np.inf], [1e30, 0, 0], [0, 0, 0], [0, 0, 5.5], [0.1, 0.1, 0.1]], F32)
    sums, bucket, s = tpr.linearize_points(bad, Rt, Tt, 1, tps.VS, ts.oracle_grid(), **tps.GATES)
    assert sums[tr.I_GATE] == 7 and sums.sum() == 7 and (bucket == tpr.GATE).all()


def test_sums_do_not_depend_on_the_point_order():
    """a permuted cloud gives equal integers, and the per-point results follow the permutation"""
    Rp, Tp = ts.perturbed_poses()[1]
    rng = np.random.default_rng(13)
    for stride, huber in ((1, 0.0), (3, 0.02)):
        want, bucket, s = tpr.linearize_points(tps.scan(), Rp, Tp, stride, tps.VS, ts.oracle_grid(), huber=huber, **tps.GATES)
        assert want[tr.I_USED] > (1000 if stride == 1 else 300)
        for _ in range(2):
            order = rng.permutation(tpr.visited(tps.scan().shape[0], stride))
            got, b2, s2 = tpr.linearize_points(tps.scan(), Rp, Tp, stride, tps.VS, ts.oracle_grid(), huber=huber, order=order, **tps.GATES)
            assert np.array_equal(got, want) and np.array_equal(b2, bucket[order]) and np.array_equal(s2.view(np.uint32), s[order].view(np.uint32))
        # permuting the cloud itself (stride 1 visits every point)
        if stride == 1:
            perm = rng.permutation(tps.scan().shape[0])
            assert np.array_equal(tpr.linearize_points(tps.scan()[perm], Rp, Tp, 1, tps.VS, ts.oracle_grid(), huber=huber, **tps.GATES)[0], want)


def test_the_depth_cloud_restates_the_image():
    """the cloud of the image's gated pixels, with a range gate that gates nothing, gives the integers of the image restatement: the scene of the GPU
    test that sets the two kernels against each other"""
    _, _, depth = ts.tracked_frame()
    cloud = tps.depth_cloud()
    for R, T in (ts.tracked_frame()[:2], ts.perturbed_poses()[1]):
        img = tr.linearize(depth, R, T, ts.intrinsics(), 1, tps.VS, ts.oracle_grid(), **ts.GATES)
        pts, _, _ = tpr.linearize_points(cloud, R, T, 1, tps.VS, ts.oracle_grid(), **dict(tps.GATES, **tps.WIDE))
        assert pts[tr.I_GATE] == 0 and cloud.shape[0] + img[tr.I_GATE] == ts.H * ts.W
        keep = [i for i in range(tr.N_SUMS) if i != tr.I_GATE]
        assert np.array_equal(pts[keep], img[keep]) and img[tr.I_USED] > 70000


def test_scene_adequacy():
    """at the true pose the spherical scan uses at least 1000 points and all six pivots of the Cholesky are positive"""
    Rt, Tt, _ = ts.tracked_frame()
    assert tps.scan().shape == (tps.RINGS * tps.AZIMUTHS, 3) and tps.scan().dtype == F32
    sums, bucket, _ = tpr.linearize_points(tps.scan(), Rt, Tt, 1, tps.VS, ts.oracle_grid(), **tps.GATES)
    H, _ = tr.system(sums)
    Hm = np.array(H)
    L = np.zeros((6, 6))
    pivots = []
    for j in range(6):                                    # the pivots of track_ref.solve
        d = Hm[j, j] - (L[j, :j] ** 2).sum()
        pivots.append(d)
        assert d > 0.0, pivots
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (Hm[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    print(f"true pose: used {int(sums[tr.I_USED])}, unknown {int(sums[tr.I_UNKNOWN])} of {tps.scan().shape[0]}; pivots {np.round(pivots, 2).tolist()}; cond(H) {np.linalg.cond(Hm):.1f}")
    assert sums[tr.I_USED] >= 1000 and not tr.solve(sums)[1]
    assert sums[tr.I_UNKNOWN] > sums[tr.I_USED]             # much of the sphere looks at walls nobody saw
    # one wall alone: three points of it give three independent rows at the most, singular
    assert tps.wall_scan().shape[0] > 500 and tps.singular_cloud().shape == (3, 3)
    _, _, info = tpr.track_points(tps.singular_cloud(), Rt, Tt, tps.VS, ts.oracle_grid(), levels=((1, 3),), min_used=1, **tps.GATES)
    assert info["status"] == 3 and info["iterations"] == 1 and info["records"][0]["sums"][tr.I_USED] == 3


def test_convergence():
    """track_points_ref.track_points over the oracle's BATCHED map, the spherical scan from the true pose of the tracked frame, the default levels
    (8, 4), (4, 4), (1, 6).  From 3 cm / 1.5 deg, 6 cm / 3 deg and 10 cm / 5 deg it ends with status 0 after 11 / 8 / 10 linearisations and the
    first level's first step lowers e / n_used.  Measured final error against the true pose: 0.001056 / 0.001070 / 0.001055 m and 0.05377 /
    0.05342 / 0.05377 deg (at the true pose 1524 of the 5760 points are used; the image tracker's 76 000 pixels reach 0.51 mm);
    track_points_scenes.TRACK_POINTS_BOUND_M / _DEG are twice the largest."""
    Rt, Tt, _ = ts.tracked_frame()
    worst_m, worst_deg = 0.0, 0.0
    for (Rp, Tp), (Rf, Tf, info) in zip(ts.perturbed_poses(), tps.reference_tracks()):
        em, ed = ts.pose_error(Rf, Tf, Rt, Tt)
        e0 = ts.pose_error(Rp, Tp, Rt, Tt)
        print(f"from {e0}: final error {em:.6f} m {ed:.5f} deg, status {info['status']}, {info['iterations']} linearisations")
        assert info["status"] == 0 and info["iterations"] == len(info["records"]) <= 14
        recs = info["records"]
        cost = [int(r["sums"][tr.I_E]) / int(r["sums"][tr.I_USED]) for r in recs]
        assert recs[1]["level"] == 0 and cost[1] < cost[0], cost
        assert em < 0.1 * e0[0] and ed < 0.1 * e0[1]
        worst_m, worst_deg = max(worst_m, em), max(worst_deg, ed)
    print(f"largest final error {worst_m:.6f} m, {worst_deg:.5f} deg; bounds {tps.TRACK_POINTS_BOUND_M} m, {tps.TRACK_POINTS_BOUND_DEG} deg")
    assert worst_m <= tps.TRACK_POINTS_BOUND_M and worst_deg <= tps.TRACK_POINTS_BOUND_DEG
    assert tps.TRACK_POINTS_BOUND_M <= 2.0 * worst_m * 1.01 and tps.TRACK_POINTS_BOUND_DEG <= 2.0 * worst_deg * 1.01      # the constants are the measured ones


def test_the_shim_binds_the_point_entry_points():
    """the configuration struct has the layout of the header and the four entry points are exported and bound (the library loads without a GPU); a
    null handle is refused by name before anything else is looked at"""
    from taichislam_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.AlignPointsCfg) == 28
    for name in ("align_points_linearize", "align_points_linearize_dev", "track_points", "track_points_dev"):
        assert "tsl_tsdf_" + name in _lib.SIGNATURES and hasattr(L, "tsl_tsdf_" + name)
    sums = _lib.AlignSums()
    cfg = _lib.AlignPointsCfg()
    cfg.stride = 1
    assert L.tsl_tsdf_align_points_linearize(None, None, None, C.byref(cfg), None, 0, C.byref(sums), None, None) == -1
    assert b"align_points_linearize: null handle" in L.tsl_last_error()
    assert L.tsl_tsdf_track_points_dev(None, None, None, C.byref(cfg), None, None, 0, None, None, None, None) == -1 and b"track_points_dev" in L.tsl_last_error()

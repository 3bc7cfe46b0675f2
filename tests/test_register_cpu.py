"""Map-to-map registration without a GPU: the numpy restatement the GPU tests compare against (tests/register_ref.py) sorts every visited voxel into
one bucket, sums in an order-free way and converges on the two overlapping maps of the box room (tests/register_scenes.py) over the oracle's BATCHED
maps; the library exports the entry points with the documented struct sizes and refuses null handles without a device."""
import ctypes as C

import numpy as np
import pytest

import register_ref as rr
import register_scenes as rs
import track_ref as tr
import track_scenes as ts

F32 = np.float32
OTHER_GATES = dict(w_min=2.0, band=0.05, r_max=0.06, g_max=1.2)


def test_buckets_partition_the_visited_voxels():
    src, grid = rs.src_voxels(), rs.dst_grid()
    poses = [rs.displacement(), rs.perturbed_poses()[2], rs.outside_pose()]
    seen = np.zeros(5, np.int64)
    for stride in rr.STRIDES:
        n = rr.visited(src, stride)
        assert n > 0
        for gates in (rs.GATES, rr.defaults(rs.VS, 10, 0.04, **OTHER_GATES)):
            for k, (R, T) in enumerate(poses):
                s = rr.linearize(src, R, T, stride, rs.VS, grid, **gates)
                assert s[tr.I_USED:].sum() == n, (stride, k, s[tr.I_USED:])
                assert (s[tr.I_USED:] >= 0).all() and s[tr.I_E] >= 0
                if s[tr.I_USED] == 0:
                    assert not s[:tr.I_USED].any()
                if k == 2:                                    # outside the destination's volume: what passes the gate is unknown
                    assert s[tr.I_UNKNOWN] == n - s[tr.I_GATE] and (s[tr.I_UNKNOWN] > 0 or gates is not rs.GATES)
                seen += s[tr.I_USED:] > 0
    assert (seen > 0).all(), f"buckets used / gate / unknown / far / grad occurred in {seen.tolist()} cases"
    # the lattice: stride 1 visits every observed voxel, stride 16 one per brick at the most
    assert rr.visited(src, 1) == src[0].shape[0] and rr.visited(src, 16) < rr.visited(src, 1) / 2048


def test_sums_do_not_depend_on_the_voxel_order():
    src, grid = rs.src_voxels(), rs.dst_grid()
    Rp, Tp = rs.perturbed_poses()[1]
    rng = np.random.default_rng(11)
    for stride, huber in ((1, 0.0), (2, 0.02)):
        want = rr.linearize(src, Rp, Tp, stride, rs.VS, grid, **dict(rs.GATES, huber=F32(huber)))
        assert want[tr.I_USED] > 1000
        for _ in range(2):
            got = rr.linearize(src, Rp, Tp, stride, rs.VS, grid, order=rng.permutation(src[0].shape[0]), **dict(rs.GATES, huber=F32(huber)))
            assert np.array_equal(got, want)


def test_convergence():
    """register_ref.register over the oracle's BATCHED maps: frames 0..5 as the destination, frames 3..8 integrated at D^-1 P as the source, D = 3 deg
    about (1, -2, 0.5) and (0.05, -0.03, 0.017) m; the default levels (4, 4), (2, 4), (1, 6) and the default band of 2 voxels.  From 3 cm / 1.5 deg,
    6 cm / 3 deg and 10 cm / 5 deg it ends with status 0 after 8 / 8 / 8 linearisations.  Measured final error against D: 0.000806 / 0.000806 /
    0.000806 m and 0.013676 / 0.013677 / 0.013677 deg; register_scenes.REGISTER_BOUND_M / REGISTER_BOUND_DEG are twice the largest.  10 cm / 5 deg
    converges too: the edge of the basin lies beyond the perturbations tested.  Of the 181 493 observed source voxels 12.3 % pass the band and
    19 954 are used at D at stride 1; cond(H) = 229."""
    Rd, Td = rs.displacement()
    worst_m, worst_deg = 0.0, 0.0
    for n, ((Rp, Tp), (Rf, Tf, info)) in enumerate(zip(rs.perturbed_poses(), rs.reference_runs())):
        sm, sd = ts.pose_error(Rp, Tp, Rd, Td)
        em, ed = ts.pose_error(Rf, Tf, Rd, Td)
        print(f"from {sm:.3f} m {sd:.2f} deg: final error {em:.6f} m {ed:.6f} deg, status {info['status']}, {info['iterations']} linearisations")
        assert info["iterations"] == len(info["records"]) <= 14
        assert (info["status"], info["iterations"]) == (rs.MEASURED_STATUS[n], rs.MEASURED_ITERATIONS[n])
        if n < 2:                                             # the conditions: status 0, below half a voxel and below the error it started with
            assert info["status"] == 0 and em < rs.HALF_VOXEL and em < sm and ed < sd
        assert em <= rs.MEASURED_M[n] and ed <= rs.MEASURED_DEG[n] and rs.MEASURED_M[n] <= em * 1.01 and rs.MEASURED_DEG[n] <= ed * 1.01      # the constants are the measured ones
        recs = info["records"]
        cost = [int(r["sums"][tr.I_E]) / int(r["sums"][tr.I_USED]) for r in recs]
        first = [k for k, r in enumerate(recs) if r["level"] == 0][0]
        assert cost[first + 1] < cost[first], cost
        worst_m, worst_deg = max(worst_m, em), max(worst_deg, ed)
    print(f"largest final error {worst_m:.6f} m, {worst_deg:.6f} deg; bounds {rs.REGISTER_BOUND_M} m, {rs.REGISTER_BOUND_DEG} deg")
    assert worst_m <= rs.REGISTER_BOUND_M and worst_deg <= rs.REGISTER_BOUND_DEG
    src = rs.src_voxels()
    s = rr.linearize(src, Rd, Td, 1, rs.VS, rs.dst_grid(), **rs.GATES)
    H, _ = tr.system(s)
    n = rr.visited(src, 1)
    print(f"at D, stride 1: {n} visited, {n - int(s[tr.I_GATE])} in the band ({100.0 * (n - int(s[tr.I_GATE])) / n:.1f} %), {int(s[tr.I_USED])} used, cond(H) {np.linalg.cond(np.array(H)):.1f}")
    assert s[tr.I_USED] >= 0.8 * (n - s[tr.I_GATE]) and 0.05 * n < n - s[tr.I_GATE] < 0.3 * n


def test_abi_without_a_device():
    """The two entry points exist, the structs have the documented sizes, and what can be refused without a device is refused with the entry point named."""
    from taichislam_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.RegisterCfg) == 28 and C.sizeof(_lib.AlignSums) == 33 * 8 and C.sizeof(_lib.TrackCfg) == 56
    assert C.sizeof(_lib.TrackReport) == 8 + 64 * C.sizeof(_lib.TrackIter)
    assert [n for n, _ in _lib.RegisterCfg._fields_] == ["stride", "w_min", "band", "r_max", "g_max", "huber", "flags"]
    assert hasattr(L, "tsl_tsdf_register_linearize") and hasattr(L, "tsl_tsdf_register_submap")
    R, T = np.eye(3).reshape(-1), np.zeros(3)
    dp = lambda a: a.ctypes.data_as(_lib.dp)
    cfg, sums, tc, rep = _lib.RegisterCfg(), _lib.AlignSums(), _lib.TrackCfg(), _lib.TrackReport()
    cfg.stride, tc.n_levels, tc.stride[0], tc.iters[0] = 1, 1, 1, 1
    Ro, To = np.zeros(9), np.zeros(3)
    assert L.tsl_tsdf_register_linearize(None, -1, None, -1, dp(R), dp(T), C.byref(cfg), C.byref(sums)) == -1
    assert b"register_linearize" in L.tsl_last_error()
    assert L.tsl_tsdf_register_submap(None, -1, None, -1, dp(R), dp(T), C.byref(cfg), C.byref(tc), dp(Ro), dp(To), C.byref(rep)) == -1
    assert b"register_submap" in L.tsl_last_error()
    from taichislam_amd.mapping import DenseTSDF, SubmapMapping
    assert callable(DenseTSDF.register_linearize) and callable(DenseTSDF.register_submap) and callable(SubmapMapping.register_submaps)

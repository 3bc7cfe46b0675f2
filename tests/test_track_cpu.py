"""Frame-to-model alignment without a GPU: the numpy restatement the GPU tests compare against (tests/track_ref.py) sorts every visited pixel into one
bucket, sums in an order-free way and converges on the box room (tests/track_scenes.py) over the oracle's BATCHED map; the library's host
functions (the step and the retraction) equal the restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import track_ref as tr
import track_scenes as ts

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.parametrize("shape", [(240, 320), (5, 7), (1, 1)])
def test_buckets_partition_the_visited_pixels(shape):
    R, T, depth = ts.tracked_frame()
    img = ts.shaped(depth, shape)
    poses = [(R, T), ts.perturbed_poses()[2], ts.away_pose()]
    for stride in (1, 2, 3):
        for Rp, Tp in poses:
            s = tr.linearize(img, Rp, Tp, ts.intrinsics(), stride, ts.VS, ts.oracle_grid(), **ts.GATES)
            assert s[tr.I_USED:].sum() == tr.visited(shape[0], shape[1], stride), (shape, stride, s[tr.I_USED:])
            assert (s[tr.I_USED:] >= 0).all() and s[tr.I_E] >= 0
            if s[tr.I_USED] == 0:
                assert not s[:tr.I_USED].any()
    # an image without depth is all gate
    s = tr.linearize(np.zeros(shape, np.uint16), R, T, ts.intrinsics(), 1, ts.VS, ts.oracle_grid(), **ts.GATES)
    assert s[tr.I_GATE] == shape[0] * shape[1] and s.sum() == s[tr.I_GATE]


def test_sums_do_not_depend_on_the_pixel_order():
    _, _, depth = ts.tracked_frame()
    Rp, Tp = ts.perturbed_poses()[1]
    rng = np.random.default_rng(11)
    for stride, huber in ((2, 0.0), (3, 0.02)):
        want = tr.linearize(depth, Rp, Tp, ts.intrinsics(), stride, ts.VS, ts.oracle_grid(), huber=huber, **ts.GATES)
        assert want[tr.I_USED] > 1000
        for _ in range(2):
            order = rng.permutation(tr.visited(ts.H, ts.W, stride))
            got = tr.linearize(depth, Rp, Tp, ts.intrinsics(), stride, ts.VS, ts.oracle_grid(), huber=huber, order=order, **ts.GATES)
            assert np.array_equal(got, want)


def test_convergence():
    """track_ref.track over the oracle's BATCHED map of the six frames, the analytic image of a pose nobody integrated, the default levels (8, 4), (4, 4),
    (2, 6).  From 3 cm / 1.5 deg, 6 cm / 3 deg and 10 cm / 5 deg it ends with status 0 after 8 / 9 / 8 linearisations, and every level's first
    step lowers e / n_used.  Measured final error against the true pose: 0.000513 / 0.000512 / 0.000512 m and 0.01826 / 0.01829 / 0.01826 deg (the map
    is the reference's projective TSDF of six frames at 0.04 m voxels); track_scenes.TRACK_BOUND_M / TRACK_BOUND_DEG are twice the largest.  At the
    true pose 99.1 % of the gated pixels are used at stride 2 (19 019 of 19 200) and 99.4 % at stride 1; cond(H) = 247."""
    Rt, Tt, depth = ts.tracked_frame()
    worst_m, worst_deg = 0.0, 0.0
    for (Rp, Tp), (Rf, Tf, info) in zip(ts.perturbed_poses(), ts.reference_tracks()):
        em, ed = ts.pose_error(Rf, Tf, Rt, Tt)
        print(f"from {ts.pose_error(Rp, Tp, Rt, Tt)}: final error {em:.6f} m {ed:.5f} deg, status {info['status']}, {info['iterations']} linearisations")
        assert info["status"] == 0 and info["iterations"] == len(info["records"]) <= 14
        recs = info["records"]
        cost = [int(r["sums"][tr.I_E]) / int(r["sums"][tr.I_USED]) for r in recs]
        for lv in range(3):
            first = [k for k, r in enumerate(recs) if r["level"] == lv][0]
            assert recs[first + 1]["level"] == lv and cost[first + 1] < cost[first], (lv, cost)
        worst_m, worst_deg = max(worst_m, em), max(worst_deg, ed)
    print(f"largest final error {worst_m:.6f} m, {worst_deg:.5f} deg; bounds {ts.TRACK_BOUND_M} m, {ts.TRACK_BOUND_DEG} deg")
    assert worst_m <= ts.TRACK_BOUND_M and worst_deg <= ts.TRACK_BOUND_DEG
    assert ts.TRACK_BOUND_M <= 2.0 * worst_m * 1.01 and ts.TRACK_BOUND_DEG <= 2.0 * worst_deg * 1.01      # the constants are the measured ones
    for stride in (1, 2):
        s = tr.linearize(depth, Rt, Tt, ts.intrinsics(), stride, ts.VS, ts.oracle_grid(), **ts.GATES)
        gated = tr.visited(ts.H, ts.W, stride) - int(s[tr.I_GATE])
        H, _ = tr.system(s)
        print(f"true pose, stride {stride}: used {int(s[tr.I_USED])} of {gated} gated pixels, cond(H) {np.linalg.cond(np.array(H)):.1f}")
        assert s[tr.I_USED] >= 0.9 * gated and gated > 0.9 * tr.visited(ts.H, ts.W, stride)


def _host_lib():
    from taichislam_amd import _lib
    return _lib, _lib.lib()


def _c_solve(L, _lib, sums, damping):
    s = _lib.AlignSums()
    C.memmove(C.byref(s), np.ascontiguousarray(sums, np.int64).ctypes.data, 33 * 8)
    xi = np.full(6, 7.0)
    sing = C.c_int32(-1)
    assert L.tsl_align_solve(C.byref(s), float(damping), xi.ctypes.data_as(_lib.dp), C.byref(sing)) == 0
    return xi, sing.value


def _c_retract(L, _lib, xi, R, T):
    x, Rc, Tc = np.array(xi, np.float64), np.array(R, np.float64).reshape(-1).copy(), np.array(T, np.float64).copy()
    assert L.tsl_pose_retract(x.ctypes.data_as(_lib.dp), Rc.ctypes.data_as(_lib.dp), Tc.ctypes.data_as(_lib.dp)) == 0
    return Rc.reshape(3, 3), Tc


def test_host_functions_equal_the_restatement():
    """tsl_align_solve and tsl_pose_retract (pure host code: the library loads without a GPU) against track_ref.solve / retract, bit for bit: on every
    system and pose of the restatement's three runs, on 100 random positive definite systems built from integer sums, with and without damping; an
    all-zero system is singular with xi = 0."""
    _lib, L = _host_lib()
    assert C.sizeof(_lib.AlignSums) == 33 * 8 and C.sizeof(_lib.AlignCfg) == 112 and C.sizeof(_lib.TrackIter) == 18 * 8 + 33 * 8
    assert C.sizeof(_lib.TrackCfg) == 56 and C.sizeof(_lib.TrackReport) == 8 + 64 * C.sizeof(_lib.TrackIter)
    n = 0
    for _, _, info in ts.reference_tracks():
        for r in info["records"]:
            for damping in (0.0, 1e-3):
                want, sing = tr.solve(r["sums"], damping)
                got, gsing = _c_solve(L, _lib, r["sums"], damping)
                assert not sing and gsing == 0 and np.array_equal(_bits(got), _bits(want))
            assert np.array_equal(_bits(r["xi"]), _bits(tr.solve(r["sums"], 0.0)[0]))
            Rw, Tw = tr.retract(r["xi"], r["R"], r["T"])
            Rg, Tg = _c_retract(L, _lib, r["xi"], r["R"], r["T"])
            assert np.array_equal(_bits(Rg), _bits(Rw)) and np.array_equal(_bits(Tg), _bits(Tw))
            assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-12
            n += 1
    assert n >= 24
    rng = np.random.default_rng(5)
    iu = np.triu_indices(6)
    for k in range(100):
        J = rng.integers(-3000, 3000, size=(40, 6)).astype(np.int64)
        res = rng.integers(-2000, 2000, size=40).astype(np.int64)
        sums = np.zeros(33, np.int64)
        sums[:21] = (J.T @ J)[iu] * 64
        sums[21:27] = (J.T @ res) * 64
        sums[27] = int(res @ res) * 64
        sums[28] = 40
        damping = (0.0, 0.25)[k & 1]
        want, sing = tr.solve(sums, damping)
        got, gsing = _c_solve(L, _lib, sums, damping)
        assert not sing and gsing == 0 and np.array_equal(_bits(got), _bits(want))
        H, b = tr.system(sums, damping)
        assert np.allclose(np.array(H) @ got, -np.array(b), rtol=1e-8, atol=1e-8)
        R0, T0 = ts.rotation(rng.standard_normal(3), 30.0 * k), rng.standard_normal(3)
        xi = rng.standard_normal(6) * 0.1
        Rw, Tw = tr.retract(xi, R0, T0)
        Rg, Tg = _c_retract(L, _lib, xi, R0, T0)
        assert np.array_equal(_bits(Rg), _bits(Rw)) and np.array_equal(_bits(Tg), _bits(Tw))
    # singular systems: all zero; rank one
    for sums in (np.zeros(33, np.int64), np.concatenate([(np.outer(np.arange(1, 7), np.arange(1, 7))[iu] << 20), np.ones(12, np.int64)])):
        want, sing = tr.solve(sums)
        got, gsing = _c_solve(L, _lib, sums, 0.0)
        assert sing and gsing == 1 and not any(want) and not got.any()
    # a zero step leaves the pose alone; the first-order behaviour of the retraction is the twist the Jacobian assumes
    R0, T0 = ts.pose(1.0)
    Rg, Tg = _c_retract(L, _lib, np.zeros(6), R0, T0)
    assert np.array_equal(Rg, R0) and np.array_equal(Tg, T0)
    xi = np.array([1e-3, -2e-3, 5e-4, 2e-3, 1e-3, -1.5e-3])
    Rg, Tg = _c_retract(L, _lib, xi, R0, T0)
    p = np.array([0.7, -1.1, 2.0])
    q = R0 @ p + T0
    assert np.abs((Rg @ p + Tg) - (q + xi[:3] + np.cross(xi[3:], q))).max() < 2e-5
    # refusals
    xi6 = np.zeros(6)
    assert L.tsl_align_solve(None, 0.0, xi6.ctypes.data_as(_lib.dp), None) == -1 and b"align_solve" in L.tsl_last_error()
    assert L.tsl_pose_retract(None, None, None) == -1 and b"pose_retract" in L.tsl_last_error()

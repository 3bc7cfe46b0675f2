"""The depth-and-colour alignment without a GPU: the numpy restatement (tests/track_rgbd_ref.py) on the scenes of tests/track_rgbd_scenes.py -- its
buckets, its independence of the pixel order, its geometric half against track_ref, the combined step against track_ref's and against the library's
host function, and what the colour term is for: on a flat textured wall the depth-only tracker cannot move along the wall, the colour tracker
converges."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import track_ref as tr
import track_rgbd_ref as trc
import track_rgbd_scenes as sc
import track_scenes as ts

SHAPES = ((1, 1), (5, 7), (17, 33), (ts.H, ts.W))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _shaped_rgb(rgb, shape):
    out = np.zeros(shape + (3,), np.uint8)
    h, w = min(shape[0], rgb.shape[0]), min(shape[1], rgb.shape[1])
    out[:h, :w] = rgb[:h, :w]
    return out


def _room_poses():
    Rt, Tt, _, _ = sc.room_tracked()
    return [("true", Rt, Tt), ("perturbed",) + ts.perturbed_poses()[1], ("away",) + ts.away_pose()]


@pytest.mark.parametrize("shape", SHAPES)
def test_both_bucket_sets_partition_the_visited_pixels(shape):
    """In the room: every visited pixel lies in exactly one geometric and exactly one colour bucket, at strides 1 to 3, at the true pose, a perturbed one
    and the away pose; gate and unknown are the same pixels in both halves; the colour half uses at least the geometrically used pixels less those
    its own gates take."""
    _, _, depth, rgb = sc.room_tracked()
    img, col = ts.shaped(depth, shape), _shaped_rgb(rgb, shape)
    for name, R, T in _room_poses():
        for stride in (1, 2, 3):
            s = trc.linearize(img, col, R, T, ts.intrinsics(), stride, sc.VS, sc.room_grid(), **sc.GATES)
            g, c = s[trc.GEO], s[trc.COL]
            v = tr.visited(shape[0], shape[1], stride)
            assert g[tr.I_USED:].sum() == v and c[tr.I_USED:].sum() == v, (name, stride, g[tr.I_USED:], c[tr.I_USED:])
            assert (s >= 0)[[28, 29, 30, 31, 32, 61, 62, 63, 64, 65]].all()
            assert g[tr.I_GATE] == c[tr.I_GATE] and g[tr.I_UNKNOWN] == c[tr.I_UNKNOWN]
            assert c[tr.I_FAR] >= g[tr.I_FAR]                                  # a pixel off the surface is colour-far too
            if name == "away":
                assert g[tr.I_USED] == 0 and c[tr.I_USED] == 0 and not s[:28].any() and not s[33:61].any()


def test_colour_gates_move_pixels_between_the_buckets():
    """rc_max and gc_max take used pixels into far and grad; the geometric half does not notice; the colour buckets do not depend on the geometric grad."""
    Rp, Tp = ts.perturbed_poses()[1]
    _, _, depth, rgb = sc.room_tracked()
    K = ts.intrinsics()
    base = trc.linearize(depth, rgb, Rp, Tp, K, 2, sc.VS, sc.room_grid(), **sc.GATES)
    tight = trc.linearize(depth, rgb, Rp, Tp, K, 2, sc.VS, sc.room_grid(), rc_max=0.05, gc_max=1.0, **sc.GATES)
    assert np.array_equal(base[trc.GEO], tight[trc.GEO])
    b, t = base[trc.COL], tight[trc.COL]
    assert t[tr.I_FAR] > b[tr.I_FAR] and t[tr.I_GRAD] > b[tr.I_GRAD] and t[tr.I_USED] < b[tr.I_USED] and t[tr.I_USED] > 1000
    # g_max so small that every geometric sample is grad: the colour half is what it was
    nog = trc.linearize(depth, rgb, Rp, Tp, K, 2, sc.VS, sc.room_grid(), **dict(sc.GATES, g_max=0.01))
    assert nog[trc.GEO][tr.I_USED] == 0 and nog[trc.GEO][tr.I_GRAD] > 10000 and np.array_equal(nog[trc.COL], base[trc.COL])
    # a robust weight on the colour residual changes the colour sums only
    hub = trc.linearize(depth, rgb, Rp, Tp, K, 2, sc.VS, sc.room_grid(), huber_c=0.02, **sc.GATES)
    assert np.array_equal(hub[trc.GEO], base[trc.GEO]) and np.array_equal(hub[trc.COL][tr.I_USED:], b[tr.I_USED:]) and hub[trc.COL][tr.I_E] < b[tr.I_E]


def test_sums_do_not_depend_on_the_pixel_order_and_the_geometric_half_is_track_ref():
    Rp, Tp = ts.perturbed_poses()[1]
    _, _, depth, rgb = sc.room_tracked()
    wd, wc = sc.wall_frame()
    rng = np.random.default_rng(11)
    cases = [(depth, rgb, Rp, Tp, ts.intrinsics(), sc.room_grid(), 2, 0.0, 0.0), (depth, rgb, Rp, Tp, ts.intrinsics(), sc.room_grid(), 3, 0.02, 0.03),
             (wd, wc) + sc.wall_starts()[2] + (sc.WALL_K, sc.wall_grid_shared(), 1, 0.0, 0.02)]
    for d, c, R, T, K, grid, stride, huber, huber_c in cases:
        want = trc.linearize(d, c, R, T, K, stride, sc.VS, grid, huber=huber, huber_c=huber_c, **sc.GATES)
        assert want[trc.COL][tr.I_USED] > 500
        assert np.array_equal(want[trc.GEO], tr.linearize(d, R, T, K, stride, sc.VS, grid[:3], huber=huber, **sc.GATES))
        for _ in range(2):
            order = rng.permutation(tr.visited(d.shape[0], d.shape[1], stride))
            assert np.array_equal(trc.linearize(d, c, R, T, K, stride, sc.VS, grid, huber=huber, huber_c=huber_c, order=order, **sc.GATES), want)


def _lib_solve(sums, lam, damping):
    from taichislam_amd import _lib
    L = _lib.lib()
    s = _lib.AlignRgbdSums()
    C.memmove(C.byref(s), np.ascontiguousarray(sums, np.int64).ctypes.data, 66 * 8)
    xi = np.full(6, 7.0)
    sing = C.c_int32(-1)
    assert L.tsl_align_rgbd_solve(C.byref(s), float(lam), float(damping), xi.ctypes.data_as(_lib.dp), C.byref(sing)) == 0, L.tsl_last_error()
    return xi, sing.value


def test_the_step():
    """With lambda = 0 the combined step is track_ref's step on the geometric half, bit for bit; tsl_align_rgbd_solve (pure host code: the library loads
    without a GPU) equals the restatement bit for bit on every system of the restatement's six runs, for several weights, with and without damping;
    the wall's geometric half alone is singular, and a weight on the colour half makes it regular."""
    from taichislam_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.AlignRgbdCfg) == 128 and C.sizeof(_lib.AlignRgbdSums) == 66 * 8 and C.sizeof(_lib.TrackRgbdIter) == 18 * 8 + 66 * 8
    assert C.sizeof(_lib.TrackRgbdReport) == 16 + 64 * C.sizeof(_lib.TrackRgbdIter) and _lib.TrackRgbdReport.lam.offset == 8
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    assert int(re.search(r"TSL_K_ALIGN_RGBD = (\d+)", hdr).group(1)) == _lib.K_ALIGN_RGBD and _lib.KERNEL_NAMES[_lib.K_ALIGN_RGBD] == "align_rgbd"
    assert int(re.search(r"TSL_K_END = (\d+)", hdr).group(1)) == max(_lib.KERNEL_NAMES) + 1
    n = 0
    for _, _, info in sc.wall_tracks() + sc.room_tracks():
        for rec in info["records"]:
            s = rec["sums"]
            for damping in (0.0, 1e-3):
                x0, sing0 = trc.solve(s, 0.0, damping)
                xg, singg = tr.solve(s[trc.GEO], damping)
                assert sing0 == singg and np.array_equal(_bits(x0), _bits(xg))
                for lam in (0.0, info["lam"], 0.5, 3.0):
                    want, sing = trc.solve(s, lam, damping)
                    got, gs = _lib_solve(s, lam, damping)
                    assert gs == int(sing) and np.array_equal(_bits(got), _bits(want)), (lam, damping, got, want)
                    n += 1
            assert np.array_equal(_bits(trc.solve(s, info["lam"])[0]), _bits(rec["xi"]))
    assert n > 300
    s = sc.wall_tracks()[0][2]["records"][0]["sums"]
    assert trc.solve(s, 0.0)[1] and _lib_solve(s, 0.0, 0.0)[1] == 1 and not _lib_solve(s, 0.0, 0.0)[0].any()
    assert not trc.solve(s, 0.2)[1]
    Hg, Hc = np.array(tr.system(s[trc.GEO])[0]), np.array(tr.system(s[trc.COL])[0])
    print(f"the wall at the first guess: cond(Hg + 0.2 Hc) = {np.linalg.cond(Hg + 0.2 * Hc):.1f}, rank(Hg) = {np.linalg.matrix_rank(Hg)}")
    assert np.linalg.matrix_rank(Hg) == 3 and np.linalg.cond(Hg + 0.2 * Hc) < 1e4
    # the automatic weight: the ratio of the translation traces, 0 for a view without texture
    assert trc.auto_lambda(s) == ((float(s[0]) + float(s[6])) + float(s[11])) / ((float(s[33]) + float(s[39])) + float(s[44]))
    z = s.copy(); z[trc.COL] = 0
    assert trc.auto_lambda(z) == 0.0 and trc.auto_lambda(s, 2.0) == 2.0 * ((float(s[0]) + float(s[6])) + float(s[11])) / ((float(s[33]) + float(s[39])) + float(s[44]))
    xi6, i32 = np.zeros(6), C.c_int32()
    sums = _lib.AlignRgbdSums()
    for lam, damping in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.2, -1.0), (0.2, float("nan"))):
        assert L.tsl_align_rgbd_solve(C.byref(sums), lam, damping, xi6.ctypes.data_as(_lib.dp), C.byref(i32)) == -1 and b"align_rgbd_solve" in L.tsl_last_error()
    assert L.tsl_align_rgbd_solve(None, 0.0, 0.0, xi6.ctypes.data_as(_lib.dp), C.byref(i32)) == -1


def test_convergence_on_the_wall():
    """One flat textured wall seen head-on, 48 x 64 pixels, 4 cm voxels, the default levels.  From 3 cm / 2 deg, 5 cm / 3 deg and 10 cm / 4 deg off (2.9 / 4.9
    / 9.8 cm of it along the wall, 1.8 / 2.7 / 3.6 deg about its normal) track_ref.track -- depth only -- ends singular at its first linearisation:
    H has rank 3.  The colour track ends with status 0 after 6 / 7 / 7 linearisations with the automatic lambda 0.222 / 0.220 / 0.201.  Measured
    final error against the true pose: 0.000220 / 0.000221 / 0.000222 m and 0.001119 / 0.001118 / 0.001118 deg; track_rgbd_scenes.WALL_BOUND_M /
    WALL_BOUND_DEG are twice the largest."""
    depth, rgb = sc.wall_frame()
    worst_m, worst_deg = 0.0, 0.0
    for (Rp, Tp), (R, T, info) in zip(sc.wall_starts(), sc.wall_tracks()):
        m0, d0 = sc.in_plane_error(Rp, Tp)
        Rg, Tg, ig = tr.track(depth, Rp, Tp, sc.WALL_K, sc.VS, sc.wall_grid_shared()[:3], **sc.GATES)
        mg, dg = sc.in_plane_error(Rg, Tg)
        print(f"from {m0:.4f} m {d0:.3f} deg in the plane: depth only status {ig['status']}, left {mg:.4f} m {dg:.3f} deg")
        assert ig["status"] in (2, 3) or (mg >= 0.5 * m0 and dg >= 0.5 * d0)
        em, ed = ts.pose_error(R, T, sc.WALL_R, sc.WALL_T)
        print(f"   depth and colour: status {info['status']}, {info['iterations']} linearisations, lambda {info['lam']:.4f}, final error {em:.6f} m {ed:.6f} deg")
        assert info["status"] == 0 and info["iterations"] == len(info["records"]) <= 14 and 0.05 < info["lam"] < 1.0
        worst_m, worst_deg = max(worst_m, em), max(worst_deg, ed)
    print(f"largest final error {worst_m:.6f} m, {worst_deg:.6f} deg; bounds {sc.WALL_BOUND_M} m, {sc.WALL_BOUND_DEG} deg")
    assert worst_m <= sc.WALL_BOUND_M and worst_deg <= sc.WALL_BOUND_DEG
    assert sc.WALL_BOUND_M <= 2.0 * worst_m * 1.01 and sc.WALL_BOUND_DEG <= 2.0 * worst_deg * 1.01      # the constants are the measured ones


def test_convergence_in_the_room():
    """The textured box room of six frames, the tracked frame and the perturbations of track_scenes.  The colour track converges from all three with status
    0 after 12 / 10 / 11 linearisations, lambda 1.363 / 1.309 / 1.178.  Measured final error: 0.003183 / 0.003254 / 0.003286 m and 0.19558 / 0.19858 /
    0.19482 deg -- against the depth-only 0.000513 m / 0.0183 deg: the room constrains all six degrees of freedom by its geometry, and the colour the
    reference's integration stores (the colour of the last ray through a voxel, over the whole band) is a blunter measurement than the distance, so
    here it costs accuracy; it is for the scenes where geometry leaves a direction free.  ROOM_BOUND_M / ROOM_BOUND_DEG are twice the largest."""
    Rt, Tt, _, _ = sc.room_tracked()
    worst_m, worst_deg = 0.0, 0.0
    for (Rp, Tp), (R, T, info), (Rg, Tg, ig) in zip(ts.perturbed_poses(), sc.room_tracks(), ts.reference_tracks()):
        em, ed = ts.pose_error(R, T, Rt, Tt)
        gm, gd = ts.pose_error(Rg, Tg, Rt, Tt)
        print(f"from {ts.pose_error(Rp, Tp, Rt, Tt)}: depth and colour status {info['status']}, {info['iterations']} linearisations, lambda {info['lam']:.4f}, "
              f"final error {em:.6f} m {ed:.5f} deg; depth only {gm:.6f} m {gd:.5f} deg")
        assert info["status"] == 0 and info["iterations"] <= 14
        worst_m, worst_deg = max(worst_m, em), max(worst_deg, ed)
    assert worst_m <= sc.ROOM_BOUND_M and worst_deg <= sc.ROOM_BOUND_DEG
    assert sc.ROOM_BOUND_M <= 2.0 * worst_m * 1.01 and sc.ROOM_BOUND_DEG <= 2.0 * worst_deg * 1.01      # the constants are the measured ones

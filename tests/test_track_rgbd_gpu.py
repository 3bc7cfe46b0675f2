"""Depth-and-colour alignment on the GPU (tsl_align_rgbd.hip): the 66 integers of a linearisation and every record of a tracking run against the numpy
restatement (tests/track_rgbd_ref.py) over the oracle's textured map of the box room and over the hand-built wall (tests/track_rgbd_scenes.py), the
geometric half against align_linearize, counts only, stored colours that are not finite, the device forms, the refusals."""
import ctypes as C

import numpy as np
import pytest

import track_ref as tr
import track_rgbd_ref as trc
import track_rgbd_scenes as sc
import track_scenes as ts
from util import assert_export_equal, lin

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (5, 7), (17, 33), (ts.H, ts.W))           # (17, 33): one pixel beyond a 16 x 16 tile on both axes
_ROOM = []


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _room():
    """(HIP textured map of the six frames, the restatement's grid of the oracle's); the two maps are compared once, colours included"""
    if not _ROOM:
        from taichislam_amd.mapping import DenseTSDF
        g = DenseTSDF(**sc.TEXTURED)
        g.set_dep_camera_intrinsic(ts.intrinsics())
        g.set_color_camera_intrinsic(ts.intrinsics())
        for R, T, d, c in sc.room_frames():
            g.recast_depth_to_map(R, T, d, c)
        got, want = g.export_submap(), sc.room_oracle().export_sparse()
        assert_export_equal(got, want, "the HIP textured map against the oracle's")
        a, b = np.argsort(lin(got["indices"]), kind="stable"), np.argsort(lin(want["indices"]), kind="stable")
        assert np.array_equal(np.asarray(got["color"])[a].view(np.uint16), np.asarray(want["color"])[b].view(np.uint16)), "the colours differ"
        _ROOM.append(g)
    return _ROOM[0], sc.room_grid()


def _wall(colour=None):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**sc.TEXTURED)
    g.set_dep_camera_intrinsic(sc.WALL_K)
    sc.load_wall(g, colour)
    return g


def _dev(depth, rgb):
    import torch
    return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda(), torch.from_numpy(np.ascontiguousarray(rgb)).cuda()


def _shaped_rgb(rgb, shape):
    out = np.zeros(shape + (3,), np.uint8)
    h, w = min(shape[0], rgb.shape[0]), min(shape[1], rgb.shape[1])
    out[:h, :w] = rgb[:h, :w]
    return out


def _both(d):
    return np.concatenate([d["geo"]["sums"], d["col"]["sums"]])


def _same_records(got, want, what):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"] == len(got["records"]), \
        f"{what}: status {got['status']} / {want['status']}, iterations {got['iterations']} / {want['iterations']}"
    assert np.array_equal(_bits(got["lambda"]), _bits(want["lam"])), f"{what}: lambda {got['lambda']!r} / {want['lam']!r}"
    for k, (a, b) in enumerate(zip(got["records"], want["records"])):
        s = _both(a)
        assert np.array_equal(s, b["sums"]), f"{what}, record {k}: sums differ at {np.nonzero(s != b['sums'])[0].tolist()}"
        for f in ("R", "T", "xi"):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), f"{what}, record {k}: {f} differs: {a[f]} / {b[f]}"


@pytest.mark.parametrize("shape", SHAPES)
def test_the_sums_equal_the_restatement(hip_lib, shape):
    """All 66 integers over the oracle's textured map, at the true pose, a perturbed pose and the away pose, strides 1 to 3, with and without Huber weights,
    in the host and the device form; the geometric half equals align_linearize's integers on the same inputs."""
    import torch
    g, grid = _room()
    Rt, Tt, depth, rgb = sc.room_tracked()
    K = ts.intrinsics()
    img, col = ts.shaped(depth, shape), _shaped_rgb(rgb, shape)
    dimg, dcol = _dev(img, col)
    seen = np.zeros(10, np.int64)
    for name, R, T in (("true", Rt, Tt), ("perturbed",) + ts.perturbed_poses()[1], ("away",) + ts.away_pose()):
        for stride in (1, 2, 3):
            for huber, huber_c in ((0.0, 0.0), (0.02, 0.03)):
                what = f"{shape}, {name}, stride {stride}, huber {huber} / {huber_c}"
                want = trc.linearize(img, col, R, T, K, stride, sc.VS, grid, huber=huber, huber_c=huber_c, **sc.GATES)
                got = _both(g.align_rgbd_linearize(img, col, R, T, K=K, stride=stride, huber=huber, huber_c=huber_c))
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, f"{what}: sums {bad.tolist()} differ: {got[bad]} / {want[bad]}"
                dev = g.align_rgbd_linearize(dimg, dcol, R, T, K=K, stride=stride, huber=huber, huber_c=huber_c, device=True)
                assert dev.is_cuda and dev.dtype == torch.int64 and dev.shape == (80,)
                dv = dev.cpu().numpy()
                assert np.array_equal(dv[:33], want[trc.GEO]) and np.array_equal(dv[40:73], want[trc.COL]) and not dv[33:40].any() and not dv[73:].any(), what
                assert np.array_equal(g.align_linearize(img, R, T, K=K, stride=stride, huber=huber)["sums"], got[trc.GEO]), what
                seen += np.concatenate([want[28:33], want[61:66]]) > 0
    if shape == SHAPES[-1]:
        assert (seen[[0, 2, 3, 4, 5, 7, 8]] > 0).all(), f"buckets used / gate / unknown / far / grad of the two halves occurred in {seen.tolist()} cases"


def test_counts_only_gates_and_the_dict(hip_lib):
    g, grid = _room()
    Rp, Tp = ts.perturbed_poses()[1]
    _, _, depth, rgb = sc.room_tracked()
    K = ts.intrinsics()
    want = trc.linearize(depth, rgb, Rp, Tp, K, 2, sc.VS, grid, **sc.GATES)
    got = g.align_rgbd_linearize(depth, rgb, Rp, Tp, stride=2)                  # the defaults: the map's K, the gates of SMALL, rc_max 1, gc_max 1 / voxel
    assert np.array_equal(_both(got), want)
    for half, sl in (("geo", trc.GEO), ("col", trc.COL)):
        d, w = got[half], want[sl]
        assert np.array_equal(d["H"][np.triu_indices(6)], w[:21]) and np.array_equal(d["H"], d["H"].T) and np.array_equal(d["b"], w[21:27]) and d["e"] == w[27]
        assert [d[n] for n in ("n_used", "n_gate", "n_unknown", "n_far", "n_grad")] == w[tr.I_USED:].tolist() and d["n_used"] > 10000
    # counts only: the sums are zero and the counts are unchanged, in both forms
    co = _both(g.align_rgbd_linearize(depth, rgb, Rp, Tp, stride=2, counts_only=True))
    dv = g.align_rgbd_linearize(*_dev(depth, rgb), Rp, Tp, stride=2, counts_only=True, device=True).cpu().numpy()
    for c in (co, np.concatenate([dv[:33], dv[40:73]])):
        assert not c[:28].any() and not c[33:61].any() and np.array_equal(c[28:33], want[28:33]) and np.array_equal(c[61:66], want[61:66])
    # the colour gates move pixels into far and grad as the restatement says; the geometric half does not notice
    gates = dict(rc_max=0.05, gc_max=1.0, huber_c=0.01)
    tight = _both(g.align_rgbd_linearize(depth, rgb, Rp, Tp, K=K, stride=2, **gates))
    assert np.array_equal(tight, trc.linearize(depth, rgb, Rp, Tp, K, 2, sc.VS, grid, **gates, **sc.GATES))
    assert np.array_equal(tight[trc.GEO], want[trc.GEO]) and tight[64] > want[64] and tight[65] > want[65]
    # the host form takes device images too
    assert np.array_equal(_both(g.align_rgbd_linearize(*_dev(depth, rgb), Rp, Tp, stride=2)), want)
    with pytest.raises(ValueError, match="align_rgbd_linearize"):
        g.align_rgbd_linearize(depth, _dev(depth, rgb)[1], Rp, Tp)
    with pytest.raises(ValueError, match="align_rgbd_linearize"):
        g.align_rgbd_linearize(depth, rgb[:, :-1], Rp, Tp)


def test_colours_that_are_not_finite(hip_lib):
    """A NaN colour and an inf colour (tsl_tsdf_import_sparse writes any bit pattern) in hand-picked voxels of the wall: the samples whose cells touch
    them are colour-far or colour-grad -- the restatement refuses a product that is not finite, and the GPU equals it -- and the geometric half is
    what it is on the clean wall."""
    idx, _, _, _, col = sc.wall_voxels()
    depth, rgb = sc.wall_frame()
    bad = col.copy()
    picks = {(37, 3, -2): (np.nan, 0.5, 0.5), (38, -7, 5): (0.5, np.inf, 0.5), (37, 10, 10): (0.5, 0.5, -np.inf), (38, -12, -9): (np.nan, np.inf, 0.25)}
    for (i, j, k), c in picks.items():
        n = np.nonzero((idx[:, 0] == i) & (idx[:, 1] == j) & (idx[:, 2] == k))[0]
        assert n.size == 1
        bad[n[0]] = np.array(c, np.float16)
    clean, dirty = _wall(), _wall(bad)
    grid = sc.wall_grid(bad)
    for R, T in [(sc.WALL_R, sc.WALL_T)] + sc.wall_starts()[:2]:
        for stride in (1, 2):
            want = trc.linearize(depth, rgb, R, T, sc.WALL_K, stride, sc.VS, grid, huber_c=0.05, **sc.GATES)
            got = _both(dirty.align_rgbd_linearize(depth, rgb, R, T, K=sc.WALL_K, stride=stride, huber_c=0.05))
            ref = _both(clean.align_rgbd_linearize(depth, rgb, R, T, K=sc.WALL_K, stride=stride, huber_c=0.05))
            assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()
            assert np.array_equal(ref, trc.linearize(depth, rgb, R, T, sc.WALL_K, stride, sc.VS, sc.wall_grid_shared(), huber_c=0.05, **sc.GATES))
            assert np.array_equal(got[trc.GEO], ref[trc.GEO])
            lost = ref[61] - got[61]
            assert lost > 0 and (got[64] - ref[64]) + (got[65] - ref[65]) == lost, (stride, got[61:], ref[61:])
    R, T, info = dirty.track_rgbd(depth, rgb, *sc.wall_starts()[0], K=sc.WALL_K)
    _same_records(info, trc.track(depth, rgb, *sc.wall_starts()[0], sc.WALL_K, sc.VS, grid, **sc.GATES)[2], "the wall with colours that are not finite")
    assert info["status"] == 0 and np.isfinite(info["lambda"])


def test_tracks_on_the_wall_equal_the_restatement(hip_lib):
    """Every record -- the poses as uint64, xi, the 66 integers -- and lambda equal the restatement's bit for bit from the three starting guesses; the final
    pose lies within WALL_BOUND_M / WALL_BOUND_DEG; depth only (track_depth, and colour_weight = 0) is singular at once."""
    g = _wall()
    depth, rgb = sc.wall_frame()
    dd, dc = _dev(depth, rgb)
    for n, ((Rp, Tp), (Rw, Tw, want)) in enumerate(zip(sc.wall_starts(), sc.wall_tracks())):
        R, T, info = g.track_rgbd(depth, rgb, Rp, Tp, K=sc.WALL_K)
        _same_records(info, want, f"start {n}")
        assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
        em, ed = ts.pose_error(R, T, sc.WALL_R, sc.WALL_T)
        print(f"start {n}: status {info['status']}, {info['iterations']} linearisations, lambda {info['lambda']:.4f}, final error {em:.6f} m {ed:.6f} deg")
        assert info["status"] == 0 and em <= sc.WALL_BOUND_M and ed <= sc.WALL_BOUND_DEG
        Rd, Td, idv = g.track_rgbd(dd, dc, Rp, Tp, K=sc.WALL_K)              # device images
        _same_records(idv, want, f"start {n}, device images")
        assert np.array_equal(_bits(Rd), _bits(Rw)) and np.array_equal(_bits(Td), _bits(Tw))
        R0, T0, i0 = g.track_rgbd(depth, rgb, Rp, Tp, K=sc.WALL_K, colour_weight=0.0)
        Rg, Tg, ig = g.track_depth(depth, Rp, Tp, K=sc.WALL_K)
        assert i0["status"] == ig["status"] == 3 and i0["iterations"] == ig["iterations"] == 1 and i0["lambda"] == 0.0
        assert np.array_equal(_bits(R0), _bits(Rp)) and np.array_equal(_bits(T0), _bits(Tp)) and np.array_equal(_bits(Rg), _bits(Rp))
    # a fixed weight, a balance, other levels, damping and robust weights, exhausted iterations: status 1
    Rp, Tp = sc.wall_starts()[1]
    kw = dict(levels=((4, 2), (3, 1)), min_step=1e-9, damping=1e-3, huber=0.02, huber_c=0.05)
    for extra in (dict(colour_weight=0.7), dict(balance=2.5)):
        R, T, info = g.track_rgbd(depth, rgb, Rp, Tp, K=sc.WALL_K, **kw, **extra)
        Rw, Tw, want = trc.track(depth, rgb, Rp, Tp, sc.WALL_K, sc.VS, sc.wall_grid_shared(), **kw, **extra, **sc.GATES)
        _same_records(info, want, str(extra))
        assert info["status"] == 1 and info["iterations"] == 3 and np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
    assert info["lambda"] == trc.auto_lambda(want["records"][0]["sums"], 2.5)
    # lost: the camera looks away; the geometric count decides, lambda is 0 (no texture in view)
    Ra, Ta = sc.wall_away()
    R, T, info = g.track_rgbd(depth, rgb, Ra, Ta, K=sc.WALL_K)
    assert info["status"] == 2 and info["iterations"] == 1 and info["lambda"] == 0.0 and info["records"][0]["geo"]["n_used"] == 0
    assert np.array_equal(_bits(R), _bits(Ra)) and np.array_equal(_bits(T), _bits(Ta))
    with pytest.raises(ValueError, match="colour_weight"):
        g.track_rgbd(depth, rgb, Rp, Tp, colour_weight=-0.5)


def test_tracks_in_the_room_equal_the_restatement(hip_lib):
    """The three perturbations of track_scenes over the textured room: every record and lambda bit for bit, the final pose within ROOM_BOUND_*; with
    colour_weight = 0 the track equals track_depth's: the poses, the steps and the geometric sums of every record."""
    g, _ = _room()
    Rt, Tt, depth, rgb = sc.room_tracked()
    K = ts.intrinsics()
    for n, ((Rp, Tp), (Rw, Tw, want)) in enumerate(zip(ts.perturbed_poses(), sc.room_tracks())):
        R, T, info = g.track_rgbd(depth, rgb, Rp, Tp, K=K)
        _same_records(info, want, f"perturbation {n}")
        assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
        em, ed = ts.pose_error(R, T, Rt, Tt)
        print(f"perturbation {n}: status {info['status']}, {info['iterations']} linearisations, lambda {info['lambda']:.4f}, final error {em:.6f} m {ed:.5f} deg")
        assert info["status"] == 0 and em <= sc.ROOM_BOUND_M and ed <= sc.ROOM_BOUND_DEG
    Rp, Tp = ts.perturbed_poses()[0]
    R0, T0, i0 = g.track_rgbd(depth, rgb, Rp, Tp, K=K, colour_weight=0.0)
    Rg, Tg, ig = g.track_depth(depth, Rp, Tp, K=K)
    assert np.array_equal(_bits(R0), _bits(Rg)) and np.array_equal(_bits(T0), _bits(Tg)) and i0["status"] == ig["status"] == 0 and i0["iterations"] == ig["iterations"]
    for a, b in zip(i0["records"], ig["records"]):
        assert np.array_equal(a["geo"]["sums"], b["sums"]) and all(np.array_equal(_bits(a[f]), _bits(b[f])) for f in ("R", "T", "xi"))


def test_refusals(hip_lib):
    import torch
    from taichislam_amd import _lib
    from taichislam_amd.mapping import DenseTSDF
    g = _wall()
    plain = DenseTSDF(**dict(sc.TEXTURED, texture_enabled=False))
    plain.set_dep_camera_intrinsic(sc.WALL_K)
    depth, rgb = sc.wall_frame()
    h, w = depth.shape
    dd, dc = _dev(depth, rgb)
    dev_sums = torch.zeros(80, dtype=torch.int64, device="cuda")
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    Ro, To = np.zeros(9), np.zeros(3)
    NULL = object()

    def call(entry, R=sc.WALL_R, T=sc.WALL_T, K=sc.WALL_K, h=h, w=w, stride=1, d_min=0.0, d_max=0.0, r_max=0.0, g_max=0.0, huber=0.0, rc_max=0.0, gc_max=0.0,
             huber_c=0.0, lam=-1.0, balance=1.0, image=None, colour=None, out=None, cfg=True, levels=((2, 1),), min_step=1e-4, damping=0.0, handle=g):
        c = _lib.AlignRgbdCfg()
        c.a.K[:] = list(np.asarray(K, np.float64).reshape(-1))
        c.a.h, c.a.w, c.a.stride, c.a.d_min, c.a.d_max, c.a.r_max, c.a.g_max, c.a.huber = h, w, stride, d_min, d_max, r_max, g_max, huber
        c.rc_max, c.gc_max, c.huber_c = rc_max, gc_max, huber_c
        t = _lib.TrackCfg()
        t.n_levels = len(levels)
        for i, (st, it) in enumerate(levels[:4]):
            t.stride[i], t.iters[i] = st, it
        t.min_step, t.damping = min_step, damping
        hd = None if handle is None else handle.h
        cp = C.byref(c) if cfg else None
        Rp, Tp = (None if R is NULL else dp(R)), (None if T is NULL else dp(T))
        dev = entry.endswith("_dev")
        ip = None if image is NULL else (C.c_void_p(dd.data_ptr()) if dev else depth.ctypes.data_as(C.c_void_p))
        kp = None if colour is NULL else (C.c_void_p(dc.data_ptr()) if dev else rgb.ctypes.data_as(C.c_void_p))
        sums = _lib.AlignRgbdSums()
        L = g.L
        if entry == "align_rgbd_linearize":
            return L.tsl_tsdf_align_rgbd_linearize(hd, Rp, Tp, cp, ip, kp, None if out is NULL else C.byref(sums))
        if entry == "align_rgbd_linearize_dev":
            return L.tsl_tsdf_align_rgbd_linearize_dev(hd, Rp, Tp, cp, ip, kp, None if out is NULL else C.c_void_p(dev_sums.data_ptr()), None)
        if entry == "track_rgbd":
            return L.tsl_tsdf_track_rgbd(hd, Rp, Tp, cp, C.byref(t), lam, balance, ip, kp, None if out is NULL else dp(Ro), dp(To), None)
        return L.tsl_tsdf_track_rgbd_dev(hd, Rp, Tp, cp, C.byref(t), lam, balance, ip, kp, None if out is NULL else dp(Ro), dp(To), None, None)

    Rn = np.array(sc.WALL_R, np.float64); Rn[1, 1] = np.nan
    nan, inf = float("nan"), float("inf")
    for entry in ("align_rgbd_linearize", "align_rgbd_linearize_dev", "track_rgbd", "track_rgbd_dev"):
        def refused(**kw):
            rc = call(entry, **kw)
            return rc == -1 and entry.encode() in g.L.tsl_last_error()
        assert call(entry) == 0, g.L.tsl_last_error()
        assert call(entry, K=np.zeros(9)) == 0                         # all zero: the map's depth intrinsics
        # everything align_linearize refuses
        assert refused(handle=None) and refused(R=NULL) and refused(T=NULL) and refused(cfg=False) and refused(image=NULL) and refused(out=NULL)
        assert refused(R=Rn) and refused(T=[0.0, np.inf, 0.0])
        assert refused(K=np.where(np.arange(9) == 4, np.nan, sc.WALL_K)) and refused(K=np.where(np.arange(9) == 2, -np.inf, sc.WALL_K))
        assert refused(d_min=nan) and refused(d_max=inf) and refused(r_max=nan) and refused(g_max=inf) and refused(huber=nan)
        assert refused(h=0) and refused(w=-3) and refused(h=32769)
        assert refused(d_min=2.0, d_max=2.0) and refused(d_min=2.0, d_max=1.0) and refused(d_min=6.0)
        assert refused(r_max=-0.1) and refused(g_max=-1.0) and refused(huber=-0.02)
        assert refused(g_max=1e6) and refused(r_max=1e7)               # the geometric overflow bound
        # a null rgb, an untextured map, the colour gates
        assert refused(colour=NULL)
        assert refused(handle=plain) and b"not textured" in g.L.tsl_last_error()
        assert refused(rc_max=nan) and refused(gc_max=inf) and refused(huber_c=nan) and refused(rc_max=-0.1) and refused(gc_max=-1.0) and refused(huber_c=-0.02)
        # the colour overflow bound: L = 5.12 m, 3072 visited pixels; gc_max = 1e4 gives Mc^2 2^20 visited = 1.05e10 * 1.05e6 * 3072 > 2^62 = 4.6e18
        assert refused(gc_max=1e4) and b"colour sums" in g.L.tsl_last_error() and refused(rc_max=1e7) and call(entry, gc_max=1e3) == 0
        if entry.startswith("align"):
            assert refused(stride=0) and refused(stride=-2)
            assert refused(gc_max=4e3, stride=1) and call(entry, gc_max=4e3, stride=2) == 0      # Mc = 40960: 1.68e9 * 2^20 * 3072 > 2^62 > 1.68e9 * 2^20 * 768
        else:
            assert refused(levels=((0, 1),)) and refused(levels=((2, 1),) * 5) and refused(levels=()) and refused(levels=((2, 33), (1, 32))) and refused(levels=((2, 65),))
            assert refused(min_step=nan) and refused(damping=-1.0)
            assert refused(lam=nan) and refused(lam=inf) and refused(balance=nan) and refused(balance=-1.0) and refused(balance=inf)
            assert call(entry, lam=0.0) == 0 and call(entry, lam=0.3, balance=0.0) == 0
            assert refused(gc_max=4e3, levels=((2, 1), (1, 1))) and call(entry, gc_max=4e3, levels=((2, 1),)) == 0      # the bound is checked for every level first
    torch.cuda.synchronize()
    with pytest.raises(_lib.TslError, match="align_rgbd_linearize"):
        plain.align_rgbd_linearize(depth, rgb, sc.WALL_R, sc.WALL_T)
    with pytest.raises(_lib.TslError, match="track_rgbd"):
        g.track_rgbd(depth, rgb, sc.WALL_R, sc.WALL_T, balance=-1.0)
    with pytest.raises(_lib.TslError, match="track_rgbd"):
        g.track_rgbd(depth, rgb, sc.WALL_R, sc.WALL_T, colour_weight=float("nan"))

"""Scan-to-model alignment on the GPU (tsl_align_points.hip): the 33 integers and the per-point bucket and signed distance of a linearisation, and every
record of a tracking run, against the numpy restatement (tests/track_points_ref.py) over the oracle's map of the box room
(tests/track_points_scenes.py); the image kernel on the cloud an image back-projects to; bad points; the device form with frames in flight; an empty
cloud, lost and singular runs, a global map, the refusals."""
import ctypes as C

import numpy as np
import pytest

import render_view_ref as rv
import track_points_ref as tpr
import track_points_scenes as tps
import track_ref as tr
import track_scenes as ts
from util import SMALL, assert_export_equal, make_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000, None)       # prefixes of the scan; None = all of it
STRIDES = (1, 3, 7, 8, None)                               # None = n + 1, larger than the cloud
_CHECKED = []


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _room(n=ts.N_FRAMES):
    """(HIP map after the first n of the six frames, the restatement's grid of the oracle's map after all six), as tests/test_track_gpu.py builds them"""
    from oracle import BATCHED
    g, o = make_pair(SMALL, ts.intrinsics())
    frames = ts.map_frames()
    for R, T, d in frames[:n]:
        g.recast_depth_to_map(R, T, d, None)
    if not _CHECKED:
        for R, T, d in frames:
            o.integrate_depth(R, T, d, mode=BATCHED)
        assert_export_equal(o.export_sparse(), ts.oracle_map().export_sparse(), "the pair's oracle against the shared one")
        _CHECKED.append(True)
    return g, ts.oracle_grid()


def _same(got, want, what):
    """the dict of align_points_linearize(per_point=True) against the restatement's (sums, bucket, s)"""
    sums, bucket, s = want
    bad = np.nonzero(got["sums"] != sums)[0]
    assert bad.size == 0, f"{what}: sums {bad.tolist()} differ: {got['sums'][bad]} / {sums[bad]}"
    assert got["bucket"].dtype == np.uint8 and got["s"].dtype == F32 and got["bucket"].shape == bucket.shape and got["s"].shape == s.shape, what
    bad = np.nonzero(got["bucket"] != bucket)[0]
    assert bad.size == 0, f"{what}: bucket differs at {bad[:8].tolist()}: {got['bucket'][bad[:8]]} / {bucket[bad[:8]]}"
    bad = np.nonzero(_bits32(got["s"]) != _bits32(s))[0]
    assert bad.size == 0, f"{what}: s differs at {bad[:8].tolist()}: {got['s'][bad[:8]]} / {s[bad[:8]]}"


def _same_records(got, want, what):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"] == len(got["records"]), \
        f"{what}: status {got['status']} / {want['status']}, iterations {got['iterations']} / {want['iterations']}"
    for k, (a, b) in enumerate(zip(got["records"], want["records"])):
        assert np.array_equal(a["sums"], b["sums"]), f"{what}, record {k}: sums differ at {np.nonzero(a['sums'] != b['sums'])[0].tolist()}"
        for f in ("R", "T", "xi"):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), f"{what}, record {k}: {f} differs: {a[f]} / {b[f]}"


def test_linearize_equals_the_restatement(hip_lib):
    """All 33 integers, bucket and s (as bit patterns): prefixes of the scan of 1, 63, 64, 65, 255, 256, 257, 1000 and all 5760 points; strides 1, 3, 7,
    8 and n + 1; the true pose, a perturbed pose and the pose that looks away; huber off and 0.02; counts only; without the per-point outputs;
    explicit gates."""
    g, grid = _room()
    Rt, Tt, _ = ts.tracked_frame()
    scan = tps.scan()
    poses = [("true", Rt, Tt), ("perturbed",) + ts.perturbed_poses()[2], ("away",) + ts.away_pose()]
    seen = np.zeros(5, np.int64)
    for n in COUNTS:
        cloud = scan if n is None else scan[:n]
        for st in STRIDES:
            stride = cloud.shape[0] + 1 if st is None else st
            for name, R, T in poses:
                for huber in (0.0, 0.02):
                    what = f"n {cloud.shape[0]}, stride {stride}, {name}, huber {huber}"
                    want = tpr.linearize_points(cloud, R, T, stride, tps.VS, grid, huber=huber, **tps.GATES)
                    got = g.align_points_linearize(cloud, R, T, stride=stride, huber=huber, per_point=True)
                    _same(got, want, what)
                    assert got["sums"][tr.I_USED:].sum() == tpr.visited(cloud.shape[0], stride) == got["bucket"].size
                    seen += want[0][tr.I_USED:] > 0
    # explicit gates: a narrow range and a short band move points between the buckets as the restatement says
    gates = dict(d_min=1.5, d_max=2.5, r_max=0.05, g_max=1.5)
    Rp, Tp = ts.perturbed_poses()[1]
    for stride in (1, 3):
        want = tpr.linearize_points(scan, Rp, Tp, stride, tps.VS, grid, **gates)
        got = g.align_points_linearize(scan, Rp, Tp, stride=stride, per_point=True, **gates)
        _same(got, want, f"explicit gates, stride {stride}")
        seen += want[0][tr.I_USED:] > 0
        assert got["n_gate"] > 500 // stride
    assert (seen > 0).all(), f"buckets used / gate / unknown / far / grad occurred in {seen.tolist()} cases"
    # the dict is that of align_linearize; without per_point there are no per-point keys and the kernel without the stores gives the same integers
    want = tpr.linearize_points(scan, Rp, Tp, 1, tps.VS, grid, **tps.GATES)[0]
    got = g.align_points_linearize(scan, Rp, Tp)
    assert "bucket" not in got and "s" not in got and np.array_equal(got["sums"], want) and np.array_equal(got["H"], got["H"].T)
    assert np.array_equal(got["H"][np.triu_indices(6)], want[:21]) and np.array_equal(got["b"], want[21:27]) and got["e"] == want[27]
    assert [got[k] for k in ("n_used", "n_gate", "n_unknown", "n_far", "n_grad")] == want[tr.I_USED:].tolist() and got["n_used"] > 1000 and got["n_far"] > 0
    for stride in (3, 8):
        assert np.array_equal(g.align_points_linearize(scan, Rp, Tp, stride=stride, huber=0.02)["sums"],
                              tpr.linearize_points(scan, Rp, Tp, stride, tps.VS, grid, huber=0.02, **tps.GATES)[0])
    # counts only: the same buckets and per-point results, no sums
    for per in (False, True):
        co = g.align_points_linearize(scan, Rp, Tp, counts_only=True, per_point=per)
        assert np.array_equal(co["sums"][tr.I_USED:], want[tr.I_USED:]) and not co["sums"][:tr.I_USED].any()
    _same(dict(co, sums=want), tpr.linearize_points(scan, Rp, Tp, 1, tps.VS, grid, **tps.GATES), "counts only, per point")


def test_agrees_with_the_image_kernel(hip_lib):
    """the depth image back-projected with the image kernel's own f32 expressions, under a range gate that gates nothing: the point kernel gives the
    image kernel's H, b, e and counts at stride 1; only n_gate differs (the cloud holds the pixels that passed the image's gate)"""
    g, _ = _room()
    Rt, Tt, depth = ts.tracked_frame()
    cloud = tps.depth_cloud()
    keep = [i for i in range(tr.N_SUMS) if i != tr.I_GATE]
    for R, T in ((Rt, Tt), ts.perturbed_poses()[1]):
        img = g.align_linearize(depth, R, T, K=ts.intrinsics(), stride=1)
        pts = g.align_points_linearize(cloud, R, T, **tps.WIDE)
        assert pts["n_gate"] == 0 and cloud.shape[0] + img["n_gate"] == ts.H * ts.W
        assert np.array_equal(pts["sums"][keep], img["sums"][keep]) and pts["n_used"] > 70000
        for k in ("H", "b"):
            assert np.array_equal(pts[k], img[k])
        assert [pts[k] for k in ("e", "n_used", "n_unknown", "n_far", "n_grad")] == [img[k] for k in ("e", "n_used", "n_unknown", "n_far", "n_grad")]


def test_bad_points(hip_lib):
    """NaN, +-inf, 1e30 (l2 overflows), the origin, a point beyond d_max and a finite point outside the volume at lane 0, 63 and 64, at a workgroup's last
    lane and as the last point: each lands in the bucket the definition gives, adds nothing to the sums and leaves s = +0.0"""
    g, grid = _room()
    Rp, Tp = ts.perturbed_poses()[0]
    gates = dict(tps.GATES, d_max=100.0)                      # 50 m passes the range gate and leaves the 10.24 m volume
    bad = [((np.nan, 0.5, 1.0), tpr.GATE), ((0.5, np.inf, 1.0), tpr.GATE), ((0.5, 0.5, -np.inf), tpr.GATE), ((1e30, 0.0, 0.0), tpr.GATE),
           ((0.0, 0.0, 0.0), tpr.GATE), ((0.0, 0.0, 200.0), tpr.GATE), ((0.0, 0.0, 50.0), tpr.UNKNOWN)]
    base = np.array(tps.scan()[:600])
    where = (0, 63, 64, 255, 599)
    clean = tpr.linearize_points(base, Rp, Tp, 1, tps.VS, grid, **gates)
    assert clean[0][tr.I_USED] > 100
    for xyz, code in bad:
        cloud = base.copy()
        cloud[list(where)] = np.array(xyz, F32)
        got = g.align_points_linearize(cloud, Rp, Tp, per_point=True, **gates)
        _same(got, tpr.linearize_points(cloud, Rp, Tp, 1, tps.VS, grid, **gates), f"bad point {xyz}")
        assert (got["bucket"][list(where)] == code).all() and not _bits32(got["s"][list(where)]).any(), (xyz, got["bucket"][list(where)], got["s"][list(where)])
        # nothing but the five points changed: the sums are those of the clean cloud without what its five points added
        rest = np.delete(base, where, 0)
        r = tpr.linearize_points(rest, Rp, Tp, 1, tps.VS, grid, **gates)[0]
        assert np.array_equal(got["sums"][:tr.I_USED], r[:tr.I_USED])
        assert got["sums"][tr.I_USED + code] == r[tr.I_USED + code] + 5
    # every kind at once, at stride 3: the bad points sit where the stride visits them and where it does not
    cloud = base.copy()
    for k, (xyz, _) in enumerate(bad):
        cloud[[3 * k, 3 * k + 100, 192 + k, 599 - k]] = np.array(xyz, F32)
    for stride in (1, 3):
        _same(g.align_points_linearize(cloud, Rp, Tp, stride=stride, huber=0.02, per_point=True, **gates),
              tpr.linearize_points(cloud, Rp, Tp, stride, tps.VS, grid, huber=0.02, **gates), f"all bad kinds, stride {stride}")


def test_track_equals_the_restatement(hip_lib):
    """From 3 cm / 1.5 deg, 6 cm / 3 deg and 10 cm / 5 deg with the default levels: every record (pose, sums, step), the status and the count equal the
    restatement's bit for bit; the final pose lies within track_points_scenes.TRACK_POINTS_BOUND_M / _DEG of the true one."""
    g, _ = _room()
    Rt, Tt, _ = ts.tracked_frame()
    scan = tps.scan()
    for n, ((Rp, Tp), (Rw, Tw, want)) in enumerate(zip(ts.perturbed_poses(), tps.reference_tracks())):
        R, T, info = g.track_points(scan, Rp, Tp)
        _same_records(info, want, f"perturbation {n}")
        assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
        em, ed = ts.pose_error(R, T, Rt, Tt)
        print(f"perturbation {n}: status {info['status']}, {info['iterations']} linearisations, final error {em:.6f} m {ed:.5f} deg")
        assert info["status"] == 0 and em <= tps.TRACK_POINTS_BOUND_M and ed <= tps.TRACK_POINTS_BOUND_DEG
    # other levels, damping and a robust weight, exhausted iterations: status 1
    Rp, Tp = ts.perturbed_poses()[0]
    kw = dict(levels=((7, 2), (3, 1)), min_step=1e-9, damping=1e-3)
    R, T, info = g.track_points(scan, Rp, Tp, huber=0.02, **kw)
    Rw, Tw, want = tpr.track_points(scan, Rp, Tp, tps.VS, ts.oracle_grid(), huber=0.02, **kw, **tps.GATES)
    _same_records(info, want, "two levels, damped")
    assert info["status"] == 1 and info["iterations"] == 3 and np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))


def test_device_form_with_work_in_flight(hip_lib):
    import torch
    g, _ = _room(4)
    g.sync()
    scan = tps.scan()
    Rp, Tp = ts.perturbed_poses()[0]
    stride = 3
    v = tpr.visited(scan.shape[0], stride)
    dev_scan = torch.from_numpy(np.array(scan)).cuda()
    before = g.align_points_linearize(scan, Rp, Tp, stride=stride)
    # the outputs with sentinel bytes behind them, filled through the C entry point
    sums_d = torch.full((48,), -7, dtype=torch.int64, device="cuda")
    bucket_d = torch.full((v + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    s_d = torch.full((v + 16,), -3.25, dtype=torch.float32, device="cuda")
    from taichislam_amd import _lib
    from taichislam_amd.mapping.dense_tsdf import align_points_config
    cfg = align_points_config(stride=stride)
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    torch.cuda.synchronize()                                         # the sentinels are in place
    side = torch.cuda.Stream()
    for R, T, d in ts.map_frames()[4:]:                              # queued frames, then the linearisation: no sync in between
        g.recast_depth_to_map(R, T, d, None)
    with torch.cuda.stream(side):
        filler = torch.ones(1 << 22, device="cuda").mul_(3.0)       # other work in flight on the stream
        dev = g.align_points_linearize(dev_scan, Rp, Tp, stride=stride, device=True)
        total = dev[28:33].sum()
        assert g.L.tsl_tsdf_align_points_linearize_dev(g.h, dp(Rp), dp(Tp), C.byref(cfg), C.c_void_p(dev_scan.data_ptr()), scan.shape[0], C.c_void_p(sums_d.data_ptr()),
                                                        C.c_void_p(bucket_d.data_ptr()), C.c_void_p(s_d.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
        devs, devb, devf = g.align_points_linearize(dev_scan, Rp, Tp, stride=stride, device=True, per_point=True)
    side.synchronize()
    assert dev.is_cuda and dev.dtype == torch.int64 and dev.shape == (40,) and float(filler[-1]) == 3.0
    got = dev.cpu().numpy()
    g.sync()
    want = g.align_points_linearize(scan, Rp, Tp, stride=stride, per_point=True)
    assert np.array_equal(got[:33], want["sums"]) and not got[33:].any() and int(total) == v
    assert (before["sums"] != want["sums"]).sum() > 20                # the queued frames were integrated before the linearisation ran
    sums_h, bucket_h, s_h = sums_d.cpu().numpy(), bucket_d.cpu().numpy(), s_d.cpu().numpy()
    assert np.array_equal(sums_h[:33], want["sums"]) and not sums_h[33:40].any() and (sums_h[40:] == -7).all()
    assert np.array_equal(bucket_h[:v], want["bucket"]) and (bucket_h[v:] == 0xA5).all()
    assert np.array_equal(_bits32(s_h[:v]), _bits32(want["s"])) and (s_h[v:] == F32(-3.25)).all()
    assert devb.dtype == torch.uint8 and devf.dtype == torch.float32 and devb.shape == devf.shape == (v,)
    assert np.array_equal(devs.cpu().numpy(), got) and np.array_equal(devb.cpu().numpy(), want["bucket"]) and np.array_equal(_bits32(devf.cpu().numpy()), _bits32(want["s"]))
    # the host form takes a device cloud too; tracking from a device cloud equals tracking from the host cloud
    assert np.array_equal(g.align_points_linearize(dev_scan, Rp, Tp, stride=stride)["sums"], want["sums"])
    Rh, Th, ih = g.track_points(scan, Rp, Tp)
    with torch.cuda.stream(side):
        Rd, Td, idv = g.track_points(dev_scan, Rp, Tp)
    _same_records(idv, ih, "device cloud")
    assert np.array_equal(_bits(Rd), _bits(Rh)) and np.array_equal(_bits(Td), _bits(Th)) and ih["status"] == 0


def test_empty_lost_and_singular(hip_lib):
    import torch
    g, grid = _room()
    Rt, Tt, _ = ts.tracked_frame()
    scan = tps.scan()
    # n = 0: zero sums, nothing launched, the tracker is lost at once and returns the guess
    empty = np.zeros((0, 3), F32)
    got = g.align_points_linearize(empty, Rt, Tt, per_point=True)
    assert not got["sums"].any() and got["bucket"].shape == (0,) and got["s"].shape == (0,)
    dev = g.align_points_linearize(torch.zeros((0, 3), device="cuda"), Rt, Tt, device=True)
    assert not dev.cpu().numpy().any()
    for cloud in (empty, torch.zeros((0, 3), device="cuda")):
        R, T, info = g.track_points(cloud, Rt, Tt)
        assert info["status"] == 2 and info["iterations"] == 1 and not info["records"][0]["sums"].any()
        assert np.array_equal(_bits(R), _bits(Rt)) and np.array_equal(_bits(T), _bits(Tt))
    # lost: looking away, every point of the depth image's cloud lies in space nobody observed (the spherical scan looks back over its shoulder)
    Ra, Ta = ts.away_pose()
    s = g.align_points_linearize(tps.depth_cloud(), Ra, Ta, stride=5)
    assert s["n_unknown"] == tpr.visited(tps.depth_cloud().shape[0], 5) and s["n_used"] == 0
    R, T, info = g.track_points(tps.depth_cloud(), Ra, Ta, min_used=100)
    assert info["status"] == 2 and info["iterations"] == 1 and info["records"][0]["n_used"] == 0 and not info["records"][0]["xi"].any()
    assert np.array_equal(_bits(R), _bits(Ra)) and np.array_equal(_bits(T), _bits(Ta))
    # singular: points of one wall only (track_points_scenes.singular_cloud), the guess comes back, as in the restatement
    wall = tps.singular_cloud()
    R, T, info = g.track_points(wall, Rt, Tt, levels=((1, 3),), min_used=1)
    _, _, want = tpr.track_points(wall, Rt, Tt, tps.VS, grid, levels=((1, 3),), min_used=1, **tps.GATES)
    _same_records(info, want, "one wall")
    assert info["status"] == 3 and info["records"][0]["n_used"] == wall.shape[0] and np.array_equal(_bits(R), _bits(Rt)) and np.array_equal(_bits(T), _bits(Tt))
    # the whole wall: ill-conditioned, and still what the restatement does
    R, T, info = g.track_points(tps.wall_scan(), Rt, Tt, levels=((1, 2),))
    Rw, Tw, want = tpr.track_points(tps.wall_scan(), Rt, Tt, tps.VS, grid, levels=((1, 2),), **tps.GATES)
    _same_records(info, want, "the whole wall")
    assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
    # lost on the way: the second level has too few points for min_used, the pose of the last step's linearisation comes back
    Rp, Tp = ts.perturbed_poses()[0]
    R, T, info = g.track_points(scan, Rp, Tp, levels=((2, 2), (64, 2)), min_step=0.0, min_used=100)
    _, _, want = tpr.track_points(scan, Rp, Tp, tps.VS, grid, levels=((2, 2), (64, 2)), min_step=0.0, min_used=100, **tps.GATES)
    _same_records(info, want, "lost at the second level")
    assert info["status"] == 2 and info["iterations"] == 3 and np.array_equal(_bits(R), _bits(info["records"][1]["R"])) and np.array_equal(_bits(T), _bits(info["records"][1]["T"]))
    # after reset() nothing is known
    g.reset()
    s = g.align_points_linearize(scan, Rt, Tt, stride=3, per_point=True)
    assert s["n_unknown"] == tpr.visited(scan.shape[0], 3) and not s["sums"][:tr.I_USED].any() and (s["bucket"] == tpr.UNKNOWN).all() and not _bits32(s["s"]).any()


def test_global_map_linearises_submap_0(hip_lib):
    from taichislam_amd.mapping import DenseTSDF
    G = DenseTSDF(**dict(SMALL, is_global_map=True))
    G.set_dep_camera_intrinsic(ts.intrinsics())
    for R, T, d in ts.map_frames():
        G.recast_depth_to_map(R, T, d, None)
    e = G.export_submap()
    grid = rv.grid_from_export(e["indices"], e["TSDF"], G.N, G.Nz)
    Rt, Tt, _ = ts.tracked_frame()
    for R, T in ((Rt, Tt), ts.perturbed_poses()[1]):
        got = G.align_points_linearize(tps.scan(), R, T, stride=3, huber=0.02, per_point=True)
        _same(got, tpr.linearize_points(tps.scan(), R, T, 3, tps.VS, grid, huber=0.02, **tps.GATES), "global map")
        assert got["n_used"] > 300


def test_refusals(hip_lib):
    import torch
    from taichislam_amd import _lib
    g, _ = _room(2)
    Rt, Tt, _ = ts.tracked_frame()
    scan = np.array(tps.scan())
    n_all = scan.shape[0]
    dev_scan = torch.from_numpy(scan).cuda()
    dev_sums = torch.full((40,), -7, dtype=torch.int64, device="cuda")
    dev_bucket = torch.full((n_all,), 0xA5, dtype=torch.uint8, device="cuda")
    dev_s = torch.full((n_all,), -3.25, dtype=torch.float32, device="cuda")
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    Ro, To = np.full(9, 7.0), np.full(3, 7.0)
    sums = _lib.AlignSums()
    bucket, sd = np.full(n_all, 0xA5, np.uint8), np.full(n_all, -3.25, F32)
    rep = _lib.TrackReport()
    rep.status, rep.iterations = -5, -5
    NULL = object()

    def reset():
        C.memset(C.byref(sums), 0x5A, C.sizeof(sums))

    def unwritten():
        torch.cuda.synchronize()
        return (bytes(sums) == b"\x5a" * C.sizeof(sums) and (bucket == 0xA5).all() and (sd == F32(-3.25)).all() and (Ro == 7.0).all() and (To == 7.0).all()
                and rep.status == -5 and rep.iterations == -5 and bool((dev_sums == -7).all()) and bool((dev_bucket == 0xA5).all()) and bool((dev_s == -3.25).all()))

    def call(entry, R=Rt, T=Tt, n=n_all, stride=1, d_min=0.0, d_max=0.0, r_max=0.0, g_max=0.0, huber=0.0, cloud=None, out=None, cfg=True, levels=((8, 1),),
             min_step=1e-4, damping=0.0, handle=True, write=False):
        c = _lib.AlignPointsCfg()
        c.stride, c.d_min, c.d_max, c.r_max, c.g_max, c.huber = stride, d_min, d_max, r_max, g_max, huber
        t = _lib.TrackCfg()
        t.n_levels = len(levels)
        for i, (st, it) in enumerate(levels[:4]):
            t.stride[i], t.iters[i] = st, it
        t.min_step, t.damping = min_step, damping
        hd = g.h if handle else None
        cp = C.byref(c) if cfg else None
        Rp, Tp = (None if R is NULL else dp(R)), (None if T is NULL else dp(T))
        host = None if cloud is NULL else scan.ctypes.data_as(C.c_void_p)
        devp = None if cloud is NULL else C.c_void_p(dev_scan.data_ptr())
        # an accepted call writes into scratch outputs, so that the sentinels keep standing for the refusals
        if write:
            s2, b2, f2, R2, T2 = _lib.AlignSums(), np.zeros(n_all, np.uint8), np.zeros(n_all, F32), np.zeros(9), np.zeros(3)
            d2 = (torch.zeros(40, dtype=torch.int64, device="cuda"), torch.zeros(n_all, dtype=torch.uint8, device="cuda"), torch.zeros(n_all, device="cuda"))
            outs = (C.byref(s2), b2.ctypes.data_as(C.c_void_p), f2.ctypes.data_as(C.c_void_p), dp(R2), dp(T2), None) + tuple(C.c_void_p(x.data_ptr()) for x in d2)
        else:
            outs = (C.byref(sums), bucket.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p), Ro.ctypes.data_as(_lib.dp), To.ctypes.data_as(_lib.dp), C.byref(rep),
                    C.c_void_p(dev_sums.data_ptr()), C.c_void_p(dev_bucket.data_ptr()), C.c_void_p(dev_s.data_ptr()))
        o_sums, o_b, o_s, o_R, o_T, o_rep, o_dsums, o_db, o_ds = outs
        if entry == "align_points_linearize":
            rc = g.L.tsl_tsdf_align_points_linearize(hd, Rp, Tp, cp, host, n, None if out is NULL else o_sums, o_b, o_s)
        elif entry == "align_points_linearize_dev":
            rc = g.L.tsl_tsdf_align_points_linearize_dev(hd, Rp, Tp, cp, devp, n, None if out is NULL else o_dsums, o_db, o_ds, None)
        elif entry == "track_points":
            rc = g.L.tsl_tsdf_track_points(hd, Rp, Tp, cp, C.byref(t), host, n, None if out is NULL else o_R, o_T, o_rep)
        else:
            rc = g.L.tsl_tsdf_track_points_dev(hd, Rp, Tp, cp, C.byref(t), devp, n, None if out is NULL else o_R, o_T, o_rep, None)
        torch.cuda.synchronize()
        return rc

    Rn = np.array(Rt, np.float64); Rn[1, 1] = np.nan
    reset()
    for entry in ("align_points_linearize", "align_points_linearize_dev", "track_points", "track_points_dev"):
        def refused(**kw):
            rc = call(entry, **kw)
            return rc == -1 and entry.encode() + b":" in g.L.tsl_last_error() and unwritten()
        assert call(entry, write=True) == 0, g.L.tsl_last_error()
        assert call(entry, n=0, cloud=NULL, write=True) == 0, g.L.tsl_last_error()             # an empty cloud needs no pointer
        assert refused(handle=False) and refused(R=NULL) and refused(T=NULL) and refused(cfg=False) and refused(cloud=NULL) and refused(out=NULL)
        assert refused(R=Rn) and refused(T=[0.0, np.inf, 0.0])
        assert refused(d_min=float("nan")) and refused(d_max=float("inf")) and refused(r_max=float("nan")) and refused(g_max=float("inf")) and refused(huber=float("nan"))
        assert refused(n=-1) and refused(n=(1 << 30) + 1)
        assert refused(d_min=2.0, d_max=2.0) and refused(d_min=2.0, d_max=1.0) and refused(d_min=6.0)          # 6 > the default d_max = 5
        assert refused(d_min=-0.5) and refused(r_max=-0.1) and refused(g_max=-1.0) and refused(huber=-0.02)
        # the overflow bound: L = 5.12 m; with g_max = 1e6 M^2 2^20 visited = 1.05e14 * 1.05e6 * 5760 > 2^62 = 4.6e18
        assert refused(g_max=1e6) and refused(r_max=1e7)
        if entry.startswith("align"):
            assert refused(stride=0) and refused(stride=-2)
            # g_max = 4000: M^2 2^20 = 1.76e15; times 5760 points it exceeds 2^62, times 1920 it does not
            assert refused(g_max=4e3, stride=1) and call(entry, g_max=4e3, stride=3, write=True) == 0
        else:
            assert refused(levels=((0, 1),)) and refused(levels=((2, 1),) * 5) and refused(levels=()) and refused(levels=((2, 33), (1, 32))) and refused(levels=((2, 65),))
            assert refused(min_step=float("nan")) and refused(damping=-1.0)
            assert call(entry, levels=((8, 16), (4, 16), (2, 16), (1, 16)), write=True) == 0          # 4 levels, 64 iterations
            assert refused(g_max=4e3, levels=((3, 1), (1, 1))) and call(entry, g_max=4e3, levels=((3, 1),), write=True) == 0      # the bound is checked for every level first
    with pytest.raises(_lib.TslError, match="align_points_linearize"):
        g.align_points_linearize(scan, Rn, Tt)
    with pytest.raises(_lib.TslError, match="track_points"):
        g.track_points(scan, Rt, Tt, levels=((2, 1),) * 5)
    with pytest.raises(_lib.TslError, match="track_points"):
        g.track_points(scan, Rt, Tt, d_min=3.0, d_max=1.0)
    with pytest.raises(ValueError, match="device=True"):
        g.align_points_linearize(scan, Rt, Tt, device=True)

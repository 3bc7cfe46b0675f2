"""Frame-to-model alignment on the GPU (tsl_align.hip): the 33 integers of a linearisation and every record of a tracking run against the numpy
restatement (tests/track_ref.py) over the oracle's map of the box room (tests/track_scenes.py), the device form with frames in flight, lost and
singular runs, a global map, the refusals."""
import ctypes as C

import numpy as np
import pytest

import render_view_ref as rv
import track_ref as tr
import track_scenes as ts
from util import SMALL, assert_export_equal, make_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = ((240, 320), (5, 7), (1, 1), (251, 333))
_CHECKED = []


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _room(n=ts.N_FRAMES):
    """(HIP map after the first n of the six frames, the restatement's grid of the oracle's map after all six); both maps of make_pair(SMALL, K) take the
    same frames, and the oracle's equals the one the shared references were computed over"""
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


def _device_depth(depth):
    import torch
    return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()


def _same_records(got, want, what):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"] == len(got["records"]), \
        f"{what}: status {got['status']} / {want['status']}, iterations {got['iterations']} / {want['iterations']}"
    for k, (a, b) in enumerate(zip(got["records"], want["records"])):
        assert np.array_equal(a["sums"], b["sums"]), f"{what}, record {k}: sums differ at {np.nonzero(a['sums'] != b['sums'])[0].tolist()}"
        for f in ("R", "T", "xi"):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), f"{what}, record {k}: {f} differs: {a[f]} / {b[f]}"


def test_linearize_equals_the_restatement(hip_lib):
    """All 33 integers, at the true pose, the three perturbed poses and a pose that looks away; strides 1, 2, 3; huber off and 0.02; the 320 x 240 image,
    crops of 5 x 7 and 1 x 1 and a zero-padded 251 x 333 (tiles that do not fill a workgroup)."""
    g, grid = _room()
    Rt, Tt, depth = ts.tracked_frame()
    K = ts.intrinsics()
    poses = [("true", Rt, Tt)] + [(f"perturbed {n}", R, T) for n, (R, T) in enumerate(ts.perturbed_poses())] + [("away",) + ts.away_pose()]
    seen = np.zeros(5, np.int64)
    for shape in SHAPES:
        img = ts.shaped(depth, shape)
        for name, R, T in poses:
            for stride in (1, 2, 3):
                for huber in (0.0, 0.02):
                    want = tr.linearize(img, R, T, K, stride, ts.VS, grid, huber=huber, **ts.GATES)
                    got = g.align_linearize(img, R, T, K=K, stride=stride, huber=huber)
                    bad = np.nonzero(got["sums"] != want)[0]
                    assert bad.size == 0, f"{shape}, {name}, stride {stride}, huber {huber}: sums {bad.tolist()} differ: {got['sums'][bad]} / {want[bad]}"
                    assert got["sums"][tr.I_USED:].sum() == tr.visited(shape[0], shape[1], stride)
                    seen += want[tr.I_USED:] > 0
                    if name == "away":
                        assert got["n_unknown"] + got["n_gate"] == tr.visited(shape[0], shape[1], stride) and got["n_unknown"] > 0
    assert (seen > 0).all(), f"buckets used / gate / unknown / far / grad occurred in {seen.tolist()} cases"
    # the dict: H symmetric with the upper triangle in row-major order, the float forms scaled by 2^-20, the defaults = the values of SMALL and the map's K
    got = g.align_linearize(depth, Rt, Tt)
    want = tr.linearize(depth, Rt, Tt, K, 1, ts.VS, grid, **ts.GATES)
    assert np.array_equal(got["sums"], want) and got["H"].dtype == np.int64 and np.array_equal(got["H"], got["H"].T)
    assert np.array_equal(got["H"][np.triu_indices(6)], want[:21]) and np.array_equal(got["b"], want[21:27]) and got["e"] == want[27]
    assert np.array_equal(got["H_f"], got["H"] * 2.0 ** -20) and np.array_equal(got["b_f"], got["b"] * 2.0 ** -20) and got["e_f"] == got["e"] * 2.0 ** -20
    # the five counts by name; at the true pose no sample lies beyond the band (n_far = 0), so the second perturbed pose, where it does, names them too
    for R, T in ((Rt, Tt), ts.perturbed_poses()[1]):
        got = g.align_linearize(depth, R, T)
        want = tr.linearize(depth, R, T, K, 1, ts.VS, grid, **ts.GATES)
        assert [got[n] for n in ("n_used", "n_gate", "n_unknown", "n_far", "n_grad")] == want[tr.I_USED:].tolist()
        assert got["n_used"] > 70000 and got["n_unknown"] > 0 and got["n_grad"] > 0
    assert got["n_far"] > 0
    want = tr.linearize(depth, Rt, Tt, K, 1, ts.VS, grid, **ts.GATES)
    # counts only (the A/B switch of tools/bench_track.py): the same buckets, no sums
    co = g.align_linearize(depth, Rt, Tt, counts_only=True)
    assert np.array_equal(co["sums"][tr.I_USED:], want[tr.I_USED:]) and not co["sums"][:tr.I_USED].any()
    # explicit gates: a narrow depth range and a short band move pixels between the buckets as the restatement says
    gates = dict(d_min=1.5, d_max=2.5, r_max=0.05, g_max=1.5)
    got = g.align_linearize(depth, Rt, Tt, K=K, stride=2, **gates)
    assert np.array_equal(got["sums"], tr.linearize(depth, Rt, Tt, K, 2, ts.VS, grid, **gates)) and got["n_gate"] > 1000


def test_track_equals_the_restatement(hip_lib):
    """From 3 cm / 1.5 deg, 6 cm / 3 deg and 10 cm / 5 deg with the default levels: every record (pose, sums, step), the status and the count equal the
    restatement's bit for bit; the final pose lies within track_scenes.TRACK_BOUND_M / TRACK_BOUND_DEG of the true one."""
    g, _ = _room()
    Rt, Tt, depth = ts.tracked_frame()
    for n, ((Rp, Tp), (Rw, Tw, want)) in enumerate(zip(ts.perturbed_poses(), ts.reference_tracks())):
        R, T, info = g.track_depth(depth, Rp, Tp, K=ts.intrinsics())
        _same_records(info, want, f"perturbation {n}")
        assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
        em, ed = ts.pose_error(R, T, Rt, Tt)
        print(f"perturbation {n}: status {info['status']}, {info['iterations']} linearisations, final error {em:.6f} m {ed:.5f} deg")
        assert info["status"] == 0 and em <= ts.TRACK_BOUND_M and ed <= ts.TRACK_BOUND_DEG
    # other levels, damping and a robust weight, exhausted iterations: status 1
    Rp, Tp = ts.perturbed_poses()[0]
    kw = dict(levels=((4, 2), (3, 1)), min_step=1e-9, damping=1e-3)
    R, T, info = g.track_depth(depth, Rp, Tp, K=ts.intrinsics(), huber=0.02, **kw)
    Rw, Tw, want = tr.track(depth, Rp, Tp, ts.intrinsics(), ts.VS, ts.oracle_grid(), huber=0.02, **kw, **ts.GATES)
    _same_records(info, want, "two levels, damped")
    assert info["status"] == 1 and info["iterations"] == 3 and np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))


def test_device_form_with_work_in_flight(hip_lib):
    import torch
    g, _ = _room(4)
    g.sync()
    Rt, Tt, depth = ts.tracked_frame()
    Rp, Tp = ts.perturbed_poses()[0]
    K = ts.intrinsics()
    dev_depth = _device_depth(depth)
    before = g.align_linearize(depth, Rp, Tp, K=K, stride=2)
    side = torch.cuda.Stream()
    for R, T, d in ts.map_frames()[4:]:                              # queued frames, then the linearisation: no sync in between
        g.recast_depth_to_map(R, T, d, None)
    with torch.cuda.stream(side):
        dev = g.align_linearize(dev_depth, Rp, Tp, K=K, stride=2, device=True)
        total = dev[28:33].sum()
    side.synchronize()
    assert dev.is_cuda and dev.dtype == torch.int64 and dev.shape == (40,)
    got = dev.cpu().numpy()
    g.sync()
    want = g.align_linearize(depth, Rp, Tp, K=K, stride=2)
    assert np.array_equal(got[:33], want["sums"]) and not got[33:].any() and int(total) == tr.visited(ts.H, ts.W, 2)
    assert (before["sums"] != want["sums"]).sum() > 20                # the queued frames were integrated before the linearisation ran
    # a second device call refills the same kind of buffer from zero; the host form takes a device image too
    with torch.cuda.stream(side):
        dev2 = g.align_linearize(dev_depth, Rp, Tp, K=K, stride=2, device=True)
    side.synchronize()
    assert np.array_equal(dev2.cpu().numpy(), got)
    assert np.array_equal(g.align_linearize(dev_depth, Rp, Tp, K=K, stride=2)["sums"], want["sums"])
    # tracking from a device image equals tracking from the host image
    Rh, Th, ih = g.track_depth(depth, Rp, Tp, K=K)
    with torch.cuda.stream(side):
        Rd, Td, idv = g.track_depth(dev_depth, Rp, Tp, K=K)
    _same_records(idv, ih, "device image")
    assert np.array_equal(_bits(Rd), _bits(Rh)) and np.array_equal(_bits(Td), _bits(Th)) and ih["status"] == 0


def test_lost_and_singular(hip_lib):
    g, grid = _room()
    Rt, Tt, depth = ts.tracked_frame()
    K = ts.intrinsics()
    Ra, Ta = ts.away_pose()
    R, T, info = g.track_depth(depth, Ra, Ta, K=K, min_used=100)
    assert info["status"] == 2 and info["iterations"] == 1 and info["records"][0]["n_used"] == 0 and not info["records"][0]["xi"].any()
    assert np.array_equal(_bits(R), _bits(Ra)) and np.array_equal(_bits(T), _bits(Ta))
    # a one-pixel image: one row of J cannot fix six unknowns -- singular, the guess comes back, as in the restatement
    one = ts.shaped(depth, (1, 1))
    R, T, info = g.track_depth(one, Rt, Tt, K=K, levels=((1, 3),), min_used=1)
    _, _, want = tr.track(one, Rt, Tt, K, ts.VS, grid, levels=((1, 3),), min_used=1, **ts.GATES)
    _same_records(info, want, "one pixel")
    assert info["status"] == 3 and info["records"][0]["n_used"] == 1 and np.array_equal(_bits(R), _bits(Rt)) and np.array_equal(_bits(T), _bits(Tt))
    # lost on the way: the second level has too few pixels for min_used, the pose of the last step's linearisation comes back
    Rp, Tp = ts.perturbed_poses()[0]
    R, T, info = g.track_depth(depth, Rp, Tp, K=K, levels=((2, 2), (16, 2)), min_step=0.0, min_used=1000)
    _, _, want = tr.track(depth, Rp, Tp, K, ts.VS, grid, levels=((2, 2), (16, 2)), min_step=0.0, min_used=1000, **ts.GATES)
    _same_records(info, want, "lost at the second level")
    assert info["status"] == 2 and info["iterations"] == 3 and np.array_equal(_bits(R), _bits(info["records"][1]["R"])) and np.array_equal(_bits(T), _bits(info["records"][1]["T"]))
    # after reset() nothing is known
    g.reset()
    for stride in (1, 3):
        s = g.align_linearize(depth, Rt, Tt, K=K, stride=stride)
        assert s["n_unknown"] + s["n_gate"] == tr.visited(ts.H, ts.W, stride) and s["n_unknown"] > 0 and not s["sums"][:tr.I_USED].any()
    R, T, info = g.track_depth(depth, Rp, Tp, K=K)
    assert info["status"] == 2 and info["iterations"] == 1 and np.array_equal(_bits(R), _bits(Rp)) and np.array_equal(_bits(T), _bits(Tp))


def test_global_map_linearises_submap_0(hip_lib):
    from taichislam_amd.mapping import DenseTSDF
    G = DenseTSDF(**dict(SMALL, is_global_map=True))
    G.set_dep_camera_intrinsic(ts.intrinsics())
    for R, T, d in ts.map_frames():
        G.recast_depth_to_map(R, T, d, None)
    e = G.export_submap()
    grid = rv.grid_from_export(e["indices"], e["TSDF"], G.N, G.Nz)
    Rt, Tt, depth = ts.tracked_frame()
    Rp, Tp = ts.perturbed_poses()[1]
    for R, T in ((Rt, Tt), (Rp, Tp)):
        got = G.align_linearize(depth, R, T, stride=2, huber=0.02)
        want = tr.linearize(depth, R, T, ts.intrinsics(), 2, ts.VS, grid, huber=0.02, **ts.GATES)
        assert np.array_equal(got["sums"], want) and got["n_used"] > 10000


def test_refusals(hip_lib):
    import torch
    from taichislam_amd import _lib
    g, _ = _room(2)
    Rt, Tt, depth = ts.tracked_frame()
    Kt = ts.intrinsics()
    h, w = depth.shape
    dev_depth = _device_depth(depth)
    dev_sums = torch.zeros(40, dtype=torch.int64, device="cuda")
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    Ro, To = np.zeros(9), np.zeros(3)
    NULL = object()

    def call(entry, R=Rt, T=Tt, K=Kt, h=h, w=w, stride=1, d_min=0.0, d_max=0.0, r_max=0.0, g_max=0.0, huber=0.0, image=None, out=None, cfg=True, levels=((2, 1),),
             min_step=1e-4, damping=0.0, handle=True):
        c = _lib.AlignCfg()
        c.K[:] = list(np.asarray(K, np.float64).reshape(-1))
        c.h, c.w, c.stride, c.d_min, c.d_max, c.r_max, c.g_max, c.huber = h, w, stride, d_min, d_max, r_max, g_max, huber
        t = _lib.TrackCfg()
        t.n_levels = len(levels)
        for i, (st, it) in enumerate(levels[:4]):
            t.stride[i], t.iters[i] = st, it
        t.min_step, t.damping = min_step, damping
        hd = g.h if handle else None
        cp = C.byref(c) if cfg else None
        Rp, Tp = (None if R is NULL else dp(R)), (None if T is NULL else dp(T))
        host = None if image is NULL else depth.ctypes.data_as(C.c_void_p)
        devp = None if image is NULL else C.c_void_p(dev_depth.data_ptr())
        sums = _lib.AlignSums()
        if entry == "align_linearize":
            return g.L.tsl_tsdf_align_linearize(hd, Rp, Tp, cp, host, None if out is NULL else C.byref(sums))
        if entry == "align_linearize_dev":
            return g.L.tsl_tsdf_align_linearize_dev(hd, Rp, Tp, cp, devp, None if out is NULL else C.c_void_p(dev_sums.data_ptr()), None)
        if entry == "track_depth":
            return g.L.tsl_tsdf_track_depth(hd, Rp, Tp, cp, C.byref(t), host, None if out is NULL else dp(Ro), dp(To), None)
        return g.L.tsl_tsdf_track_depth_dev(hd, Rp, Tp, cp, C.byref(t), devp, None if out is NULL else dp(Ro), dp(To), None, None)

    Rn = np.array(Rt, np.float64); Rn[1, 1] = np.nan
    for entry in ("align_linearize", "align_linearize_dev", "track_depth", "track_depth_dev"):
        def refused(**kw):
            rc = call(entry, **kw)
            return rc == -1 and entry.encode() in g.L.tsl_last_error()
        assert call(entry) == 0, g.L.tsl_last_error()
        assert call(entry, K=np.zeros(9)) == 0                         # all zero: the map's depth intrinsics
        assert refused(handle=False) and refused(R=NULL) and refused(T=NULL) and refused(cfg=False) and refused(image=NULL) and refused(out=NULL)
        assert refused(R=Rn) and refused(T=[0.0, np.inf, 0.0])
        assert refused(K=np.where(np.arange(9) == 4, np.nan, Kt)) and refused(K=np.where(np.arange(9) == 2, -np.inf, Kt))
        assert refused(d_min=float("nan")) and refused(d_max=float("inf")) and refused(r_max=float("nan")) and refused(g_max=float("inf")) and refused(huber=float("nan"))
        assert refused(h=0) and refused(w=-3) and refused(h=32769)
        assert refused(d_min=2.0, d_max=2.0) and refused(d_min=2.0, d_max=1.0) and refused(d_min=6.0)          # 6 > the default d_max = 5
        assert refused(r_max=-0.1) and refused(g_max=-1.0) and refused(huber=-0.02)
        # the overflow bound: L = 5.12 m; with g_max = 1e6 M^2 2^20 visited = 1.05e14 * 1.05e6 * 76800 > 2^62 = 4.6e18
        assert refused(g_max=1e6) and refused(r_max=1e7)
        if entry.startswith("align"):
            assert refused(stride=0) and refused(stride=-2)
            # g_max = 1000: M^2 2^20 = 100 * 2^40; times 76 800 pixels it exceeds 2^62, times 19 200 it does not
            assert call(entry, g_max=1e6, stride=64) == -1 and refused(g_max=1e3, stride=1) and call(entry, g_max=1e3, stride=2) == 0
        else:
            assert refused(levels=((0, 1),)) and refused(levels=((2, 1),) * 5) and refused(levels=()) and refused(levels=((2, 33), (1, 32))) and refused(levels=((2, 65),))
            assert refused(min_step=float("nan")) and refused(damping=-1.0)
            assert call(entry, levels=((8, 16), (4, 16), (2, 16), (1, 16))) == 0          # 4 levels, 64 iterations
            assert refused(g_max=1e3, levels=((2, 1), (1, 1))) and call(entry, g_max=1e3, levels=((2, 1),)) == 0      # the bound is checked for every level first
    torch.cuda.synchronize()
    with pytest.raises(_lib.TslError, match="align_linearize"):
        g.align_linearize(depth, Rn, Tt)
    with pytest.raises(_lib.TslError, match="track_depth"):
        g.track_depth(depth, Rt, Tt, levels=((2, 1),) * 5)
    with pytest.raises(_lib.TslError, match="track_depth"):
        g.track_depth(depth, Rt, Tt, d_min=3.0, d_max=1.0)

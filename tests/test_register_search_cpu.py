"""The pose search for the registration without a GPU: the numpy restatement (tests/register_search_ref.py) scores as register_ref.linearize does,
enumerates, ranks and refines as DESIGN.md section 4.10 says, and recovers from the two guesses the plain registration loses (the maps of
tests/register_scenes.py); the library exports the entry points with the documented struct sizes and refuses null handles without a device."""
import ctypes as C

import numpy as np
import pytest

import register_ref as rr
import register_scenes as rs
import register_search_ref as sr
import register_search_scenes as ss
import track_ref as tr
import track_scenes as ts

F32 = np.float32
OTHER_GATES = dict(w_min=2.0, band=0.05, r_max=0.06, g_max=1.2)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _poses(n, seed=5):
    """D, the three perturbed poses, the outside pose, then D moved by up to 0.5 m / 40 deg (default_rng(seed)) up to n"""
    Rd, Td = rs.displacement()
    out = [(Rd, Td)] + rs.perturbed_poses() + [rs.outside_pose()]
    rng = np.random.default_rng(seed)
    while len(out) < n:
        out.append((ts.rotation(rng.standard_normal(3), rng.uniform(-40, 40)) @ Rd, Td + rng.uniform(-0.5, 0.5, 3)))
    return np.stack([p[0] for p in out]), np.stack([p[1] for p in out])


def test_fast_score_equals_linearize():
    """22 poses: the fast path of register_search_ref.score against register_ref.linearize per pose, strides 1 and 4, huber, other gates, counts only;
    every bucket occurs; gate() against the n_gate of the linearisation and the visited count."""
    src, grid = rs.src_voxels(), rs.dst_grid()
    R, T = _poses(22)
    seen = np.zeros(5, np.int64)
    for stride, gates in ((4, rs.GATES), (1, dict(rs.GATES, huber=F32(0.02))), (2, rr.defaults(rs.VS, 10, 0.04, **OTHER_GATES))):
        want = sr.score_slow(src, R, T, stride, rs.VS, grid, **gates)
        got = sr.score(src, R, T, stride, rs.VS, grid, chunk=7, **gates)
        for f in sr.FIELDS:
            assert np.array_equal(got[f], want[f]), (stride, f, np.nonzero(got[f] != want[f])[0])
        g = sr.gate(src, stride, **gates)
        n_gate = int(rr.linearize(src, R[0], T[0], stride, rs.VS, grid, **gates)[tr.I_GATE])
        assert g["n_gate"] == n_gate and g["n_gate"] + g["n_pass"] == rr.visited(src, stride)
        assert ((got["n_used"] + got["n_unknown"] + got["n_far"] + got["n_grad"]) == g["n_pass"]).all()
        seen += [(got["n_used"] > 0).any(), g["n_gate"] > 0, (got["n_unknown"] > 0).any(), (got["n_far"] > 0).any(), (got["n_grad"] > 0).any()]
        assert (got["e"][got["n_used"] > 0] > 0).all()
    assert (seen > 0).all(), f"buckets used / gate / unknown / far / grad occurred in {seen.tolist()} cases"
    co = sr.score(src, R, T, 4, rs.VS, grid, counts_only=True, **rs.GATES)
    full = sr.score(src, R, T, 4, rs.VS, grid, **rs.GATES)
    assert not co["e"].any() and all(np.array_equal(co[f], full[f]) for f in sr.FIELDS[1:])


def test_enumeration_order_and_count():
    """k runs over (r0, r1, r2, t0, t1, t2), the last fastest; offsets are (index - n) * step; the formation is the one written in the header."""
    R0, T0 = ss.guess("B")
    pivot = np.array([1.5, 2.0, 0.1])
    n_t, step_t, n_r, step_r = (1, 0, 2), (0.2, 0.3, 0.05), (1, 2, 0), (0.1, 0.07, 0.3)
    Rs, Ts = sr.candidates(R0, T0, pivot, n_t, step_t, n_r, step_r)
    dims = (3, 5, 1, 3, 1, 5)
    assert Rs.shape == (225, 3, 3) and Ts.shape == (225, 3) and int(np.prod(dims)) == 225
    for k in (0, 1, 4, 5, 14, 15, 74, 75, 112, 200, 224):
        ix = np.unravel_index(k, dims)
        om = [(ix[0] - 1) * step_r[0], (ix[1] - 2) * step_r[1], 0.0 * step_r[2]]
        v = np.array([(ix[3] - 1) * step_t[0], 0.0 * step_t[1], (ix[5] - 2) * step_t[2]])
        if k == 112:                                          # the centre
            assert np.array_equal(_bits(Rs[k]), _bits(R0)) and np.array_equal(_bits(Ts[k]), _bits(T0))
            continue
        Rk, Tp = tr.retract([0.0, 0.0, 0.0] + om, R0, T0 - pivot)
        assert np.array_equal(_bits(Rs[k]), _bits(Rk)) and np.array_equal(_bits(Ts[k]), _bits((Tp + pivot) + v)), k
    # the rotation is about the pivot: a candidate without a translation offset leaves the pivot where the guess puts it
    k = int(np.ravel_multi_index((2, 4, 0, 1, 0, 2), dims))
    back = R0.T @ (pivot - T0)
    assert np.allclose(Rs[k] @ back + Ts[k], pivot, rtol=0, atol=1e-12) and ts.pose_error(Rs[k], Ts[k], R0, T0)[1] > 5.0
    # the angle of an offset omega is 2 atan(|omega| / 2)
    Rz, _ = sr.candidates(np.eye(3), np.zeros(3), np.zeros(3), (0, 0, 0), (1, 1, 1), (0, 0, 1), (1, 1, 0.5))
    assert abs(np.degrees(np.arccos(Rz[2][0, 0])) - np.degrees(2 * np.arctan(0.25))) < 1e-9
    with pytest.raises(AssertionError):
        sr.candidates(R0, T0, pivot, (8, 8, 8), (1, 1, 1), (8, 8, 0), (1, 1, 1))      # 17^5 > 65536


def test_zero_offset_is_the_guess():
    """All n = 0: one candidate, the guess bit for bit, and the search is the registration from the guess."""
    src, grid = rs.src_voxels(), rs.dst_grid()
    R0, T0 = rs.perturbed_poses()[1]
    Rs, Ts = sr.candidates(R0, T0, [1.0, 2.0, 3.0], (0, 0, 0), (0.2,) * 3, (0, 0, 0), (0.1,) * 3)
    assert Rs.shape[0] == 1 and np.array_equal(_bits(Rs[0]), _bits(R0)) and np.array_equal(_bits(Ts[0]), _bits(T0))
    R, T, info = sr.search(src, R0, T0, rs.VS, grid, ss.VOXEL, (0, 0, 0), (0.2,) * 3, (0, 0, 0), (0.1,) * 3, **rs.GATES)
    Rw, Tw, want = rs.reference_runs()[1]
    assert info["search"]["best"] == 0 and info["search"]["n_candidates"] == 1 and info["status"] == want["status"] == info["search"]["status"]
    assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw)) and info["iterations"] == want["iterations"]


def test_ties_and_validity():
    """Equal costs go to the lower index; a candidate below min_used never wins; a huge min_used leaves none: status 2, the guess, no records."""
    src, grid = rs.src_voxels(), rs.dst_grid()
    R0, T0 = rs.perturbed_poses()[0]
    lattice = dict(n_t=(1, 0, 0), step_t=(0.02,) * 3, n_r=(0, 0, 1), step_r=(0.01,) * 3)

    def stub(e, used):
        def fn(src_, R, T, *a, **kw):
            z = np.zeros(len(e), np.int64)
            return dict(e=np.array(e, np.int64), n_used=np.array(used, np.int64), n_unknown=z.copy(), n_far=z.copy(), n_grad=z.copy())
        return fn
    kw = dict(register_kw=dict(levels=((4, 1),)), **rs.GATES)
    nine = lambda v: [v] * 9
    _, _, info = sr.search(src, R0, T0, rs.VS, grid, ss.VOXEL, score_fn=stub([9, 7, 5, 8, 5, 5, 9, 9, 9], nine(100)), **lattice, **kw)
    assert info["search"]["best"] == 2 and info["search"]["J_best"] == 5 and info["search"]["n_valid"] == 9
    _, _, info = sr.search(src, R0, T0, rs.VS, grid, ss.VOXEL, score_fn=stub([9, 7, 5, 8, 5, 5, 9, 9, 9], [100, 100, 5, 100, 6, 100, 100, 100, 100]), **lattice, **kw)
    assert info["search"]["best"] == 4 and info["search"]["n_valid"] == 8          # candidate 2 has n_used 5 < 6
    # the cost: F = rint(r_max^2 2^20), U = rint(miss^2 2^20) in f32; miss 0 = r_max
    sc = dict(e=np.array([10]), n_far=np.array([2]), n_unknown=np.array([3]), n_grad=np.array([4]))
    F = int(np.rint(np.float64(F32(0.4) * F32(0.4)) * 2 ** 20))
    U = int(np.rint(np.float64(F32(0.08) * F32(0.08)) * 2 ** 20))
    assert sr.cost(sc, F32(0.4), 0.0)[0] == 10 + F * 9 and sr.cost(sc, F32(0.4), 0.08)[0] == 10 + 2 * F + 7 * U
    # a huge min_used
    R, T, info = sr.search(src, R0, T0, rs.VS, grid, ss.VOXEL, min_used=10 ** 9, **lattice, **rs.GATES)
    assert info["status"] == 2 and info["iterations"] == 0 and info["records"] == [] and info["search"]["best"] == -1 and info["search"]["n_valid"] == 0
    assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(T), _bits(T0)) and info["search"]["n_candidates"] == 9


def test_automatic_pivot_is_the_centroid():
    """The pivot of a search without one is R0 qbar + T0, qbar the centroid of the source voxels that pass the gate at the scoring stride, computed
    here from the export."""
    e = rs.src_export()
    idx = np.asarray(e["indices"]).astype(np.int64)
    t = np.asarray(e["TSDF"]).view(np.float16).astype(np.float64)
    for stride in (1, 4):
        keep = ((idx % stride) == 0).all(1) & (np.abs(t) <= float(rs.GATES["band"]))
        qb = idx[keep].mean(0) * ss.VOXEL
        R0, T0 = ss.guess("C")
        pivot, g = sr.auto_pivot(rs.src_voxels(), R0, T0, stride, ss.VOXEL, **rs.GATES)
        assert g["n_pass"] == keep.sum() and np.allclose(pivot, R0 @ qb + T0, rtol=0, atol=1e-9)
    assert np.allclose(ss.centroid()[0], idx[np.abs(t) <= float(rs.GATES["band"])].mean(0) * ss.VOXEL, rtol=0, atol=1e-9)
    # nothing passes the gate: no pivot, status 2
    none = (rs.src_voxels()[0][:10], np.full(10, 0.5, F32), np.ones(10, F32))
    R0, T0 = rs.displacement()
    R, T, info = sr.search(none, R0, T0, rs.VS, rs.dst_grid(), ss.VOXEL, ss.N_T, ss.STEPS_T, ss.N_R, ss.STEPS_R, **rs.GATES)
    assert info["status"] == 2 and info["search"]["gate"]["n_pass"] == 0 and info["search"]["pivot"] is None and np.array_equal(_bits(T), _bits(T0))


@pytest.mark.parametrize("name", ["B", "C"])
def test_search_recovers_what_the_registration_loses(name):
    """Guess B: D turned 55 deg about z through the centroid and shifted (0.7, -0.6, 0.3) m; guess C: -58 deg about (0.05, 0.1, 1), (-0.7, -0.7, -0.3) m.
    register_ref.register from the guess ends more than 1 m or 45 deg from D (measured: 3.64 m / 91.97 deg, status 1, and 1.94 m / 38.39 deg, status 2
    -- lost).  The search with the defaults of DenseTSDF.register_search (5265 candidates, stride 4, miss = r_max = 0.4) ends with status 0 within
    register_scenes.REGISTER_BOUND_M / REGISTER_BOUND_DEG (measured: 0.000806 m / 0.013677 deg for both, 8 linearisations; the best candidate lies
    0.150 m / 0.27 deg and 0.290 m / 6.63 deg from D)."""
    Rd, Td = rs.displacement()
    assert (ss.N_T, ss.N_R) == ((4, 4, 2), (0, 0, 6))
    R, T, info = ss.direct_run(name)
    dm, dd = ts.pose_error(R, T, Rd, Td)
    print(f"{name}: directly from the guess: {dm:.6f} m {dd:.6f} deg, status {info['status']}")
    assert dm > 1.0 or dd > 45.0
    assert abs(dm - ss.MEASURED_DIRECT[name][0]) < 1e-5 and abs(dd - ss.MEASURED_DIRECT[name][1]) < 1e-5 and info["status"] == ss.MEASURED_DIRECT[name][2]
    R, T, info = ss.reference_search(name)
    s = info["search"]
    em, ed = ts.pose_error(R, T, Rd, Td)
    bm, bd = ts.pose_error(s["R_best"], s["T_best"], Rd, Td)
    print(f"{name}: best {s['best']}, J {s['J_best']}, {s['n_valid']} of {s['n_candidates']} valid, best candidate {bm:.6f} m {bd:.6f} deg; "
          f"final {em:.6f} m {ed:.6f} deg, status {info['status']}, {info['iterations']} linearisations")
    assert s["n_candidates"] == ss.N_CANDIDATES == 5265 and s["status"] == info["status"] == 0
    assert em <= rs.REGISTER_BOUND_M and ed <= rs.REGISTER_BOUND_DEG
    assert (s["best"], s["J_best"], s["n_valid"]) == ss.MEASURED_BEST[name]
    assert abs(bm - ss.MEASURED_BEST_ERROR[name][0]) < 1e-5 and abs(bd - ss.MEASURED_BEST_ERROR[name][1]) < 1e-5
    fm, fd, fs, fi = ss.MEASURED_FINAL[name]
    assert em <= fm and ed <= fd and fm <= em * 1.01 and fd <= ed * 1.01 and (info["status"], info["iterations"]) == (fs, fi)


def test_abi_without_a_device():
    """The two entry points exist, the structs have the documented sizes, the profiling id is the one of the header, and what can be refused without
    a device is refused with the entry point named."""
    import os
    import re
    from taichislam_amd import _lib
    L = _lib.lib()
    assert C.sizeof(_lib.RegisterScore) == 24 and C.sizeof(_lib.RegisterGate) == 40 and C.sizeof(_lib.SearchCfg) == 120 and C.sizeof(_lib.SearchReport) == 208
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "taichislam_hip.h")).read()
    assert int(re.search(r"TSL_K_REGISTER_SCORE = (\d+)", hdr).group(1)) == _lib.K_REGISTER_SCORE and _lib.KERNEL_NAMES[_lib.K_REGISTER_SCORE] == "register_score"
    R, T = np.eye(3).reshape(-1), np.zeros(3)
    dp = lambda a: a.ctypes.data_as(_lib.dp)
    cfg, tc, sc, rep, trk = _lib.RegisterCfg(), _lib.TrackCfg(), _lib.SearchCfg(), _lib.SearchReport(), _lib.TrackReport()
    cfg.stride, tc.n_levels, tc.stride[0], tc.iters[0], sc.stride = 1, 1, 1, 1, 4
    out, gate = (_lib.RegisterScore * 1)(), _lib.RegisterGate()
    Ro, To = np.zeros(9), np.zeros(3)
    assert L.tsl_tsdf_register_score(None, -1, None, -1, dp(R), dp(T), 1, C.byref(cfg), out, C.byref(gate)) == -1
    assert b"register_score" in L.tsl_last_error()
    assert L.tsl_tsdf_register_search(None, -1, None, -1, dp(R), dp(T), C.byref(cfg), C.byref(sc), C.byref(tc), dp(Ro), dp(To), C.byref(rep), C.byref(trk), None) == -1
    assert b"register_search" in L.tsl_last_error()
    from taichislam_amd.mapping import DenseTSDF, SubmapMapping
    assert callable(DenseTSDF.register_score) and callable(DenseTSDF.register_search) and callable(SubmapMapping.search_submaps)

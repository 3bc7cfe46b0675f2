"""The numpy restatement of the B-spline trajectory linearisation and descent (tests/traj_opt_ref.py) on hand-built dense grids whose answers are worked
out by hand here: it is what the GPU tests compare the kernel with (tests/test_traj_opt_gpu.py), so it is checked on its own first.  No GPU."""
import os
import re

import numpy as np

import traj_opt_ref as ref
from taichislam_amd.utils import nav

F32 = np.float32
VS = F32(0.25)
N = 32                                   # voxel indices -16 .. 15: x in [-4, 3.75]
LO = np.array([-16, -16, -16], np.int64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2 ** 20                              # one metre (gradients) or square metre (costs) of the fixed point


def _wall():
    """val = x: a wall at x = 0, free space at x > 0; every voxel known.  The interpolant is x up to one rounding and its gradient is (1, 0, 0) exactly
    (the differences along x are 0.25 exactly, those along y and z are 0)."""
    i = np.arange(N) + LO[0]
    val = np.broadcast_to((i.astype(F32) * VS)[:, None, None], (N, N, N)).copy()
    return val, np.ones((N, N, N), bool)


def _lin(c, clearance, sub, val, known, lengths=None, unknown=np.nan):
    return ref.linearize(c, clearance, sub, lengths, VS, val, known, LO, unknown)


def _opt(c, clearance, sub, iters, val, known, **kw):
    return ref.optimize(c, clearance, sub, iters, kw.pop("lengths", None), VS, val, known, LO, **kw)


def test_basis_and_positions():
    sixth = F32(6.0)
    for sub in (1, 2, 3, 4, 7, 16, 64):
        b = ref.basis(sub)
        assert b.shape == (sub + 1, 4) and b.dtype == F32
        assert np.array_equal(b[0], np.array([1, 4, 1, 0], F32) / sixth) and np.array_equal(b[-1], np.array([0, 1, 4, 1], F32) / sixth)
        assert np.array_equal(b, nav.bspline_basis(sub))
        assert np.abs(b.astype(np.float64).sum(1) - 1.0).max() < 4 * 2.0 ** -24
    # fl(fl(fl(1/6) + fl(2/3)) + fl(1/6)) = 1 (0.16666667163 + 0.66666668653 = 0.83333335817 -> 0.83333337307; + 0.16666667163 = 1.0000000447 -> 1):
    # at u = 0 and u = 1 a coordinate that all four control points share, and that is a power of two, is sampled exactly
    c = np.zeros((1, 9, 3), F32)
    c[0, :, 0], c[0, :, 1], c[0, :, 2] = 0.25, -2.0, 0.0
    p, valid, seg, _ = ref.sample_points(c, 1)
    assert valid.all() and p.shape == (1, 7, 3) and seg[0].tolist() == [0, 1, 2, 3, 4, 5, 5] and (p == c[:, :7]).all()
    # collinear, equally spaced control points at quarter-metre coordinates: the spline is the line, sample j of span seg lies at c[seg + 1] + u * h.  In
    # f32 this is NOT exact -- the weights b_i / 6 are rounded, their sum is 1 - 2^-24 at some u -- so the bound is derived instead: four products
    # and three sums and the rounded weights, each at most 2^-24 relative to a magnitude of at most max |c|: 8 * 2^-24 * max |c| (found: one ulp)
    for sub in (1, 2, 4, 8):
        for x0, h in ((-1.0, 0.25), (0.25, 0.25), (-3.0, 0.5), (1.0, 0.5)):
            c = np.zeros((1, 8, 3), F32)
            c[0, :, 0] = x0 + h * np.arange(8)
            c[0, :, 2] = 2.0 - 0.25 * np.arange(8)
            p, valid, _, _ = ref.sample_points(c, sub)
            j = np.arange(5 * sub + 1) / sub
            assert valid.all() and p.shape == (1, 5 * sub + 1, 3)
            assert np.abs(p[0, :, 0] - (x0 + h + h * j)).max() <= 8 * 2.0 ** -24 * np.abs(c[0, :, 0]).max()
            assert np.abs(p[0, :, 2] - (1.75 - 0.25 * j)).max() <= 8 * 2.0 ** -24 * 2.0 and (p[0, :, 1] == 0).all()
            assert np.array_equal(p[0], nav.bspline_points(c[0], sub)) and np.array_equal(p, nav.bspline_points(c, sub))
    # lengths: S = (L - 3) * sub + 1, the last sample has m = sub, and the helper pads a row with its last sample
    c = np.random.default_rng(0).uniform(-1, 1, (3, 9, 3)).astype(F32)
    ln = np.array([4, 9, 6])
    p, valid, seg, _ = ref.sample_points(c, 4, ln)
    assert valid.sum(1).tolist() == [5, 25, 13] and seg[0, :5].tolist() == [0] * 5 and seg[2, :13].tolist() == [0] * 4 + [1] * 4 + [2] * 5
    q = nav.bspline_points(c, 4, ln)
    assert np.array_equal(q[valid], p[valid]) and np.array_equal(q[0, 5:], np.repeat(q[0, 4:5], 20, 0))
    for one in range(3):                                                          # a shorter trajectory is the longer one's prefix
        assert np.array_equal(ref.sample_points(c[one:one + 1, :ln[one]], 4)[0][0], p[one, :valid[one].sum()])


def test_wall_cost_and_gradient_by_hand():
    val, known = _wall()
    # parallel to the wall at x = 0.25 (a power of two: sampled exactly at sub = 1, above), clearance 0.5: c = 0.25 at each of the S = 9 samples
    c = np.zeros((1, 11, 3), F32)
    c[0, :, 0], c[0, :, 1] = 0.25, 0.5 * np.arange(11) - 2.5
    rec, gc, gs = _lin(c, 0.5, 1, val, known)
    S = 9
    assert (rec["n_samples"][0], rec["n_pen"][0], rec["n_unknown"][0], rec["n_outside"][0], rec["argmin"][0]) == (S, S, 0, 0, 0)
    assert rec["min_dist"][0] == F32(0.25) and rec["cost_collision"][0] == S * 2 ** 16 and rec["cost_smooth"][0] == 0 and rec["iters_done"][0] == 0
    assert (gc[0, :, 1:] == 0).all() and (gs == 0).all()
    # Gp = -(2 * 0.25 * 1) = -0.5; per sample the terms are A = trunc(-0.5 * 2^20 / 6) = -87381 twice and B = trunc(-0.5 * 2^20 * 2 / 3) = -349525,
    # -(2^19 - 1) together: sample j < 8 puts A, B, A on the points j, j + 1, j + 2, the last one (u = 1 in span 7) on the points 8, 9, 10
    assert gc[0, :, 0].sum() == -S * (2 ** 19 - 1)
    assert gc[0, :, 0].tolist() == [-87381, -436906] + [-524287] * 7 + [-436906, -87381]
    # the same wall at sub = 4: c is 0.25 up to the rounding of the position, and the x gradients sum to -S * 2^19 give or take: each of the 4 S terms
    # loses less than 1 to the truncation, and the roundings of w_i and of c move a term by less than 2^-5 + 2^20 * 2 * 2^-24 < 1/4
    rec, gc, gs = _lin(c, 0.5, 4, val, known)
    S = 33
    assert rec["n_samples"][0] == S and rec["n_pen"][0] == S and abs(int(rec["cost_collision"][0]) - S * 2 ** 16) <= S * 2
    assert (gc[0, :, 1:] == 0).all() and abs(int(gc[0, :, 0].sum()) + S * 2 ** 19) <= 4 * S * 1.25
    # clearance 0.25: c = 0 is not penalised
    rec, gc, _ = _lin(c, 0.25, 1, val, known)
    assert rec["n_pen"][0] == 0 and rec["cost_collision"][0] == 0 and (gc == 0).all()
    # the clamp of c at 1024 and of a gradient term at 1024: a wall of slope 1 far below
    deep = (val - F32(5000.0)).astype(F32)
    rec, gc, _ = _lin(c, 0.5, 1, deep, known)
    assert rec["cost_collision"][0] == 9 * 2 ** 40 and gc[0, 3, 0] == -(2 ** 30) - 2 * int(np.trunc(F32(2048.0) * (F32(1.0) / F32(6.0)) * F32(U)))


def test_gradient_against_float64_finite_differences():
    val, known = _wall()
    rng = np.random.default_rng(5)
    K, sub, cl = 9, 4, 0.5
    # control points on the 2^-10 grid: the second differences are exact in f32 and the smoothness terms are whole units.  0.125 <= x <= 0.4: every
    # sample is penalised with a margin, so the float64 cost is one quadratic around the point and a central difference of it is exact
    c = np.empty((1, K, 3))
    c[0, :, 0] = rng.integers(128, 410, K) / 1024.0
    c[0, :, 1:] = rng.integers(-1024, 1024, (K, 2)) / 1024.0
    rec, gc, gs = _lin(c.astype(F32), cl, sub, val, known)
    S = (K - 3) * sub + 1
    assert rec["n_pen"][0] == S

    def cost(cc):
        u = np.arange(sub + 1) / sub
        B = np.stack([(1 - u) ** 3, 3 * u ** 3 - 6 * u ** 2 + 4, -3 * u ** 3 + 3 * u ** 2 + 3 * u + 1, u ** 3], 1) / 6.0
        j = np.arange(S)
        seg = np.minimum(j // sub, K - 4)
        p = sum(B[j - seg * sub, i][:, None] * cc[seg + i] for i in range(4))
        a = cc[:-2] - 2 * cc[1:-1] + cc[2:]
        return (np.maximum(cl - p[:, 0], 0.0) ** 2).sum(), (a ** 2).sum()
    h = 2.0 ** -12
    terms = np.zeros(K)
    j = np.arange(S)
    for i in range(4):
        np.add.at(terms, np.minimum(j // sub, K - 4) + i, 1)
    for i in range(K):
        for ax in range(3):
            e = np.zeros((K, 3))
            e[i, ax] = h
            (c1, s1), (c0, s0) = cost(c[0] + e), cost(c[0] - e)
            fd_c, fd_s = (c1 - c0) / (2 * h) * U, (s1 - s0) / (2 * h) * U
            # collision: per term less than 1 for the truncation and less than 1 for f32 (the position is off by at most 8 * 2^-24, the interpolant
            # adds 2^-24 and c another 2^-25: 2 * 6e-7 * 2/3 * 2^20 = 0.84, the three products 3 * 2^-24 * 7e5 = 0.13); smoothness: exact
            assert abs(gc[0, i, ax] - fd_c) <= 2 * terms[i] + 1e-3, (i, ax, gc[0, i, ax], fd_c)
            assert abs(gs[0, i, ax] - fd_s) <= 1e-3, (i, ax, gs[0, i, ax], fd_s)
    assert abs(int(rec["cost_smooth"][0]) - cost(c[0])[1] * U) <= 1e-3 and abs(int(rec["cost_collision"][0]) - cost(c[0])[0] * U) <= 2 * S


def test_smoothness_stencil_by_hand():
    val, known = _wall()
    c = np.zeros((1, 5, 3), F32)
    c[0, :, 0] = (2, 2, 3, 2, 2)                  # a = 1, -2, 1: cost 6; gradients 2, -4 - 4, 2 + 8 + 2, -4 - 4, 2
    c[0, :, 1] = (0, 0.5, 1, 1.5, 2)              # straight: nothing
    rec, gc, gs = _lin(c, 0.5, 4, val, known)
    assert rec["n_pen"][0] == 0 and (gc == 0).all() and rec["cost_smooth"][0] == 6 * U
    assert gs[0, :, 0].tolist() == [2 * U, -8 * U, 12 * U, -8 * U, 2 * U] and (gs[0, :, 1:] == 0).all()
    # a length cuts the terms: L = 4 keeps a = 1, -2
    c6 = np.concatenate([c, c[:, -1:]], 1)
    rec, _, gs = _lin(c6, 0.5, 4, val, known, lengths=np.array([4]))
    assert rec["cost_smooth"][0] == 5 * U and gs[0, :, 0].tolist() == [2 * U, -8 * U, 10 * U, -4 * U, 0, 0]
    # the clamps: a = 2000 costs 1024^2 and every gradient term is +-1024
    c[0, :, 0] = (2, 2, 2002, 4002, 6002)         # a = 2000, 0, 0
    rec, _, gs = _lin(c, 0.5, 1, val, known)
    assert rec["cost_smooth"][0] == 2 ** 40 and gs[0, :, 0].tolist() == [2 ** 30, -(2 ** 30), 2 ** 30, 0, 0]


def test_movement_limits():
    val, known = _wall()
    rng = np.random.default_rng(7)
    c = np.zeros((4, 12, 3), F32)
    c[:, :, 0] = rng.uniform(0.05, 0.45, (4, 12))
    c[:, :, 1] = 0.3 * np.arange(12) - 1.5
    c[:, :, 2] = rng.uniform(-0.2, 0.2, (4, 12))
    ln = np.array([12, 12, 9, 7])
    c[2, 9:], c[3, 7:] = np.nan, 77.0             # rows past a length are copied through, whatever they hold
    out, rec, hist, _ = _opt(c, 0.5, 4, 0, val, known, lengths=ln)
    ref.assert_bits(out, c, "iters = 0")
    assert (rec["iters_done"] == 0).all() and hist.shape == (4, 1, 2) and np.array_equal(hist[:, 0, 0], rec["cost_collision"])
    lin = _lin(c, 0.5, 4, val, known, lengths=ln)[0]
    ref.assert_equal(rec, lin, "iters = 0 is the linearisation")
    mm = F32(0.01)
    out, rec, hist, n_clamped = _opt(c, 0.5, 4, 1, val, known, lengths=ln, w_smooth=0.0, step=10.0, max_move=mm, fix_head=3, fix_tail=2)
    for t, L in enumerate(ln):
        assert np.array_equal(out[t, :3].view(np.uint32), c[t, :3].view(np.uint32)) and np.array_equal(out[t, L - 2:].view(np.uint32), c[t, L - 2:].view(np.uint32))
        mid = slice(3, L - 2)
        # step 10 on gradients of about a metre: every x moves by exactly max_move, away from the wall
        assert np.array_equal(out[t, mid, 0], (c[t, mid, 0] + mm).astype(F32))
        assert (np.abs(out[t, mid].astype(np.float64) - c[t, mid]) <= float(mm) * (1 + 2.0 ** -20)).all()
    assert (n_clamped >= np.array([7, 7, 4, 2])).all() and (rec["iters_done"] == 1).all()
    out5, _, _, _ = _opt(c, 0.5, 4, 5, val, known, lengths=ln, w_smooth=0.0, step=10.0, max_move=mm, fix_head=3, fix_tail=2)
    assert (np.abs(out5[0].astype(np.float64) - c[0]) <= 5 * float(mm) * (1 + 2.0 ** -18)).all() and (out5[0, 3:10, 0] > out[0, 3:10, 0]).all()
    # everything fixed: nothing moves, whatever the gradients
    out, _, _, _ = _opt(c, 0.5, 4, 3, val, known, lengths=ln, fix_head=6, fix_tail=6)
    ref.assert_bits(out, c, "all fixed")
    # weights 0: nothing moves either
    out, _, _, _ = _opt(c, 0.5, 4, 3, val, known, lengths=ln, w_collision=0.0, w_smooth=0.0, fix_head=0, fix_tail=0)
    ref.assert_bits(out, c, "weights 0")


def test_unknown_outside_and_nan_points_are_counted_not_penalised():
    val, known = _wall()
    known[(np.arange(N) + LO[0]) >= 8] = False                                    # x >= 2 m is unknown
    c = np.zeros((1, 8, 3), F32)
    c[0, :, 0] = 0.3 + 0.7 * np.arange(8)
    # sub = 1: the 6 samples lie at control points 1 .. 6: x = 1.0 and 1.7 are known; 2.4 and 3.1 have a corner at x >= 2; 3.8 is in the last cell,
    # whose +1 corner leaves the volume, and 4.5 is beyond it
    rec, gc, gs = _lin(c, 1.2, 1, val, known, unknown=F32(-3.5))
    assert (rec["n_samples"][0], rec["n_pen"][0], rec["n_unknown"][0], rec["n_outside"][0], rec["argmin"][0]) == (6, 1, 2, 2, 0)
    assert abs(rec["min_dist"][0] - 1.0) <= 2.0 ** -22 and abs(int(rec["cost_collision"][0]) - 0.04 * U) <= 2
    assert (gc[0, 4:] == 0).all() and (gc[0, :3, 0] < 0).all()
    assert (np.abs(gs) <= 8).all()                # 0.3 + 0.7 i is not exact in f32: a is off by up to an ulp of 5.2, 4 a by 2 units, three terms
    # nothing known: no status-0 sample at all
    rec, gc, _ = _lin(c, 1.2, 1, val, np.zeros_like(known))
    assert (rec["n_unknown"][0], rec["n_outside"][0], rec["n_pen"][0], rec["argmin"][0]) == (4, 2, 0, -1) and np.isposinf(rec["min_dist"][0]) and (gc == 0).all()
    # a NaN value or a NaN gradient makes a sample unknown
    nv = val.copy()
    nv[16 + 4, 16, 16] = np.nan                                                   # the voxel at (1, 0, 0): a corner of the cell of sample 0
    rec, gc, _ = _lin(c, 1.2, 1, nv, np.ones_like(known))
    assert (rec["n_unknown"][0], rec["n_pen"][0]) == (1, 0) and (gc == 0).all() and rec["argmin"][0] == 1
    # a NaN control point: every sample whose span holds it is outside, every smoothness term that holds it is skipped
    val, known = _wall()
    c = np.zeros((1, 10, 3), F32)
    c[0, :, 0] = 0.2
    c[0, :, 1] = 0.25 * np.arange(10)
    c[0, 1, 1] = 0.75                                                             # a bend at the head, on the axis of the NaN
    c[0, 4, 1] = np.nan
    rec, gc, gs = _lin(c, 0.5, 2, val, known)
    S = 15                                                                        # span 0 (samples 0, 1) is free of point 4; spans 1 .. 4 (samples 2 .. 9) hold it
    assert (rec["n_samples"][0], rec["n_outside"][0], rec["n_pen"][0], rec["n_unknown"][0]) == (S, 8, 7, 0)
    # y: a_0 = (0 - 1.5) + 0.5 = -1, a_1 = (0.75 - 1) + 0.75 = 0.5, the terms 2, 3, 4 are skipped, the rest is straight
    assert gs[0, :, 1].tolist() == [-2 * U, 5 * U, -4 * U, U] + [0] * 6 and (gs[0, :, (0, 2)] == 0).all()
    out, rec, _, _ = _opt(c, 0.5, 2, 6, val, known, w_collision=0.0, fix_head=0, fix_tail=0)
    assert np.isnan(out[0, 4, 1]) and np.array_equal(out[0, 4, (0, 2)], c[0, 4, (0, 2)])
    ref.assert_bits(out[:, 5:], c[:, 5:], "behind the NaN point nothing pulls")
    assert (out[0, :4, 1] != c[0, :4, 1]).all() and np.array_equal(out[0, :, 0], c[0, :, 0])
    out, rec, _, _ = _opt(c, 0.5, 2, 3, val, known, w_smooth=0.0, fix_head=0, fix_tail=0, max_move=0.01)
    assert np.isnan(out[0, 4, 1]) and (out[0, (0, 1, 2, 3, 5, 6, 7, 8, 9), 0] > F32(0.2)).all() and out[0, 4, 0] == F32(0.2)


def _sphere():
    """the analytic distance to a sphere of 0.8 m on a 64^3 grid of 0.1 m, every voxel known"""
    i = (np.arange(64) - 32) * 0.1
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - 0.8).astype(F32), np.ones((64, 64, 64), bool), np.array([-32, -32, -32], np.int64)


def test_convergence_on_the_analytic_sphere():
    val, known, lo = _sphere()
    c = np.zeros((1, 24, 3), F32)
    c[0, :, 0] = np.linspace(-2.3, 2.3, 24)
    c[0, :, 1], c[0, :, 2] = 0.15, 0.1                                            # beside the centre: on the axis the gradient has no lateral part
    kw = dict(w_collision=1.0, w_smooth=1.0, step=0.05, momentum=0.8, max_move=0.05, fix_head=3, fix_tail=3)
    start = ref.linearize(c, 0.4, 4, None, F32(0.1), val, known, lo)[0]
    assert start["n_pen"][0] > 20 and start["min_dist"][0] < -0.5 and start["n_unknown"][0] == 0 and start["n_outside"][0] == 0
    out, rec, hist, _ = ref.optimize(c, 0.4, 4, 50, None, F32(0.1), val, known, lo, **kw)
    print(f"sphere: n_pen {start['n_pen'][0]} -> {rec['n_pen'][0]}, min_dist {start['min_dist'][0]:.3f} -> {rec['min_dist'][0]:.3f}, history {hist[0, ::10, 0].tolist()}")
    # the trajectory is free WITHIN iters: the first free linearisation is where stop_when_free ends.  Without the stop the descent goes on to the
    # balance of the two terms, where the smoothness holds a few samples a centimetre inside the clearance: a soft penalty, as in the planners
    assert rec["iters_done"][0] == 50 and rec["n_unknown"][0] == 0 and rec["min_dist"][0] > F32(0.35) and rec["cost_collision"][0] < start["cost_collision"][0] // 10000
    assert hist.shape == (1, 51, 2) and (hist >= 0).all() and hist[0, 0, 0] == start["cost_collision"][0] and hist[0, 0, 1] == 0
    assert (hist[0, 50] == (rec["cost_collision"][0], rec["cost_smooth"][0])).all()
    free = np.nonzero(hist[0, :, 0] == 0)[0][0]
    assert 0 < free <= 50
    ref.assert_bits(out[:, :3], c[:, :3], "fixed head")
    ref.assert_bits(out[:, -3:], c[:, -3:], "fixed tail")
    # stop_when_free: iters_done is the first free linearisation, the history ends there and the control points are those of that step
    out2, rec2, hist2, _ = ref.optimize(c, 0.4, 4, 50, None, F32(0.1), val, known, lo, flags=ref.STOP_FREE, **kw)
    assert rec2["iters_done"][0] == free and rec2["n_pen"][0] == 0 and rec2["min_dist"][0] >= F32(0.4) and rec2["n_unknown"][0] == 0 and np.array_equal(hist2[0, :free + 1], hist[0, :free + 1]) and (hist2[0, free + 1:] == -1).all()
    out3, rec3, _, _ = ref.optimize(c, 0.4, 4, int(free), None, F32(0.1), val, known, lo, **kw)
    ref.assert_bits(out2, out3, "stopped = as many iterations")
    ref.assert_equal(rec2, rec3, "stopped = as many iterations")
    # the result re-checked by the path scoring's restatement at the same samples
    import path_score_ref as pref
    p = nav.bspline_points(out2, 4)
    ps = pref.score(p, 0.4, 0.0, 1, None, 1, 6, F32(0.1), val, known, lo)[0]
    assert ps["first_stop"][0] == -1 and ps["argmin"][0] == rec2["argmin"][0] and ps["min_dist"][0] == rec2["min_dist"][0]


def test_bspline_from_path():
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 2, 0]], np.float64)     # length 3, a repeated point
    c = nav.bspline_from_path(pts, 11)
    assert c.shape == (11, 3) and c.dtype == F32
    assert (c[:3] == pts[0]).all() and (c[-3:] == pts[-1]).all()
    assert np.allclose(c[2:9], [[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [1, 0.5, 0], [1, 1, 0], [1, 1.5, 0], [1, 2, 0]], atol=1e-6)
    p = nav.bspline_points(c, 4)
    assert (p[0] == pts[0]).all() and np.abs(p[-1] - pts[-1]).max() < 1e-6      # the spline starts and ends at the ends of the path
    assert (nav.bspline_from_path(pts[:1], 6) == pts[0]).all()


def test_abi_and_header():
    from taichislam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("tsl_esdf_traj_linearize", "tsl_esdf_traj_linearize_dev", "tsl_esdf_traj_optimize", "tsl_esdf_traj_optimize_dev"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert re.search(r"TSL_K_NAV_TERRAIN_WINDOW = 29,\s*TSL_K_COUNT\b", code)      # the kernel-id enum ends where it did
    import ctypes as C
    from taichislam_amd.mapping import dense_tsdf
    assert C.sizeof(_lib.TrajScore) == 48 == dense_tsdf.TRAJ_SCORE_DTYPE.itemsize and C.sizeof(_lib.TrajOpt) == 48
    for name, _ in _lib.TrajScore._fields_:
        assert getattr(_lib.TrajScore, name).offset == dense_tsdf.TRAJ_SCORE_DTYPE.fields[name][1], name
    assert tuple(dense_tsdf.TRAJ_SCORE_DTYPE.names) == ref.FIELDS
    m = re.search(r"typedef struct \{([^}]*)\} tsl_traj_score;", code)
    assert [w for w in re.findall(r"\b[a-z_0-9]+\b", m.group(1)) if w not in ("int32_t", "int64_t", "float")] == list(ref.FIELDS)

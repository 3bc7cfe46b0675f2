"""The numpy restatement of the path scoring (tests/path_score_ref.py) on hand-built dense grids whose answers are worked out by hand here: it is what
the GPU tests compare the kernel with (tests/test_path_score_gpu.py), so it is checked on its own first.  No GPU."""
import numpy as np

import path_score_ref as ref

F32 = np.float32
VS = F32(0.25)
N = 32                                   # voxel indices -16 .. 15: x in [-4, 3.75]
LO = np.array([-16, -16, -16], np.int64)
ALL = ref.UNKNOWN_BLOCKS | ref.OUTSIDE_BLOCKS


def _wall():
    """val = x: a wall at x = 0, free space at x > 0; every voxel known.  The trilinear value at a point with y = z = 0 is x exactly (quarter metres)."""
    i = np.arange(N) + LO[0]
    val = np.broadcast_to((i.astype(F32) * VS)[:, None, None], (N, N, N)).copy()
    return val, np.ones((N, N, N), bool)


def _line(x0, x1, k):
    w = np.zeros((1, k, 3), F32)
    w[0, :, 0] = np.linspace(x0, x1, k).astype(F32)
    return w


def _score(w, radius, margin, sub, flags, val, known, mode=1, lengths=None, unknown=np.nan):
    return ref.score(w, radius, margin, sub, lengths, mode, flags, VS, val, known, LO, unknown)


def _one(rec):
    return {k: v[0] for k, v in rec.items()}


def test_straight_path_into_a_wall():
    val, known = _wall()
    w = _line(2.0, -1.0, 7)                       # waypoints every 0.5 m; sub = 2: samples x_j = 2 - 0.25 j, j = 0 .. 12, all exact
    rec, sd, ss = _score(w, 0.5, 0.5, 2, ALL, val, known)
    assert np.array_equal(sd[0], (2.0 - 0.25 * np.arange(13)).astype(F32)) and (ss == 0).all()
    r = _one(rec)
    # d < 0.5 first at x = 0.25 (j = 7); hits are j = 7 .. 12; the least value is the last sample; rm = 1: c_j = 1 - x_j > 0 for j = 5 .. 12,
    # 0.25 + 0.5 + .. + 2.0 = 9 m = 9 * 2^20
    assert (r["n_samples"], r["first_stop"], r["n_hit"], r["n_unknown"], r["n_outside"]) == (13, 7, 6, 0, 0)
    assert r["argmin"] == 12 and r["min_dist"] == F32(-1.0) and r["cost"] == 9 * 2 ** 20 and r["short_update"] == 0
    rec, sd, ss = _score(w, 0.5, 0.5, 2, ALL | ref.STOP, val, known, unknown=F32(-7.0))
    r = _one(rec)
    # stop: samples 0 .. 7 are counted; one hit; the least value is 0.25 at j = 7; c = 0.25 + 0.5 + 0.75 = 1.5 m
    assert (r["n_samples"], r["first_stop"], r["n_hit"], r["n_unknown"], r["n_outside"]) == (8, 7, 1, 0, 0)
    assert r["argmin"] == 7 and r["min_dist"] == F32(0.25) and r["cost"] == 3 * 2 ** 19
    assert (ss[0, :8] == 0).all() and (ss[0, 8:] == 0xff).all() and (sd[0, 8:] == F32(-7.0)).all() and sd[0, 7] == F32(0.25)


def test_outside_and_unknown_block_only_when_asked():
    val, known = _wall()
    known[:, :, :] = True
    known[(np.arange(N) + LO[0]) >= 8] = False                                   # x >= 2 m is unknown
    # x = 5, 4.5, 4: outside (the +1 corner of the cell leaves the volume at x >= 3.75); 3.5 .. 2: unknown (a corner at x >= 2); 1.5, 1: free
    w = _line(5.0, 1.0, 9)
    rec, _, ss = _score(w, 0.5, 0.0, 1, 0, val, known)
    assert list(ss[0]) == [2, 2, 2, 1, 1, 1, 1, 0, 0]
    r = _one(rec)
    assert (r["first_stop"], r["n_outside"], r["n_unknown"], r["n_hit"], r["argmin"], r["min_dist"]) == (-1, 3, 4, 0, 8, F32(1.0))
    assert _one(_score(w, 0.5, 0.0, 1, ref.UNKNOWN_BLOCKS, val, known)[0])["first_stop"] == 3
    assert _one(_score(w, 0.5, 0.0, 1, ref.OUTSIDE_BLOCKS, val, known)[0])["first_stop"] == 0
    r = _one(_score(w, 0.5, 0.0, 1, ref.UNKNOWN_BLOCKS | ref.STOP, val, known)[0])
    assert (r["n_samples"], r["n_outside"], r["n_unknown"], r["argmin"], r["cost"]) == (4, 3, 1, -1, 0) and np.isposinf(r["min_dist"])


def test_ties_go_to_the_lowest_index_and_minus_zero_sorts_first():
    val = np.full((N, N, N), F32(0.75), F32)
    known = np.ones((N, N, N), bool)
    w = _line(-1.0, 1.0, 9)
    r = _one(_score(w, 0.5, 0.0, 1, ALL, val, known, mode=0)[0])
    assert r["argmin"] == 0 and r["min_dist"] == F32(0.75) and r["first_stop"] == -1
    val[:] = F32(0.0)
    val[16 + 2, 16, 16] = F32(-0.0)               # the voxel at x = 0.5: sample 6 of x = -1, -0.75, .., 1
    r = _one(_score(w, 0.5, 0.0, 1, ALL, val, known, mode=0)[0])
    assert r["argmin"] == 6 and np.float32(r["min_dist"]).view(np.uint32) == 0x80000000 and r["first_stop"] == 0
    assert ref.key(np.array([-0.0, 0.0, -1.0, 1.0, -np.inf, np.inf], F32)).tolist() == [0x7fffffff, 0x80000000, 0x407fffff, 0xbf800000, 0x007fffff, 0xff800000]
    assert np.array_equal(ref.unkey(ref.key(np.array([-0.0, 0.0, -1.5, 3.0], F32))).view(np.uint32), np.array([-0.0, 0.0, -1.5, 3.0], F32).view(np.uint32))


def test_a_nan_value_counts_as_unknown():
    val, known = _wall()
    val[16 + 4, 16, 16] = np.nan                  # the voxel at x = 1
    w = _line(2.0, 0.5, 7)                        # x = 2, 1.75, .., 0.5: sample 4 reads the NaN voxel
    rec, sd, ss = _score(w, 0.25, 0.0, 1, ALL, val, known, mode=0, unknown=F32(-3.5))
    r = _one(rec)
    assert list(ss[0]) == [0, 0, 0, 0, 1, 0, 0] and sd[0, 4] == F32(-3.5)
    assert (r["first_stop"], r["n_unknown"], r["n_hit"], r["argmin"], r["min_dist"]) == (4, 1, 0, 6, F32(0.5))
    # trilinear: the two cells along x that have the voxel as a corner
    rec, sd, ss = _score(w, 0.25, 0.0, 1, 0, val, known, mode=1, unknown=F32(-3.5))
    assert list(ss[0]) == [0, 0, 0, 0, 1, 1, 0] and _one(rec)["n_unknown"] == 2 and _one(rec)["first_stop"] == -1


def test_a_path_of_one_waypoint_and_sub_one():
    val, known = _wall()
    w = _line(1.0, -1.0, 5)                       # x = 1, 0.5, 0, -0.5, -1
    r = _one(_score(w, 0.75, 0.25, 3, ALL, val, known, lengths=np.array([1]))[0])
    assert (r["n_samples"], r["first_stop"], r["n_hit"], r["argmin"], r["min_dist"], r["cost"]) == (1, -1, 0, 0, F32(1.0), 0)
    rec, sd, ss = _score(w, 0.75, 0.25, 3, ALL, val, known, lengths=np.array([1]))
    assert sd.shape == (1, 13) and (ss[0, 1:] == 0xff).all() and np.isnan(sd[0, 1:]).all()
    rec, sd, ss = _score(w, 0.75, 0.25, 1, ALL, val, known)
    assert np.array_equal(sd[0], w[0, :, 0]) and (ss == 0).all()                 # sub = 1: the samples are the waypoints
    r = _one(rec)
    # hits x = 0.5, 0, -0.5, -1; rm = 1: c = 0.5 + 1 + 1.5 + 2 = 5 m
    assert (r["n_samples"], r["first_stop"], r["n_hit"], r["argmin"], r["cost"]) == (5, 1, 4, 4, 5 * 2 ** 20)
    # lengths cut the path: the waypoints behind it may hold anything
    w2 = np.concatenate([w, w], 0)
    w2[1, 3:] = np.nan
    rec, _, _ = _score(w2, 0.75, 0.25, 1, ALL, val, known, lengths=np.array([5, 3]))
    assert rec["n_samples"].tolist() == [5, 3] and rec["n_outside"].tolist() == [0, 0] and rec["argmin"].tolist() == [4, 2]


def test_the_waypoint_itself_when_the_next_one_is_not_finite():
    val, known = _wall()
    w = np.zeros((1, 2, 3), F32)
    w[0, 0] = (1.25, 0.0, 0.0)
    w[0, 1] = (np.inf, 0.0, 0.0)
    p, valid = ref.sample_points(w, 2)
    assert valid.all() and np.array_equal(p[0, 0].view(np.uint32), w[0, 0].view(np.uint32)) and not np.isfinite(p[0, 1, 0]) and np.isposinf(p[0, 2, 0])
    rec, sd, ss = _score(w, 0.5, 0.0, 2, ref.OUTSIDE_BLOCKS, val, known)
    r = _one(rec)
    assert list(ss[0]) == [0, 2, 2] and sd[0, 0] == F32(1.25)
    assert (r["first_stop"], r["n_outside"], r["argmin"], r["min_dist"]) == (1, 2, 0, F32(1.25))


def test_the_stop_flag_keeps_first_stop_and_changes_nothing_on_free_paths():
    val, known = _wall()
    rng = np.random.default_rng(1)
    w = rng.uniform(-1.5, 3.0, (200, 6, 3)).astype(F32)
    w[:, :, 1:] *= F32(0.3)
    w[:50, :, 0] = np.abs(w[:50, :, 0]) * F32(0.5) + F32(0.8)                    # free paths: 0.8 <= x <= 2.3
    for flags in (0, ref.UNKNOWN_BLOCKS, ALL):
        a, _, _ = _score(w, 0.5, 0.5, 4, flags, val, known)
        b, _, _ = _score(w, 0.5, 0.5, 4, flags | ref.STOP, val, known)
        assert np.array_equal(a["first_stop"], b["first_stop"])
        free = a["first_stop"] < 0
        assert free.sum() >= 50 and (~free).sum() >= 50
        for k in ref.FIELDS:
            assert np.array_equal(a[k][free], b[k][free]), k
        assert np.array_equal(b["n_samples"][~free], b["first_stop"][~free] + 1)
        assert (b["cost"] <= a["cost"]).all() and (b["n_hit"][~free] <= 1).all()


def test_the_cost_term_is_clamped_at_1024():
    val = np.full((N, N, N), F32(-2000.0), F32)
    known = np.ones((N, N, N), bool)
    w = _line(0.0, 0.5, 3)
    r = _one(_score(w, 0.5, 0.5, 1, 0, val, known, mode=0)[0])
    assert r["cost"] == 3 * 2 ** 30 and r["n_hit"] == 3                          # min(1 + 2000, 1024) * 2^20 per sample
    val[:] = F32(-1022.5)
    r = _one(_score(w, 0.5, 0.5, 1, 0, val, known, mode=0)[0])
    assert r["cost"] == 3 * 2047 * 2 ** 19                                       # 1023.5 m, below the clamp
    val[:] = F32(1.0)
    r = _one(_score(w, 0.5, 0.5, 1, 0, val, known, mode=0)[0])
    assert r["cost"] == 0                                                        # c = 0 is not counted
    val[:] = F32(0.9999995)
    r = _one(_score(w, 0.5, 0.5, 1, 0, val, known, mode=0)[0])
    assert r["cost"] == 0                                                        # c = 2^-21 truncates to 0

"""B-spline trajectory linearisation and descent on the GPU (tsl_traj_opt.hip): records, both gradient planes, control points and histories bit for bit
against the numpy restatement (tests/traj_opt_ref.py) over the oracle's ESDF; the records against score_paths at the same samples; a spline seeded along
a path that ends free; an imported NaN; the device form against the host form with work in flight; a volume with N != Nz; and the refusals.  The scene is the one of
tests/test_path_score_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import esdf_query_ref as qref
import traj_opt_ref as ref
from util import SLAB, SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

UNK = np.float32(-3.5)
CLEAR = 0.3
_CACHE = {}


@pytest.fixture(autouse=True, params=[1, 0], ids=["wavefront", "regional"])
def esdf_mode(request, monkeypatch):
    """Every test runs for both forms of the incremental update (esdf_mode 1 and 0), as tests/test_path_score_gpu.py does."""
    monkeypatch.setenv("TSL_ESDF_MODE", str(request.param))
    return request.param


def oracle_grid(cfg=SMALL, name="grid", nframes=2, max_dist=2.0):
    """(val, known, lo) of the oracle's BATCHED ESDF after nframes frames, computed once and shared (it does not depend on the form of the update); no GPU"""
    if name not in _CACHE:
        from oracle import BATCHED, OracleTSDF
        K, frames = small_stream(nframes)
        o = OracleTSDF(**cfg)
        o.set_intrinsics(K, K)
        for R, T, d in frames:
            o.integrate_depth(R, T, d, mode=BATCHED)
        oi, oe = o.esdf(max_dist=max_dist)
        vs = cfg["voxel_scale"]
        _CACHE[name] = qref.grid_from_export(oi, oe, int(round(cfg["map_scale"][0] / vs)), int(round(cfg["map_scale"][1] / vs)))
        for a in _CACHE[name]:
            a.setflags(write=False)
    return _CACHE[name]


def _scene(cfg=SMALL, name="grid", nframes=2, max_dist=2.0):
    K, frames = small_stream(nframes)
    g, _ = make_pair(cfg, K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    g.update_esdf(max_dist=max_dist)
    val, known, lo = oracle_grid(cfg, name, nframes, max_dist)
    assert val.shape == (g.N, g.N, g.Nz)
    return g, val, known, lo


def polygons(val, known, lo, vs, rng, n, K, bad=8):
    """n control polygons of K points, random walks like walks() of tests/test_path_score_gpu.py with steps of 2 to 6 voxels: two in three start at a known
    voxel within 0.5 m of a surface and keep a heading (they run along walls, into them and into the unknown), one in three starts up to 12 voxels outside
    the volume and walks in; `bad` of them hold NaN / inf points, first, middle and last"""
    half = np.array(val.shape) // 2
    near = np.argwhere(known & (val > 0.05) & (val < 0.5)) + lo
    start = (near[rng.integers(0, len(near), n)] + rng.uniform(-0.5, 0.5, (n, 3))) * vs
    out = rng.random(n) < 0.34
    ax = rng.integers(0, 3, n)
    beyond = rng.choice([-1.0, 1.0], n) * (half[ax] + rng.uniform(0.0, 12.0, n)) * vs
    start[out, ax[out]] = beyond[out]
    head = rng.normal(size=(n, 3))
    head[out] = -start[out] + rng.normal(size=(int(out.sum()), 3))
    c = np.empty((n, K, 3))
    c[:, 0] = start
    for k in range(1, K):
        head = head / np.linalg.norm(head, axis=1, keepdims=True) + 0.3 * rng.normal(size=(n, 3))
        c[:, k] = c[:, k - 1] + head / np.linalg.norm(head, axis=1, keepdims=True) * (rng.uniform(2.0, 6.0, n) * vs)[:, None]
    c = c.astype(np.float32)
    for i, b in enumerate(rng.choice(n, min(bad, n), replace=False) if bad else ()):
        c[b, (0, K // 2, K - 1, 1)[i % 4], i % 3] = (np.nan, np.inf, -np.inf, np.nan)[i % 4]
    return c


# name: (seed, n, K, subs, lengths, NaN / inf polygons).  n = 1, 4, 5 and 203 (a partial workgroup); K = 4 (one span), 5, 64 / 65 (control points past
# one lane set), 67 / 68 (S = 64 / 65 at sub = 1), 256; K = 19 at sub = 4 has S = 65; mixed lengths hold 4.  The seeds are chosen on the restatement (no GPU):
# the main batch meets check_purpose(), every small batch has penalised, unknown and (but for k4) outside samples
BATCHES = {
    "main": (31, 203, 19, (1, 4, 16), "mixed", 8),
    "k4": (32, 1, 4, (1, 4), None, 0),
    "k5": (143, 4, 5, (1, 16), None, 1),
    "k64": (64, 5, 64, (1,), None, 1),
    "k65": (55, 5, 65, (4,), "mixed", 0),
    "k67": (56, 4, 67, (1,), None, 1),
    "k68": (37, 5, 68, (1,), None, 0),
    "k256": (38, 5, 256, (1, 4), "mixed", 1),
}


def batch(name):
    if ("batch", name) not in _CACHE:
        seed, n, K, subs, lengths, bad = BATCHES[name]
        val, known, lo = oracle_grid()
        rng = np.random.default_rng(seed)
        c = polygons(val, known, lo, SMALL["voxel_scale"], rng, n, K, bad)
        ln = None
        if lengths:
            ln = rng.integers(4, K + 1, n).astype(np.int32)
            ln[: (2 * n) // 3] = K                                                # most are whole
            ln[-1] = 4
        c.setflags(write=False)
        _CACHE["batch", name] = (c, ln, subs)
    return _CACHE["batch", name]


def ref_linearize(name, sub):
    k = ("lin", name, sub)
    if k not in _CACHE:
        c, ln, _ = batch(name)
        val, known, lo = oracle_grid()
        _CACHE[k] = ref.linearize(c, CLEAR, sub, ln, np.float32(SMALL["voxel_scale"]), val, known, lo, UNK)
    return _CACHE[k]


def ref_optimize(name, sub, iters, stop, fix):
    k = ("opt", name, sub, iters, stop, fix)
    if k not in _CACHE:
        c, ln, _ = batch(name)
        val, known, lo = oracle_grid()
        _CACHE[k] = ref.optimize(c, CLEAR, sub, iters, ln, np.float32(SMALL["voxel_scale"]), val, known, lo, fix_head=fix, fix_tail=fix,
                                 flags=ref.STOP_FREE if stop else 0, unknown=UNK)
    return _CACHE[k]


def check_purpose():
    """conditions on the restatement alone: the main batch reaches what it is there for (also run without a GPU when the seed is chosen)"""
    seen = {}
    for sub in BATCHES["main"][3]:
        rec = ref_linearize("main", sub)[0]
        out, end, hist, n_clamped = ref_optimize("main", sub, 25, False, 0)        # with free ends: a polygon whose fixed ends are too close stays so
        _, stopped, _, _ = ref_optimize("main", sub, 25, True, 0)
        seen[sub] = dict(pen=int((rec["n_pen"] > 0).sum()), unknown=int((rec["n_unknown"] > 0).sum()), outside=int((rec["n_outside"] > 0).sum()),
                         end_free=int(((rec["n_pen"] > 0) & (end["n_pen"] == 0)).sum()), clamped=int((n_clamped > 0).sum()),
                         early=int(((stopped["iters_done"] > 0) & (stopped["iters_done"] < 25)).sum()), at_once=int((stopped["iters_done"] == 0).sum()))
    for sub, s in seen.items():
        assert s["pen"] >= 50 and s["unknown"] >= 50 and s["outside"] >= 50 and s["end_free"] >= 20 and s["clamped"] >= 20 and s["early"] >= 5, (sub, s)
    return seen


def _np(r):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


@pytest.mark.parametrize("name", list(BATCHES))
def test_equals_the_restatement_over_the_oracle(hip_lib, name):
    g, val, known, lo = _scene()
    c, ln, subs = batch(name)
    if name == "main":
        print(check_purpose())
        assert sorted(((ln.astype(np.int64) - 3) * 4 + 1).tolist())[-1] == 65 and ln.min() == 4
    for sub in subs:
        want, wgc, wgs = ref_linearize(name, sub)
        got = g.traj_linearize(c, CLEAR, sub=sub, lengths=ln, unknown_value=UNK, refresh=False)
        ref.assert_equal(got, want, f"{name}, sub {sub}, linearize")
        ref.assert_bits(got["grad_collision"], wgc, f"{name}, sub {sub}, grad_collision")
        ref.assert_bits(got["grad_smooth"], wgs, f"{name}, sub {sub}, grad_smooth")
        plain = g.traj_linearize(c, CLEAR, sub=sub, lengths=ln, gradients=False, unknown_value=UNK, refresh=False)
        assert "grad_collision" not in plain
        ref.assert_equal(plain, want, f"{name}, sub {sub}, linearize without gradients")
        for iters in (0, 1, 25):
            for stop in (False, True):
                for fix in (0, min(3, c.shape[1] // 2)):                   # fix_head + fix_tail <= K
                    what = f"{name}, sub {sub}, iters {iters}, stop {stop}, fix_ends {fix}"
                    wout, wrec, whist, _ = ref_optimize(name, sub, iters, stop, fix)
                    got = g.traj_optimize(c, CLEAR, sub=sub, iters=iters, fix_ends=fix, stop_when_free=stop, history=True, lengths=ln, unknown_value=UNK,
                                          refresh=False)
                    ref.assert_equal(got, wrec, what)
                    ref.assert_bits(got["ctrl"], wout, what + ", ctrl")
                    ref.assert_bits(got["history"], whist, what + ", history")
                    if iters == 0:
                        ref.assert_bits(got["ctrl"], c, what + ": the identity")
    one = g.traj_optimize(c[0], CLEAR, sub=subs[0], iters=1, fix_ends=1, lengths=None, unknown_value=UNK, refresh=False)      # a [K, 3] input is one trajectory
    assert one["ctrl"].shape == c[0].shape and one["n_samples"].shape == (1,) and "history" not in one


def test_records_equal_score_paths_at_the_same_samples(hip_lib):
    from taichislam_amd.utils import bspline_points
    g, val, known, lo = _scene()
    vs = np.float32(g.voxel_scale)
    c, ln, _ = batch("main")
    for sub in (1, 4, 16):
        d, grad, st, valid, _, _ = ref.sample_values(c, sub, ln, vs, val, known, lo, UNK)
        pd, _, pst = qref.query(ref.sample_points(c, sub, ln)[0][valid], 1, vs, val, known, lo, unknown=UNK)
        # no sample became unknown through its gradient alone: then the two calls count the same samples (asserted on the restatement)
        assert np.array_equal(st[valid] == 0, (pst == 0) & ~np.isnan(pd)) and (st[valid] == 0).sum() > 400
        got = g.traj_linearize(c, CLEAR, sub=sub, lengths=ln, gradients=False, unknown_value=UNK, refresh=False)
        p = bspline_points(c, sub, ln)
        ps = g.score_paths(p, CLEAR, sub=1, lengths=(ln.astype(np.int64) - 3) * sub + 1, unknown_blocks=False, outside_blocks=False, unknown_value=UNK,
                           refresh=False)
        for a, b in (("n_samples", "n_samples"), ("n_pen", "n_hit"), ("n_unknown", "n_unknown"), ("n_outside", "n_outside"), ("argmin", "argmin")):
            assert np.array_equal(got[a], ps[b]), (sub, a)
        assert np.array_equal(got["min_dist"].view(np.uint32), ps["min_dist"].view(np.uint32))
        assert (got["n_pen"] > 0).sum() >= 50 and (got["argmin"] > 0).sum() >= 50


def _bent_candidates(val, known, lo, vs, rng, n, K):
    """(splines, their first linearisation): seeded with bspline_from_path along A - M - B -- A and B known voxels at least 0.45 m from every surface, M a
    known free voxel 0.1 to 0.2 m from one, 0.35 to 0.7 m apart -- and kept when every sample is known and more than 3 are penalised"""
    from taichislam_amd.utils import bspline_from_path
    far = (np.argwhere(known & (val > 0.45) & (val < 1.5)) + lo) * vs
    close = (np.argwhere(known & (val > 0.1) & (val < 0.2)) + lo) * vs
    out = []
    while len(out) < 1500:
        m = close[rng.integers(len(close))]
        r = np.linalg.norm(far - m, axis=1)
        ok = far[(r > 0.35) & (r < 0.7)]
        if len(ok) >= 2:
            a, b = ok[rng.integers(len(ok), size=2)]
            if np.linalg.norm(a - b) > 0.4:
                out.append(bspline_from_path(np.array([a, m, b]), K))
    out = np.array(out)
    start = ref.linearize(out, CLEAR, 4, None, np.float32(vs), val, known, lo, UNK)[0]
    keep = np.nonzero((start["n_pen"] > 3) & (start["n_unknown"] == 0) & (start["n_outside"] == 0))[0][:n]
    return out[keep], {k: v[keep] for k, v in start.items()}


def test_a_spline_seeded_along_a_path_ends_free(hip_lib):
    from taichislam_amd.utils import bspline_points
    g, val, known, lo = _scene()
    vs = np.float32(g.voxel_scale)
    kw = dict(sub=4, iters=60, step=0.05, momentum=0.8, max_move=0.02, fix_ends=3)
    if "bent" not in _CACHE:
        cand, start = _bent_candidates(val, known, lo, float(vs), np.random.default_rng(9), 24, 16)
        out, rec, _, _ = ref.optimize(cand, CLEAR, 4, 60, None, vs, val, known, lo, step=0.05, momentum=0.8, max_move=0.02, flags=ref.STOP_FREE, unknown=UNK)
        good = np.nonzero((rec["n_pen"] == 0) & (rec["n_unknown"] == 0) & (rec["n_outside"] == 0))[0]       # chosen from the restatement, on the CPU
        assert len(cand) >= 10 and good.size >= 5, (len(cand), start["n_pen"], rec["n_pen"], rec["n_unknown"])
        _CACHE["bent"] = (cand[good], out[good], {k: v[good] for k, v in rec.items()})
    cand, wout, wrec = _CACHE["bent"]
    got = g.traj_optimize(cand, CLEAR, stop_when_free=True, unknown_value=UNK, refresh=False, **kw)
    ref.assert_equal(got, wrec, "seeded along a path")
    ref.assert_bits(got["ctrl"], wout, "seeded along a path, ctrl")
    assert (got["n_pen"] == 0).all() and (got["n_unknown"] == 0).all() and (got["iters_done"] > 0).all() and (got["min_dist"] >= np.float32(CLEAR)).all()
    # and the path scoring agrees that the result is free
    ps = g.score_paths(bspline_points(got["ctrl"], 4), CLEAR, sub=1, unknown_value=UNK, refresh=False)
    assert (ps["first_stop"] == -1).all() and np.array_equal(ps["min_dist"].view(np.uint32), got["min_dist"].view(np.uint32))


def test_imported_nan_counts_as_unknown(hip_lib):
    """a NaN TSDF that came in through load_numpy: the point query reports sign(NaN) * magnitude = 0 there, the trajectory samples that read such a
    voxel are unknown and pull nowhere (the scene of the same test of tests/test_path_score_gpu.py)"""
    g, val, known, lo = _scene()
    vs = np.float32(g.voxel_scale)
    e = g.export_submap()
    idx = e["indices"].astype(np.int64)
    free = np.argwhere(known & (val > 0.8)) + lo
    ctr = free[len(free) // 2]
    ball = ((idx - ctr) ** 2).sum(1) <= 9                                        # a ball of 3 voxels around a free voxel
    assert 50 < ball.sum() < 200
    t = np.asarray(e["TSDF"]).copy()
    t[ball] = np.nan
    h, _ = make_pair(SMALL, small_stream(1)[0])
    h.load_numpy(h.get_active_submap_id(), e["indices"], t, e["W_TSDF"], e["occupy"], np.array([]))
    h.update_esdf(max_dist=2.0)
    hi, he = h.export_esdf()
    hval, hknown, hlo = qref.grid_from_export(hi, he, h.N, h.Nz)
    bi = idx[ball] - hlo
    nknown = hknown.copy()
    nknown[bi[:, 0], bi[:, 1], bi[:, 2]] = False
    rng = np.random.default_rng(2)
    a = (ctr + rng.normal(size=(100, 3)) * 12.0) * vs                            # straight splines through the ball
    b = 2.0 * ctr * vs - a
    c = (a[:, None, :] + (b - a)[:, None, :] * np.linspace(0.0, 1.0, 9)[None, :, None]).astype(np.float32)
    clear = 1.5                                                                  # the samples around the ball are penalised
    want, wgc, wgs = ref.linearize(c, clear, 4, None, vs, hval, nknown, hlo, UNK)
    plain = ref.linearize(c, clear, 4, None, vs, hval, hknown, hlo, UNK)[0]
    assert (want["n_unknown"] > plain["n_unknown"]).sum() >= 80 and (want["n_pen"] > 0).sum() >= 80
    got = h.traj_linearize(c, clear, sub=4, unknown_value=UNK, refresh=False)
    ref.assert_equal(got, want, "imported NaN")
    ref.assert_bits(got["grad_collision"], wgc, "imported NaN, grad_collision")
    wout, wrec, _, _ = ref.optimize(c, clear, 4, 5, None, vs, hval, nknown, hlo, fix_head=0, fix_tail=0, unknown=UNK)
    got = h.traj_optimize(c, clear, sub=4, iters=5, fix_ends=0, unknown_value=UNK, refresh=False)
    ref.assert_equal(got, wrec, "imported NaN, optimize")
    ref.assert_bits(got["ctrl"], wout, "imported NaN, ctrl")
    assert not np.isnan(got["min_dist"]).any() and np.isfinite(got["ctrl"]).all()


@pytest.mark.parametrize("overlap", [1, 0])
def test_device_form_equals_host_form_with_work_in_flight(hip_lib, overlap):
    import torch
    K, frames = small_stream(8)
    g, _ = make_pair(SMALL, K)
    g.set_option("esdf_overlap", overlap)
    for R, T, d in frames[:2]:
        g.recast_depth_to_map(R, T, d, None)
    g.update_esdf(max_dist=1.0)
    rng = np.random.default_rng(12)
    a = rng.uniform([0.6, -1.5, -1.5], [3.2, 1.5, 1.5], (1001, 1, 3))            # around the observed cone
    c = (a + np.cumsum(rng.normal(size=(1001, 12, 3)) * 0.12, axis=1)).astype(np.float32)
    lengths = rng.integers(4, 13, 1001).astype(np.int32)
    c_t, len_t = torch.from_numpy(c).cuda(), torch.from_numpy(lengths).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for R, T, d in frames[2:]:                                   # queued frames and an enqueued update, then the calls: no sync in between
        g.recast_depth_to_map(R, T, d, None)
    assert g.update_esdf(max_dist=1.0, wait=False) is None
    kw = dict(sub=4, unknown_value=UNK, refresh=False)
    with torch.cuda.stream(side):
        lin = g.traj_linearize(c_t, CLEAR, lengths=len_t, **kw)
        opt = g.traj_optimize(c_t, CLEAR, iters=10, history=True, stop_when_free=True, lengths=len_t, **kw)
    side.synchronize()
    g.sync()
    wlin = g.traj_linearize(c, CLEAR, lengths=lengths, **kw)
    wopt = g.traj_optimize(c, CLEAR, iters=10, history=True, stop_when_free=True, lengths=lengths, **kw)
    assert (wlin["n_pen"] > 0).sum() > 100 and (wlin["argmin"] >= 0).sum() > 300 and ((wopt["iters_done"] > 0) & (wopt["iters_done"] < 10)).sum() >= 5
    for res, want, extra in ((lin, wlin, ("grad_collision", "grad_smooth")), (opt, wopt, ("ctrl", "history"))):
        res = _np(res)
        ref.assert_equal(res, want, f"device vs host, esdf_overlap {overlap}")
        for k in extra:
            ref.assert_bits(res[k], want[k], f"device vs host, esdf_overlap {overlap}, {k}")
    # the device form clamps lengths into 4 .. K; the host form refuses them
    odd = torch.tensor([0, -5, 13, 4000, 3, 7], dtype=torch.int32).cuda()
    got = _np(g.traj_optimize(c_t[:6], CLEAR, iters=3, lengths=odd, **kw))
    torch.cuda.synchronize()
    want = g.traj_optimize(c[:6], CLEAR, iters=3, lengths=np.array([4, 4, 12, 12, 4, 7], np.int32), **kw)
    ref.assert_equal(got, want, "clamped lengths")
    ref.assert_bits(got["ctrl"], want["ctrl"], "clamped lengths, ctrl")
    with pytest.raises(ValueError):
        g.traj_optimize(c[:6], CLEAR, iters=3, lengths=np.array([0, -5, 13, 4000, 3, 7]), **kw)


def test_a_volume_whose_height_differs_from_its_width(hip_lib):
    g, val, known, lo = _scene(SLAB, "slab")
    assert g.N != g.Nz
    vs = np.float32(g.voxel_scale)
    c = polygons(val, known, lo, SLAB["voxel_scale"], np.random.default_rng(41), 67, 19, bad=2)
    if "slab_ref" not in _CACHE:
        _CACHE["slab_ref"] = (ref.linearize(c, CLEAR, 4, None, vs, val, known, lo, UNK), ref.optimize(c, CLEAR, 4, 10, None, vs, val, known, lo, unknown=UNK))
    (want, wgc, wgs), (wout, wrec, whist, _) = _CACHE["slab_ref"]
    assert (want["n_pen"] > 0).sum() >= 15 and (want["n_outside"] > 0).sum() >= 15 and (want["n_unknown"] > 0).sum() >= 15
    got = g.traj_linearize(c, CLEAR, sub=4, unknown_value=UNK, refresh=False)
    ref.assert_equal(got, want, "slab, linearize")
    ref.assert_bits(got["grad_collision"], wgc, "slab, grad_collision")
    ref.assert_bits(got["grad_smooth"], wgs, "slab, grad_smooth")
    got = g.traj_optimize(c, CLEAR, sub=4, iters=10, history=True, unknown_value=UNK, refresh=False)
    ref.assert_equal(got, wrec, "slab, optimize")
    ref.assert_bits(got["ctrl"], wout, "slab, ctrl")
    ref.assert_bits(got["history"], whist, "slab, history")


def test_refusals_and_sizes(hip_lib):
    import torch
    from taichislam_amd import _lib
    K, frames = small_stream(2)
    g, _ = make_pair(SMALL, K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    rng = np.random.default_rng(3)
    c = rng.uniform(0.5, 2.5, (5, 6, 3)).astype(np.float32)
    for refresh in (False, True):
        with pytest.raises(_lib.TslError):
            g.traj_linearize(c, CLEAR, refresh=refresh)           # before any update
        with pytest.raises(_lib.TslError):
            g.traj_optimize(c, CLEAR, refresh=refresh)
    g.update_esdf(max_dist=1.0)
    base = g.traj_optimize(c, CLEAR, iters=2, history=True, refresh=False)
    assert base["n_samples"].tolist() == [13] * 5 and base["history"].shape == (5, 3, 2) and base["ctrl"].shape == (5, 6, 3)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = g.L
    lengths = np.full(5, 6, np.int32)
    inf, nan = float("inf"), float("nan")

    def opt(**kw):
        a = dict(clearance=0.3, w_collision=1.0, w_smooth=1.0, step=0.05, momentum=0.8, max_move=0.02, sub=4, iters=2, fix_head=1, fix_tail=1, flags=0)
        a.update(kw)
        return _lib.TrajOpt(**a)

    def call(w=c, ln=lengths, n=5, K=6, sub=4, clearance=0.3, co=True, out=True, o=None, lin=False):
        rec = np.full((5, 12), 0x5a5a5a5a, np.int32)
        cout = np.full((5, 6, 3), 77.0, np.float32)
        p1 = np.full((5, 6, 3), 0x5a, np.int64)
        p2 = np.full((5, 3, 2), 0x5a, np.int64)
        if lin:
            rc = L.tsl_esdf_traj_linearize(g.h, float(UNK), vp(w), vp(ln), n, K, sub, clearance, vp(rec) if out else None, vp(p1), None)
        else:
            rc = L.tsl_esdf_traj_optimize(g.h, float(UNK), vp(w), vp(ln), n, K, C.byref(o or opt()), vp(cout) if co else None, vp(rec) if out else None, vp(p2))
        return rc, bool((rec == 0x5a5a5a5a).all() and (cout == 77.0).all() and (p1 == 0x5a).all() and (p2 == 0x5a).all())
    assert call() == (0, False) and call(lin=True) == (0, False)
    assert call(out=False)[0] == 0 and call(lin=True, out=False)[0] == 0          # the record is optional
    short, long_ = np.array([6, 6, 3, 6, 6], np.int32), np.array([6, 6, 6, 7, 6], np.int32)
    refused = [dict(w=None), dict(co=False), dict(n=-1), dict(n=(1 << 20) + 1), dict(K=3), dict(K=257), dict(ln=short), dict(ln=long_),
               dict(o=opt(sub=0)), dict(o=opt(sub=65)), dict(o=opt(iters=-1)), dict(o=opt(iters=1025)), dict(o=opt(flags=2)), dict(o=opt(flags=-1)),
               dict(o=opt(fix_head=-1)), dict(o=opt(fix_tail=-1)), dict(o=opt(fix_head=4, fix_tail=3)), dict(o=opt(fix_head=2 ** 31 - 1, fix_tail=2 ** 31 - 1))]
    for f in ("clearance", "w_collision", "w_smooth", "step", "momentum", "max_move"):
        refused += [dict(o=opt(**{f: v})) for v in (-0.1, nan, inf)]
    for kw in refused:
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, kw
        assert b"esdf_traj_optimize" in L.tsl_last_error(), kw
    assert call(o=opt(fix_head=3, fix_tail=3))[0] == 0 and call(o=opt(iters=0))[0] == 0
    for kw in (dict(w=None), dict(n=-1), dict(K=3), dict(K=257), dict(ln=short), dict(ln=long_), dict(sub=0), dict(sub=65), dict(clearance=-0.1),
               dict(clearance=nan), dict(clearance=inf)):
        rc, untouched = call(lin=True, **kw)
        assert rc == -1 and untouched, kw
        assert b"esdf_traj_linearize" in L.tsl_last_error(), kw
    # the device forms: the same refusals, nothing launched
    t = torch.from_numpy(c).cuda()
    rec_t = torch.full((5, 12), 7, dtype=torch.int32, device="cuda")
    co_t = torch.full((5, 6, 3), 7.0, device="cuda")
    for kw in (dict(w=0), dict(co=0), dict(n=-1), dict(K=3), dict(K=257), dict(o=opt(sub=65)), dict(o=opt(iters=1025)), dict(o=opt(flags=2)),
               dict(o=opt(step=nan)), dict(o=opt(fix_head=4, fix_tail=3))):
        a = dict(w=t.data_ptr(), n=5, K=6, o=opt(), co=co_t.data_ptr())
        a.update(kw)
        rc = L.tsl_esdf_traj_optimize_dev(g.h, float(UNK), a["w"] or None, None, a["n"], a["K"], C.byref(a["o"]), a["co"] or None, rec_t.data_ptr(), None, None)
        torch.cuda.synchronize()
        assert rc == -1 and (rec_t == 7).all() and (co_t == 7.0).all() and b"esdf_traj_optimize_dev" in L.tsl_last_error(), kw
    for kw in (dict(w=0), dict(n=-1), dict(K=257), dict(sub=0), dict(clearance=nan)):
        a = dict(w=t.data_ptr(), n=5, K=6, sub=4, clearance=0.3)
        a.update(kw)
        rc = L.tsl_esdf_traj_linearize_dev(g.h, float(UNK), a["w"] or None, None, a["n"], a["K"], a["sub"], a["clearance"], rec_t.data_ptr(), None, None, None)
        torch.cuda.synchronize()
        assert rc == -1 and (rec_t == 7).all() and b"esdf_traj_linearize_dev" in L.tsl_last_error(), kw
    # sizes: n = 0, 1, 5; host and device form
    for dev in (False, True):
        conv = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
        r0 = _np(g.traj_optimize(conv(np.zeros((0, 6, 3), np.float32)), CLEAR, iters=2, history=True, refresh=False))
        assert all(r0[k].shape == (0,) for k in ref.FIELDS) and r0["ctrl"].shape == (0, 6, 3) and r0["history"].shape == (0, 3, 2) and r0["cost_smooth"].dtype == np.int64
        l0 = _np(g.traj_linearize(conv(np.zeros((0, 6, 3), np.float32)), CLEAR, refresh=False))
        assert l0["grad_collision"].shape == (0, 6, 3) and l0["grad_collision"].dtype == np.int64
        r1 = _np(g.traj_optimize(conv(c[2:3]), CLEAR, iters=2, history=True, refresh=False))
        r5 = _np(g.traj_optimize(conv(c), CLEAR, iters=2, history=True, refresh=False))
        ref.assert_equal(r5, base, "n = 5")
        ref.assert_equal(r1, {k: base[k][2:3] for k in ref.FIELDS}, "n = 1")
        ref.assert_bits(r5["ctrl"], base["ctrl"], "n = 5, ctrl")
        ref.assert_bits(r1["history"], base["history"][2:3], "n = 1, history")
    # what Python refuses itself
    with pytest.raises(TypeError):
        g.traj_linearize(c, CLEAR, lengths=np.full(5, 6.0), refresh=False)
    with pytest.raises(TypeError):
        g.traj_optimize(t, CLEAR, lengths=lengths, refresh=False)
    with pytest.raises(ValueError):
        g.traj_optimize(c, CLEAR, lengths=np.array([6, 6, 6]), refresh=False)
    with pytest.raises(ValueError):
        g.traj_linearize(c[:, :, :2], CLEAR, refresh=False)
    half = g.traj_optimize(c, CLEAR, iters=1, step=10.0, fix_ends=0, refresh=False)      # max_move=None is half a voxel
    assert np.abs(half["ctrl"].astype(np.float64) - c).max() <= 0.5 * g.voxel_scale * (1 + 1e-6)
    # after reset / switch_to_next_submap the calls raise, as query_esdf does
    g.reset()
    with pytest.raises(_lib.TslError):
        g.traj_optimize(c, CLEAR, refresh=False)
    g.update_esdf(max_dist=1.0)
    g.traj_linearize(c, CLEAR, refresh=False)
    g.switch_to_next_submap()
    with pytest.raises(_lib.TslError):
        g.traj_linearize(c, CLEAR, refresh=False)
    rc, untouched = call()
    assert rc == -1 and untouched

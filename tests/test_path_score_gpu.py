"""Path scoring on the GPU (tsl_path_score.hip): bit for bit against the numpy restatement (tests/path_score_ref.py) over the oracle's ESDF, the
per-sample rows against query_esdf, the stop flag, an imported NaN, the device form against the host form with work in flight, an analytic sphere,
and the refusals.  The scene is the one of tests/test_esdf_query_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import esdf_query_ref as qref
import path_score_ref as ref
from util import SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

UNK = np.float32(-3.5)
RADIUS, MARGIN = 0.25, 0.15
ALL = ref.UNKNOWN_BLOCKS | ref.OUTSIDE_BLOCKS
_CACHE = {}


@pytest.fixture(autouse=True, params=[1, 0], ids=["wavefront", "regional"])
def esdf_mode(request, monkeypatch):
    """Every test runs for both forms of the incremental update (esdf_mode 1 and 0), as tests/test_esdf_query_gpu.py does."""
    monkeypatch.setenv("TSL_ESDF_MODE", str(request.param))
    return request.param


def _scene(nframes=2, max_dist=2.0):
    """the _scene() of tests/test_esdf_query_gpu.py; the oracle's grid is computed once and shared (it does not depend on the form of the update)"""
    K, frames = small_stream(nframes)
    g, o = make_pair(SMALL, K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    g.update_esdf(max_dist=max_dist)
    if "grid" not in _CACHE:
        from oracle import BATCHED
        for R, T, d in frames:
            o.integrate_depth(R, T, d, mode=BATCHED)
        oi, oe = o.esdf(max_dist=max_dist)
        _CACHE["grid"] = qref.grid_from_export(oi, oe, g.N, g.Nz)
        for a in _CACHE["grid"]:
            a.setflags(write=False)
    return (g,) + _CACHE["grid"]


def walks(val, known, lo, vs, half, rng, n, K):
    """n random walks of K waypoints, 2 to 10 voxels per segment: most start at known free voxels and keep a heading (they run from free space into
    walls and into the unknown, early or late), some start outside the volume and walk in, and a handful hold NaN / inf waypoints"""
    free = np.argwhere(known & (val > 0.5)) + lo
    start = (free[rng.integers(0, len(free), n)] + rng.uniform(-0.5, 0.5, (n, 3))) * vs
    out = rng.random(n) < 0.12                                  # outside the volume, up to 12 voxels beyond a face, heading back in
    ax = rng.integers(0, 3, n)
    sgn = rng.choice([-1.0, 1.0], n)
    beyond = sgn * (half[ax] + rng.uniform(0.0, 12.0, n)) * vs
    start[out, ax[out]] = beyond[out]
    head = rng.normal(size=(n, 3))
    head[out] = -start[out] + rng.normal(size=(int(out.sum()), 3))
    wp = np.empty((n, K, 3))
    wp[:, 0] = start
    slow = rng.random(n) < 0.5                                  # half of the walks take short steps: they stay in free space longer
    for k in range(1, K):
        head = head / np.linalg.norm(head, axis=1, keepdims=True) + 0.35 * rng.normal(size=(n, 3))
        step = np.where(slow, rng.uniform(2.0, 4.0, n), rng.uniform(2.0, 10.0, n)) * vs
        wp[:, k] = wp[:, k - 1] + head / np.linalg.norm(head, axis=1, keepdims=True) * step[:, None]
    wp = wp.astype(np.float32)
    bad = rng.choice(n, 8, replace=False)
    for i, b in enumerate(bad):                                 # NaN / inf waypoints, first, middle and last
        wp[b, (0, K // 2, K - 1, 1)[i % 4], i % 3] = (np.nan, np.inf, -np.inf, np.nan)[i % 4]
    return wp


def lane_paths(vs, half):
    """straight paths of 9 waypoints for sub = 16 along +x whose sample j* is the first outside the volume, j* = 1, 63, 64, 127, 128: with only
    `outside` blocking, first_stop sits on the last lane of a chunk and on the first lane of the next (they run through space nothing was observed in).
    One set per mode: the trilinear cell needs its +1 corner in the volume (x < (half - 1) voxels), the nearest voxel x < (half - 0.5) voxels."""
    d = 0.02
    wp = []
    for edge in ((half[0] - 1.0) * vs, (half[0] - 0.5) * vs):
        for j in (1, 63, 64, 127, 128):
            x0 = edge - (j - 0.5) * d                           # sample j lies at x0 + j d: half a step beyond the edge
            p = np.zeros((9, 3))
            p[:, 0] = x0 + 16 * d * np.arange(9)
            p[:, 1:] = (3.02, -0.31)                            # far from the observed cone
            wp.append(p)
    return np.array(wp, np.float32)


def _gpu(g, wp, sub, lengths, mode, flags, **kw):
    return g.score_paths(wp, RADIUS, margin=MARGIN, sub=sub, lengths=lengths, interpolate=bool(mode), stop=bool(flags & 1),
                         unknown_blocks=bool(flags & 2), outside_blocks=bool(flags & 4), unknown_value=UNK, refresh=False, **kw)


def _main_set(g, val, known, lo):
    if "main" not in _CACHE:
        rng = np.random.default_rng(21)
        vs, half = np.float32(g.voxel_scale), np.array([g.N // 2, g.N // 2, g.Nz // 2])
        wp = walks(val, known, lo, vs, half, rng, 2047, 9)
        lengths = rng.integers(1, 10, 2047).astype(np.int32)
        lengths[:1200] = 9                                      # most paths are whole: S = 129 at sub = 16
        wp128 = walks(val, known, lo, vs, half, rng, 401, 128)
        len128 = np.array([63, 64, 65, 128], np.int32)[np.arange(401) % 4]
        _CACHE["main"] = (wp, lengths, wp128, len128, lane_paths(vs, half))
        for a in _CACHE["main"]:
            a.setflags(write=False)
    return _CACHE["main"]


def _values(name, wp, sub, lengths, mode, vs, val, known, lo):
    """the restatement's sample values of a batch, computed once"""
    k = (name, sub, mode)
    if k not in _CACHE:
        _CACHE[k] = ref.sample_values(wp, sub, lengths, mode, vs, val, known, lo, UNK)
    return _CACHE[k]


def test_records_equal_the_restatement_over_the_oracle(hip_lib):
    g, val, known, lo = _scene()
    vs = np.float32(g.voxel_scale)
    wp, lengths, wp128, len128, lanes = _main_set(g, val, known, lo)
    assert set(((lengths.astype(np.int64) - 1) * s + 1).max() for s in (1, 8, 16)) == {9, 65, 129} and lengths.min() == 1
    for mode in (0, 1):
        for name, w, ln, subs in (("walks", wp, lengths, (1, 8, 16)), ("s63-128", wp128, len128, (1,)), ("lanes", lanes, None, (16,))):
            for sub in subs:
                d, st, valid, _ = _values(name, w, sub, ln, mode, vs, val, known, lo)
                for flags in range(8):
                    want, wd, ws = ref.records(d, st, valid, RADIUS, MARGIN, flags, UNK)
                    got = _gpu(g, w, sub, ln, mode, flags, samples=True)
                    ref.assert_equal(got, want, f"{name}, mode {mode}, sub {sub}, flags {flags}", rows=((got["sample_dist"], got["sample_status"]), (wd, ws)))
                    if name == "walks" and sub == 16 and flags in (ALL, ALL | ref.STOP):
                        # the input reaches what it is there for (conditions on the restatement alone)
                        f = want["first_stop"]
                        assert ((f >= 0) & (f < 64)).sum() >= 100 and (f >= 64).sum() >= 100 and (f < 0).sum() >= 100, np.bincount(np.clip(f, -1, 128) // 64 + 1)
                        assert (want["n_unknown"] > 0).sum() >= 100 and (want["n_outside"] > 0).sum() >= 100 and (want["argmin"] > 0).sum() >= 20
                        assert flags & ref.STOP or ((want["n_hit"] > 0).sum() >= 100 and (want["cost"] > 0).sum() >= 100)
                    if name == "lanes" and flags == ref.OUTSIDE_BLOCKS:
                        assert {63, 64, 127, 128} <= set(want["first_stop"].tolist()), want["first_stop"]
    # first_stop on lane 0 of the first chunk: the walks that start outside
    for mode in (0, 1):
        d, st, valid, _ = _values("walks", wp, 16, lengths, mode, vs, val, known, lo)
        assert (ref.records(d, st, valid, RADIUS, MARGIN, ref.OUTSIDE_BLOCKS, UNK)[0]["first_stop"] == 0).sum() >= 20
    one = _gpu(g, wp[5], 8, None, 1, ALL)                                       # a [K, 3] input is one path
    d, st, valid, _ = ref.sample_values(wp[5:6], 8, None, 1, vs, val, known, lo, UNK)
    ref.assert_equal(one, ref.records(d, st, valid, RADIUS, MARGIN, ALL, UNK)[0], "one path")


def test_sample_rows_equal_query_esdf_at_the_sample_positions(hip_lib):
    g, val, known, lo = _scene()
    wp, lengths, _, _, _ = _main_set(g, val, known, lo)
    for mode in (0, 1):
        for sub in (1, 8):
            p, valid = ref.sample_points(wp, sub, lengths)
            qd, _, qs = g.query_esdf(p[valid], interpolate=bool(mode), gradient=False, unknown_value=UNK, refresh=False)
            got = _gpu(g, wp, sub, lengths, mode, 0, samples=True)
            assert (got["sample_status"][valid] <= 2).all() and np.array_equal(got["sample_status"][valid], qs) and (qs == 0).sum() > 1000
            assert np.array_equal(got["sample_dist"][valid].view(np.uint32), qd.view(np.uint32))
            assert (got["sample_status"][~valid] == 0xff).all() and (got["sample_dist"][~valid] == UNK).all() and (~valid).sum() > 1000
            # with the stop flag the entries behind first_stop are uncounted too
            stop = _gpu(g, wp, sub, lengths, mode, ALL | ref.STOP, samples=True)
            j = np.arange(valid.shape[1])[None, :]
            cnt = valid & ((stop["first_stop"][:, None] < 0) | (j <= stop["first_stop"][:, None]))
            assert np.array_equal(stop["sample_status"][cnt], got["sample_status"][cnt]) and (stop["sample_status"][~cnt] == 0xff).all()
            assert np.array_equal(stop["sample_dist"][cnt].view(np.uint32), got["sample_dist"][cnt].view(np.uint32)) and (stop["sample_dist"][~cnt] == UNK).all()
            only_d = _gpu(g, wp[:5], sub, lengths[:5], mode, 0)                  # the rows are optional
            assert "sample_dist" not in only_d


def test_stop_flag(hip_lib):
    g, val, known, lo = _scene()
    wp, lengths, _, _, _ = _main_set(g, val, known, lo)
    for mode in (0, 1):
        for flags in (0, ref.UNKNOWN_BLOCKS, ALL):
            a, b = _gpu(g, wp, 16, lengths, mode, flags), _gpu(g, wp, 16, lengths, mode, flags | ref.STOP)
            assert np.array_equal(a["first_stop"], b["first_stop"])
            free = a["first_stop"] < 0
            assert free.sum() >= 100 and (~free).sum() >= 100
            for k in ref.FIELDS:
                assert np.array_equal(a[k][free], b[k][free]), k
            assert np.array_equal(b["n_samples"][~free], b["first_stop"][~free] + 1)


def test_imported_nan_counts_as_unknown(hip_lib):
    g, val, known, lo = _scene()
    vs = np.float32(g.voxel_scale)
    e = g.export_submap()
    idx = e["indices"].astype(np.int64)
    free = np.argwhere(known & (val > 0.8)) + lo
    c = free[len(free) // 2]
    ball = ((idx - c) ** 2).sum(1) <= 9                                          # a ball of 3 voxels around a free voxel
    assert 50 < ball.sum() < 200
    t = np.asarray(e["TSDF"]).copy()
    t[ball] = np.nan
    h, o = make_pair(SMALL, small_stream(1)[0])
    h.load_numpy(h.get_active_submap_id(), e["indices"], t, e["W_TSDF"], e["occupy"], np.array([]))
    h.update_esdf(max_dist=2.0)
    hi, he = h.export_esdf()
    hval, hknown, hlo = qref.grid_from_export(hi, he, h.N, h.Nz)
    bi = idx[ball] - hlo
    assert hknown[bi[:, 0], bi[:, 1], bi[:, 2]].all()                            # observed voxels: the point query answers there with status 0
    nknown = hknown.copy()
    nknown[bi[:, 0], bi[:, 1], bi[:, 2]] = False                                 # ... and the path scoring counts them as unknown
    rng = np.random.default_rng(2)
    a = (c + rng.normal(size=(300, 3)) * 12.0) * vs                              # straight lines through the ball
    b = 2.0 * c * vs - a
    wp = (a[:, None, :] + (b - a)[:, None, :] * np.linspace(0.0, 1.0, 5)[None, :, None]).astype(np.float32)
    for mode in (0, 1):
        for flags in (ref.UNKNOWN_BLOCKS, ref.UNKNOWN_BLOCKS | ref.STOP, 0):
            want, wd, ws = ref.score(wp, RADIUS, MARGIN, 8, None, mode, flags, vs, hval, nknown, hlo, UNK)
            got = h.score_paths(wp, RADIUS, margin=MARGIN, sub=8, interpolate=bool(mode), stop=bool(flags & 1), unknown_blocks=bool(flags & 2),
                                outside_blocks=False, samples=True, unknown_value=UNK, refresh=False)
            ref.assert_equal(got, want, f"imported NaN, mode {mode}, flags {flags}", rows=((got["sample_dist"], got["sample_status"]), (wd, ws)))
            assert not np.isnan(got["min_dist"]).any() and not np.isnan(got["sample_dist"]).any()
        # the samples that read a voxel of the ball are unknown: they are the difference to the restatement that takes the ball for known
        plain = ref.score(wp, RADIUS, MARGIN, 8, None, mode, 0, vs, hval, hknown, hlo, UNK)[0]
        assert (got["n_unknown"] > plain["n_unknown"]).sum() >= 250 and (got["n_unknown"] >= plain["n_unknown"]).all()


@pytest.mark.parametrize("overlap", [1, 0])
def test_device_form_equals_host_form_with_work_in_flight(hip_lib, overlap):
    import torch
    K, frames = small_stream(8)
    g, _ = make_pair(SMALL, K)
    g.set_option("esdf_overlap", overlap)
    for R, T, d in frames[:2]:
        g.recast_depth_to_map(R, T, d, None)
    g.update_esdf(max_dist=1.0)
    rng = np.random.default_rng(11)
    a = rng.uniform([0.6, -1.5, -1.5], [3.2, 1.5, 1.5], (3001, 1, 3))            # around the observed cone
    wp = (a + np.cumsum(rng.normal(size=(3001, 9, 3)) * 0.15, axis=1)).astype(np.float32)
    lengths = rng.integers(1, 10, 3001).astype(np.int32)
    wp_t, len_t = torch.from_numpy(wp).cuda(), torch.from_numpy(lengths).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for R, T, d in frames[2:]:                                   # queued frames and an enqueued update, then the call: no sync in between
        g.recast_depth_to_map(R, T, d, None)
    assert g.update_esdf(max_dist=1.0, wait=False) is None
    kw = dict(margin=MARGIN, sub=8, unknown_value=UNK, refresh=False, samples=True)
    with torch.cuda.stream(side):
        got = g.score_paths(wp_t, RADIUS, lengths=len_t, **kw)
        got0 = g.score_paths(wp_t, RADIUS, interpolate=False, stop=True, **kw)
    side.synchronize()
    g.sync()
    for res, extra in ((got, dict(lengths=lengths)), (got0, dict(interpolate=False, stop=True))):
        want = g.score_paths(wp, RADIUS, **extra, **kw)
        res = {k: v.cpu().numpy() for k, v in res.items()}
        assert (want["argmin"] >= 0).sum() > 300 and (want["first_stop"] >= 0).sum() > 300
        ref.assert_equal(res, want, f"device vs host, esdf_overlap {overlap}", rows=((res["sample_dist"], res["sample_status"]), (want["sample_dist"], want["sample_status"])))
    # the device form clamps lengths into 1 .. K; the host form refuses them
    odd = torch.tensor([0, -5, 10, 4000, 3], dtype=torch.int32).cuda()
    got = g.score_paths(wp_t[:5], RADIUS, lengths=odd, **kw)
    torch.cuda.synchronize()
    want = g.score_paths(wp[:5], RADIUS, lengths=np.array([1, 1, 9, 9, 3], np.int32), **kw)
    ref.assert_equal({k: v.cpu().numpy() for k, v in got.items()}, want, "clamped lengths")


def test_analytic_sphere(hip_lib):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(map_scale=[6.4, 6.4], voxel_scale=0.05, num_voxel_per_blk_axis=16)
    g.init_sphere(voxels=60, radius=0.8)
    g.update_esdf(max_dist=3.0)
    hi, he = g.export_esdf()
    val, known, lo = qref.grid_from_export(hi, he, g.N, g.Nz)
    yz = np.linspace(-0.95, 0.95, 39)
    y, z = (a.reshape(-1) for a in np.meshgrid(yz, yz, indexing="ij"))
    n, K, sub = y.size, 14, 64                                                   # waypoints every 0.2 m, samples every 3.1 mm: far below the bound
    wp = np.zeros((n, K, 3), np.float32)
    wp[:, :, 0] = np.linspace(-1.3, 1.3, K).astype(np.float32)[None, :]
    wp[:, :, 1], wp[:, :, 2] = y[:, None], z[:, None]
    got = g.score_paths(wp, 0.2, sub=sub, refresh=False, samples=True)
    want, _, _ = ref.score(wp, 0.2, 0.0, sub, None, 1, ALL, np.float32(0.05), val, known, lo)
    assert (got["n_unknown"] == 0).all() and (got["n_outside"] == 0).all()
    assert np.array_equal(got["first_stop"] >= 0, want["first_stop"] >= 0) and np.array_equal(got["first_stop"], want["first_stop"])
    # the bound of test_analytic_sphere (tests/test_esdf_query_gpu.py): 0.09 * max|true| + 0.05 over the cube of side 2.6 m, max|true| = |(1.3, 1.3, 1.3)| - 0.8
    bound = 0.09 * (np.sqrt(3.0) * 1.3 - 0.8) + 0.05
    rho = np.hypot(y.astype(np.float64), z)
    near = rho < 0.9
    assert near.sum() > 500 and (got["first_stop"][near] >= 0).all()
    p, _ = ref.sample_points(wp, sub)
    x_stop = p[np.arange(n), np.maximum(got["first_stop"], 0), 0].astype(np.float64)
    # the true distance falls below the radius at x = -sqrt(1 - rho^2)
    e_stop = np.abs(x_stop[near] + np.sqrt(1.0 - rho[near] ** 2)).max()
    e_min = np.abs(got["min_dist"][near] - (rho[near] - 0.8)).max()
    print(f"analytic sphere: stop position off by at most {e_stop:.4f} m, min_dist by at most {e_min:.4f} m, bound {bound:.4f} m")
    assert e_stop < bound
    assert e_min < bound
    assert (got["first_stop"][rho > 1.0 + bound] < 0).all() and (rho > 1.0 + bound).sum() > 50


def test_refusals_and_sizes(hip_lib):
    from taichislam_amd import _lib
    K, frames = small_stream(2)
    g, _ = make_pair(SMALL, K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    rng = np.random.default_rng(3)
    wp = rng.uniform(0.5, 2.5, (5, 4, 3)).astype(np.float32)
    for refresh in (False, True):
        with pytest.raises(_lib.TslError):
            g.score_paths(wp, RADIUS, refresh=refresh)           # before any update
    g.update_esdf(max_dist=1.0)
    base = g.score_paths(wp, RADIUS, sub=4, samples=True, refresh=False)
    assert base["n_samples"].tolist() == [13] * 5 and base["sample_dist"].shape == (5, 13)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = g.L
    n, Kw = 5, 4
    lengths = np.full(n, 4, np.int32)

    def call(mode=1, w=wp, ln=lengths, n=n, K=Kw, sub=4, radius=0.25, margin=0.1, flags=6, out=True, sd=True, ss=True):
        rec = np.full((5, 10), 0x5a5a5a5a, np.int32)
        d = np.full((5, 13), 77.0, np.float32)
        s = np.full((5, 13), 0x5a, np.uint8)
        rc = L.tsl_esdf_score_paths(g.h, mode, float(UNK), vp(w), vp(ln), n, K, sub, radius, margin, flags, vp(rec) if out else None, vp(d) if sd else None,
                                    vp(s) if ss else None)
        untouched = (rec == 0x5a5a5a5a).all() and (d == 77.0).all() and (s == 0x5a).all()
        return rc, untouched
    assert call() == (0, False)
    inf, nan = float("inf"), float("nan")
    refused = [dict(mode=2), dict(mode=-1), dict(w=None), dict(out=False), dict(n=-1), dict(n=(1 << 20) + 1), dict(K=0), dict(K=4097), dict(sub=0),
               dict(sub=257), dict(K=4096, sub=256, n=2049), dict(ln=np.array([4, 4, 0, 4, 4], np.int32)), dict(ln=np.array([4, 4, 4, 5, 4], np.int32)),
               dict(radius=-0.1), dict(radius=nan), dict(radius=inf), dict(margin=-1.0), dict(margin=nan), dict(margin=inf), dict(flags=8), dict(flags=-1)]
    for kw in refused:
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, kw
        assert b"esdf_score_paths" in L.tsl_last_error(), kw
    # n * S_max >= 2^31 is refused only when a per-sample output is asked for (K = 4096, sub = 256, n = 2049: S_max = 1048321)
    for kw in (dict(w=None, n=2049), dict(out=False, n=2049)):                   # without rows it gets as far as the null buffers
        rc, untouched = call(K=4096, sub=256, sd=False, ss=False, **kw)
        assert rc == -1 and untouched and b"null buffer" in L.tsl_last_error()
    import torch
    t = torch.from_numpy(wp).cuda()
    rec_t = torch.full((5, 10), 7, dtype=torch.int32, device="cuda")
    for kw in (dict(mode=2), dict(n=-1), dict(K=0), dict(sub=257), dict(radius=nan), dict(flags=8), dict(w=0), dict(out=0)):
        a = dict(mode=1, w=t.data_ptr(), n=5, K=4, sub=4, radius=0.25, flags=6, out=rec_t.data_ptr())
        a.update(kw)
        rc = L.tsl_esdf_score_paths_dev(g.h, a["mode"], float(UNK), a["w"] or None, None, a["n"], a["K"], a["sub"], a["radius"], 0.1, a["flags"], a["out"] or None,
                                        None, None, None)
        torch.cuda.synchronize()
        assert rc == -1 and (rec_t == 7).all() and b"esdf_score_paths_dev" in L.tsl_last_error(), kw
    # sizes: n = 0, 1, 5; K = 1; host and device form
    for dev in (False, True):
        conv = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
        back = (lambda r: {k: v.cpu().numpy() for k, v in r.items()}) if dev else (lambda r: r)
        r0 = back(g.score_paths(conv(np.zeros((0, 4, 3), np.float32)), RADIUS, sub=4, samples=True, refresh=False))
        assert all(r0[k].shape == (0,) for k in ref.FIELDS) and r0["sample_dist"].shape == (0, 13) and r0["cost"].dtype == np.int64
        r1 = back(g.score_paths(conv(wp[2:3]), RADIUS, sub=4, samples=True, refresh=False))
        r5 = back(g.score_paths(conv(wp), RADIUS, sub=4, samples=True, refresh=False))
        ref.assert_equal(r5, base, "n = 5", rows=((r5["sample_dist"], r5["sample_status"]), (base["sample_dist"], base["sample_status"])))
        ref.assert_equal(r1, {k: base[k][2:3] for k in ref.FIELDS}, "n = 1")
        k1 = back(g.score_paths(conv(wp[:, :1].copy()), RADIUS, sub=7, samples=True, refresh=False))       # K = 1: one sample per path, whatever sub
        assert k1["n_samples"].tolist() == [1] * 5 and k1["sample_dist"].shape == (5, 1) and np.array_equal(k1["sample_dist"][:, 0].view(np.uint32), base["sample_dist"][:, 0].view(np.uint32))
        assert np.array_equal(k1["argmin"], np.where(base["sample_status"][:, 0] == 0, 0, -1))
    # lengths of the wrong dtype raise in Python, and so do lengths outside 1 .. K and a sub below 1
    with pytest.raises(TypeError):
        g.score_paths(wp, RADIUS, lengths=np.full(5, 4.0), refresh=False)
    with pytest.raises(TypeError):
        g.score_paths(t, RADIUS, lengths=torch.full((5,), 4, dtype=torch.int64, device="cuda"), refresh=False)
    with pytest.raises(TypeError):
        g.score_paths(t, RADIUS, lengths=lengths, refresh=False)
    with pytest.raises(ValueError):
        g.score_paths(wp, RADIUS, lengths=np.array([1, 2, 3, 4, 5]), refresh=False)
    with pytest.raises(ValueError):
        g.score_paths(wp, RADIUS, sub=0, refresh=False)
    assert np.array_equal(g.score_paths(wp, RADIUS, sub=4, lengths=[4, 4, 4, 4, 4], refresh=False)["cost"], base["cost"])
    # after reset / switch_to_next_submap the call raises, as query_esdf does
    g.reset()
    with pytest.raises(_lib.TslError):
        g.score_paths(wp, RADIUS, refresh=False)
    g.update_esdf(max_dist=1.0)
    g.score_paths(wp, RADIUS, refresh=False)
    g.switch_to_next_submap()
    with pytest.raises(_lib.TslError):
        g.score_paths(wp, RADIUS, refresh=False)
    rc, untouched = call()
    assert rc == -1 and untouched

"""ESDF point queries on the GPU (tsl_esdf_query.hip): bit for bit against the numpy restatement (tests/esdf_query_ref.py) over the oracle's
ESDF, against an analytic sphere, the device form against the host form with frames and updates still in flight, the early-stop flag, the
refusals, and refresh."""
import ctypes as C

import numpy as np
import pytest

import esdf_query_ref as ref
from util import SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

UNK = np.float32(-3.5)


@pytest.fixture(autouse=True, params=[1, 0], ids=["wavefront", "regional"])
def esdf_mode(request, monkeypatch):
    """Every test runs for both forms of the incremental update (esdf_mode 1 and 0), as tests/test_esdf_gpu.py does."""
    monkeypatch.setenv("TSL_ESDF_MODE", str(request.param))
    return request.param


def _scene(nframes=2, max_dist=2.0):
    K, frames = small_stream(nframes)
    g, o = make_pair(SMALL, K)
    from oracle import BATCHED
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
        o.integrate_depth(R, T, d, mode=BATCHED)
    g.update_esdf(max_dist=max_dist)
    oi, oe = o.esdf(max_dist=max_dist)
    val, known, lo = ref.grid_from_export(oi, oe, g.N, g.Nz)
    return g, val, known, lo


def _points(g, known, lo, rng, n=200_000):
    """known voxel centres, random points in the observed region, cells crossing 2 / 4 / 8 bricks, cells next to unknown voxels, points outside
    the volume and a few non-finite ones"""
    vs = np.float32(g.voxel_scale)
    kidx = np.argwhere(known) + lo
    m = n // 8
    parts = [kidx[rng.integers(0, len(kidx), m)].astype(np.float32) * vs]
    bmin, bmax = kidx.min(0) - 1, kidx.max(0) + 2
    parts.append((rng.uniform(bmin, bmax, (2 * m, 3)) * vs).astype(np.float32))
    half = np.array([g.N // 2, g.N // 2, g.Nz // 2])
    for axes in ([0], [1], [2], [0, 1], [1, 2], [0, 1, 2], [0, 1, 2]):
        v = kidx[rng.integers(0, len(kidx), m // 2)].copy()
        for a in axes:                                         # local index 15 on these axes: the +1 corner is in the next brick
            v[:, a] = ((v[:, a] + half[a]) | 15) - half[a]
        parts.append(((v + rng.uniform(0, 1, v.shape)) * vs).astype(np.float32))
    # next to unknown voxels: known voxels with an unknown 26-neighbour
    pad = np.pad(known, 1)
    inner = np.ones_like(known)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                inner &= pad[1 + dx:1 + dx + known.shape[0], 1 + dy:1 + dy + known.shape[1], 1 + dz:1 + dz + known.shape[2]]
    edge = np.argwhere(known & ~inner) + lo
    parts.append(((edge[rng.integers(0, len(edge), m)] + rng.uniform(-1, 1, (m, 3))) * vs).astype(np.float32))
    out = rng.uniform(-1, 1, (m // 2, 3)) * half * vs
    ax = rng.integers(0, 3, m // 2)
    out[np.arange(m // 2), ax] = np.sign(out[np.arange(m // 2), ax] + 1e-9) * (half[ax] + rng.uniform(0, 20, m // 2)) * vs
    parts.append(out.astype(np.float32))
    parts.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32))
    return np.concatenate(parts)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_equal(got, want, what):
    (d, g, s), (wd, wg, ws) = got, want
    bad = np.nonzero((_bits(d) != _bits(wd)) | (s != ws))[0]
    assert bad.size == 0, f"{what}: {bad.size} queries differ, first {bad[:5]}: {d[bad[:5]]} / {wd[bad[:5]]}, status {s[bad[:5]]} / {ws[bad[:5]]}"
    if g is not None:
        assert np.array_equal(_bits(g), _bits(wg)), f"{what}: gradient differs at {(_bits(g) != _bits(wg)).any(1).sum()} queries"


def test_queries_equal_the_restatement_over_the_oracle(hip_lib):
    g, val, known, lo = _scene()
    rng = np.random.default_rng(7)
    pts = _points(g, known, lo, rng)
    vs = np.float32(g.voxel_scale)
    for mode in (0, 1):
        got = g.query_esdf(pts, interpolate=bool(mode), unknown_value=UNK, refresh=False)
        wd, wg, ws = ref.query(pts, mode, vs, val, known, lo, unknown=UNK)
        _check_equal(got, (wd, wg if mode else None, ws), f"mode {mode}")
        assert (got[1] is None) == (mode == 0)
        counts = np.bincount(got[2], minlength=3)
        assert counts[0] > 50_000 and counts[1] > 5_000 and counts[2] > 10_000, counts
    # every brick-crossing class has fully known cells (the 2-, 4- and 8-lookup paths are exercised)
    b = ((np.floor(np.nan_to_num(pts / vs, posinf=0.0, neginf=0.0)).astype(np.int64) + np.array([g.N // 2, g.N // 2, g.Nz // 2])) & 15) == 15
    _, _, s1 = g.query_esdf(pts, refresh=False)
    for k in (1, 2, 3):
        assert ((b.sum(1) == k) & (s1 == 0)).sum() > 20, k
    # the default unknown value is NaN, the gradient of a refused query 0
    d, gr, s = g.query_esdf(pts[:20000], refresh=False)
    assert np.isnan(d[s != 0]).all() and (gr[s != 0] == 0).all() and not np.isnan(d[s == 0]).any()


def test_mode1_at_known_voxel_centres_equals_mode0(hip_lib):
    g, val, known, lo = _scene()
    vs = np.float32(g.voxel_scale)
    kidx = np.argwhere(known) + lo
    pts = kidx.astype(np.float32) * vs
    pts = pts[(np.floor(pts / vs) == pts / vs).all(1)]                  # x / vs is the index exactly: f = 0
    d0, _, s0 = g.query_esdf(pts, interpolate=False, refresh=False)
    d1, _, s1 = g.query_esdf(pts, interpolate=True, refresh=False)
    full = s1 == 0
    assert full.sum() > 20_000 and (s0 == 0).all()
    assert np.array_equal(_bits(d1[full]), _bits(d0[full]))


def test_analytic_sphere(hip_lib):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(map_scale=[6.4, 6.4], voxel_scale=0.05, num_voxel_per_blk_axis=16)
    g.init_sphere(voxels=60, radius=0.8)
    g.update_esdf(max_dist=3.0)
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1.3, 1.3, (200_000, 3)).astype(np.float32)
    d, gr, s = g.query_esdf(pts, refresh=False)
    assert (s == 0).all()
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    true = r - 0.8
    assert np.abs(d - true).max() < 0.09 * np.abs(true).max() + 0.05          # the bound of test_esdf_analytic_sphere
    # the gradient points away from the centre.  The 26-neighbour distance has kinks between lattice paths, so pointwise it is only roughly
    # radial away from the surface; in the band (ESDF = TSDF) it is the analytic SDF's.
    sel = r > 0.25
    dot = (gr[sel] * (pts[sel] / r[sel, None])).sum(1)
    assert dot.min() > 0.5 and (dot >= 0.9).mean() > 0.9 and np.median(dot) > 0.98
    shell = np.abs(r[sel] - 0.8) < 0.05
    assert shell.sum() > 1000 and dot[shell].min() >= 0.9
    # a central difference inside one cell matches the gradient (the interpolant is linear along each axis within a cell)
    vs = np.float32(0.05)
    c = ((np.floor(pts[:20000] / vs) + rng.uniform(0.3, 0.7, (20000, 3))) * vs).astype(np.float32)
    h = np.float32(0.2) * vs
    _, gc, sc = g.query_esdf(c, refresh=False)
    for a in range(3):
        e = np.zeros(3, np.float32); e[a] = h
        dp, _, sp = g.query_esdf(c + e, gradient=False, refresh=False)
        dm, _, sm = g.query_esdf(c - e, gradient=False, refresh=False)
        ok = (sc == 0) & (sp == 0) & (sm == 0)
        assert ok.sum() > 15000
        fd = (dp[ok].astype(np.float64) - dm[ok]) / ((c + e)[ok, a].astype(np.float64) - (c - e)[ok, a])
        assert np.abs(fd - gc[ok, a]).max() < 2e-3
    # status 1 in cells that touch the unobserved shell (indices -30..29 are observed) and in unallocated bricks, 2 beyond +-3.2 m
    shell_pts = np.array([[29.5 * 0.05, 0, 0], [0, -30.5 * 0.05, 0.3], [2.5, 0, 0], [-2.0, 1.0, 2.9]], np.float32)
    _, _, s = g.query_esdf(shell_pts, refresh=False)
    assert list(s) == [1, 1, 1, 1]
    _, _, s = g.query_esdf(np.array([[2.5, 0, 0], [-2.0, 1.0, 2.9]], np.float32), interpolate=False, refresh=False)
    assert list(s) == [1, 1]
    far = np.array([[3.25, 0, 0], [0, -3.3, 0], [0, 0, 4.0], [-3.21, 3.21, 3.21]], np.float32)
    for interp in (False, True):
        d, _, s = g.query_esdf(far, interpolate=interp, refresh=False)
        assert list(s) == [2, 2, 2, 2] and np.isnan(d).all()


def _torch_query(g, pts_t, stream, **kw):
    import torch
    with torch.cuda.stream(stream):
        d, gr, s = g.query_esdf(pts_t, **kw)
    stream.synchronize()
    return d.cpu().numpy(), None if gr is None else gr.cpu().numpy(), s.cpu().numpy()


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
    pts = (rng.uniform(-2.0, 2.0, (300_000, 3))).astype(np.float32)
    pts_t = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for R, T, d in frames[2:]:                                   # queued frames and an enqueued update, then the query: no sync in between
        g.recast_depth_to_map(R, T, d, None)
    assert g.update_esdf(max_dist=1.0, wait=False) is None
    got = _torch_query(g, pts_t, side, refresh=False, unknown_value=UNK)
    g.sync()
    want = g.query_esdf(pts, refresh=False, unknown_value=UNK)
    assert (want[2] == 0).sum() > 10_000
    _check_equal(got, want, f"device vs host, esdf_overlap {overlap}")
    got0 = _torch_query(g, pts_t, side, interpolate=False, refresh=False, unknown_value=UNK)
    _check_equal(got0, g.query_esdf(pts, interpolate=False, refresh=False, unknown_value=UNK), "device vs host, mode 0")


def test_early_stop_is_flagged(hip_lib):
    import torch
    K, frames = small_stream(2)
    g, val, known, lo = _scene()
    rng = np.random.default_rng(5)
    pts = _points(g, known, lo, rng, n=80_000)
    want = ref.query(pts, 1, np.float32(g.voxel_scale), val, known, lo, unknown=UNK)
    h, _ = make_pair(SMALL, K)
    h.set_option("esdf_round_cap", 1)
    for R, T, d in frames:
        h.recast_depth_to_map(R, T, d, None)
    h.update_esdf(max_dist=2.0, wait=False)                      # a full update at reach 4 needs many more rounds than one
    pts_t = torch.from_numpy(pts).cuda()
    d, gr, s = _torch_query(h, pts_t, torch.cuda.current_stream(), refresh=False, unknown_value=UNK)
    flagged = (s & 0x80) != 0
    assert flagged.sum() > 0
    clean = ~flagged
    assert np.array_equal(_bits(d[clean]), _bits(want[0][clean])) and np.array_equal(s[clean], want[2][clean])
    assert np.array_equal(s & 0x7f, np.where(flagged, s & 0x7f, want[2]))
    # the host form waits for the update and repairs it: converged values, no flag -- and so does the device form afterwards
    _check_equal(h.query_esdf(pts, refresh=False, unknown_value=UNK), want, "host form after the repair")
    _check_equal(_torch_query(h, pts_t, torch.cuda.current_stream(), refresh=False, unknown_value=UNK), want, "device form after the repair")


def test_refusals_and_sizes(hip_lib):
    from taichislam_amd import _lib
    from taichislam_amd.mapping import DenseTSDF
    K, frames = small_stream(2)
    pts = np.zeros((4, 3), np.float32)
    g, _ = make_pair(SMALL, K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    for refresh in (False, True):
        with pytest.raises(_lib.TslError):
            g.query_esdf(pts, refresh=refresh)                   # before any update
    g.update_esdf(max_dist=1.0)
    g.query_esdf(pts, refresh=False)
    # bad modes / buffers through the C-ABI
    dist, grad, st = np.zeros(4, np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L = g.L
    assert L.tsl_esdf_query_points(g.h, 2, 0.0, vp(pts), 4, vp(dist), None, vp(st)) != 0
    assert L.tsl_esdf_query_points(g.h, 0, 0.0, vp(pts), 4, vp(dist), vp(grad), vp(st)) != 0
    assert L.tsl_esdf_query_points(g.h, 1, 0.0, vp(pts), 4, None, None, vp(st)) != 0
    assert L.tsl_esdf_query_points(g.h, 1, 0.0, vp(pts), 4, vp(dist), None, vp(st)) == 0
    with pytest.raises(ValueError):
        g.query_esdf(pts, interpolate=False, gradient=True)
    # n = 0 and a count that is not a multiple of 256, host and device form
    d, gr, s = g.query_esdf(np.zeros((0, 3), np.float32), refresh=False)
    assert d.shape == (0,) and gr.shape == (0, 3) and s.shape == (0,)
    import torch
    rng = np.random.default_rng(9)
    big = rng.uniform(-3, 3, (3_000_001, 3)).astype(np.float32)
    d, gr, s = g.query_esdf(big, refresh=False)
    assert d.shape == (3_000_001,) and gr.shape == (3_000_001, 3)
    tail = g.query_esdf(big[-1000:], refresh=False)
    _check_equal((d[-1000:], gr[-1000:], s[-1000:]), tail, "tail of 3 000 001 queries")
    td, tg, ts = g.query_esdf(torch.from_numpy(big).cuda(), refresh=False)
    torch.cuda.synchronize()
    _check_equal((td.cpu().numpy(), tg.cpu().numpy(), ts.cpu().numpy()), (d, gr, s), "device form, 3 000 001 queries")
    td, _, _ = g.query_esdf(torch.zeros((0, 3), device="cuda"), refresh=False)
    assert td.shape == (0,)
    # reset, an import, a switch of the active submap: the ESDF no longer belongs to what is queried
    e = g.export_submap()
    g.reset()
    with pytest.raises(_lib.TslError):
        g.query_esdf(pts, refresh=False)
    g.update_esdf(max_dist=1.0)
    g.query_esdf(pts, refresh=False)
    g.load_numpy(g.get_active_submap_id(), e["indices"][:100], e["TSDF"][:100], e["W_TSDF"][:100], e["occupy"][:100], np.array([]))
    with pytest.raises(_lib.TslError):
        g.query_esdf(pts, refresh=False)
    g.update_esdf(max_dist=1.0)
    g.query_esdf(pts, refresh=False)
    g.switch_to_next_submap()
    with pytest.raises(_lib.TslError):
        g.query_esdf(pts, refresh=False)
    # an esdf_mode switch keeps the values: the query still answers from the last update
    h = DenseTSDF(**SMALL); h.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        h.recast_depth_to_map(R, T, d, None)
    h.update_esdf(max_dist=1.0)
    a = h.query_esdf(pts, refresh=False)
    h.set_option("esdf_mode", 1 - h.get_option("esdf_mode"))
    _check_equal(h.query_esdf(pts, refresh=False), a, "after an esdf_mode switch")


@pytest.mark.parametrize("is_global", [False, True], ids=["submap", "global"])
def test_refresh_equals_explicit_update(hip_lib, is_global):
    from taichislam_amd.mapping import DenseTSDF
    K, frames = small_stream(6)
    a, b = (DenseTSDF(**dict(SMALL, is_global_map=is_global)) for _ in range(2))
    for m in (a, b):
        m.set_dep_camera_intrinsic(K)
        for R, T, d in frames[:3]:
            m.recast_depth_to_map(R, T, d, None)
        m.update_esdf(max_dist=1.0)
    rng = np.random.default_rng(4)
    pts = rng.uniform(-2.5, 2.5, (200_000, 3)).astype(np.float32)
    before = a.query_esdf(pts, refresh=False)
    for m in (a, b):
        for R, T, d in frames[3:]:
            m.recast_depth_to_map(R, T, d, None)
    got = a.query_esdf(pts)                                       # refresh=True: an update is enqueued first
    b.update_esdf(max_dist=1.0)
    want = b.query_esdf(pts, refresh=False)
    assert (want[2] == 0).sum() > 5_000 and (_bits(before[0]) != _bits(want[0])).sum() > 1000
    _check_equal(got, want, "refresh vs explicit update")

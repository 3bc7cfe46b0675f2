"""Navigation grids on the GPU (tsl_nav_grid.hip): every plane -- classes, counts, spans, squared distances, costs -- equals the numpy restatement
(tests/nav_grid_ref.py) over the oracle's export byte for byte, on the hand-built scenes of tests/nav_grid_scenes.py on three geometries and on a room
map; plus ordering behind queued frames, the device form, repeatability, null planes and the refusals."""
import ctypes as C

import numpy as np
import pytest

import frontier_scenes as fs
import nav_grid_ref as ref
import nav_grid_scenes as ns
from taichislam_amd import _lib
from taichislam_amd.utils import inflation_lut
from util import SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

VS = SMALL["voxel_scale"]
GEOS = ["SMALL", "SLAB", "TALL"]
_MAPS = {}


def _map(geo):
    """one GPU map per geometry for the whole module, reset before every use"""
    from taichislam_amd.mapping import DenseTSDF
    if geo not in _MAPS:
        _MAPS[geo] = DenseTSDF(**fs.GEOMETRIES[geo]["cfg"])
    g = _MAPS[geo]
    g.reset()
    g.active_submap_id[None] = 0
    return g


def _loaded(geo, sc, hip_lib):
    from oracle import OracleTSDF
    g, o = _map(geo), OracleTSDF(**fs.GEOMETRIES[geo]["cfg"])
    fs.load_pair(g, o, sc)
    return g, o


def _call(g, bands, R, flags=0, lut=None, **kw):
    got = g.nav_grid(bands=bands, radius=R * VS, unknown_is_obstacle=bool(flags & 1), wall_is_obstacle=bool(flags & 2), lut=lut, counts=True, span=True, **kw)
    assert got["radius_vox"] == R and got["bands"] == [tuple(b) for b in bands]
    return got


def _compare(g, o, what, bands, R, flags=0, lut=None, **kw):
    """nav_grid against the restatement over the oracle's export: every plane"""
    want = ref.nav_grid(o.export_sparse(), o.N, o.Nz, VS, bands, R, flags=flags, lut=lut, **kw)
    got = _call(g, bands, R, flags, lut, **kw)
    ref.assert_equal(got, want, what, keys=("cls", "counts", "span", "d2") + (("cost",) if lut is not None else ()))
    return got, want


def _bands(geo):
    """a single layer, a band across a brick face of SMALL and TALL, the same across a brick face of the geometry, the whole height"""
    N, Nz, oz = ns.dims(geo)
    return [(oz, oz), (-3, 5), (oz - 3, oz + 5), (-(Nz // 2), Nz // 2 - 1)]


@pytest.mark.parametrize("geo", GEOS)
def test_columns_equal_the_restatement(hip_lib, geo):
    N, Nz, oz = ns.dims(geo)
    g, o = _loaded(geo, ns.put(ns.columns(), geo), hip_lib)
    for band in _bands(geo):
        _compare(g, o, f"columns on {geo}, band {band}", [band], 5)
    whole = _bands(geo)[3]
    got, _ = _compare(g, o, f"columns on {geo}, unknown cells are obstacles", [whole, (oz, oz)], 5, flags=1)
    u = lambda c: (c[0] + fs.GEOMETRIES[geo]["o"][0] + N // 2, c[1] + fs.GEOMETRIES[geo]["o"][1] + N // 2)
    gap, lone, nan = u(ns.COL_GAP), u(ns.COL_LONE), u(ns.COL_NAN)
    assert got["counts"][0][gap].tolist() == [1, 1, Nz - 2] and got["span"][0][gap].tolist() == [oz - 20, oz - 20]      # the absent middle brick is unknown
    assert got["counts"][0][lone].tolist() == [0, 1, Nz - 1] and got["cls"][0][lone] == ref.FREE and got["cls"][1][lone] == ref.UNKNOWN
    assert got["counts"][0][nan].tolist() == [0, 2, Nz - 2] and got["counts"][1][nan].tolist() == [0, 1, 0]            # the NaN voxel reads as unknown
    assert got["d2"][1][lone] == 0 and got["d2"][0][lone] == 1                                                          # unknown is an obstacle: the lone cell's neighbours
    # min_occ / min_free / max_unknown: the columns built to sit on each side of each limit
    lb = (oz + ns.LIMIT_BAND[0], oz + ns.LIMIT_BAND[1])
    for mo, mf, mu in ((2, 3, 0), (2, 3, None), (1, 1, None), (0, 0, 2)):
        got, _ = _compare(g, o, f"columns on {geo}, limits {mo} {mf} {mu}", [lb], 3, min_occ=mo, min_free=mf, max_unknown=mu)
        cells = [got["cls"][0][u((n - 10, -10))] for n in range(len(ns.LIMIT_COLUMNS))]
        assert cells == ns.limit_classes(max(1, mo), max(1, mf), mu), (mo, mf, mu)
    a, _ = _compare(g, o, f"columns on {geo}, free_thres 0.6", [whole], 3, free_thres=0.6)          # every observed voxel of the scene is below 0.6
    assert (a["counts"][0][..., 1] == 0).all() and a["counts"][0][nan].tolist() == [2, 0, Nz - 2]


@pytest.mark.parametrize("geo", GEOS)
def test_sixteen_bands_at_once_equal_the_single_band_calls(hip_lib, geo):
    N, Nz, oz = ns.dims(geo)
    g, o = _loaded(geo, ns.put(ns.columns(), geo), hip_lib)
    lo, hi = -(Nz // 2), Nz // 2 - 1
    bands = _bands(geo) + [(oz, oz + 5), (oz, oz + 5), (lo, lo), (hi, hi), (lo, oz), (oz + 1, hi), (oz - 20, oz - 20), (oz - 19, oz + 4), (oz + 1, oz + 1),
                           (oz + 5, oz + 8), (lo, lo + 15), (hi - 16, hi)]
    assert len(bands) == 16
    lut = (np.arange(4 * 4 + 2) % 251).astype(np.uint8)
    got, _ = _compare(g, o, f"16 bands on {geo}", bands, 4, lut=lut, cost_unknown=77)
    for k in ("cls", "counts", "span", "d2", "cost"):
        assert np.array_equal(got[k][4], got[k][5]), k                      # two equal bands
    for b in (0, 2, 3, 9, 15):
        one = _call(g, [bands[b]], 4, lut=lut, cost_unknown=77)
        for k in ("cls", "counts", "span", "d2", "cost"):
            assert np.array_equal(one[k][0], got[k][b]), (k, b)


@pytest.mark.parametrize("geo", GEOS)
def test_distances_of_the_hand_worked_scenes(hip_lib, geo):
    N, Nz, oz = ns.dims(geo)
    c = fs.GEOMETRIES[geo]["o"][0] + N // 2                          # the scene's (0, 0) in unsigned indices
    g, o = _loaded(geo, ns.put(ns.three_four_five(), geo), hip_lib)
    got, _ = _compare(g, o, f"3-4-5 on {geo}", [(oz, oz)], 5)
    d = got["d2"][0]
    assert d[c, c] == 0 and d[c + 3, c + 4] == 25 and d[c + 5, c] == 25 and d[c - 4, c + 3] == 25 and d[c, c - 5] == 25
    assert d[c + 4, c + 4] == 26 and d[c + 6, c] == 26 and d[c, c + 6] == 26 and d[0, 0] == 26
    got, _ = _compare(g, o, f"3-4-5 on {geo}, R = 0", [(oz, oz)], 0)
    assert got["d2"][0][c, c] == 0 and int(got["d2"][0].astype(np.int64).sum()) == N * N - 1
    _compare(g, o, f"3-4-5 on {geo}, R = 0, wall", [(oz, oz)], 0, flags=2)
    g, o = _loaded(geo, ns.put(ns.row_versus_plane(), geo), hip_lib)
    got, _ = _compare(g, o, f"row versus plane on {geo}", [(oz, oz)], 5)
    assert got["d2"][0][c + 1, c] == 1 and got["d2"][0][c + 1, c - 1] == 2
    # an empty band: all far, and all unknown; with the wall the rim counts
    got, _ = _compare(g, o, f"empty band on {geo}", [(oz + 1, oz + 1)], 3)
    assert (got["d2"] == 10).all() and (got["cls"] == ref.UNKNOWN).all()
    got, _ = _compare(g, o, f"empty band on {geo}, unknown is an obstacle", [(oz + 1, oz + 1)], 3, flags=1)
    assert (got["d2"] == 0).all()


@pytest.mark.parametrize("geo", GEOS)
def test_corners_and_edges_with_and_without_the_wall(hip_lib, geo):
    g, o = _loaded(geo, ns.corners(geo, 2), hip_lib)
    for flags in (0, 2):
        got, _ = _compare(g, o, f"corners on {geo}, flags {flags}", [(2, 2)], 6, flags=flags)
    assert got["d2"][0][0, 0] == 0 and got["d2"][0][1, 1] == 2 and got["d2"][0][0, 5] == 1 and got["d2"][0][3, 3] == 16
    g, o = _loaded(geo, ns.edges(geo, 2), hip_lib)
    for flags in (0, 2, 3):
        _compare(g, o, f"edges on {geo}, flags {flags}", [(2, 2)], 6, flags=flags)


@pytest.mark.parametrize("geo,R", [("SMALL", 20), ("SMALL", 70), ("SLAB", 20), ("TALL", 40)])
def test_lines_across_every_brick_and_strip(hip_lib, geo, R):
    g, o = _loaded(geo, ns.lines(geo, 1), hip_lib)
    _compare(g, o, f"lines on {geo}, R = {R}", [(1, 1)], R, flags=2 if R == 70 else 0)


def test_scatter_with_costs(hip_lib):
    R = 20
    g, o = _loaded("SMALL", ns.put(ns.scatter(), "SMALL"), hip_lib)
    got, _ = _compare(g, o, "scatter, inflation table", [(0, 0)], R, lut=inflation_lut(VS, R, 0.12, 0.6, scale=4.0), cost_unknown=255)
    assert 150 <= int((got["cls"] == ref.OCCUPIED).sum()) <= 200 and len(np.unique(got["cost"])) > 20
    got, _ = _compare(g, o, "scatter, arange % 251, unknown is an obstacle", [(0, 0), (-1, 1)], R, flags=1, lut=(np.arange(R * R + 2) % 251).astype(np.uint8), cost_unknown=9)
    assert (got["cost"][got["cls"] == ref.UNKNOWN] == 9).all() and (got["cost"][1][got["cls"][1] == ref.FREE] != 9).any()
    got, _ = _compare(g, o, "scatter, arange % 251", [(0, 0)], R, flags=2, lut=(np.arange(R * R + 2) % 251).astype(np.uint8), cost_unknown=9)
    assert (got["cost"][got["cls"] == ref.OCCUPIED] == 0).all()


def test_radius_254_on_tall(hip_lib):
    """the window is wider than the grid"""
    g, o = _loaded("TALL", ns.put(ns.posts([(0, 0), (-20, 13)]), "TALL"), hip_lib)
    got, _ = _compare(g, o, "R = 254 on TALL", [(0, 0)], 254, lut=(np.arange(254 * 254 + 2) % 251).astype(np.uint8))
    assert got["d2"].max() < 254 * 254 and got["d2"][0][0, 0] == 32 * 32 + 32 * 32
    _compare(g, o, "R = 254 on TALL, wall", [(0, 0)], 254, flags=2)
    g.reset()
    e = g.nav_grid(bands=[(0, 0)], radius=254 * VS)
    assert (e["d2"] == 254 * 254 + 1).all() and (e["cls"] == ref.UNKNOWN).all()


def test_room_with_frames_still_queued(hip_lib):
    """nav_grid straight after recast_depth_to_map, nothing waited for: the grids are those of all the frames"""
    from oracle import BATCHED
    K, frames = small_stream(3)
    g, o = make_pair(SMALL, K)
    R = 10
    lut = inflation_lut(VS, R, 0.1, 0.3)
    kw = dict(z_range=[(-0.3, 0.5), (0.5, 1.21), (-9.0, 9.0)], radius=R * VS, lut=lut, counts=True, span=True, min_occ=2, max_unknown=30)
    for R_, T_, d in frames[:2]:
        g.recast_depth_to_map(R_, T_, d, None)
        o.integrate_depth(R_, T_, d, mode=BATCHED)
    two = g.nav_grid(**kw)
    assert two["bands"] == [(-7, 12), (13, 30), (-128, 127)] and two["origin_xy"] == (-128 - 0.5) * VS and two["voxel"] == VS
    rk = dict(min_occ=2, max_unknown=30, lut=lut)
    ref.assert_equal(two, ref.nav_grid(o.export_sparse(), o.N, o.Nz, VS, two["bands"], R, **rk), "two frames", keys=("cls", "counts", "span", "d2", "cost"))
    R_, T_, d = frames[2]
    g.recast_depth_to_map(R_, T_, d, None)
    three = g.nav_grid(**kw)
    o.integrate_depth(R_, T_, d, mode=BATCHED)
    ref.assert_equal(three, ref.nav_grid(o.export_sparse(), o.N, o.Nz, VS, two["bands"], R, **rk), "three frames", keys=("cls", "counts", "span", "d2", "cost"))
    assert not np.array_equal(three["counts"], two["counts"])
    n = [int((three["cls"][0] == c).sum()) for c in (ref.FREE, ref.OCCUPIED, ref.UNKNOWN)]
    print(f"room, band {three['bands'][0]}: {n[0]} free, {n[1]} occupied, {n[2]} unknown cells")
    assert min(n) > 0


def test_device_form_equals_the_host_form(hip_lib):
    import torch
    g, o = _loaded("SMALL", ns.put(ns.scatter(), "SMALL"), hip_lib)
    lut = inflation_lut(VS, 12, 0.1, 0.4)
    kw = dict(bands=[(0, 0), (-3, 5)], radius=12 * VS, lut=lut, counts=True, span=True, wall_is_obstacle=True, cost_unknown=3)
    host = g.nav_grid(**kw)
    a = torch.ones(1 << 25, device="cuda")
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            for _ in range(8):
                a = a * 0.5 + 1.0                                    # work in flight on the caller's stream
            dev = g.nav_grid(device=True, **kw)
            got = {k: dev[k].clone() for k in ("cls", "d2", "cost", "counts", "span")}
        torch.cuda.synchronize()
        for k, v in got.items():
            assert v.is_cuda and v.cpu().numpy().tobytes() == host[k].tobytes(), k
    only = g.nav_grid(device=True, bands=[(0, 0)], radius=12 * VS)
    torch.cuda.synchronize()
    assert sorted(k for k in only if hasattr(only[k], "is_cuda")) == ["cls", "d2"] and only["cls"].cpu().numpy().tobytes() == host["cls"][0].tobytes()


def _raw(L, g, cfg, lut, shape, cls=False, d2=False, cost=False, counts=False, span=False):
    """tsl_tsdf_nav_grid with exactly the planes asked for; every buffer starts as 0xAB"""
    B, N = shape
    bufs = {"cls": np.full((B, N, N), 0xAB, np.uint8) if cls else None, "d2": np.full((B, N, N), 0xABAB, np.uint16) if d2 else None,
            "cost": np.full((B, N, N), 0xAB, np.uint8) if cost else None, "counts": np.full((B, N, N, 3), 0xABAB, np.uint16) if counts else None,
            "span": np.full((B, N, N, 2), 0x2B2B, np.int16) if span else None}
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.tsl_tsdf_nav_grid(g.h, C.byref(cfg), p(lut), p(bufs["cls"]), p(bufs["d2"]), p(bufs["cost"]), p(bufs["counts"]), p(bufs["span"]))
    return rc, bufs


def _cfg(bands=((8, 8), (5, 13)), R=7, **kw):
    c = _lib.NavCfg()
    c.n_bands = len(bands)
    for b, (k0, k1) in enumerate(bands):
        c.k_min[b], c.k_max[b] = k0, k1
    c.radius, c.max_unknown, c.cost_unknown = R, -1, 200
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_two_calls_give_the_same_bytes_and_null_planes_are_skipped(hip_lib):
    g, o = _loaded("SLAB", ns.put(ns.columns(), "SLAB"), hip_lib)
    L, N = hip_lib, 144
    lut = (np.arange(7 * 7 + 2) % 251).astype(np.uint8)
    rc, full = _raw(L, g, _cfg(), lut, (2, N), cls=True, d2=True, cost=True, counts=True, span=True)
    assert rc == 0
    rc, again = _raw(L, g, _cfg(), lut, (2, N), cls=True, d2=True, cost=True, counts=True, span=True)
    assert rc == 0 and all(full[k].tobytes() == again[k].tobytes() for k in full)
    want = ref.nav_grid(o.export_sparse(), o.N, o.Nz, VS, [(8, 8), (5, 13)], 7, lut=lut, cost_unknown=200)
    ref.assert_equal(full, want, "every plane", keys=("cls", "counts", "span", "d2", "cost"))
    for planes in (("cls",), ("d2",), ("cost",), ("counts",), ("span",), ("counts", "span"), ("cls", "cost"), ("d2", "span"), ("d2", "cost")):
        rc, part = _raw(L, g, _cfg(), lut if "cost" in planes else None, (2, N), **{k: True for k in planes})
        assert rc == 0, (planes, L.tsl_last_error())
        for k in planes:
            assert part[k].tobytes() == full[k].tobytes(), (planes, k)


def test_refusals_leave_the_handle_usable(hip_lib):
    g, o = _loaded("SLAB", ns.put(ns.columns(), "SLAB"), hip_lib)
    L, N = hip_lib, 144
    lut = np.zeros(7 * 7 + 2, np.uint8)
    nan, inf = float("nan"), float("inf")
    bad = [("n_bands", dict(n_bands=0)), ("n_bands", dict(n_bands=17)), ("n_bands", dict(n_bands=-1)), ("free_thres", dict(free_thres=nan)), ("free_thres", dict(free_thres=inf)),
           ("min_occ", dict(min_occ=-1)), ("min_free", dict(min_free=-2)), ("radius", dict(radius=-1)), ("radius", dict(radius=255)), ("flags", dict(flags=4)),
           ("flags", dict(flags=-1))]
    cases = [(w, _cfg(**kw), lut, dict(cls=True, cost=True)) for w, kw in bad]
    cases += [("band", _cfg(bands=((-25, 0),)), lut, dict(cls=True, cost=True)), ("band", _cfg(bands=((0, 24),)), lut, dict(cls=True, cost=True)),
              ("band", _cfg(bands=((0, 0), (3, 2))), lut, dict(cls=True, cost=True)),
              ("cost and lut", _cfg(), None, dict(cls=True, cost=True)), ("cost and lut", _cfg(), lut, dict(cls=True)), ("every output", _cfg(), None, dict())]
    good = dict(cls=True, d2=True, cost=True, counts=True, span=True)
    rc, full = _raw(L, g, _cfg(), lut, (2, N), **good)
    assert rc == 0
    for word, cfg, lt, planes in cases:
        rc, bufs = _raw(L, g, cfg, lt, (2, N), **planes)
        msg = L.tsl_last_error().decode()
        assert rc == -1 and "nav_grid:" in msg and word in msg, (word, msg)
        assert all((b.view(np.uint8) == (0xAB if k != "span" else 0x2B)).all() for k, b in bufs.items() if b is not None), word      # nothing was written
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        assert L.tsl_tsdf_nav_grid_dev(g.h, C.byref(cfg), p(lt), p(bufs["cls"]), None, p(bufs["cost"]), None, None, None) == -1
        assert "nav_grid_dev:" in L.tsl_last_error().decode()
        rc, ok = _raw(L, g, _cfg(), lut, (2, N), **good)              # a good call still succeeds, with the same bytes
        assert rc == 0 and all(ok[k].tobytes() == full[k].tobytes() for k in ok), word
    cls = np.zeros((2, N, N), np.uint8)
    assert L.tsl_tsdf_nav_grid(g.h, None, None, cls.ctypes.data_as(C.c_void_p), None, None, None, None) == -1 and "null cfg" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_grid(None, C.byref(_cfg()), None, cls.ctypes.data_as(C.c_void_p), None, None, None, None) == -1 and "null handle" in L.tsl_last_error().decode()
    with pytest.raises(ValueError):
        g.nav_grid(z_range=(0.01, 0.02))                              # no voxel layer
    with pytest.raises(ValueError):
        g.nav_grid(z_range=(2.0, 3.0))                                # above the volume
    with pytest.raises(ValueError):
        g.nav_grid(bands=[(0, 0)], z_range=(0.0, 0.1))
    with pytest.raises(ValueError):
        g.nav_grid(radius=7 * VS, lut=np.zeros(5, np.uint8))
    with pytest.raises(_lib.TslError, match="radius"):
        g.nav_grid(radius=255 * VS)
    _compare(g, o, "after the refusals", [(8, 8)], 7)


def test_too_large_a_grid_is_refused(hip_lib):
    """N * N * n_bands >= 2^31: 16384 x 16384 cells and 8 bands (a sparse map: only the brick table is that large)"""
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(map_scale=[655.36, 0.64], voxel_scale=0.04, num_voxel_per_blk_axis=16, max_submap_num=1, max_bricks=64)
    assert (g.N, g.Nz) == (16384, 16)
    cfg = _cfg(bands=((0, 0),) * 8)
    one = np.zeros(16, np.uint8)                                      # never written: the call is refused before anything is launched
    assert hip_lib.tsl_tsdf_nav_grid(g.h, C.byref(cfg), None, one.ctypes.data_as(C.c_void_p), None, None, None, None) == -1
    assert "nav_grid:" in hip_lib.tsl_last_error().decode() and "too large" in hip_lib.tsl_last_error().decode()
    assert g.count_active() == 0

"""Terrain layers on the GPU (tsl_nav_terrain.hip): every plane -- height, col, step, nsup, slope2, cls, d2, cost -- equals the numpy restatement
(tests/nav_terrain_ref.py) over the oracle's export byte for byte, on the hand-built scenes of tests/nav_terrain_scenes.py on three geometries and on a
room map; plus ordering behind queued frames, the device form, repeatability, null planes, the refusals, and the ramp scene end to end through nav_field
and nav_paths."""
import ctypes as C

import numpy as np
import pytest

import frontier_scenes as fs
import nav_grid_ref as gref
import nav_grid_scenes as ns
import nav_terrain_ref as ref
import nav_terrain_scenes as ts
from taichislam_amd import _lib
from util import SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

VS = SMALL["voxel_scale"]
GEOS = ["SMALL", "SLAB", "TALL"]
KINDS = {"height": np.int16, "col": np.uint8, "step": np.uint16, "nsup": np.uint16, "slope2": np.uint32, "cls": np.uint8, "d2": np.uint16, "cost": np.uint8}
ORDER = ("height", "col", "step", "nsup", "slope2", "cls", "d2", "cost")          # the order of the C arguments
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


def _loaded(geo, sc):
    from oracle import OracleTSDF
    g, o = _map(geo), OracleTSDF(**fs.GEOMETRIES[geo]["cfg"])
    fs.load_pair(g, o, sc)
    return g, o


def _cfg(bands, clearance=2, free_run=1, pick=0, window=1, slope_base=1, max_step=65534, max_slope2=ref.NO_SLOPE, min_support=1, R=0, flags=0, cost_unknown=255,
         free_thres=None, **over):
    c = _lib.NavTerrainCfg()
    c.n_bands = len(bands)
    for b, (k0, k1) in enumerate(bands[:16]):
        c.k_min[b], c.k_max[b] = k0, k1
    c.free_thres = 0.0 if free_thres is None else free_thres
    c.clearance, c.free_run, c.pick, c.window, c.slope_base, c.max_step, c.max_slope2, c.min_support = clearance, free_run, pick, window, slope_base, max_step, max_slope2, min_support
    c.radius, c.flags, c.cost_unknown = R, flags, cost_unknown
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _raw(L, g, cfg, lut, shape, planes):
    """tsl_tsdf_nav_terrain with exactly the planes asked for; every byte of every buffer starts as 0xAB"""
    B, N = shape
    bufs = {k: (np.full((B, N, N, np.dtype(KINDS[k]).itemsize), 0xAB, np.uint8).view(KINDS[k])[..., 0] if k in planes else None) for k in ORDER}
    assert all(b is None or b.flags["C_CONTIGUOUS"] for b in bufs.values())
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.tsl_tsdf_nav_terrain(g.h, C.byref(cfg), p(lut), *[p(bufs[k]) for k in ORDER])
    return rc, bufs


def _untouched(bufs):
    return all((b.view(np.uint8) == 0xAB).all() for b in bufs.values() if b is not None)


def _compare(L, g, o, what, bands, lut=None, **kw):
    """every plane of the C entry point against the restatement over the oracle's export"""
    want = ref.nav_terrain(o.export_sparse(), o.N, o.Nz, VS, bands, lut=lut, **kw)
    planes = ORDER if lut is not None else ORDER[:-1]
    rc, got = _raw(L, g, _cfg(bands, **kw), lut, (len(bands), o.N), planes)
    assert rc == 0, (what, L.tsl_last_error())
    ref.assert_equal(got, want, what, keys=planes)
    return got, want


def _u(geo, ij):
    gm = fs.GEOMETRIES[geo]
    return ij[0] + gm["o"][0] + gm["N"] // 2, ij[1] + gm["o"][1] + gm["N"] // 2


@pytest.mark.parametrize("geo", GEOS)
def test_columns_equal_the_restatement_and_the_hand_worked_supports(hip_lib, geo):
    N, Nz, oz = ns.dims(geo)
    g, o = _loaded(geo, ns.put(ts.columns(), geo))
    band = (ts.COLUMN_BAND[0] + oz, ts.COLUMN_BAND[1] + oz)
    for (fr, pick), answers in ts.COLUMN_ANSWERS.items():
        got, _ = _compare(hip_lib, g, o, f"columns on {geo}, free_run {fr}, pick {pick}", [band], clearance=17, free_run=fr, pick=pick, window=0, free_thres=ts.THRES)
        for name, want in answers.items():
            c = _u(geo, ts.COLUMNS[name][0])
            exp = (want, 32767) if isinstance(want, int) else (0, 16 * (want[0] + oz) + want[1])
            assert (int(got["col"][0][c]), int(got["height"][0][c])) == exp, (geo, fr, pick, name)
    whole = (-(Nz // 2), Nz // 2 - 1)
    for cl, fr, pick, th in ((0, 0, 0, None), (1, 1, 1, None), (1, 0, 0, ts.THRES), (16, 1, 0, ts.THRES), (17, 2, 1, None), (Nz, 1, 0, None), (Nz, 0, 1, ts.THRES), (17, 1, 0, 0.6)):
        _compare(hip_lib, g, o, f"columns on {geo}, clearance {cl}, free_run {fr}, pick {pick}, thres {th}", [band, whole, (oz - 8, oz - 8)], clearance=cl, free_run=fr, pick=pick,
                 window=1, free_thres=th)
    got, _ = _compare(hip_lib, g, o, f"columns on {geo}, the bands around a support", [(a + oz, b + oz) for a, b in ts.EDGE_BANDS], clearance=17, window=0, free_thres=ts.THRES)
    c = _u(geo, ts.COLUMNS["CLEAR1"][0])
    for b, want in enumerate(ts.EDGE_ANSWERS):
        assert (int(got["col"][b][c]), int(got["height"][b][c])) == ((want, 32767) if isinstance(want, int) else (0, 16 * (want[0] + oz) + want[1])), (geo, b)
    # the top of the volume
    t = Nz // 2 - 1
    g, o = _loaded(geo, ts.top(geo))
    for cl, fr in ((17, 1), (Nz, 0), (3, 1), (2, 2)):
        got, _ = _compare(hip_lib, g, o, f"top on {geo}, clearance {cl}, free_run {fr}", [(t - 5, t), (t, t), whole], clearance=cl, free_run=fr, window=0, free_thres=ts.THRES)
    g.reset()
    rc, got = _raw(hip_lib, g, _cfg([whole]), None, (1, N), ORDER[:-1])
    assert rc == 0 and (got["col"] == 2).all() and (got["height"] == 32767).all() and (got["cls"] == ref.UNKNOWN).all() and (got["slope2"] == ref.NO_SLOPE).all()


@pytest.mark.parametrize("geo", GEOS)
def test_surfaces_equal_the_restatement(hip_lib, geo):
    N, Nz, oz = ns.dims(geo)
    heights = dict(ts.plane_heights())
    heights.update({(i + 20, j - 14): h for (i, j), h in ts.hole_heights().items()})          # the hole's patch beside the plane's (scene cells 15 .. 25, -19 .. -9)
    g, o = _loaded(geo, ns.put(ts.surface(heights), geo))
    band = [(oz - 10, oz + 10)]
    for w, s in ((0, 1), (1, 1), (3, 2), (16, 16), (2, 16), (16, 1)):
        got, _ = _compare(hip_lib, g, o, f"plane and hole on {geo}, window {w}, slope_base {s}", band, clearance=2, window=w, slope_base=s, max_step=30, max_slope2=6000,
                          min_support=8, free_thres=ts.THRES)
        if s <= 2 and w <= 3:
            c = _u(geo, (0, 0))
            assert int(got["slope2"][0][c]) == ts.plane_slope2(s) and int(got["step"][0][c]) == ts.plane_step(w) and int(got["nsup"][0][c]) == (2 * w + 1) ** 2
    # cliffs across the tile border of the window kernel and in the corners of the grid (the geometry's own indices)
    g, o = _loaded(geo, ts.surface(ts.cliff_heights(geo)))
    rise = ts.CLIFF_HIGH - ts.CLIFF_LOW
    for w, s in ((1, 1), (2, 3), (16, 16), (0, 4)):
        got, _ = _compare(hip_lib, g, o, f"cliffs on {geo}, window {w}, slope_base {s}", [(0, 8)], clearance=2, window=w, slope_base=s, max_step=16, max_slope2=40000, min_support=5,
                          free_thres=ts.THRES)
        if (w, s) == (1, 1):
            st, sl = got["step"][0], got["slope2"][0]
            assert st[31, 28] == rise and st[32, 28] == rise and st[30, 28] == 0 and sl[31, 28] == (4 * rise) ** 2 and sl[31, 31] == 2 * (2 * rise) ** 2
            assert st[0, 0] == rise and got["nsup"][0][0, 0] == 4 and sl[1, 1] == (4 * rise) ** 2 and sl[N - 2, N - 2] == (4 * rise) ** 2 and sl[N - 1, N - 2] == ref.NO_SLOPE
    # the order of the class tests
    g, o = _loaded(geo, ns.put(ts.surface(ts.limit_heights()), geo))
    for ms, msl, mn in ts.LIMIT_SETS:
        got, _ = _compare(hip_lib, g, o, f"limits on {geo}: {ms} {msl} {mn}", [(oz - 2, oz + 2)], clearance=2, max_step=ms, max_slope2=msl, min_support=mn, free_thres=ts.THRES)
        assert [int(got["cls"][0][_u(geo, cell)]) for cell, _, _, _ in ts.LIMIT_CELLS.values()] == ts.limit_classes(ms, msl, mn)


@pytest.mark.parametrize("geo", GEOS)
def test_sixteen_bands_at_once_equal_the_single_band_calls(hip_lib, geo):
    N, Nz, oz = ns.dims(geo)
    g, o = _loaded(geo, ns.put(ts.columns(), geo))
    lo, hi = -(Nz // 2), Nz // 2 - 1
    bands = [(oz - 20, oz + 8), (lo, hi), (oz - 8, oz - 8), (oz - 3, oz + 5), (oz, oz + 5), (oz, oz + 5), (lo, lo), (hi, hi), (lo, oz), (oz + 1, hi), (oz - 20, oz - 20),
             (oz - 19, oz + 4), (oz - 17, oz - 17), (oz - 18, oz - 16), (lo, lo + 15), (hi - 16, hi)]
    assert len(bands) == 16
    lut = (np.arange(4 * 4 + 2) % 251).astype(np.uint8)
    for pick in (0, 1):
        kw = dict(clearance=17, pick=pick, window=1, slope_base=1, max_step=8, min_support=2, R=4, cost_unknown=77, free_thres=ts.THRES)
        got, _ = _compare(hip_lib, g, o, f"16 bands on {geo}, pick {pick}", bands, lut=lut, **kw)
        for k in ORDER:
            assert np.array_equal(got[k][4], got[k][5]), k                      # two equal bands
        for b in (0, 1, 2, 9, 12, 15):
            rc, one = _raw(hip_lib, g, _cfg([bands[b]], **kw), lut, (1, N), ORDER)
            assert rc == 0
            for k in ORDER:
                assert np.array_equal(one[k][0], got[k][b]), (k, b)


@pytest.fixture(scope="module")
def room():
    """the room of tests/render_view_scenes.py after its four frames: (GPU map, oracle)"""
    import render_view_scenes as rs
    from oracle import BATCHED
    K, frames = rs.room_scene()
    g, o = make_pair(SMALL, K)
    for R_, T_, d in frames:
        g.recast_depth_to_map(R_, T_, d, None)
        o.integrate_depth(R_, T_, d, mode=BATCHED)
    return g, o


def test_room_equals_the_restatement(hip_lib, room):
    g, o = room
    lut = (np.arange(6 * 6 + 2) % 251).astype(np.uint8)
    bands = [(-40, 0), (-128, 127), (-60, -10), (-30, 30), (-10, 10), (-39, -20), (0, 39), (-128, -30), (-20, -20), (20, 127), (-35, -5), (-1, 0), (-128, -1), (0, 127),
             (-100, 100), (-25, 25)]                              # (the frames see the wall between layers -39 and 39)
    kw = dict(clearance=4, free_run=1, window=1, slope_base=1, max_step=40, max_slope2=int((np.tan(np.radians(60.0)) * 128) ** 2), min_support=4, R=6, flags=1, cost_unknown=250)
    got, want = _compare(hip_lib, g, o, "room, 16 bands", bands, lut=lut, **kw)
    n = [int((got["cls"][0] == c).sum()) for c in (ref.FREE, ref.OCCUPIED, ref.UNKNOWN)]
    print(f"room, band {bands[0]}: {n[0]} free, {n[1]} occupied, {n[2]} unknown cells; {int((got['col'][0] == 0).sum())} supports, {int((got['slope2'][0] != ref.NO_SLOPE).sum())} slopes")
    assert min(n) > 0 and len(np.unique(got["height"][0][got["col"][0] == 0] & 15)) == 16
    for b in (0, 1, 8, 15):
        rc, one = _raw(hip_lib, g, _cfg([bands[b]], **kw), lut, (1, o.N), ORDER)
        assert rc == 0 and all(np.array_equal(one[k][0], got[k][b]) for k in ORDER), b
    _compare(hip_lib, g, o, "room, the highest support", bands[:2], clearance=3, free_run=2, pick=1, window=16, slope_base=16, max_step=100, min_support=300)
    # the Python method: metres and degrees become the integers it reports
    py = g.nav_terrain(z_range=(-1.61, 0.01), clearance=4 * VS, window=VS, slope_base=VS, max_step=40 * VS / 16, max_slope_deg=60.0, min_support=4, radius=6 * VS,
                       unknown_is_obstacle=True, lut=lut, cost_unknown=250)
    assert py["bands"] == [(-40, 0)] and (py["clearance_vox"], py["window_vox"], py["slope_base_vox"], py["max_step_units"], py["radius_vox"]) == (4, 1, 1, 40, 6)
    assert py["max_slope2"] == kw["max_slope2"] and py["height_unit"] == VS / 16 and py["origin_xy"] == (-128 - 0.5) * VS and py["pick"] == "lowest"
    for k in ORDER:
        assert py[k].dtype == KINDS[k] and np.array_equal(py[k][0], got[k][0]), k


@pytest.mark.parametrize("R", [0, 5, 254])
def test_distances_and_costs_are_nav_grids_transform_of_the_classes(hip_lib, R):
    geo = "TALL"
    N, Nz, oz = ns.dims(geo)
    heights = dict(ts.limit_heights())
    heights.update({(i, j + 14): h for (i, j), h in ts.hole_heights().items()})
    g, o = _loaded(geo, ns.put(ts.surface(heights), geo))
    lut = (np.arange(R * R + 2) % 251).astype(np.uint8)
    for flags in (0, 1, 2, 3):
        got, _ = _compare(hip_lib, g, o, f"R = {R}, flags {flags}", [(oz - 2, oz + 6), (oz, oz)], lut=lut, clearance=2, max_step=ts.LIMIT_D - 1, min_support=2, R=R, flags=flags,
                          cost_unknown=201, free_thres=ts.THRES)
        assert np.array_equal(got["d2"], gref.distances(got["cls"], R, flags)) and np.array_equal(got["cost"], gref.costs(got["cls"], got["d2"], lut, 201))
        assert len(np.unique(got["cls"][0])) == 3


def test_device_form_equals_the_host_form(hip_lib):
    import torch
    g, o = _loaded("SMALL", ns.put(ts.surface(ts.ramp_heights()), "SMALL"))
    lut = (np.arange(12 * 12 + 2) % 251).astype(np.uint8)
    kw = dict(bands=[(-2, 8), (0, 0)], clearance=3 * VS, window=2 * VS, slope_base=VS, max_step=2 * VS, max_slope_deg=20.0, min_support=9, radius=12 * VS, lut=lut,
              wall_is_obstacle=True, cost_unknown=3, free_thres=ts.THRES)
    host = g.nav_terrain(**kw)
    a = torch.ones(1 << 25, device="cuda")
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            for _ in range(8):
                a = a * 0.5 + 1.0                                    # work in flight on the caller's stream
            dev = g.nav_terrain(device=True, **kw)
            got = {k: dev[k].clone() for k in ORDER}
        torch.cuda.synchronize()
        for k, v in got.items():
            assert v.is_cuda and v.cpu().numpy().tobytes() == host[k].tobytes(), k
    only = g.nav_terrain(device=True, bands=[(-2, 8)], clearance=3 * VS, free_thres=ts.THRES)
    torch.cuda.synchronize()
    assert "cost" not in only and only["height"].cpu().numpy().tobytes() == host["height"][0].tobytes()


def test_room_with_frames_still_queued(hip_lib):
    """nav_terrain straight after recast_depth_to_map, nothing waited for: the layers are those of all the frames"""
    from oracle import BATCHED
    K, frames = small_stream(3)
    g, o = make_pair(SMALL, K)
    kw = dict(clearance=10, window=1, slope_base=1, max_step=20, min_support=4, R=5)
    bands = [(-40, 0), (-128, 127)]
    for R_, T_, d in frames[:2]:
        g.recast_depth_to_map(R_, T_, d, None)
        o.integrate_depth(R_, T_, d, mode=BATCHED)
    two, _ = _compare(hip_lib, g, o, "two frames", bands, **kw)
    R_, T_, d = frames[2]
    g.recast_depth_to_map(R_, T_, d, None)
    rc, three = _raw(hip_lib, g, _cfg(bands, **kw), None, (2, o.N), ORDER[:-1])
    assert rc == 0
    o.integrate_depth(R_, T_, d, mode=BATCHED)
    ref.assert_equal(three, ref.nav_terrain(o.export_sparse(), o.N, o.Nz, VS, bands, **kw), "three frames", keys=ORDER[:-1])
    assert not np.array_equal(three["height"], two["height"]) and (three["col"] == 0).any()


def test_two_calls_give_the_same_bytes_and_null_planes_are_skipped(hip_lib):
    geo = "SLAB"
    N, Nz, oz = ns.dims(geo)
    g, o = _loaded(geo, ns.put(ts.surface(ts.ramp_heights()), geo))
    lut = (np.arange(7 * 7 + 2) % 251).astype(np.uint8)
    bands = [(oz - 2, oz + 8), (oz, oz + 3)]
    kw = dict(clearance=3, window=1, max_step=32, max_slope2=2170, min_support=9, R=7, cost_unknown=200, free_thres=ts.THRES)
    full, _ = _compare(hip_lib, g, o, "every plane", bands, lut=lut, **kw)
    rc, again = _raw(hip_lib, g, _cfg(bands, **kw), lut, (2, N), ORDER)
    assert rc == 0 and all(full[k].tobytes() == again[k].tobytes() for k in ORDER)
    for planes in [(k,) for k in ORDER] + [("height", "col"), ("step", "cost"), ("slope2", "d2"), ("nsup", "cls"), ("col", "cls", "cost"), ORDER[1:], ORDER[:-1]]:
        rc, part = _raw(hip_lib, g, _cfg(bands, **kw), lut if "cost" in planes else None, (2, N), planes)
        assert rc == 0, (planes, hip_lib.tsl_last_error())
        for k in planes:
            assert part[k].tobytes() == full[k].tobytes(), (planes, k)


def test_refusals_leave_the_handle_usable(hip_lib):
    geo = "SLAB"
    N, Nz, oz = ns.dims(geo)
    g, o = _loaded(geo, ns.put(ts.surface(ts.ramp_heights()), geo))
    L = hip_lib
    lut = np.zeros(7 * 7 + 2, np.uint8)
    nan, inf = float("nan"), float("inf")
    bands = [(oz - 2, oz + 8), (oz, oz + 3)]
    base = dict(clearance=3, window=1, max_step=32, min_support=9, R=7, free_thres=ts.THRES)
    bad = [("n_bands", dict(n_bands=0)), ("n_bands", dict(n_bands=17)), ("n_bands", dict(n_bands=-1)), ("free_thres", dict(free_thres=nan)), ("free_thres", dict(free_thres=-inf)),
           ("clearance", dict(clearance=-1, free_run=0)), ("clearance", dict(clearance=Nz + 1)), ("free_run", dict(free_run=-1)), ("free_run", dict(free_run=4)),
           ("pick", dict(pick=2)), ("pick", dict(pick=-1)), ("window", dict(window=-1)), ("window", dict(window=17)), ("slope_base", dict(slope_base=0)),
           ("slope_base", dict(slope_base=17)), ("max_step", dict(max_step=-1)), ("max_step", dict(max_step=65535)), ("min_support", dict(min_support=-1)),
           ("radius", dict(radius=-1)), ("radius", dict(radius=255)), ("flags", dict(flags=4)), ("flags", dict(flags=-1))]
    both = ("cls", "cost")
    cases = [(w, _cfg(bands, **dict(base, **{k: v for k, v in kw.items() if k in base}), **{k: v for k, v in kw.items() if k not in base}), lut, both) for w, kw in bad]
    cases += [("band", _cfg([(-25, 0)], **base), lut, both), ("band", _cfg([(0, 24)], **base), lut, both), ("band", _cfg([(0, 0), (3, 2)], **base), lut, both),
              ("cost and lut", _cfg(bands, **base), None, both), ("cost and lut", _cfg(bands, **base), lut, ("cls",)), ("every output", _cfg(bands, **base), None, ())]
    rc, full = _raw(L, g, _cfg(bands, **base), lut, (2, N), ORDER)
    assert rc == 0
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for word, cfg, lt, planes in cases:
        rc, bufs = _raw(L, g, cfg, lt, (2, N), planes)
        msg = L.tsl_last_error().decode()
        assert rc == -1 and "nav_terrain:" in msg and word in msg, (word, msg)
        assert _untouched(bufs), word                                 # nothing was written
        assert L.tsl_tsdf_nav_terrain_dev(g.h, C.byref(cfg), p(lt), None, None, None, None, None, p(bufs["cls"]), None, p(bufs["cost"]), None) == -1
        assert "nav_terrain_dev:" in L.tsl_last_error().decode()
        rc, ok = _raw(L, g, _cfg(bands, **base), lut, (2, N), ORDER)    # a good call still succeeds, with the same bytes
        assert rc == 0 and all(ok[k].tobytes() == full[k].tobytes() for k in ORDER), word
    cls = np.zeros((2, N, N), np.uint8)
    assert L.tsl_tsdf_nav_terrain(g.h, None, None, None, None, None, None, None, p(cls), None, None) == -1 and "null cfg" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_terrain(None, C.byref(_cfg(bands)), None, None, None, None, None, None, p(cls), None, None) == -1 and "null handle" in L.tsl_last_error().decode()
    with pytest.raises(ValueError):
        g.nav_terrain(z_range=(0.01, 0.02))                           # no voxel layer
    with pytest.raises(ValueError):
        g.nav_terrain(pick="middle")
    with pytest.raises(ValueError):
        g.nav_terrain(max_slope_deg=90.0)
    with pytest.raises(ValueError):
        g.nav_terrain(radius=7 * VS, lut=np.zeros(5, np.uint8))
    with pytest.raises(_lib.TslError, match="window"):
        g.nav_terrain(window=17 * VS)
    _compare(L, g, o, "after the refusals", bands, **base)


def test_too_high_a_volume_and_too_large_a_grid_are_refused(hip_lib):
    """Nz > 4094: height would not fit; N * N * n_bands >= 2^31 (sparse maps: only the brick tables are that large)"""
    from taichislam_amd.mapping import DenseTSDF
    one = np.zeros(16, np.uint8)                                      # never written: the calls are refused before anything is launched
    g = DenseTSDF(map_scale=[0.64, 163.84], voxel_scale=0.04, num_voxel_per_blk_axis=16, max_submap_num=1, max_bricks=64)
    assert (g.N, g.Nz) == (16, 4096)
    assert hip_lib.tsl_tsdf_nav_terrain(g.h, C.byref(_cfg([(0, 0)])), None, None, None, None, None, None, one.ctypes.data_as(C.c_void_p), None, None) == -1
    assert "nav_terrain:" in hip_lib.tsl_last_error().decode() and "too high" in hip_lib.tsl_last_error().decode()
    g = DenseTSDF(map_scale=[655.36, 0.64], voxel_scale=0.04, num_voxel_per_blk_axis=16, max_submap_num=1, max_bricks=64)
    assert (g.N, g.Nz) == (16384, 16)
    assert hip_lib.tsl_tsdf_nav_terrain(g.h, C.byref(_cfg([(0, 0)] * 8)), None, None, None, None, None, None, one.ctypes.data_as(C.c_void_p), None, None) == -1
    assert "nav_terrain:" in hip_lib.tsl_last_error().decode() and "too large" in hip_lib.tsl_last_error().decode()
    assert g.count_active() == 0


def test_ramp_end_to_end(hip_lib):
    """nav_grid calls the ramp an obstacle; nav_terrain lets the robot up the ramp and not up the cliff; with a slope limit under the ramp's the platform is
    out of reach"""
    geo = "SMALL"
    N = 256
    g, o = _loaded(geo, ns.put(ts.surface(ts.ramp_heights()), geo))
    u = lambda i, j: (i + N // 2, j + N // 2)
    ramp = [u(i, j) for i in range(ts.RAMP_I[0], ts.RAMP_I[1] + 1) for j in range(ts.RAMP_J[0], ts.RAMP_J[1] + 1)]
    grid = g.nav_grid(bands=[(1, 8)], radius=0.0, free_thres=ts.THRES)
    assert all(grid["cls"][0][c] == ref.OCCUPIED for c in ramp if c[0] - N // 2 >= 1)          # every ramp cell with a voxel in the band (heights 16 and up)
    lut = np.array([254, 0], np.uint8)
    kw = dict(bands=[(-2, 8)], clearance=3 * VS, window=VS, slope_base=VS, max_step=2 * VS, min_support=9, radius=0.0, lut=lut, free_thres=ts.THRES)
    t = g.nav_terrain(**kw)
    assert t["max_step_units"] == 32 and t["window_vox"] == 1 and t["max_slope2"] == ref.NO_SLOPE
    ref.assert_equal(t, ref.nav_terrain(o.export_sparse(), N, 256, VS, [(-2, 8)], clearance=3, max_step=32, min_support=9, R=0, lut=lut, free_thres=ts.THRES), "ramp")
    inner = [c for c in ramp if ts.RAMP_J[0] < c[1] - N // 2 < ts.RAMP_J[1] - 2]
    assert all(t["cls"][0][c] == ref.FREE for c in inner)
    assert all(t["cls"][0][u(i, j)] == ref.OCCUPIED for i in (5, 6) for j in range(ts.CLIFF_J[0], ts.CLIFF_J[1]))          # the cliff's edge
    goal, start = u(*ts.RAMP_GOAL), u(*ts.RAMP_START)
    from taichislam_amd.utils.ros_adapters import occupancy_grid_fields
    og = occupancy_grid_fields(t, 0, cost=True)                      # the dict goes where nav_grid's goes
    assert og["data"][u(5, -4)[1] * N + u(5, -4)[0]] == 0 and og["data"][u(5, 3)[1] * N + u(5, 3)[0]] == 100 and og["data"][0] == -1 and og["origin"][2] == -2 * VS
    f = g.nav_field(t, [(0,) + goal])
    p = g.nav_paths(f, [(0,) + start], 200)
    assert p["status"][0] == 0 and 24 < p["length"][0] < 60
    cells = [tuple(int(v) for v in c) for c in p["cells"][0][:p["length"][0]]]
    assert cells[0] == start and cells[-1] == goal
    allowed = {u(i, j) for (i, j) in ts.ramp_heights()}
    assert all(c in allowed and t["cls"][0][c] == ref.FREE for c in cells)
    crossing = [c for c in cells if ts.RAMP_I[0] <= c[0] - N // 2 <= ts.RAMP_I[1]]
    assert crossing and all(ts.RAMP_J[0] <= c[1] - N // 2 <= ts.RAMP_J[1] for c in crossing)                              # it goes up the ramp, not up the cliff
    steep = g.nav_terrain(max_slope_deg=20.0, **kw)
    assert steep["max_slope2"] == 2170 and all(steep["cls"][0][u(i, -4)] == ref.OCCUPIED for i in range(0, 11))
    f = g.nav_field(steep, [(0,) + goal])
    p = g.nav_paths(f, [(0,) + start], 200)
    assert p["status"][0] == 2 and f["field"][0][start] == 0xffffffff and f["field"][0][u(15, -4)] != 0xffffffff

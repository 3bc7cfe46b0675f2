"""The terrain layers without a GPU: the numpy restatement (tests/nav_terrain_ref.py) against the hand-worked values of every scene of
tests/nav_terrain_scenes.py, written out as numbers, and against a second, independent brute-force statement that takes one column or one cell at a time
-- on the scenes and on a seeded random map; plus the bindings and the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nav_grid_scenes as ns
import nav_terrain_ref as ref
import nav_terrain_scenes as ts
from frontier_scenes import GEOMETRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = 0.04


def _u(geo, ij):
    """a scene column in unsigned cell indices"""
    g = GEOMETRIES[geo]
    return ij[0] + g["o"][0] + g["N"] // 2, ij[1] + g["o"][1] + g["N"] // 2


def _run(geo, sc, bands, **kw):
    N, Nz, oz = ns.dims(geo)
    return ref.nav_terrain(sc, N, Nz, VS, [(a + oz, b + oz) for a, b in bands], **kw)


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
def test_columns_have_their_hand_worked_supports(geo):
    N, Nz, oz = ns.dims(geo)
    sc = ns.put(ts.columns(), geo)
    for (fr, pick), answers in ts.COLUMN_ANSWERS.items():
        r = _run(geo, sc, [ts.COLUMN_BAND], clearance=17, free_run=fr, pick=pick, window=0, free_thres=ts.THRES)
        for name, want in answers.items():
            c = _u(geo, ts.COLUMNS[name][0])
            got = (int(r["col"][0][c]), int(r["height"][0][c]))
            exp = (want, 32767) if isinstance(want, int) else (0, 16 * (want[0] + oz) + want[1])
            assert got == exp, (geo, fr, pick, name, got, exp)
        assert int((r["col"][0] != 2).sum()) == len(ts.COLUMNS) - 1                   # every other column of the grid is empty
    # a support exactly at k_min, exactly at k_max, and just outside on either side
    r = _run(geo, sc, ts.EDGE_BANDS, clearance=17, window=0, free_thres=ts.THRES)
    c = _u(geo, ts.COLUMNS["CLEAR1"][0])
    for b, want in enumerate(ts.EDGE_ANSWERS):
        got = (int(r["col"][b][c]), int(r["height"][b][c]))
        assert got == ((want, 32767) if isinstance(want, int) else (0, 16 * (want[0] + oz) + want[1])), (geo, b, got)
    # one layer less of clearance: the blocked columns stand
    r = _run(geo, sc, [ts.COLUMN_BAND], clearance=16, window=0, free_thres=ts.THRES)
    for name, k in (("BLOCK1", -8), ("BLOCK2", -17)):
        assert int(r["height"][0][_u(geo, ts.COLUMNS[name][0])]) == 16 * (k + oz) + 8, name
    # the top of the volume, in the geometry's own indices
    t = Nz // 2 - 1
    r = ref.nav_terrain(ts.top(geo), N, Nz, VS, [(t - 5, t)], clearance=17, window=0, free_thres=ts.THRES)
    assert int(r["height"][0][-20 + N // 2, -20 + N // 2]) == 16 * (t - 3) + 8 and int(r["col"][0][-18 + N // 2, -20 + N // 2]) == 1
    r = ref.nav_terrain(ts.top(geo), N, Nz, VS, [(t - 5, t)], clearance=Nz, free_run=0, window=0, free_thres=ts.THRES)
    assert int(r["height"][0][-18 + N // 2, -20 + N // 2]) == 16 * t and int(r["height"][0][-20 + N // 2, -20 + N // 2]) == 16 * (t - 3) + 8


def test_plane_has_its_closed_form_slope_and_step():
    geo = "SLAB"
    N, Nz, oz = ns.dims(geo)
    sc = ns.put(ts.surface(ts.plane_heights()), geo)
    for s, w in ((1, 1), (2, 3), (4, 0)):
        r = _run(geo, sc, [(-10, 10)], clearance=2, window=w, slope_base=s, free_thres=ts.THRES)
        for (i, j), h in ts.plane_heights().items():
            c = _u(geo, (i, j))
            assert int(r["height"][0][c]) == h + 16 * oz
            inner = lambda m: max(abs(i), abs(j)) <= ts.PLANE_HALF - m
            assert int(r["slope2"][0][c]) == (ts.plane_slope2(s) if inner(s) else ref.NO_SLOPE), (s, i, j)
            if inner(w):
                assert int(r["step"][0][c]) == ts.plane_step(w) and int(r["nsup"][0][c]) == (2 * w + 1) ** 2
    assert ts.plane_slope2(1) == 5120 and ts.plane_slope2(2) == 20480 and ts.plane_step(1) == 24 and ts.plane_step(3) == 72
    # the corner cell of the patch with window 3: a 4 x 4 quarter of the window
    c = _u(geo, (ts.PLANE_HALF, ts.PLANE_HALF))
    r = _run(geo, sc, [(-10, 10)], clearance=2, window=3, slope_base=1, free_thres=ts.THRES)
    assert int(r["nsup"][0][c]) == 16 and int(r["step"][0][c]) == 3 * 4 * 3


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
def test_cliffs_at_the_tile_border_and_the_grid_edges(geo):
    N, Nz, oz = ns.dims(geo)
    r = ref.nav_terrain(ts.surface(ts.cliff_heights(geo)), N, Nz, VS, [(0, 8)], clearance=2, window=1, slope_base=1, max_step=16, free_thres=ts.THRES)
    rise = ts.CLIFF_HIGH - ts.CLIFF_LOW
    assert rise == 53
    st, cl, sl, h = r["step"][0], r["cls"][0], r["slope2"][0], r["height"][0]
    assert h[31, 28] == ts.CLIFF_LOW and h[32, 28] == ts.CLIFF_HIGH and h[28, 32] == ts.CLIFF_HIGH and h[33, 33] == ts.CLIFF_LOW
    assert st[31, 28] == rise and st[32, 28] == rise and st[30, 28] == 0 and st[33, 28] == 0 and st[28, 31] == rise and st[28, 33] == 0
    assert cl[31, 28] == 1 and cl[32, 28] == 1 and cl[30, 28] == 0 and cl[33, 28] == 0 and cl[31, 31] == 1
    assert sl[31, 28] == (4 * rise) ** 2 and sl[28, 32] == (4 * rise) ** 2 and sl[29, 29] == 0 and sl[26, 28] == ref.NO_SLOPE
    assert sl[31, 31] == 2 * (2 * rise) ** 2                 # the corner where the four quadrants meet: gx = gy = -2 * rise
    # the corners of the grid: windows clipped to the grid, no valid stencil on the rim
    assert st[0, 0] == rise and r["nsup"][0][0, 0] == 4 and st[0, 2] == rise and r["nsup"][0][0, 2] == 6 and st[2, 1] == 0 and r["nsup"][0][2, 1] == 9
    assert sl[0, 0] == ref.NO_SLOPE and sl[1, 1] == (4 * rise) ** 2 and sl[2, 2] == 0 and sl[3, 2] == ref.NO_SLOPE
    assert st[N - 1, N - 1] == 0 and st[N - 1, N - 2] == rise and st[N - 2, N - 3] == rise and st[N - 1, N - 4] == 0 and r["nsup"][0][N - 1, N - 1] == 4
    assert sl[N - 2, N - 2] == (4 * rise) ** 2 and sl[N - 1, N - 2] == ref.NO_SLOPE


def test_a_missing_cell_costs_one_support_and_nine_slopes():
    geo = "SLAB"
    sc = ns.put(ts.surface(ts.hole_heights()), geo)
    r = _run(geo, sc, [(0, 6)], clearance=2, window=1, slope_base=2, free_thres=ts.THRES)
    sl, nsup = r["slope2"][0], r["nsup"][0]
    c0 = _u(geo, (0, 0))
    assert r["col"][0][c0] == 2 and nsup[c0] == ref.NO_STAT and sl[c0] == ref.NO_SLOPE
    invalid = [(a, b) for a in range(-3, 4) for b in range(-3, 4) if sl[_u(geo, (a, b))] == ref.NO_SLOPE]
    assert sorted(invalid) == sorted((2 * a, 2 * b) for a in (-1, 0, 1) for b in (-1, 0, 1))          # the nine cells whose stencil holds the hole
    assert all(sl[_u(geo, (a, b))] == 0 for a in range(-3, 4) for b in range(-3, 4) if (a, b) not in invalid)
    assert int((sl != ref.NO_SLOPE).sum()) == 7 * 7 - 9                                             # (the patch's rim of two cells has no stencil either)
    for a in range(-4, 5):
        for b in range(-4, 5):
            if (a, b) != (0, 0):
                assert nsup[_u(geo, (a, b))] == (8 if max(abs(a), abs(b)) == 1 else 9), (a, b)
    assert int((r["step"][0][r["col"][0] == 0] != 0).sum()) == 0


def test_classes_follow_the_order_of_the_tests():
    geo = "TALL"
    sc = ns.put(ts.surface(ts.limit_heights()), geo)
    N, Nz, oz = ns.dims(geo)
    expected = {0: [0, 0, 0, 0], 1: [0, 0, 0, 0], 2: [0, 1, 0, 1], 3: [0, 1, 0, 0], 4: [0, 0, 2, 0], 5: [0, 0, 2, 2], 6: [2, 1, 2, 1], 7: [2, 1, 2, 2], 8: [2, 2, 2, 2],
                9: [0, 1, 0, 1]}
    for n, (ms, msl, mn) in enumerate(ts.LIMIT_SETS):
        r = _run(geo, sc, [(-2, 2)], clearance=2, window=1, slope_base=1, max_step=ms, max_slope2=msl, min_support=mn, free_thres=ts.THRES)
        got = [int(r["cls"][0][_u(geo, cell)]) for cell, _, _, _ in ts.LIMIT_CELLS.values()]
        assert got == ts.limit_classes(ms, msl, mn) == expected[n], (n, got)
        for cell, step, nsup, slope2 in ts.LIMIT_CELLS.values():
            c = _u(geo, cell)
            assert (int(r["step"][0][c]), int(r["nsup"][0][c]), int(r["slope2"][0][c])) == (step, nsup, ref.NO_SLOPE if slope2 is None else slope2)
        assert int((r["cls"][0] != ref.UNKNOWN).sum()) <= 22 and r["cls"][0][0, 0] == ref.UNKNOWN      # empty columns are unknown
    # obstructed columns are occupied whatever the limits, and the distance and the cost follow nav_grid's transform of these classes
    cs = ns.put(ts.columns(), geo)
    lut = (np.arange(3 * 3 + 2) % 7).astype(np.uint8)
    r = _run(geo, cs, [ts.COLUMN_BAND], clearance=17, window=0, min_support=0, R=3, lut=lut, cost_unknown=99, free_thres=ts.THRES)
    w = _u(geo, ts.COLUMNS["WALL"][0])
    assert r["cls"][0][w] == ref.OCCUPIED and r["d2"][0][w] == 0 and r["d2"][0][w[0], w[1] + 2] == 4 and r["cost"][0][w] == 0 and r["cost"][0][0, 0] == 99
    e = _u(geo, ts.COLUMNS["EMPTY"][0])
    assert r["cls"][0][e] == ref.UNKNOWN and r["cost"][0][e] == 99 and r["d2"][0][e] == 4                # two cells from WALL


def test_ramp_scene_by_hand():
    geo = "SMALL"
    sc = ns.put(ts.surface(ts.ramp_heights()), geo)
    r = _run(geo, sc, [(-2, 8)], clearance=3, window=1, slope_base=1, max_step=32, min_support=9, free_thres=ts.THRES)
    cl, st, sl = r["cls"][0], r["step"][0], r["slope2"][0]
    u = lambda i, j: _u(geo, (i, j))
    assert st[u(5, -4)] == 16 and sl[u(5, -4)] == 64 * 64 and cl[u(5, -4)] == 0                        # the ramp: 8 per cell
    assert st[u(5, 3)] == 96 and cl[u(5, 3)] == 1 and cl[u(6, 3)] == 1 and cl[u(4, 3)] == 0 and cl[u(7, 3)] == 0      # the cliff's edge
    assert cl[u(-6, -4)] == 0 and cl[u(18, -4)] == 0 and cl[u(-12, -4)] == 2 and cl[u(5, -8)] == 2      # floor, platform; the rim lacks support
    assert st[u(-1, -4)] == 8 and sl[u(-1, -4)] == 32 * 32 and sl[u(0, -4)] == 64 * 64 and sl[u(11, -4)] == 32 * 32 and sl[u(12, -4)] == 0
    from taichislam_amd.utils import terrain_slope2, terrain_slope_deg
    lim = terrain_slope2(20.0, 1)
    assert lim == 2170 and terrain_slope2(None, 3) == 0xffffffff and terrain_slope2(26.0, 1) < 4096 < terrain_slope2(27.0, 1)
    assert abs(float(terrain_slope_deg(np.array([4096], np.uint32), 1)[0]) - 26.565) < 1e-3 and np.isnan(terrain_slope_deg(np.array([0xffffffff], np.uint32), 1)[0])
    r = _run(geo, sc, [(-2, 8)], clearance=3, window=1, slope_base=1, max_step=32, max_slope2=lim, min_support=9, free_thres=ts.THRES)
    assert all(r["cls"][0][u(i, -4)] == 1 for i in range(0, 11)) and r["cls"][0][u(-1, -4)] == 0 and r["cls"][0][u(11, -4)] == 0


def _against_brute(sc, N, Nz, bands, what, cells=None, **kw):
    """the restatement against brute_column on every column that holds a voxel (and a ring around them) and brute_cell on `cells` or all of those"""
    thres = kw.get("free_thres") or ref.surf_thres(VS)
    r = ref.nav_terrain(sc, N, Nz, VS, bands, **kw)
    look = ref.lookup(sc)
    cols = {(i + a, j + b) for (i, j, _) in look for a in (-1, 0, 1) for b in (-1, 0, 1)}
    cols = sorted(c for c in cols if -(N // 2) <= c[0] < N // 2 and -(N // 2) <= c[1] < N // 2)
    for b, (k0, k1) in enumerate(bands):
        for (i, j) in cols:
            h, c = ref.brute_column(look, Nz, thres, i, j, k0, k1, kw["clearance"], kw.get("free_run", 1), kw.get("pick", 0))
            assert (int(r["height"][b][i + N // 2, j + N // 2]), int(r["col"][b][i + N // 2, j + N // 2])) == (h, c), (what, b, i, j)
        for (i, j) in (cells or cols):
            got = tuple(int(r[k][b][i + N // 2, j + N // 2]) for k in ("step", "nsup", "slope2", "cls"))
            want = ref.brute_cell(r["height"][b], r["col"][b], i + N // 2, j + N // 2, kw.get("window", 1), kw.get("slope_base", 1), kw.get("max_step", 65534),
                                  kw.get("max_slope2", ref.NO_SLOPE), kw.get("min_support", 1))
            assert got == want, (what, b, i, j, got, want)
    return r


def test_restatement_equals_the_brute_force_on_the_scenes():
    for geo in ("SLAB", "TALL"):
        N, Nz, oz = ns.dims(geo)
        sc = ns.put(ts.columns(), geo)
        band = (ts.COLUMN_BAND[0] + oz, ts.COLUMN_BAND[1] + oz)
        for cl, fr, pick, th in ((17, 1, 0, ts.THRES), (17, 0, 1, ts.THRES), (1, 1, 0, None), (0, 0, 1, None), (Nz, 2, 0, ts.THRES), (16, 1, 1, 0.6)):
            _against_brute(sc, N, Nz, [band, (oz - 8, oz - 8), (-(Nz // 2), Nz // 2 - 1)], f"columns on {geo}", clearance=cl, free_run=fr, pick=pick, window=1, free_thres=th)
        t = Nz // 2 - 1
        _against_brute(ts.top(geo), N, Nz, [(t - 5, t), (t, t)], f"top on {geo}", clearance=17, window=0)
        _against_brute(ts.surface(ts.cliff_heights(geo)), N, Nz, [(0, 8)], f"cliffs on {geo}", clearance=2, window=2, slope_base=1, max_step=16, max_slope2=40000, min_support=7,
                       free_thres=ts.THRES)
    N, Nz, oz = ns.dims("SLAB")
    for name, hs, w, s in (("plane", ts.plane_heights(), 3, 2), ("hole", ts.hole_heights(), 1, 2), ("limits", ts.limit_heights(), 1, 1), ("ramp", ts.ramp_heights(), 2, 3)):
        _against_brute(ns.put(ts.surface(hs), "SLAB"), N, Nz, [(oz - 10, oz + 10)], name, clearance=2, window=w, slope_base=s, max_step=20, max_slope2=3000, min_support=8,
                       free_thres=ts.THRES)


def test_restatement_equals_the_brute_force_on_a_random_map():
    rng = np.random.default_rng(4117)
    N, Nz = 64, 128                                              # TALL
    occ_v, free_v = [0.0, 0.03, 0.0712, -0.2, -np.inf, 2.0 ** -24], [0.0725, 0.1, 0.3, 0.5, np.inf]
    vox = {}
    for i in range(-12, 12):                                     # a rough ground: three occupied layers under three free ones in most columns ...
        for j in range(-12, 12):
            if rng.random() < 0.85:
                kg = int(rng.integers(-6, 4))
                for d in range(-2, 4):
                    vox[(i, j, kg + d)] = rng.choice(occ_v if d <= 0 else free_v)
    for i, j, k in zip(rng.integers(-12, 12, 1500), rng.integers(-12, 12, 1500), rng.integers(-20, 12, 1500)):      # ... and noise of every kind of value
        vox[(int(i), int(j), int(k))] = rng.choice(occ_v + free_v + [np.nan])
    sc = {"indices": np.array(list(vox), np.int16), "TSDF": np.array(list(vox.values()), np.float16)}
    cells = [(int(a), int(b)) for a, b in rng.integers(-14, 14, (150, 2))]
    seen = set()
    for cl, fr, pick, w, s in ((3, 1, 0, 1, 1), (0, 0, 1, 2, 2), (6, 2, 0, 0, 3), (20, 1, 1, 3, 1)):
        r = _against_brute(sc, N, Nz, [(-20, 11), (-5, 3), (0, 0)], "random", cells=cells, clearance=cl, free_run=fr, pick=pick, window=w, slope_base=s, max_step=40,
                           max_slope2=20000, min_support=3)
        assert len(np.unique(r["col"])) == (3 if cl else 2) and (r["slope2"] != ref.NO_SLOPE).any()      # (clearance 0, free_run 0: every occupied voxel stands)
        assert len(np.unique(r["height"][r["col"] == 0] & 15)) > 4
        seen |= set(np.unique(r["cls"]).tolist())
    assert seen == {0, 1, 2}


def test_bindings_header_and_refusals_that_need_no_device():
    from taichislam_amd import _lib
    from taichislam_amd.mapping import dense_tsdf
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    for name, kid, text in (("TSL_K_NAV_TERRAIN_COLUMNS", _lib.K_NAV_TERRAIN_COLUMNS, "nav_terrain_columns"), ("TSL_K_NAV_TERRAIN_WINDOW", _lib.K_NAV_TERRAIN_WINDOW, "nav_terrain_window")):
        assert int(re.search(name + r" = (\d+)", hdr).group(1)) == kid and _lib.KERNEL_NAMES[kid] == text
    assert re.search(r"TSL_K_NAV_TERRAIN_WINDOW = 29,\s*TSL_K_COUNT", hdr)
    assert int(re.search(r"#define TSL_TERRAIN_NO_HEIGHT (\d+)", hdr).group(1)) == ref.NO_HEIGHT == _lib.TERRAIN_NO_HEIGHT == dense_tsdf.TERRAIN_NO_HEIGHT
    assert int(re.search(r"#define TSL_TERRAIN_NO_SLOPE (0x[0-9a-f]+)u", hdr).group(1), 16) == ref.NO_SLOPE == _lib.TERRAIN_NO_SLOPE == dense_tsdf.TERRAIN_NO_SLOPE
    assert C.sizeof(_lib.NavTerrainCfg) == 4 + 64 + 64 + 4 + 7 * 4 + 4 + 8 + 4 == 180 and _lib.NavTerrainCfg.max_slope2.offset == 164 and _lib.NavTerrainCfg.cost_unknown.offset == 176
    L = _lib.lib()
    for name in ("tsl_tsdf_nav_terrain", "tsl_tsdf_nav_terrain_dev"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    cfg = _lib.NavTerrainCfg()
    assert L.tsl_tsdf_nav_terrain(None, C.byref(cfg), None, None, None, None, None, None, None, None, None) == -1 and "nav_terrain: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_terrain_dev(None, C.byref(cfg), None, None, None, None, None, None, None, None, None, None) == -1
    assert "nav_terrain_dev: null handle" in L.tsl_last_error().decode()

"""The navigation grids without a GPU: the numpy restatement's distance transform (tests/nav_grid_ref.py) against an independent brute-force distance
and against hand-worked answers, the inflation table, the OccupancyGrid fields, and the bindings."""
import re
import os

import numpy as np
import pytest

import nav_grid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("R", [0, 1, 5, 20, 254])
@pytest.mark.parametrize("wall", [False, True])
def test_restatement_equals_the_brute_force_distance(R, wall):
    rng = np.random.default_rng(100 + R)
    for n, m, density in ((48, 48, 0.004), (48, 48, 0.05), (17, 31, 0.02), (1, 9, 0.3), (40, 23, 0.0)):
        obst = rng.random((n, m)) < density
        got, want = ref.edt(obst, R, wall), ref.brute_d2(obst, R, wall)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (n, m, density)


def test_hand_worked_distances():
    o = np.zeros((21, 21), bool)
    o[10, 10] = True
    d = ref.edt(o, 5)
    assert d[10, 10] == 0 and d[13, 14] == 25 and d[15, 10] == 25 and d[10, 5] == 25 and d[7, 6] == 25
    assert d[14, 14] == 26 and d[16, 10] == 26 and d[10, 4] == 26 and d[0, 0] == 26          # (4, 4): 32 > 25; (6, 0): 36 > 25
    assert d[11, 12] == 5 and d[12, 12] == 8
    d0 = ref.edt(o, 0)
    assert set(np.unique(d0).tolist()) == {0, 1} and d0[10, 10] == 0 and d0.sum() == 21 * 21 - 1
    # obstacles at (0, 0) and (1, -3): at (1, 0) the nearest obstacle of the row is 3 away, the nearest of the plane 1
    o = np.zeros((9, 9), bool)
    o[4, 4] = True
    o[5, 1] = True
    d = ref.edt(o, 5)
    assert d[5, 4] == 1 and d[5, 2] == 1 and d[5, 3] == 2 and d[6, 4] == 4
    assert (ref.edt(np.zeros((12, 7), bool), 3) == 10).all()                                 # an empty grid is all far
    assert (ref.edt(np.ones((12, 7), bool), 3) == 0).all()                                   # a full grid is all 0
    w = ref.edt(np.zeros((6, 6), bool), 2, wall=True)                                        # the wall alone: 1 at the rim, 4 next to it, far in the middle
    assert w[0, 3] == 1 and w[3, 5] == 1 and w[1, 3] == 4 and w[2, 2] == 5 and w[0, 0] == 1 and w[1, 1] == 4


def test_cell_classes_follow_the_order_of_the_tests():
    import nav_grid_scenes as ns
    c = np.array([[no, nf, 6 - no - nf] for no, nf in ns.LIMIT_COLUMNS], np.uint16)
    assert ref.cell_classes(c, 2, 3, 0).tolist() == ns.limit_classes(2, 3, 0) == [0, 1, 2, 2, 0, 2, 2, 2, 1, 2]
    assert ref.cell_classes(c, 2, 3, None).tolist() == ns.limit_classes(2, 3, None) == [0, 1, 2, 0, 0, 0, 0, 2, 1, 2]
    assert ref.cell_classes(c, 0, 0, None).tolist() == ns.limit_classes(1, 1, None) == [1, 1, 1, 1, 0, 0, 0, 0, 1, 1]


def test_restatement_of_the_columns_scene():
    """voxel classes, counts and spans of the hand-built columns, from their definition"""
    import nav_grid_scenes as ns
    N, Nz, oz = ns.dims("SLAB")
    sc = ns.put(ns.columns(), "SLAB")
    r = ref.nav_grid(sc, N, Nz, 0.04, [(-Nz // 2, Nz // 2 - 1), (oz, oz + 2)], 3)
    o = 8 + N // 2                                              # scene (0, 0) in unsigned indices
    gap, nan = (o + ns.COL_GAP[0], o + ns.COL_GAP[1]), (o + ns.COL_NAN[0], o + ns.COL_NAN[1])
    assert r["counts"][0][gap].tolist() == [1, 1, Nz - 2] and r["span"][0][gap].tolist() == [-20 + oz, -20 + oz] and r["cls"][0][gap] == ref.OCCUPIED
    assert r["counts"][1][gap].tolist() == [0, 0, 3] and r["span"][1][gap].tolist() == [32767, -32768] and r["cls"][1][gap] == ref.UNKNOWN
    assert r["counts"][1][nan].tolist() == [0, 2, 1] and r["cls"][1][nan] == ref.FREE          # the NaN between two free voxels is unknown
    assert r["d2"][0][gap] == 0 and r["d2"][0][gap[0] + 1, gap[1] + 1] == 2


def test_inflation_lut():
    from taichislam_amd.utils import inflation_lut
    for R, ins, infl in ((25, 0.2, 0.8), (5, 0.0, 0.1), (0, 0.1, 0.3), (254, 1.0, 12.0)):
        lut = inflation_lut(0.04, R, ins, infl)
        assert lut.dtype == np.uint8 and lut.shape == (R * R + 2,)
        assert lut[0] == 254 and lut[-1] == 0 and (np.diff(lut.astype(np.int64)) <= 0).all()
    lut = inflation_lut(0.04, 25, 0.21, 0.81, scale=3.0)
    assert lut[1] == 253 and lut[25] == 253 and lut[26] == 253 and lut[28] == int(np.floor(252 * np.exp(-3.0 * (np.sqrt(28.0) * 0.04 - 0.21)))) == 250      # d = 0.04, 0.2, 0.204, 0.2117
    assert lut[400] == int(np.floor(252 * np.exp(-3.0 * (0.8 - 0.21)))) == 42 and lut[410] == 41 and lut[411] == 0      # 0.04 * sqrt(410) = 0.8099 is inside the inflation radius, 0.04 * sqrt(411) = 0.8109 is not
    with pytest.raises(ValueError):
        inflation_lut(0.04, 255, 0.1, 0.2)
    with pytest.raises(ValueError):
        inflation_lut(0.04, 5, 0.3, 0.2)


def test_occupancy_grid_fields_transpose():
    from taichislam_amd.utils.ros_adapters import occupancy_grid_fields
    cls = np.full((2, 4, 4), ref.UNKNOWN, np.uint8)
    cls[1, 3, 0] = ref.OCCUPIED                  # x = 3, y = 0
    cls[1, 0, 2] = ref.FREE                      # x = 0, y = 2
    cls[1, 1, 2] = ref.FREE                      # x = 1, y = 2
    cost = np.zeros((2, 4, 4), np.uint8)
    cost[1, 3, 0], cost[1, 0, 2], cost[1, 1, 2] = 254, 127, 1
    grid = {"cls": cls, "cost": cost, "voxel": 0.5, "origin_xy": -1.25, "bands": [(0, 0), (-2, 3)]}
    f = occupancy_grid_fields(grid, 1)
    assert f["resolution"] == 0.5 and f["width"] == 4 and f["height"] == 4 and f["origin"] == (-1.25, -1.25, -1.0)
    d = f["data"]
    assert d.dtype == np.int8 and d.shape == (16,)
    assert d[0 * 4 + 3] == 100 and d[2 * 4 + 0] == 0 and d[2 * 4 + 1] == 0 and (np.delete(d, [3, 8, 9]) == -1).all()
    c = occupancy_grid_fields(grid, 1, cost=True)["data"]
    assert c[3] == 100 and c[8] == 50 and c[9] == 0 and (np.delete(c, [3, 8, 9]) == -1).all()
    assert (occupancy_grid_fields(grid, 0)["data"] == -1).all()
    with pytest.raises(ValueError):
        occupancy_grid_fields(grid, 2)
    with pytest.raises(ValueError):
        occupancy_grid_fields({k: v for k, v in grid.items() if k != "cost"}, 1, cost=True)


def test_bindings_and_header():
    import ctypes as C
    from taichislam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    for name, kid, text in (("TSL_K_NAV_PROJECT", _lib.K_NAV_PROJECT, "nav_project"), ("TSL_K_NAV_EDT", _lib.K_NAV_EDT, "nav_edt"),
                            ("TSL_K_NAV_EDT_ROWS", _lib.K_NAV_EDT_ROWS, "nav_edt_rows")):
        assert int(re.search(name + r" = (\d+)", hdr).group(1)) == kid and _lib.KERNEL_NAMES[kid] == text
    assert C.sizeof(_lib.NavCfg) == 4 * (1 + 16 + 16 + 1 + 5) + 4 and _lib.NavCfg.free_thres.offset == 132 and _lib.NavCfg.cost_unknown.offset == 156
    L = _lib.lib()
    for name in ("tsl_tsdf_nav_grid", "tsl_tsdf_nav_grid_dev"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # a null handle is refused by name before anything touches a device
    cfg = _lib.NavCfg()
    assert L.tsl_tsdf_nav_grid(None, C.byref(cfg), None, None, None, None, None, None) == -1 and "nav_grid: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_grid_dev(None, C.byref(cfg), None, None, None, None, None, None, None) == -1 and "nav_grid_dev: null handle" in L.tsl_last_error().decode()
    for k, v in (("TSL_NAV_FREE", ref.FREE), ("TSL_NAV_OCCUPIED", ref.OCCUPIED), ("TSL_NAV_UNKNOWN", ref.UNKNOWN)):
        assert int(re.search(r"#define " + k + r" (\d+)", hdr).group(1)) == v
    from taichislam_amd.mapping import dense_tsdf
    assert (dense_tsdf.NAV_FREE, dense_tsdf.NAV_OCCUPIED, dense_tsdf.NAV_UNKNOWN) == (ref.FREE, ref.OCCUPIED, ref.UNKNOWN)

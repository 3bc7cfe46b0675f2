"""The cost-to-go field without a GPU: the two restatements of tests/nav_field_ref.py (whole-grid relaxation and a heap Dijkstra) against each other on
every scene of tests/nav_field_scenes.py and against hand-worked answers, the parents and the path walk, frontier_reach, and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nav_field_ref as ref
import nav_field_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenes():
    out = [(f"random {H} x {W}", random[0], random[1], {}) for H, W in sc.SHAPES for random in [sc.random_plane(H, W)]]
    out += [("serpentine", *sc.serpentine(), {}), ("corner block", *sc.corner_block(), {}), ("diagonal corridor", *sc.diagonal_corridor(), {}),
            ("staircase, 4", *sc.staircase_corridor(), dict(connectivity=4)), ("staircase, 8", *sc.staircase_corridor(), {}),
            ("uniform", *sc.uniform(), {}), ("uniform, 4", *sc.uniform(), dict(connectivity=4)), ("checkerboard", *sc.checkerboard(), {}),
            ("seeds", *sc.many_seeds()[:2], {}), ("16 planes", *sc.sixteen_planes(), {}), ("walled in", *sc.walled_in(), {}),
            ("lethal 1, 4", *sc.binary_plane(4)[:2], dict(lethal=1, connectivity=4)), ("lethal 1, neutral 255", *sc.binary_plane()[:2], dict(lethal=1, neutral=255)),
            ("lethal 255, neutral 255", *sc.random_plane(33, 31)[:2], dict(lethal=255, neutral=255)),
            ("neutral 1", *sc.random_plane(33, 31)[:2], dict(neutral=1)), ("ribbon", sc.ribbon(300)[0], sc.ribbon(300)[1], {})]
    return out


@pytest.mark.parametrize("name,cost,goals,kw", _scenes(), ids=[s[0] for s in _scenes()])
def test_the_two_restatements_agree(name, cost, goals, kw):
    a, bad_a = ref.relax(cost, goals, **kw)
    b, bad_b = ref.dijkstra(cost, goals, **kw)
    assert a.dtype == np.uint32 and np.array_equal(a, b) and bad_a == bad_b, name
    par = ref.parents(cost, a, goals, **kw)
    trav = ref.planes(cost) < kw.get("lethal", 253)
    assert ((par == 255) == (a == ref.UNREACHED)).all() and (a[~trav] == ref.UNREACHED).all()


def test_scenes_reach_what_they_are_there_for():
    for H, W in sc.SHAPES:
        cost, goals, comp = sc.random_plane(H, W)
        f, bad = ref.relax(cost, goals)
        assert bad == 0 and np.array_equal(f[0] != ref.UNREACHED, comp), (H, W)            # exactly the goal's component, the largest
        assert comp.sum() * 2 >= (cost < 253).sum() or H * W < 100, (H, W)
    cost, goals = sc.serpentine()
    f, _ = ref.relax(cost, goals)
    assert f[0, 95, 0] != ref.UNREACHED and f[0, 95, 95] != ref.UNREACHED
    assert f[0, 95, 0] > 5 * 50 * 95 * 5                                                    # far longer than the straight way down: it crosses the plane per wall
    cost, goals = sc.corner_block()
    assert ref.relax(cost, goals)[0][0, 2, 2] == ref.UNREACHED and ref.relax(cost, goals)[0][0, 1, 1] == 0
    cost, goals = sc.diagonal_corridor()
    f, _ = ref.relax(cost, goals)
    assert (f != ref.UNREACHED).sum() == 1
    cost, goals = sc.staircase_corridor()
    for conn in (4, 8):
        f, _ = ref.relax(cost, goals, connectivity=conn)
        assert f[0, 11, 11] == 22 * 5 * 50                                                  # 22 axis moves: the diagonals stay corner cuts with 8 too
    cost, goals = sc.walled_in()
    f, _ = ref.relax(cost, goals)
    assert f[0, 5, 5] == ref.UNREACHED and cost[5, 5] == 0 and (f[0] != ref.UNREACHED).sum() == 400 - 9
    cost, goals, n_bad = sc.many_seeds()
    r = ref.field_and_parent(cost, goals)
    assert r["n_bad_seeds"] == n_bad and r["parent"][0, 10, 41] != 8 and r["parent"][0, 10, 40] == 8 and r["field"][0, 30, 30] == 700
    assert r["field"][0, 10, 41] == 250 + 5 * (50 + int(cost[10, 41]))
    cost, goals = sc.sixteen_planes()
    f, _ = ref.relax(cost, goals)
    assert all((f[b] != ref.UNREACHED).sum() * 2 >= (cost[b] < 253).sum() for b in range(16))


def test_hand_worked_field_and_parents():
    cost = np.array([[0, 10, 0], [0, 254, 0], [0, 0, 0]], np.uint8)
    f, bad = ref.relax(cost, [[0, 0, 0]])
    assert bad == 0 and f[0, 0, 0] == 0 and f[0, 0, 1] == 5 * 60 and f[0, 1, 0] == 250 and f[0, 0, 2] == 250 + 300
    assert f[0, 1, 1] == ref.UNREACHED
    assert f[0, 2, 1] == 250 + 250 + 250                       # (2, 1) -> (2, 0) -> (1, 0) -> (0, 0): the diagonal past the wall is a corner cut
    assert f[0, 2, 2] == min(4 * 250, 250 + 300 + 500)
    par = ref.parents(cost, f, [[0, 0, 0]])
    assert par[0, 0, 0] == 8 and par[0, 1, 1] == 255 and par[0, 0, 1] == 6 and par[0, 1, 0] == 4 and par[0, 2, 1] == 6 and par[0, 2, 2] == 6
    cells, length, status, c = ref.follow(f, par, [[0, 2, 2], [0, 1, 1], [0, 3, 0], [0, 0, 0], [0, 2, 2]], 5)
    assert status.tolist() == [0, 2, 3, 0, 0] and length.tolist() == [5, 0, 0, 1, 5] and c[0] == 1000 and c[1] == ref.UNREACHED and c[2] == ref.UNREACHED
    assert cells[0].tolist() == [[2, 2], [2, 1], [2, 0], [1, 0], [0, 0]] and (cells[1] == -1).all() and cells[3].tolist() == [[0, 0]] + [[-1, -1]] * 4
    ref.check_path(cost, f, par, [[0, 0, 0]], cells[0], length[0])
    _, length, status, _ = ref.follow(f, par, [[0, 2, 2]], 4)
    assert status.tolist() == [1] and length.tolist() == [4]
    # ties on a uniform plane take the lowest code; saturation clips and never wraps
    u, g = sc.uniform()
    r = ref.field_and_parent(u, g)
    assert r["parent"][0, 16, 19] == 1 and r["parent"][0, 18, 21] == 5 and r["parent"][0, 16, 20] == 0 and r["parent"][0, 17, 10] == 2
    assert r["parent"][0, 15, 19] == 0                          # (15, 19) to (17, 20): down then diagonal or diagonal then down, both 12 * 50: code 0 wins over 1
    row = np.zeros((1, 70), np.uint8)
    f, _ = ref.relax(row, [[0, 0, 0, (1 << 32) - 100]])
    assert f[0, 0, 0] == (1 << 32) - 100 and f[0, 0, 1] == ref.MAXV and (f[0, 0, 1:] == ref.MAXV).all()
    f2, _ = ref.dijkstra(row, [[0, 0, 0, -100]])                # the value is read as uint32
    assert np.array_equal(f, f2)


def test_a_partial_field_relaxes_to_the_same_fixed_point():
    """the property the max_rounds test leans on: relaxation started from upper bounds that are costs of real move sequences ends on the field"""
    cost, goals = sc.serpentine(48, 8, 3)
    f, _ = ref.relax(cost, goals)
    part = f.astype(np.int64)
    part[0, 24:] = ref.UNREACHED                                # the lower half not reached yet
    part[0, 10, 5] += 35                                        # one value not settled yet
    g, _ = ref.relax(cost, goals, start=part)
    assert np.array_equal(g, f)


def test_frontier_reach_on_a_hand_made_cluster_list():
    from taichislam_amd.utils import frontier_reach
    N = 8
    field = np.full((2, N, N), ref.UNREACHED, np.uint32)
    field[1, 4, 4], field[1, 4, 5], field[1, 0, 0], field[1, 7, 7] = 500, 300, 40, 7
    idx = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 9],            # cluster 0: columns (4, 4) = 500 and (4, 5) = 300; the third voxel is above the band
                    [-4, -4, 0], [-4, -4, 2],                   # cluster 1: column (0, 0) = 40, twice: the first row wins
                    [1, 1, 1],                                  # cluster 2: column (5, 5) is unreached
                    [3, 3, 5]], np.int16)                       # cluster 3: column (7, 7) = 7, but no voxel in the band
    fr = {"indices": idx, "cluster": np.array([0, 0, 0, 1, 1, 2, 3], np.int32), "clusters": np.zeros(5)}      # cluster 4 has no voxel at all
    got = frontier_reach(fr, {"field": field}, (0, 2), N, plane=1)
    assert got["value"].dtype == np.uint32 and got["value"].tolist() == [300, 40, ref.UNREACHED, ref.UNREACHED, ref.UNREACHED]
    assert got["voxel"].tolist() == [1, 3, -1, -1, -1] and got["reached"].tolist() == [True, True, False, False, False]
    wide = frontier_reach(fr, field[1], (0, 9))                 # a bare plane, N from its shape
    assert wide["value"].tolist() == [300, 40, ref.UNREACHED, 7, ref.UNREACHED] and wide["voxel"].tolist() == [1, 3, -1, 6, -1]
    # a torch build without uint32 hands the field's bits over as int32, -1 in an unreached cell: the same answer
    signed = field.view(np.int32)
    assert signed.dtype == np.int32 and signed[1, 5, 5] == -1
    for args, kw, want in (((fr, {"field": signed}, (0, 2), N), dict(plane=1), got), ((fr, signed[1], (0, 9)), {}, wide)):
        again = frontier_reach(*args, **kw)
        for k in ("value", "voxel", "reached"):
            assert again[k].dtype == want[k].dtype and np.array_equal(again[k], want[k]), k


def test_bindings_header_and_refusals_that_need_no_device():
    from taichislam_amd import _lib
    from taichislam_amd.mapping import dense_tsdf
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    for name, kid, text in (("TSL_K_NAV_FIELD_SEED", _lib.K_NAV_FIELD_SEED, "nav_field_seed"), ("TSL_K_NAV_FIELD_ROUND", _lib.K_NAV_FIELD_ROUND, "nav_field_round"),
                            ("TSL_K_NAV_FIELD_PARENT", _lib.K_NAV_FIELD_PARENT, "nav_field_parent"), ("TSL_K_NAV_FIELD_PATHS", _lib.K_NAV_FIELD_PATHS, "nav_field_paths")):
        assert int(re.search(name + r" = (\d+)", hdr).group(1)) == kid and _lib.KERNEL_NAMES[kid] == text
    assert int(re.search(r"#define TSL_NAV_UNREACHED (0x[0-9a-f]+)u", hdr).group(1), 16) == ref.UNREACHED == _lib.NAV_UNREACHED == dense_tsdf.NAV_UNREACHED
    assert C.sizeof(_lib.NavFieldCfg) == 40 and _lib.NavFieldCfg.check_every.offset == 32
    assert C.sizeof(_lib.NavFieldStats) == 24 and _lib.NavFieldStats.tile_visits.offset == 8 and _lib.NavFieldStats.n_bad_seeds.offset == 16
    L = _lib.lib()
    names = ("tsl_tsdf_nav_field", "tsl_tsdf_nav_field_dev", "tsl_tsdf_nav_field_paths", "tsl_tsdf_nav_field_paths_dev")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(L, name)
    # a null handle is refused by name before anything touches a device
    cfg = _lib.NavFieldCfg()
    st = _lib.NavFieldStats()
    assert L.tsl_tsdf_nav_field(None, C.byref(cfg), None, None, 0, None, None, C.byref(st)) == -1 and "nav_field: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field_dev(None, C.byref(cfg), None, None, 0, None, None, None, None) == -1 and "nav_field_dev: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field_paths(None, C.byref(cfg), None, None, None, 0, 1, None, None, None, None) == -1
    assert "nav_field_paths: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field_paths_dev(None, C.byref(cfg), None, None, None, 0, 1, None, None, None, None, None) == -1
    assert "nav_field_paths_dev: null handle" in L.tsl_last_error().decode()

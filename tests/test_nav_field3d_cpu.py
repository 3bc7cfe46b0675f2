"""The 3-D cost-to-go field without a GPU: the two restatements of tests/nav_field3d_ref.py (whole-volume relaxation and a heap Dijkstra) against each
other on every scene of tests/nav_field3d_scenes.py, against the 2-D restatement on volumes of one layer and against hand-worked answers; the parents and
the path walk; distance_cost, flight_lut and frontier_reach3d; and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nav_field3d_ref as ref
import nav_field3d_scenes as sc
import nav_field_ref as ref2
import nav_field_scenes as sc2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenes():
    out = []
    for s in sc.SHAPES:
        cost, goals, _ = sc.random_volume(*s)
        out += [(f"random {s}, {conn}", cost, goals, dict(connectivity=conn)) for conn in (6, 18, 26)]
    out += [(f"serpentine, {conn}", *sc.serpentine(), dict(connectivity=conn)) for conn in (6, 26)]
    out += [(f"face diagonal, {w} walled", *sc.face_diagonal(w), {}) for w in (None, 0, 1)]
    out += [(f"space diagonal, {w} walled", *sc.space_diagonal(w), {}) for w in (None, 0, 1, 2, 3, 4, 5)]
    out += [(f"uniform, {conn}", *sc.uniform(), dict(connectivity=conn)) for conn in (6, 18, 26)]
    out += [("uniform, two seeds", *sc.uniform_two_seeds(), {})]
    out += [(f"checkerboard, {conn}", *sc.checkerboard(), dict(connectivity=conn)) for conn in (6, 18, 26)]
    out += [("seeds", *sc.many_seeds()[:2], {}), ("saturated", *sc.saturated(), {}), ("walled in", *sc.walled_in(), {}),
            ("lethal 1, 6", *sc.binary_volume(6)[:2], dict(lethal=1, connectivity=6)), ("lethal 1, neutral 255", *sc.binary_volume()[:2], dict(lethal=1, neutral=255)),
            ("lethal 255, neutral 255", *sc.random_volume(*sc.SHAPES[4])[:2], dict(lethal=255, neutral=255)),
            ("neutral 1", *sc.random_volume(*sc.SHAPES[4])[:2], dict(neutral=1))]
    return out


_SCENES = _scenes()


@pytest.mark.parametrize("name,cost,goals,kw", _SCENES, ids=[s[0] for s in _SCENES])
def test_the_two_restatements_agree(name, cost, goals, kw):
    assert cost.size <= 40000
    a, bad_a = ref.relax(cost, goals, **kw)
    b, bad_b = ref.dijkstra(cost, goals, **kw)
    assert a.dtype == np.uint32 and np.array_equal(a, b) and bad_a == bad_b, name
    par = ref.parents(cost, a, goals, **kw)
    trav = cost < kw.get("lethal", 253)
    assert ((par == 255) == (a == ref.UNREACHED)).all() and (a[~trav] == ref.UNREACHED).all()
    codes = par[par < ref.SEED]
    assert all(ref.NZ[d] <= ref.MAXNZ[kw.get("connectivity", 26)] for d in np.unique(codes).tolist())


def test_direction_codes_are_the_contract():
    assert len(ref.DIRS) == 26 and len(set(ref.DIRS)) == 26
    assert ref.DIRS[:8] == tuple((0,) + d for d in ref2.DIRS)                              # codes 0 .. 7: nav_field's, in its order
    assert ref.DIRS[8] == (1, 0, 0) and ref.DIRS[9:17] == tuple((1,) + d for d in ref2.DIRS)
    assert ref.DIRS[17] == (-1, 0, 0) and ref.DIRS[18:] == tuple((-1,) + d for d in ref2.DIRS)
    assert sorted(ref.STEP) == [5] * 6 + [7] * 12 + [9] * 8 and ref.STEP[:8] == ref2.STEP


@pytest.mark.parametrize("H,W", sc2.SHAPES + [(40, 45)])
def test_one_layer_is_the_2d_problem(H, W):
    cost, goals, _ = sc2.random_plane(H, W) if (H, W) != (40, 45) else sc2.checkerboard() + (None,)
    for c3, c2 in ((26, 8), (6, 4)):
        f3, bad3 = ref.relax(cost[None], goals, connectivity=c3)
        f2, bad2 = ref2.relax(cost, goals, connectivity=c2)
        assert np.array_equal(f3, f2) and bad3 == bad2, (H, W, c3)
        p3 = ref.parents(cost[None], f3, goals, connectivity=c3)
        p2 = ref2.parents(cost, f2, goals, connectivity=c2)
        assert np.array_equal(p3, np.where(p2 == 8, ref.SEED, p2)), (H, W, c3)
    f18, _ = ref.relax(cost[None], goals, connectivity=18)                               # with one layer 18 has the same moves as 26
    assert np.array_equal(f18, ref.relax(cost[None], goals, connectivity=26)[0])


def test_scenes_reach_what_they_are_there_for():
    for s in sc.SHAPES:
        cost, goals, comp = sc.random_volume(*s)
        f, bad = ref.relax(cost, goals)
        assert bad == 0 and np.array_equal(f != ref.UNREACHED, comp), s                    # exactly the goal's component, the largest
        assert 0.25 < (cost >= 253).mean() < 0.45 or cost.size < 200, s
    cost, goals = sc.serpentine()
    f, _ = ref.relax(cost, goals)
    assert (f != ref.UNREACHED).sum() == (cost < 253).sum()                              # one component: the snake reaches every free cell
    far = int(f[f != ref.UNREACHED].max())
    assert far > 20 * 5 * 50 * 23                                                         # far longer than any straight way: it crosses every slab band by band
    par = ref.parents(cost, f, goals)
    start = np.argwhere(f == far)[0]
    cells, length, status, _ = ref.walk(f, par, [start], 4000)
    p = cells[0, :length[0]].astype(int)
    tiles = np.stack([p[:, 0] // sc.TK, p[:, 1] // sc.TI, p[:, 2] // sc.TJ], 1)
    cross = int((np.diff(tiles, axis=0) != 0).any(1).sum())
    assert status[0] == 0 and len(np.unique(tiles, axis=0)) == 18 and cross > 2 * 18      # the way re-enters tiles: more crossings than there are tiles
    for w in (0, 1):                                                                      # a face diagonal with either of its two cells walled: round the corner
        assert ref.relax(*sc.face_diagonal(w))[0][1, 2, 2] == 2 * 5 * 50
    assert ref.relax(*sc.face_diagonal(None))[0][1, 2, 2] == 7 * 50
    for w in range(6):                                                                    # a space diagonal with any of its six cells walled: 7 + 5 at best
        r = ref.field_and_parent(*sc.space_diagonal(w))
        assert r["field"][2, 2, 2] == (7 + 5) * 50 and ref.NZ[r["parent"][2, 2, 2]] < 3, w
    r = ref.field_and_parent(*sc.space_diagonal(None))
    assert r["field"][2, 2, 2] == 9 * 50 and r["parent"][2, 2, 2] == 23                   # (-1, -1, -1)
    cost, goals = sc.walled_in()
    f, _ = ref.relax(cost, goals)
    assert f[5, 5, 5] == ref.UNREACHED and cost[5, 5, 5] == 0 and (f != ref.UNREACHED).sum() == cost.size - 27
    cost, goals, n_bad = sc.many_seeds()
    r = ref.field_and_parent(cost, goals)
    assert r["n_bad_seeds"] == n_bad and r["parent"][3, 10, 31] != ref.SEED and r["parent"][3, 10, 30] == ref.SEED and r["field"][15, 12, 22] == 700
    assert r["field"][3, 10, 31] == 250 + 5 * (50 + int(cost[3, 10, 31]))
    for k, i, j, v in goals[7:11].tolist():                                               # the seeds on a tile face, edge and corners hold their values
        assert r["field"][k, i, j] == v and r["parent"][k, i, j] == ref.SEED
    assert (k % sc.TK in (0, sc.TK - 1) and i % sc.TI in (0, sc.TI - 1) and j % sc.TJ in (0, sc.TJ - 1))


def test_hand_worked_ties_take_the_lowest_code():
    """uniform cost 0, neutral 50: the field is 50 times the <5, 7, 9> chamfer distance to the seed, and every parent can be read off it"""
    r = ref.field_and_parent(*sc.uniform())
    s = np.array(sc.UNIFORM_SEED)
    f, par = r["field"], r["parent"]
    at = lambda *d: tuple(s + np.array(d))
    assert f[at(0, 0, 3)] == 15 * 50 and f[at(-1, 2, 0)] == 12 * 50 and f[at(2, 2, 2)] == 18 * 50 and f[at(3, -2, 1)] == (9 + 7 + 5) * 50
    assert par[at(0, 0, 0)] == 26 and par[at(0, 0, 3)] == 6 and par[at(1, 0, 0)] == 17 and par[at(-1, 0, 0)] == 8
    assert par[at(-1, -1, -1)] == 10 and par[at(2, 2, 2)] == 23
    # (-1, 2, 0): (0, -1, 0) = code 4 leaves (-1, 1, 0) = 7, (1, -1, 0) = code 13 leaves (0, 1, 0) = 5: both 12 -- in-plane against dk = +1, 4 wins
    assert par[at(-1, 2, 0)] == 4
    # (-2, 1, 0): (1, 0, 0) = code 8 leaves (-1, 1, 0) = 7, (1, -1, 0) = code 13 leaves (-1, 0, 0) = 5: both 12 -- two codes with dk = +1, 8 wins
    assert par[at(-2, 1, 0)] == 8
    # (1, 2, 0): code 4 against (-1, -1, 0) = code 22 -- in-plane against dk = -1
    assert par[at(1, 2, 0)] == 4
    # two seeds above one another: half way up the move up (code 8) ties with the move down (code 17)
    r2 = ref.field_and_parent(*sc.uniform_two_seeds())
    assert r2["field"][8, 9, 17] == 4 * 5 * 50 and r2["parent"][8, 9, 17] == 8 and r2["parent"][7, 9, 17] == 17 and r2["parent"][9, 9, 17] == 8
    f, _ = ref.relax(*sc.saturated())
    assert f[0, 0, 0] == (1 << 32) - 100 and (f.reshape(-1)[1:] == ref.MAXV).all()


def test_walk_and_check_path():
    cost, goals, _ = sc.random_volume(*sc.SHAPES[4])
    r = ref.field_and_parent(cost, goals)
    reached = np.argwhere(r["field"] != ref.UNREACHED)
    wall = np.argwhere(cost >= 253)[0]
    starts = np.concatenate([reached[::97], [wall], [[-1, 0, 0]], [[0, 0, cost.shape[2]]], [goals[0, :3]]])
    cells, length, status, c = ref.walk(r["field"], r["parent"], starts, 64)
    n = len(reached[::97])
    assert status[:n].tolist() == [0] * n and status[n:].tolist() == [2, 3, 3, 0] and length[n:].tolist() == [0, 0, 0, 1]
    assert c[n] == ref.UNREACHED and c[n + 1] == ref.UNREACHED and c[n + 3] == 0 and (cells[n:n + 3] == -1).all()
    for q in range(n):
        assert c[q] == r["field"][tuple(starts[q])]
        ref.check_path(cost, r["field"], r["parent"], goals, cells[q], length[q])
    q = int(np.argmax(length[:n]))
    assert length[q] > 4
    _, l2, s2, _ = ref.walk(r["field"], r["parent"], starts[q:q + 1], int(length[q]) - 1)
    assert s2.tolist() == [1] and l2.tolist() == [length[q] - 1]


def test_a_partial_field_relaxes_to_the_same_fixed_point():
    """the property the max_rounds test leans on: relaxation started from upper bounds that are costs of real move sequences ends on the field"""
    cost, goals = sc.serpentine(12, 4, 4)
    f, _ = ref.relax(cost, goals)
    part = f.astype(np.int64)
    part[6:] = ref.UNREACHED                                     # the upper half not reached yet
    part[1, 1, 5] += 35                                          # one value not settled yet
    g, _ = ref.relax(cost, goals, start=part)
    assert np.array_equal(g, f)


def test_distance_cost_and_flight_lut_by_hand():
    from taichislam_amd.utils import distance_cost, flight_lut
    vs = 0.04
    lut = flight_lut(vs, 0.1, 0.5, scale=3.0)
    assert lut.dtype == np.uint8 and lut.shape == (256,) and lut[0] == 254 and (np.diff(lut.astype(int)) <= 0).all()
    # d = q * 0.01 m: inscribed up to q = 10, then floor(252 * exp(-3 * (d - 0.1))) up to q = 50, 0 beyond
    assert (lut[1:11] == 253).all() and lut[11] == int(np.floor(252 * np.exp(-3.0 * (0.11 - 0.1)))) == 244 and lut[50] == int(np.floor(252 * np.exp(-1.2))) == 75
    assert lut[51] == 0 and lut[255] == 0
    with pytest.raises(ValueError):
        flight_lut(vs, 0.5, 0.1)
    ramp = np.arange(256, dtype=np.uint8)                         # lut[q] = q shows q itself
    k = np.float32(4.0 / vs)
    on = np.float32(0.07)                                        # float32(0.07) * float32(100) is exactly 7: on the quarter-voxel boundary it belongs to q = 7
    assert np.float32(on * k) == np.float32(7.0)
    below = np.nextafter(on, np.float32(0.0))
    dist = np.array([-0.3, 0.0, 0.0099, below, on, 1.0, 2.5499, 2.56, 9.0, np.inf, np.nan, 0.5, 0.5, 0.5], np.float32)
    status = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 0x80], np.uint8)
    got = distance_cost(dist, status, vs, ramp, cost_unknown=201, cost_outside=202)
    assert got.dtype == np.uint8 and got.tolist() == [0, 0, 0, 6, 7, 100, 254, 255, 255, 255, 0, 201, 202, 50]
    assert distance_cost(dist.reshape(2, 7), status.reshape(2, 7), vs, ramp, 201, 202).shape == (2, 7)
    assert distance_cost(dist, status, vs, lut).tolist()[:3] == [254, 254, 254] and distance_cost(dist, status, vs, lut)[11] == 255


def test_frontier_reach3d_on_a_hand_made_cluster_list():
    from taichislam_amd.utils import frontier_reach3d
    # a map of N = 16, Nz = 8 voxels at stride 2, the layers from unsigned 2 on: 3 x 8 x 8 cells
    vol = {"cost": None, "origin": (2, 0, 0), "stride": 2, "voxel": 0.04, "half": (4, 8, 8)}
    field = np.full((3, 8, 8), ref.UNREACHED, np.uint32)
    field[0, 4, 4], field[1, 4, 4], field[0, 0, 0], field[2, 7, 7], field[1, 4, 5] = 500, 300, 40, 7, 300
    idx = np.array([[0, 0, -2], [1, 1, 1], [0, 2, 0], [0, 0, -3],   # cluster 0: cells (0, 4, 4) = 500, (1, 4, 4) = 300, (1, 4, 5) = 300: the first 300 wins; the last is below the volume
                    [-8, -8, -1], [-7, -7, -2],                  # cluster 1: cell (0, 0, 0) = 40, twice: the first row wins
                    [2, 2, 2],                                   # cluster 2: cell (2, 5, 5) is unreached
                    [7, 7, 3], [7, 7, 4],                        # cluster 3: cell (2, 7, 7) = 7; the second voxel is above the volume
                    [8, 0, 0]], np.int16)                        # cluster 4: outside in x
    fr = {"indices": idx, "cluster": np.array([0, 0, 0, 0, 1, 1, 2, 3, 3, 4], np.int32), "clusters": np.zeros(6)}      # cluster 5 has no voxel at all
    got = frontier_reach3d(fr, {"field": field}, vol)
    U = ref.UNREACHED
    assert got["value"].dtype == np.uint32 and got["value"].tolist() == [300, 40, U, 7, U, U]
    assert got["voxel"].tolist() == [1, 4, -1, 7, -1, -1] and got["reached"].tolist() == [True, True, False, True, False, False]
    assert frontier_reach3d(fr, field, vol)["value"].tolist() == got["value"].tolist()      # a bare field


def test_bindings_header_and_refusals_that_need_no_device():
    from taichislam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "taichislam_hip.h")).read()
    assert int(re.search(r"#define TSL_NAV3_SEED (\d+)", hdr).group(1)) == ref.SEED == _lib.NAV3_SEED == 26
    assert re.search(r"TSL_K_NAV_TERRAIN_WINDOW = 29,?\s*(/\*.*?\*/)?\s*TSL_K_COUNT", hdr, re.S)       # the kernel ids stay as they are: the 3-D kernels have none
    assert C.sizeof(_lib.NavField3Cfg) == 40 and _lib.NavField3Cfg.D.offset == 0 and _lib.NavField3Cfg.connectivity.offset == 20 and _lib.NavField3Cfg.check_every.offset == 32
    assert [f[0] for f in _lib.NavField3Cfg._fields_] == ["D", "H", "W", "neutral", "lethal", "connectivity", "max_rounds", "rounds_fixed", "check_every", "reserved_"]
    assert C.sizeof(_lib.NavField3Stats) == 24 and _lib.NavField3Stats.tile_visits.offset == 8 and _lib.NavField3Stats.n_bad_seeds.offset == 16
    assert [(f[0], C.sizeof(f[1])) for f in _lib.NavField3Stats._fields_] == [(f[0], C.sizeof(f[1])) for f in _lib.NavFieldStats._fields_]
    L = _lib.lib()
    names = ("tsl_tsdf_nav_field3", "tsl_tsdf_nav_field3_dev", "tsl_tsdf_nav_field3_paths", "tsl_tsdf_nav_field3_paths_dev")
    for name, two in zip(names, ("tsl_tsdf_nav_field", "tsl_tsdf_nav_field_dev", "tsl_tsdf_nav_field_paths", "tsl_tsdf_nav_field_paths_dev")):
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[two][1])                # the entry points mirror the 2-D ones
    # a null handle is refused by name before anything touches a device
    cfg = _lib.NavField3Cfg()
    st = _lib.NavField3Stats()
    assert L.tsl_tsdf_nav_field3(None, C.byref(cfg), None, None, 0, None, None, C.byref(st)) == -1 and "nav_field3: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field3_dev(None, C.byref(cfg), None, None, 0, None, None, None, None) == -1 and "nav_field3_dev: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field3_paths(None, C.byref(cfg), None, None, None, 0, 1, None, None, None, None) == -1
    assert "nav_field3_paths: null handle" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field3_paths_dev(None, C.byref(cfg), None, None, None, 0, 1, None, None, None, None, None) == -1
    assert "nav_field3_paths_dev: null handle" in L.tsl_last_error().decode()

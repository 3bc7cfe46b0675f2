"""Cost-to-go fields on the GPU (tsl_nav_field.hip): `field` and `parent` equal the restatement (tests/nav_field_ref.py) byte for byte on the hand-built
planes of tests/nav_field_scenes.py -- partial tiles, a serpentine that re-enters tiles, corner cutting, ties, seeds of every kind, saturation, the
limits of lethal and neutral, 16 planes -- plus a capped run, the device form and its ordering, the paths, one chain from the room map through nav_grid
to frontier_reach, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import nav_field_ref as ref
import nav_field_scenes as sc
from taichislam_amd import _lib
from util import SMALL, TALL

pytestmark = pytest.mark.gpu

_MAP = []
_REF = {}


def _map():
    """one small handle for the whole module: it lends the device, the stream and scratch, its map is never read"""
    from taichislam_amd.mapping import DenseTSDF
    if not _MAP:
        _MAP.append(DenseTSDF(**TALL))
    return _MAP[0]


def _want(name, cost, goals, **kw):
    """the restatement of a scene, computed once and shared"""
    if name not in _REF:
        _REF[name] = ref.field_and_parent(cost, goals, **kw)
    return _REF[name]


def _equal(got, want, what):
    assert got["field"].dtype == np.uint32 and got["parent"].dtype == np.uint8
    bad = np.argwhere(got["field"] != want["field"])
    assert bad.size == 0, f"{what}: field differs at {len(bad)} cells, first {bad[0].tolist()}: {got['field'][tuple(bad[0])]} != {want['field'][tuple(bad[0])]}"
    bad = np.argwhere(got["parent"] != want["parent"])
    assert bad.size == 0, f"{what}: parent differs at {len(bad)} cells, first {bad[0].tolist()}: {got['parent'][tuple(bad[0])]} != {want['parent'][tuple(bad[0])]}"
    assert got["n_bad_seeds"] == want["n_bad_seeds"] and got["converged"] == 1, what


def _compare(name, cost, goals, **kw):
    got = _map().nav_field(cost, goals, **kw)
    _equal(got, _want(name, cost, goals, **kw), name)
    return got


@pytest.mark.parametrize("H,W", sc.SHAPES)
def test_partial_tiles_equal_the_restatement(hip_lib, H, W):
    cost, goals, comp = sc.random_plane(H, W)
    got = _compare(f"random {H} x {W}", cost, goals)
    assert np.array_equal(got["field"][0] != ref.UNREACHED, comp) and comp.any()          # the goal's component, the largest, and nothing else
    four = _compare(f"random {H} x {W}, 4", cost, goals, connectivity=4)
    assert (four["parent"][four["parent"] < 8] % 2 == 0).all()


def test_serpentine_reenters_tiles_and_converges_under_the_default_cap(hip_lib):
    cost, goals = sc.serpentine()
    got = _compare("serpentine", cost, goals)
    assert got["field"][0, 95, 0] != ref.UNREACHED and got["field"][0, 95, 95] != ref.UNREACHED
    print(f"serpentine 96 x 96: {got['rounds']} rounds, {got['tile_visits']} tile visits")
    assert 8 < got["rounds"] <= 4 * 9 + 64 and got["tile_visits"] > 9                      # at least one check of the counter did not stop it; tiles were visited again


def test_no_corner_cutting(hip_lib):
    got = _compare("corner block", *sc.corner_block())
    assert got["field"][0, 2, 2] == ref.UNREACHED and got["parent"][0, 2, 2] == 255 and got["field"][0, 1, 1] == 0
    got = _compare("diagonal corridor", *sc.diagonal_corridor())
    assert (got["field"] != ref.UNREACHED).sum() == 1
    for conn in (4, 8):
        got = _compare(f"staircase {conn}", *sc.staircase_corridor(), connectivity=conn)
        assert got["field"][0, 11, 11] == 22 * 5 * 50 and (got["parent"][got["parent"] < 8] % 2 == 0).all()


def test_ties_take_the_lowest_code(hip_lib):
    got = _compare("uniform", *sc.uniform())
    p = got["parent"][0]
    assert p[16, 19] == 1 and p[18, 21] == 5 and p[16, 20] == 0 and p[17, 10] == 2 and p[15, 19] == 0 and p[17, 20] == 8
    _compare("uniform 4", *sc.uniform(), connectivity=4)
    _compare("checkerboard", *sc.checkerboard())
    _compare("checkerboard 4", *sc.checkerboard(), connectivity=4)


def test_seeds_of_every_kind(hip_lib):
    cost, goals, n_bad = sc.many_seeds()
    got = _compare("seeds", cost, goals)
    assert got["n_bad_seeds"] == n_bad
    assert got["parent"][0, 10, 41] != 8 and got["parent"][0, 10, 40] == 8 and got["field"][0, 30, 30] == 700 and got["parent"][0, 30, 30] == 8
    assert got["field"][0, 45, 60] == 1000 and got["field"][0, 3, 3] == 0
    none = _map().nav_field(cost, np.zeros((0, 4), np.int32))                            # S = 0 is no error: everything is unreached
    assert (none["field"] == ref.UNREACHED).all() and (none["parent"] == 255).all() and none["converged"] == 1 and none["rounds"] == 0 and none["n_bad_seeds"] == 0
    allbad = _map().nav_field(cost, goals[7:])
    assert (allbad["field"] == ref.UNREACHED).all() and allbad["n_bad_seeds"] == 6 and allbad["converged"] == 1
    three = _map().nav_field(cost, goals[:3, :3])                                         # [S, 3]: value 0
    _equal(three, ref.field_and_parent(cost, goals[:3, :3]), "[S, 3] goals")
    assert three["field"][0, 45, 60] == 0


def test_saturation_clips_and_never_wraps(hip_lib):
    row = np.zeros((1, 70), np.uint8)
    got = _compare("saturated row", row, np.array([[0, 0, 0, -100]], np.int64))          # read as uint32: 2^32 - 100
    assert got["field"][0, 0, 0] == (1 << 32) - 100 and (got["field"][0, 0, 1:] == (1 << 32) - 2).all()


@pytest.mark.parametrize("kw", [dict(lethal=1, connectivity=4), dict(lethal=1, neutral=255), dict(lethal=255, neutral=255), dict(neutral=1)], ids=str)
def test_lethal_and_neutral_at_their_limits(hip_lib, kw):
    cost, goals, comp = sc.binary_plane(kw.get("connectivity", 8)) if kw.get("lethal") == 1 else sc.random_plane(33, 31)
    got = _compare(f"limits {kw}", cost, goals, **kw)
    reached = got["field"][0] != ref.UNREACHED
    if kw.get("lethal") == 1:
        assert np.array_equal(reached, comp) and comp.sum() > 100 and (cost[comp] == 0).all()      # only cost 0 is traversable
    elif kw.get("lethal") == 255:
        assert reached.all() and (cost == sc.LETHAL).any()                                # 254 is traversable under lethal = 255
        assert got["field"].max() > 5 * (255 + 254)
    else:
        assert np.array_equal(reached, comp)


def test_sixteen_planes_equal_sixteen_calls(hip_lib):
    cost, goals = sc.sixteen_planes()
    got = _compare("16 planes", cost, goals)
    for b in (0, 5, 15):
        g1 = goals[b:b + 1].copy()
        g1[:, 0] = 0
        one = _map().nav_field(cost[b], g1)
        assert np.array_equal(one["field"][0], got["field"][b]) and np.array_equal(one["parent"][0], got["parent"][b]), b


def test_the_widest_plane(hip_lib):
    """3 x 4096 and 4096 x 2: 128 tiles in a row, the way runs through all of them"""
    cost, goals = sc.ribbon()
    want = ref.field_and_parent(cost, goals, how=ref.dijkstra)
    assert (want["field"][0, 1] != ref.UNREACHED).all() and want["field"][0, 1, 4095] > 4095 * 5 * 50
    got = _map().nav_field(cost, goals)
    _equal(got, want, "3 x 4096")
    assert 128 <= got["rounds"] <= 4 * 128 + 64
    tall = np.ascontiguousarray(cost[:2].T)
    _equal(_map().nav_field(tall, goals), ref.field_and_parent(tall, goals, how=ref.dijkstra), "4096 x 2")


def test_two_calls_give_identical_bytes(hip_lib):
    cost, goals, _ = sc.random_plane(65, 97)
    a, b = _map().nav_field(cost, goals), _map().nav_field(cost, goals)
    assert a["field"].tobytes() == b["field"].tobytes() and a["parent"].tobytes() == b["parent"].tobytes()
    nop = _map().nav_field(cost, goals, parent=False)
    assert "parent" not in nop and nop["field"].tobytes() == a["field"].tobytes()


def test_a_capped_run_holds_upper_bounds_that_are_real_costs(hip_lib):
    cost, goals = sc.serpentine()
    want = _want("serpentine", cost, goals)
    part = _map().nav_field(cost, goals, max_rounds=1)
    assert part["converged"] == 0 and part["rounds"] == 1
    pf = part["field"]
    assert (pf >= want["field"]).all() and (pf != want["field"]).any() and (pf != ref.UNREACHED).sum() > 1
    # every finite value is the cost of a move sequence: relaxation started from these values must end on the field, nothing below it
    again, _ = ref.relax(cost, goals, start=pf)
    assert np.array_equal(again, want["field"])
    full = _map().nav_field(cost, goals)
    _equal(full, want, "after the capped run")
    for cap in (2, 9, 17):                                                                # caps that are no multiple of check_every
        mid = _map().nav_field(cost, goals, max_rounds=cap)
        assert mid["converged"] == 0 and mid["rounds"] == cap and (mid["field"] >= want["field"]).all()
    for ce in (1, 3, 32):
        _equal(_map().nav_field(cost, goals, check_every=ce), want, f"check_every {ce}")


def test_device_form_equals_the_host_form_and_is_ordered(hip_lib):
    import torch
    cost, goals = sc.serpentine()
    want = _want("serpentine", cost, goals)
    host = _map().nav_field(cost, goals)
    _equal(host, want, "host")
    dev = _map().nav_field(torch.from_numpy(cost).cuda(), goals)                          # rounds_fixed = 0: the host checks, the call waits
    assert dev["field"].is_cuda and dev["parent"].is_cuda and dev["converged"] == 1
    assert dev["field"].cpu().numpy().tobytes() == want["field"].tobytes() and dev["parent"].cpu().numpy().tobytes() == want["parent"].tobytes()
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            ct = torch.full((96, 96), 254, dtype=torch.uint8, device="cuda")             # all walls ...
            a = torch.ones(1 << 24, device="cuda")
            for _ in range(8):
                a = a * 0.5 + 1.0                                                         # work in flight on the caller's stream
            ct.copy_(torch.from_numpy(cost).cuda())                                       # ... overwritten right before the call, on the caller's stream
            fix = _map().nav_field(ct, goals, rounds_fixed=host["rounds"])
            f, p = fix["field"].clone(), fix["parent"].clone()
        torch.cuda.synchronize()
        assert fix["converged"] == 1 and fix["rounds"] == host["rounds"] and fix["n_bad_seeds"] == 0
        assert f.cpu().numpy().tobytes() == want["field"].tobytes() and p.cpu().numpy().tobytes() == want["parent"].tobytes()
    short = _map().nav_field(torch.from_numpy(cost).cuda(), goals, rounds_fixed=3)
    assert short["converged"] == 0 and short["rounds"] == 3
    paths = _map().nav_paths(fix, [[0, 95, 95], [0, 0, 0]], 2000)
    hp = _map().nav_paths(host, [[0, 95, 95], [0, 0, 0]], 2000)
    torch.cuda.synchronize()
    for k in ("cells", "length", "status", "cost"):
        assert paths[k].is_cuda and paths[k].cpu().numpy().tobytes() == hp[k].tobytes(), k


def test_paths_follow_the_parents_to_a_seed(hip_lib):
    cost, goals, n_bad = sc.many_seeds()
    res = _compare("seeds", cost, goals)
    rng = np.random.default_rng(3)
    starts = np.stack([np.zeros(40, np.int64), rng.integers(0, 50, 40), rng.integers(0, 70, 40)], 1)
    starts = np.concatenate([starts, [[0, 3, 3], [0, 30, 30], [0, 20, 30], [0, 50, 0], [1, 3, 3], [0, 0, -1], [0, 49, 69]]])
    L = 200
    got = _map().nav_paths(res, starts, L)
    want = ref.follow(res["field"], res["parent"], starts, L)
    for k, w in zip(("cells", "length", "status", "cost"), want):
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), k
    st = got["status"]
    assert st[40] == 0 and got["length"][40] == 1 and got["cells"][40, 0].tolist() == [3, 3]          # a start on a seed
    assert st[41] == 0 and got["length"][41] == 1 and got["cost"][41] == 700
    assert st[42] == 2 and got["length"][42] == 0 and got["cost"][42] == ref.UNREACHED                 # on the wall
    assert st[43] == 3 and st[44] == 3 and st[45] == 3 and (got["cells"][43:46] == -1).all()
    done = np.nonzero(st == 0)[0]
    assert len(done) >= 30
    for n in done:
        assert got["cost"][n] == res["field"][0, starts[n, 1], starts[n, 2]]
        ref.check_path(cost, res["field"], res["parent"], goals, got["cells"][n], got["length"][n])
    # L one short of the path: truncated; exactly its length: ends on the seed
    n = int(done[np.argmax(got["length"][done])])
    full = int(got["length"][n])
    assert full > 5
    short = _map().nav_paths(res, starts[n:n + 1], full - 1)
    assert short["status"].tolist() == [1] and short["length"].tolist() == [full - 1] and np.array_equal(short["cells"][0], got["cells"][n, :full - 1])
    exact = _map().nav_paths(res, starts[n:n + 1], full)
    assert exact["status"].tolist() == [0] and exact["length"].tolist() == [full]
    # a walled-in start is traversable and reaches nothing
    wc, wg = sc.walled_in()
    wr = _compare("walled in", wc, wg)
    w = _map().nav_paths(wr, [[0, 5, 5], [0, 0, 0]], 64)
    assert w["status"].tolist() == [2, 0] and w["length"][0] == 0 and w["cost"][0] == ref.UNREACHED and (w["cells"][0] == -1).all()
    ref.check_path(wc, wr["field"], wr["parent"], wg, w["cells"][1], w["length"][1])
    empty = _map().nav_paths(wr, np.zeros((0, 3), np.int32), 8)
    assert empty["cells"].shape == (0, 8, 2) and empty["status"].shape == (0,)


def test_room_chain_from_the_map_to_frontier_reach(hip_lib):
    """nav_grid with an inflation table, nav_field on its cost plane, frontier_reach over extract_frontiers: the chain an exploration loop runs"""
    import render_view_scenes as rv
    from taichislam_amd.mapping import DenseTSDF
    from taichislam_amd.utils import frontier_reach, inflation_lut
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    vs = float(m.voxel_scale)
    band = (-8, 8)
    grid = m.nav_grid(bands=[band], radius=10 * vs, lut=inflation_lut(vs, 10, 2 * vs, 8 * vs, scale=3.0), min_free=4)
    cost = grid["cost"]
    trav = cost[0] < 253
    cand = np.argwhere(trav)
    goal = cand[np.argmin(((cand - m.N // 2) ** 2).sum(1))]                              # the traversable cell nearest the camera's column
    goals = np.array([[0, goal[0], goal[1]]], np.int32)
    want = ref.field_and_parent(cost, goals, how=ref.dijkstra)
    reached = int((want["field"] != ref.UNREACHED).sum())
    assert reached >= 1000 and len(np.unique(cost[0][trav])) > 5, (reached, int(trav.sum()))          # a real floor with graded costs
    got = m.nav_field(grid, goals)                                                        # the dict nav_grid returns
    _equal(got, want, "room")
    print(f"room: {reached} of {int(trav.sum())} traversable cells reached in {got['rounds']} rounds, {got['tile_visits']} tile visits")
    fr = m.extract_frontiers(z_range=(band[0] * vs, band[1] * vs))
    assert len(fr["clusters"]) >= 1
    reach = frontier_reach(fr, got, band, m.N)
    n_hit = 0
    for c in range(len(fr["clusters"])):                                                  # against a plain gather
        rows = np.nonzero(fr["cluster"] == c)[0]
        v = got["field"][0][fr["indices"][rows, 0].astype(int) + m.N // 2, fr["indices"][rows, 1].astype(int) + m.N // 2]
        if v.min() == ref.UNREACHED:
            assert reach["value"][c] == ref.UNREACHED and reach["voxel"][c] == -1 and not reach["reached"][c]
        else:
            n_hit += 1
            assert reach["value"][c] == v.min() and reach["voxel"][c] == rows[np.argmin(v)] and reach["reached"][c]
    print(f"room: {n_hit} of {len(fr['clusters'])} frontier clusters reached")
    assert n_hit >= 1
    best = int(np.argmin(reach["value"]))
    i, j, _ = fr["indices"][reach["voxel"][best]].astype(int)
    path = m.nav_paths(got, [[0, i + m.N // 2, j + m.N // 2]], 1024)
    assert path["status"].tolist() == [0] and path["cost"][0] == reach["value"][best]
    ref.check_path(cost, got["field"], got["parent"], goals, path["cells"][0], path["length"][0])


def _raw(L, g, cfg, cost, seeds, S, shape):
    """tsl_tsdf_nav_field on buffers that start as 0xAB"""
    field = np.full(shape, 0xABABABAB, np.uint32)
    par = np.full(shape, 0xAB, np.uint8)
    st = _lib.NavFieldStats()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.tsl_tsdf_nav_field(g.h, C.byref(cfg), p(cost), p(seeds), S, p(field), p(par), C.byref(st))
    return rc, field, par, st


def _cfg(shape, **kw):
    c = _lib.NavFieldCfg()
    c.B, c.H, c.W = shape
    c.neutral, c.lethal, c.connectivity = 50, 253, 8
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_refusals_leave_the_handle_usable(hip_lib):
    L, g = hip_lib, _map()
    cost, goals, _ = sc.random_plane(33, 31)
    cost = cost[None].copy()
    seeds = np.array([[0, goals[0, 1], goals[0, 2], 0]], np.int32)
    want = _want("random 33 x 31", cost, goals)
    shape = cost.shape
    rc, field, par, st = _raw(L, g, _cfg(shape), cost, seeds, 1, shape)
    assert rc == 0 and np.array_equal(field, want["field"]) and np.array_equal(par, want["parent"]) and st.converged == 1
    bad = [("B", dict(B=0)), ("B", dict(B=17)), ("H", dict(H=0)), ("H", dict(H=4097)), ("W", dict(W=-1)), ("W", dict(W=4097)), ("neutral", dict(neutral=0)),
           ("neutral", dict(neutral=256)), ("lethal", dict(lethal=0)), ("lethal", dict(lethal=256)), ("connectivity", dict(connectivity=6)),
           ("connectivity", dict(connectivity=0)), ("max_rounds", dict(max_rounds=-1)), ("rounds_fixed", dict(rounds_fixed=-2)), ("check_every", dict(check_every=-1))]
    cases = [(w, _cfg(shape, **kw), cost, seeds, 1) for w, kw in bad]
    cases += [("S must", _cfg(shape), cost, seeds, -1), ("S must", _cfg(shape), cost, seeds, 65537), ("null seeds", _cfg(shape), cost, None, 1), ("null cost", _cfg(shape), None, seeds, 1)]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for word, cfg, cs, sd, S in cases:
        rc, f2, p2, _ = _raw(L, g, cfg, cs, sd, S, shape)
        msg = L.tsl_last_error().decode()
        assert rc == -1 and "nav_field:" in msg and word in msg, (word, msg)
        assert (f2 == 0xABABABAB).all() and (p2 == 0xAB).all(), word                      # nothing was written
        assert L.tsl_tsdf_nav_field_dev(g.h, C.byref(cfg), p(cs), p(sd), S, p(field), None, None, None) == -1      # (refused before any pointer is used)
        assert "nav_field_dev:" in L.tsl_last_error().decode()
        rc, f3, p3, st = _raw(L, g, _cfg(shape), cost, seeds, 1, shape)                          # a good call still succeeds, with the same bytes
        assert rc == 0 and f3.tobytes() == field.tobytes() and p3.tobytes() == par.tobytes(), word
    assert L.tsl_tsdf_nav_field(g.h, None, p(cost), p(seeds), 1, p(field), None, None) == -1 and "null cfg" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field(g.h, C.byref(_cfg(shape)), p(cost), p(seeds), 1, None, None, None) == -1 and "null field" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field(None, C.byref(_cfg(shape)), p(cost), p(seeds), 1, p(field), None, None) == -1 and "null handle" in L.tsl_last_error().decode()
    # the paths
    starts = np.array([[0, 0, 0]], np.int32)
    cells = np.full((1, 4, 2), 0x2B2B, np.int16)
    for word, cfg, f_, p_, s_, P, Lmax in (("L must", _cfg(shape), field, par, starts, 1, 0), ("L must", _cfg(shape), field, par, starts, 1, -3), ("null field", _cfg(shape), None, par, starts, 1, 4),
                                           ("null parent", _cfg(shape), field, None, starts, 1, 4), ("null starts", _cfg(shape), field, par, None, 1, 4),
                                           ("P must", _cfg(shape), field, par, starts, -1, 4), ("H", _cfg(shape, H=0), field, par, starts, 1, 4), ("B", _cfg(shape, B=17), field, par, starts, 1, 4)):
        assert L.tsl_tsdf_nav_field_paths(g.h, C.byref(cfg), p(f_), p(p_), p(s_), P, Lmax, p(cells), None, None, None) == -1
        msg = L.tsl_last_error().decode()
        assert "nav_field_paths:" in msg and word in msg and (cells == 0x2B2B).all(), (word, msg)
        assert L.tsl_tsdf_nav_field_paths_dev(g.h, C.byref(cfg), p(f_), p(p_), p(s_), P, Lmax, p(cells), None, None, None, None) == -1
        assert "nav_field_paths_dev:" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field_paths(g.h, None, p(field), p(par), p(starts), 1, 4, p(cells), None, None, None) == -1 and "null cfg" in L.tsl_last_error().decode()
    with pytest.raises(ValueError):
        g.nav_field(cost.astype(np.int32), goals)
    with pytest.raises(ValueError):
        g.nav_field(cost, np.zeros((2, 5), np.int32))
    with pytest.raises(ValueError):
        g.nav_paths({"field": field}, starts, 4)
    with pytest.raises(_lib.TslError, match="neutral"):
        g.nav_field(cost, goals, neutral=0)
    with pytest.raises(_lib.TslError, match="L must"):
        g.nav_paths({"field": field, "parent": par}, starts, 0)
    _compare("random 33 x 31", cost[0], goals)

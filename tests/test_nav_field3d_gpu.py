"""3-D cost-to-go fields on the GPU (tsl_nav_field3.hip): `field` and `parent` equal the restatement (tests/nav_field3d_ref.py) byte for byte on the
hand-built volumes of tests/nav_field3d_scenes.py -- partial tiles on every axis, a serpentine that re-enters tiles, corner cutting across faces and cubes,
ties, seeds of every kind, saturation, the limits of lethal and neutral -- plus one layer against nav_field, a capped run, the device form and its
ordering, the paths, one chain from the room map through flight_volume to frontier_reach3d, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import nav_field3d_ref as ref
import nav_field3d_scenes as sc
from taichislam_amd import _lib
from util import SMALL, TALL

pytestmark = pytest.mark.gpu

_MAP = []
_REF = {}
TILES_SERPENTINE = 3 * 3 * 2                                      # 24 x 24 x 24 cells in tiles of 8 x 8 x 16


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
        for a in ("field", "parent"):
            _REF[name][a].setflags(write=False)
    return _REF[name]


def _equal(got, want, what):
    assert got["field"].dtype == np.uint32 and got["parent"].dtype == np.uint8
    bad = np.argwhere(got["field"] != want["field"])
    assert bad.size == 0, f"{what}: field differs at {len(bad)} cells, first {bad[0].tolist()}: {got['field'][tuple(bad[0])]} != {want['field'][tuple(bad[0])]}"
    bad = np.argwhere(got["parent"] != want["parent"])
    assert bad.size == 0, f"{what}: parent differs at {len(bad)} cells, first {bad[0].tolist()}: {got['parent'][tuple(bad[0])]} != {want['parent'][tuple(bad[0])]}"
    assert got["n_bad_seeds"] == want["n_bad_seeds"] and got["converged"] == 1, what


def _compare(name, cost, goals, **kw):
    got = _map().nav_field3d(cost, goals, **kw)
    _equal(got, _want(name, cost, goals, **kw), name)
    return got


def _only_codes(parent, connectivity):
    codes = np.unique(parent[parent < ref.SEED]).tolist()
    return all(ref.NZ[d] <= ref.MAXNZ[connectivity] for d in codes)


@pytest.mark.parametrize("D,H,W", sc.SHAPES)
def test_partial_tiles_equal_the_restatement(hip_lib, D, H, W):
    cost, goals, comp = sc.random_volume(D, H, W)
    got = _compare(f"random {D} x {H} x {W}", cost, goals)
    assert np.array_equal(got["field"] != ref.UNREACHED, comp) and comp.any()             # the goal's component, the largest, and nothing else
    for conn in (6, 18):
        less = _compare(f"random {D} x {H} x {W}, {conn}", cost, goals, connectivity=conn)
        assert _only_codes(less["parent"], conn)


def test_serpentine_reenters_tiles_and_converges_under_the_default_cap(hip_lib):
    cost, goals = sc.serpentine()
    got = _compare("serpentine", cost, goals)
    assert (got["field"] != ref.UNREACHED).sum() == (cost < 253).sum()
    print(f"serpentine 24^3: {got['rounds']} rounds, {got['tile_visits']} tile visits")
    # at least one check of the counter did not stop it; tiles were visited again; the default cap was not needed
    assert 8 < got["rounds"] <= 4 * TILES_SERPENTINE + 64 and got["tile_visits"] > TILES_SERPENTINE
    six = _compare("serpentine, 6", cost, goals, connectivity=6)
    assert _only_codes(six["parent"], 6)


def test_no_corner_cutting(hip_lib):
    for w in (0, 1):
        got = _compare(f"face diagonal {w}", *sc.face_diagonal(w))
        assert got["field"][1, 2, 2] == 2 * 5 * 50 and ref.NZ[got["parent"][1, 2, 2]] == 1
    got = _compare("face diagonal free", *sc.face_diagonal(None))
    assert got["field"][1, 2, 2] == 7 * 50 and got["parent"][1, 2, 2] == 5                # (0, -1, -1)
    for w in range(6):
        got = _compare(f"space diagonal {w}", *sc.space_diagonal(w))
        assert got["field"][2, 2, 2] == (7 + 5) * 50 and ref.NZ[got["parent"][2, 2, 2]] < 3, w      # the cube is not whole: a face diagonal and an axis move
    got = _compare("space diagonal free", *sc.space_diagonal(None))
    assert got["field"][2, 2, 2] == 9 * 50 and got["parent"][2, 2, 2] == 23               # (-1, -1, -1)


def test_ties_take_the_lowest_code(hip_lib):
    got = _compare("uniform", *sc.uniform())
    s = np.array(sc.UNIFORM_SEED)
    p = lambda *d: got["parent"][tuple(s + np.array(d))]
    assert p(0, 0, 0) == 26 and p(0, 0, 3) == 6 and p(1, 0, 0) == 17 and p(-1, 0, 0) == 8 and p(-1, -1, -1) == 10 and p(2, 2, 2) == 23
    assert p(-1, 2, 0) == 4 and p(-2, 1, 0) == 8 and p(1, 2, 0) == 4                      # in-plane against dk = +1, two codes with dk = +1, in-plane against dk = -1
    two = _compare("uniform, two seeds", *sc.uniform_two_seeds())
    assert two["parent"][8, 9, 17] == 8 and two["parent"][7, 9, 17] == 17                 # up (code 8) ties with down (code 17) half way between the seeds
    for conn in (6, 18):
        assert _only_codes(_compare(f"uniform {conn}", *sc.uniform(), connectivity=conn)["parent"], conn)
    for conn in (6, 18, 26):
        _compare(f"checkerboard {conn}", *sc.checkerboard(), connectivity=conn)


def test_seeds_of_every_kind(hip_lib):
    cost, goals, n_bad = sc.many_seeds()
    got = _compare("seeds", cost, goals)
    assert got["n_bad_seeds"] == n_bad
    assert got["parent"][3, 10, 31] != 26 and got["parent"][3, 10, 30] == 26 and got["field"][15, 12, 22] == 700 and got["parent"][15, 12, 22] == 26
    for k, i, j, v in goals[7:11].tolist():                                               # on a tile face, a tile edge, two tile corners
        assert got["field"][k, i, j] == v and got["parent"][k, i, j] == 26
    none = _map().nav_field3d(cost, np.zeros((0, 4), np.int32))                           # S = 0 is no error: everything is unreached
    assert (none["field"] == ref.UNREACHED).all() and (none["parent"] == 255).all() and none["converged"] == 1 and none["rounds"] == 0 and none["n_bad_seeds"] == 0
    allbad = _map().nav_field3d(cost, goals[11:])
    assert (allbad["field"] == ref.UNREACHED).all() and allbad["n_bad_seeds"] == 7 and allbad["converged"] == 1
    three = _map().nav_field3d(cost, goals[:3, :3])                                       # [S, 3]: value 0
    _equal(three, ref.field_and_parent(cost, goals[:3, :3]), "[S, 3] goals")
    assert three["field"][18, 17, 36] == 0


def test_saturation_clips_and_never_wraps(hip_lib):
    got = _compare("saturated", *sc.saturated())                                          # the value is read as uint32: 2^32 - 100
    assert got["field"][0, 0, 0] == (1 << 32) - 100 and (got["field"].reshape(-1)[1:] == (1 << 32) - 2).all()


@pytest.mark.parametrize("kw", [dict(lethal=1, connectivity=6), dict(lethal=1, neutral=255), dict(lethal=255, neutral=255), dict(neutral=1)], ids=str)
def test_lethal_and_neutral_at_their_limits(hip_lib, kw):
    cost, goals, comp = sc.binary_volume(kw.get("connectivity", 26)) if kw.get("lethal") == 1 else sc.random_volume(*sc.SHAPES[4])
    got = _compare(f"limits {kw}", cost, goals, **kw)
    reached = got["field"] != ref.UNREACHED
    if kw.get("lethal") == 1:
        assert np.array_equal(reached, comp) and comp.sum() > 100 and (cost[comp] == 0).all()      # only cost 0 is traversable
    elif kw.get("lethal") == 255:
        assert reached.all() and (cost == sc.LETHAL).any()                                # 254 is traversable under lethal = 255
        assert got["field"].max() > 5 * (255 + 254)
    else:
        assert np.array_equal(reached, comp)


def test_one_layer_equals_nav_field(hip_lib):
    """D = 1 is nav_field's problem: the same field on a random plane with partial tiles in both kernels, and the same parents with 8 read as 26"""
    import nav_field_scenes as sc2
    cost, goals, _ = sc2.random_plane(65, 97)
    for c3, c2 in ((26, 8), (6, 4)):
        three = _map().nav_field3d(cost[None], goals, connectivity=c3)
        two = _map().nav_field(cost, goals, connectivity=c2)
        assert three["converged"] == 1 and two["converged"] == 1
        assert three["field"].tobytes() == two["field"].tobytes(), c3
        assert np.array_equal(three["parent"], np.where(two["parent"] == 8, 26, two["parent"])), c3


def _interleaved_calls():
    """the calls of the two tests below with their restatements, computed once: a 2-D field over [2, 33, 40], a 3-D field over [9, 17, 33], a larger 2-D
    field over [1, 70, 65] and the 3-D call again.  Every shape is one partial tile beyond a tile edge on each axis: the smallest at which both round
    kernels use halo tiles and the activity map has more than one word per axis."""
    import nav_field_ref as ref2
    import nav_field_scenes as sc2
    if "interleaved" not in _REF:
        p0, p1 = sc2.random_plane(33, 40), sc2.random_plane(33, 40, seed=8)
        two = np.stack([p0[0], p1[0]])
        g2 = np.array([[0, p0[1][0, 1], p0[1][0, 2], 0], [1, p1[1][0, 1], p1[1][0, 2], 40], [2, 0, 0, 0]], np.int32)      # a goal per plane, one in a plane that is not there
        c3, g3, _ = sc.random_volume(9, 17, 33)
        big, gb, _ = sc2.random_plane(70, 65)
        calls = [("nav_field", two, g2, ref2.field_and_parent(two, g2)), ("nav_field3d", c3, g3, ref.field_and_parent(c3, g3)),
                 ("nav_field", big[None], gb, ref2.field_and_parent(big, gb))]
        for c in calls:
            for a in ("field", "parent"):
                c[3][a].setflags(write=False)
        _REF["interleaved"] = calls + [calls[1]]
    return _REF["interleaved"]


def test_interleaved_2d_and_3d_calls_on_one_handle_keep_their_scratch_apart(hip_lib):
    """the two solvers are two instances of one state type behind one grow helper: calls that alternate between them, and a 2-D call that outgrows the
    scratch of the one before, must each see their own buffers -- in the numpy form and in the device form"""
    import torch
    g = _map()
    host = []
    for how, cost, goals, want in _interleaved_calls():
        got = getattr(g, how)(cost, goals)
        _equal(got, want, f"{how} {cost.shape}")
        assert got["n_bad_seeds"] == (1 if cost.shape[0] == 2 else 0) and 1 <= got["rounds"] and got["tile_visits"] >= got["rounds"]
        host.append(got)
    assert host[3]["field"].tobytes() == host[1]["field"].tobytes() and host[3]["parent"].tobytes() == host[1]["parent"].tobytes()
    dev = []
    for (how, cost, goals, want), h in zip(_interleaved_calls(), host):
        fixed = h["rounds"] + 4                                                           # (a halo read that races a write-back may move the last change by a round)
        got = getattr(g, how)(torch.from_numpy(cost).cuda(), goals, rounds_fixed=fixed)
        assert got["field"].is_cuda and got["parent"].is_cuda and 1 <= got["rounds"] <= fixed and got["tile_visits"] >= got["rounds"]
        dev.append({**got, "field": got["field"].cpu().numpy().view(np.uint32), "parent": got["parent"].cpu().numpy()})
        _equal(dev[-1], want, f"{how} {cost.shape}, device form")
    assert dev[3]["field"].tobytes() == dev[1]["field"].tobytes() and dev[3]["parent"].tobytes() == dev[1]["parent"].tobytes()


def test_profiling_ids_count_the_2d_launches_and_none_of_the_3d(hip_lib):
    """one bracket per seed pass, per round, per parent pass (the seed-parent pass inside it) and per paths launch of the 2-D solver; the 3-D solver has
    no id and adds nothing to them"""
    import torch
    g = _map()
    ids = [_lib.K_NAV_FIELD_SEED, _lib.K_NAV_FIELD_ROUND, _lib.K_NAV_FIELD_PARENT, _lib.K_NAV_FIELD_PATHS]
    (_, cost2, goals2, _), (_, cost3, goals3, _) = _interleaved_calls()[:2]
    g.enable_profiling(True, only=ids)
    try:
        for k in ids:
            g.kernel_time(k)                                                              # (a query returns what was recorded since the one before)
        res = g.nav_field(torch.from_numpy(cost2).cuda(), goals2, rounds_fixed=3)
        g.nav_paths(res, goals2[:1, :3], 16)
        got = [g.kernel_time(k) for k in ids]
        print("nav_field profiling (ms, launches) of seed, round, parent, paths:", got)
        assert [n for _, n in got] == [1, 3, 1, 1] and all(ms > 0.0 for ms, _ in got)
        res3 = g.nav_field3d(torch.from_numpy(cost3).cuda(), goals3, rounds_fixed=3)
        g.nav_paths3d(res3, goals3[:1, :3], 16)
        assert [g.kernel_time(k)[1] for k in ids] == [0, 0, 0, 0]
    finally:
        g.enable_profiling(False)


def test_two_calls_give_identical_bytes(hip_lib):
    cost, goals, _ = sc.random_volume(*sc.SHAPES[4])
    a, b = _map().nav_field3d(cost, goals), _map().nav_field3d(cost, goals)
    assert a["field"].tobytes() == b["field"].tobytes() and a["parent"].tobytes() == b["parent"].tobytes()
    nop = _map().nav_field3d(cost, goals, parent=False)
    assert "parent" not in nop and nop["field"].tobytes() == a["field"].tobytes()


def test_a_capped_run_holds_upper_bounds_that_are_real_costs(hip_lib):
    cost, goals = sc.serpentine()
    want = _want("serpentine", cost, goals)
    part = _map().nav_field3d(cost, goals, max_rounds=1)                                  # TSL_OK (no exception) with converged = 0
    assert part["converged"] == 0 and part["rounds"] == 1
    pf = part["field"]
    assert (pf >= want["field"]).all() and (pf != want["field"]).any() and (pf != ref.UNREACHED).sum() > 1
    assert (pf[want["field"] == ref.UNREACHED] == ref.UNREACHED).all()                   # no unreached cell of the true field is reached
    # every finite value is the cost of a move sequence: relaxation started from these values must end on the field, nothing below it
    again, _ = ref.relax(cost, goals, start=pf)
    assert np.array_equal(again, want["field"])
    full = _map().nav_field3d(cost, goals)
    _equal(full, want, "after the capped run")
    for cap in (2, 9, 17):                                                                # caps that are no multiple of check_every
        mid = _map().nav_field3d(cost, goals, max_rounds=cap)
        assert mid["converged"] == 0 and mid["rounds"] == cap and (mid["field"] >= want["field"]).all()
    for ce in (1, 3, 32):
        _equal(_map().nav_field3d(cost, goals, check_every=ce), want, f"check_every {ce}")
    fixed = _map().nav_field3d(cost, goals, rounds_fixed=full["rounds"])                 # the rounds of an earlier call: equal volumes, converged
    _equal(fixed, want, "rounds_fixed")
    assert fixed["rounds"] == full["rounds"]


def test_device_form_equals_the_host_form_and_is_ordered(hip_lib):
    import torch
    cost, goals = sc.serpentine()
    want = _want("serpentine", cost, goals)
    host = _map().nav_field3d(cost, goals)
    _equal(host, want, "host")
    dev = _map().nav_field3d(torch.from_numpy(cost).cuda(), goals)                        # rounds_fixed = 0: the host checks, the call waits
    assert dev["field"].is_cuda and dev["parent"].is_cuda and dev["converged"] == 1
    assert dev["field"].cpu().numpy().tobytes() == want["field"].tobytes() and dev["parent"].cpu().numpy().tobytes() == want["parent"].tobytes()
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            ct = torch.full(cost.shape, 254, dtype=torch.uint8, device="cuda")            # all walls ...
            a = torch.ones(1 << 24, device="cuda")
            for _ in range(8):
                a = a * 0.5 + 1.0                                                         # work in flight on the caller's stream
            ct.copy_(torch.from_numpy(cost).cuda())                                       # ... overwritten right before the call, on the caller's stream
            fix = _map().nav_field3d(ct, goals, rounds_fixed=host["rounds"])
            f, p = fix["field"].clone(), fix["parent"].clone()
        torch.cuda.synchronize()
        assert fix["converged"] == 1 and fix["rounds"] == host["rounds"] and fix["n_bad_seeds"] == 0
        assert f.cpu().numpy().tobytes() == want["field"].tobytes() and p.cpu().numpy().tobytes() == want["parent"].tobytes()
    short = _map().nav_field3d(torch.from_numpy(cost).cuda(), goals, rounds_fixed=3)
    assert short["converged"] == 0 and short["rounds"] == 3
    starts = [[23, 23, 23], [0, 0, 0], [3, 0, 0]]
    paths = _map().nav_paths3d(fix, starts, 2000)
    hp = _map().nav_paths3d(host, starts, 2000)
    torch.cuda.synchronize()
    for k in ("cells", "length", "status", "cost"):
        assert paths[k].is_cuda and paths[k].cpu().numpy().tobytes() == hp[k].tobytes(), k
    assert hp["status"].tolist() == [0, 0, 2]                                             # (3, 0, 0) lies in a wall layer


def test_paths_follow_the_parents_to_a_seed(hip_lib):
    cost, goals, n_bad = sc.many_seeds()
    res = _compare("seeds", cost, goals)
    rng = np.random.default_rng(3)
    starts = np.stack([rng.integers(0, 20, 40), rng.integers(0, 20, 40), rng.integers(0, 40, 40)], 1)
    starts = np.concatenate([starts, [[1, 3, 3], [15, 12, 22], [10, 10, 20], [20, 0, 0], [0, 20, 0], [0, 0, -1], [19, 19, 39]]])
    L = 200
    got = _map().nav_paths3d(res, starts, L)
    want = ref.walk(res["field"], res["parent"], starts, L)
    for k, w in zip(("cells", "length", "status", "cost"), want):
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), k
    st = got["status"]
    assert st[40] == 0 and got["length"][40] == 1 and got["cells"][40, 0].tolist() == [1, 3, 3]       # a start on a seed
    assert st[41] == 0 and got["length"][41] == 1 and got["cost"][41] == 700
    assert st[42] == 2 and got["length"][42] == 0 and got["cost"][42] == ref.UNREACHED                 # on the wall
    assert st[43] == 3 and st[44] == 3 and st[45] == 3 and (got["cells"][43:46] == -1).all()
    done = np.nonzero(st == 0)[0]
    assert len(done) >= 30
    for n in done:
        assert got["cost"][n] == res["field"][tuple(starts[n])]
        ref.check_path(cost, res["field"], res["parent"], goals, got["cells"][n], got["length"][n])    # follows the parents, allowed moves, ends on a seed
    # L one short of the path: truncated; exactly its length: ends on the seed
    n = int(done[np.argmax(got["length"][done])])
    full = int(got["length"][n])
    assert full > 5
    short = _map().nav_paths3d(res, starts[n:n + 1], full - 1)
    assert short["status"].tolist() == [1] and short["length"].tolist() == [full - 1] and np.array_equal(short["cells"][0], got["cells"][n, :full - 1])
    exact = _map().nav_paths3d(res, starts[n:n + 1], full)
    assert exact["status"].tolist() == [0] and exact["length"].tolist() == [full]
    # a walled-in start is traversable and reaches nothing
    wc, wg = sc.walled_in()
    wr = _compare("walled in", wc, wg)
    w = _map().nav_paths3d(wr, [[5, 5, 5], [0, 0, 0]], 64)
    assert w["status"].tolist() == [2, 0] and w["length"][0] == 0 and w["cost"][0] == ref.UNREACHED and (w["cells"][0] == -1).all()
    ref.check_path(wc, wr["field"], wr["parent"], wg, w["cells"][1], w["length"][1])
    empty = _map().nav_paths3d(wr, np.zeros((0, 3), np.int32), 8)
    assert empty["cells"].shape == (0, 8, 3) and empty["status"].shape == (0,)


def volume_restatement(N, Nz, vs, stride, grid, lut, cost_unknown=255, cost_outside=255):
    """flight_volume restated: the lattice of cell centres through the numpy restatement of the nearest-voxel ESDF query and distance_cost"""
    import esdf_query_ref as qref
    from taichislam_amd.utils import distance_cost
    val, known, lo = grid
    D, H, W = Nz // stride, N // stride, N // stride
    k, i, j = (np.arange(n, dtype=np.int64) * stride + stride // 2 - h for n, h in ((D, Nz // 2), (H, N // 2), (W, N // 2)))
    xyz = np.empty((D, H, W, 3), np.float32)
    xyz[..., 0] = (i.astype(np.float32) * np.float32(vs))[None, :, None]
    xyz[..., 1] = (j.astype(np.float32) * np.float32(vs))[None, None, :]
    xyz[..., 2] = (k.astype(np.float32) * np.float32(vs))[:, None, None]
    dist, _, status = qref.query(xyz.reshape(-1, 3), 0, vs, val, known, lo)
    return distance_cost(dist, status, vs, lut, cost_unknown, cost_outside).reshape(D, H, W)


ROOM_STRIDE, ROOM_MAX_DIST = 4, 2.0


def room_lut(vs):
    from taichislam_amd.utils import flight_lut
    return flight_lut(vs, 0.1 + ROOM_STRIDE * vs * np.sqrt(3.0) / 2.0, 0.8, scale=3.0)    # a 10 cm vehicle plus half a cell diagonal


def room_seed(cost, T, vs, vol):
    """the traversable cell nearest the camera's"""
    cam = np.array([T[2], T[0], T[1]], np.float64) / vs + np.array(vol["half"]) - np.array(vol["origin"])
    cand = np.argwhere(cost < 253)
    return cand[np.argmin(((cand * vol["stride"] + vol["stride"] // 2 - cam) ** 2).sum(1))]


def test_room_chain_from_the_map_to_frontier_reach3d(hip_lib):
    """update_esdf, flight_volume, nav_field3d from the camera's cell, frontier_reach3d over extract_frontiers, nav_paths3d: the chain a drone's exploration loop runs"""
    import esdf_query_ref as qref
    import render_view_scenes as rv
    from oracle import BATCHED
    from taichislam_amd.mapping import DenseTSDF
    from taichislam_amd.utils import frontier_reach3d
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.update_esdf(max_dist=ROOM_MAX_DIST)
    vs = float(m.voxel_scale)
    lut = room_lut(vs)
    vol = m.flight_volume(stride=ROOM_STRIDE, lut=lut)
    cost = vol["cost"]
    assert cost.dtype == np.uint8 and cost.shape == (m.Nz // 4, m.N // 4, m.N // 4) and vol["origin"] == (0, 0, 0) and vol["stride"] == 4
    o = rv.room_oracle(K, frames)
    oi, oe = o.esdf(max_dist=ROOM_MAX_DIST)
    want_cost = volume_restatement(m.N, m.Nz, vs, ROOM_STRIDE, qref.grid_from_export(oi, oe, m.N, m.Nz), lut)
    assert cost.tobytes() == want_cost.tobytes()
    import torch
    dv = m.flight_volume(stride=ROOM_STRIDE, lut=lut, device=True)                        # the lattice, the query and the cost on the device
    assert dv["cost"].is_cuda and dv["cost"].cpu().numpy().tobytes() == want_cost.tobytes()
    trav = cost < 253
    assert trav.sum() > 1000 and len(np.unique(cost[trav])) > 5                           # real free space with graded costs
    seed = room_seed(cost, frames[0][1], vs, vol)
    goals = np.array([seed], np.int32)
    got = m.nav_field3d(vol, goals)                                                       # the dict flight_volume returns
    assert got["converged"] == 1 and got["n_bad_seeds"] == 0 and got["field"][tuple(seed)] == 0
    reached = got["field"] != ref.UNREACHED
    assert reached.sum() > 1000 and not reached[~trav].any()
    print(f"room: {int(reached.sum())} of {int(trav.sum())} traversable cells reached in {got['rounds']} rounds, {got['tile_visits']} tile visits")
    fr = m.extract_frontiers()
    assert len(fr["clusters"]) >= 1
    reach = frontier_reach3d(fr, got, vol)
    n_hit = 0
    for c in range(len(fr["clusters"])):                                                  # against a plain gather
        rows = np.nonzero(fr["cluster"] == c)[0]
        u = fr["indices"][rows].astype(int)
        v = got["field"][(u[:, 2] + m.Nz // 2) // 4, (u[:, 0] + m.N // 2) // 4, (u[:, 1] + m.N // 2) // 4]
        if v.min() == ref.UNREACHED:
            assert reach["value"][c] == ref.UNREACHED and reach["voxel"][c] == -1 and not reach["reached"][c]
        else:
            n_hit += 1
            assert reach["value"][c] == v.min() and reach["voxel"][c] == rows[np.argmin(v)] and reach["reached"][c]
    print(f"room: {n_hit} of {len(fr['clusters'])} frontier clusters reached")
    assert n_hit >= 1
    best = int(np.argmax(np.where(reach["reached"], reach["value"], 0)))                 # the reached cluster that is furthest away: a path of some length
    assert reach["value"][best] > 10 * 5 * 50
    i, j, k = fr["indices"][reach["voxel"][best]].astype(int)
    start = [(k + m.Nz // 2) // 4, (i + m.N // 2) // 4, (j + m.N // 2) // 4]
    path = m.nav_paths3d(got, [start], 1024)
    assert path["status"].tolist() == [0] and path["cost"][0] == reach["value"][best]
    cells = path["cells"][0, :path["length"][0]].astype(int)
    assert (cost[cells[:, 0], cells[:, 1], cells[:, 2]] < 253).all() and cells[-1].tolist() == seed.tolist()      # every cell is free; it ends on the seed
    ref.check_path(cost, got["field"], got["parent"], goals, path["cells"][0], path["length"][0])


def _raw(L, g, cfg, cost, seeds, S, shape):
    """tsl_tsdf_nav_field3 on buffers that start as 0xAB"""
    field = np.full(shape, 0xABABABAB, np.uint32)
    par = np.full(shape, 0xAB, np.uint8)
    st = _lib.NavField3Stats()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = L.tsl_tsdf_nav_field3(g.h, C.byref(cfg), p(cost), p(seeds), S, p(field), p(par), C.byref(st))
    return rc, field, par, st


def _cfg(shape, **kw):
    c = _lib.NavField3Cfg()
    c.D, c.H, c.W = shape
    c.neutral, c.lethal, c.connectivity = 50, 253, 26
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_refusals_leave_the_handle_usable(hip_lib):
    L, g = hip_lib, _map()
    shape = sc.SHAPES[4]
    cost, goals, _ = sc.random_volume(*shape)
    seeds = np.array([[goals[0, 0], goals[0, 1], goals[0, 2], 0]], np.int32)
    want = _want("random %d x %d x %d" % shape, cost, goals)
    rc, field, par, st = _raw(L, g, _cfg(shape), cost, seeds, 1, shape)
    assert rc == 0 and np.array_equal(field, want["field"]) and np.array_equal(par, want["parent"]) and st.converged == 1
    bad = [("D", dict(D=0)), ("D", dict(D=1025)), ("H", dict(H=0)), ("H", dict(H=1025)), ("W", dict(W=-1)), ("W", dict(W=1025)), ("2^27", dict(D=1024, H=1024, W=129)),
           ("neutral", dict(neutral=0)), ("neutral", dict(neutral=256)), ("lethal", dict(lethal=0)), ("lethal", dict(lethal=256)), ("connectivity", dict(connectivity=8)),
           ("connectivity", dict(connectivity=0)), ("max_rounds", dict(max_rounds=-1)), ("rounds_fixed", dict(rounds_fixed=-2)), ("check_every", dict(check_every=-1))]
    cases = [(w, _cfg(shape, **kw), cost, seeds, 1) for w, kw in bad]
    cases += [("S must", _cfg(shape), cost, seeds, -1), ("S must", _cfg(shape), cost, seeds, 65537), ("null seeds", _cfg(shape), cost, None, 1), ("null cost", _cfg(shape), None, seeds, 1)]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for word, cfg, cs, sd, S in cases:
        rc, f2, p2, _ = _raw(L, g, cfg, cs, sd, S, shape)
        msg = L.tsl_last_error().decode()
        assert rc == -1 and "nav_field3:" in msg and word in msg, (word, msg)
        assert (f2 == 0xABABABAB).all() and (p2 == 0xAB).all(), word                      # nothing was written
        assert L.tsl_tsdf_nav_field3_dev(g.h, C.byref(cfg), p(cs), p(sd), S, p(field), None, None, None) == -1      # (refused before any pointer is used)
        assert "nav_field3_dev:" in L.tsl_last_error().decode()
        rc, f3, p3, st = _raw(L, g, _cfg(shape), cost, seeds, 1, shape)                   # a good call still succeeds, with the same bytes
        assert rc == 0 and f3.tobytes() == field.tobytes() and p3.tobytes() == par.tobytes(), word
    assert L.tsl_tsdf_nav_field3(g.h, None, p(cost), p(seeds), 1, p(field), None, None) == -1 and "null cfg" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field3(g.h, C.byref(_cfg(shape)), p(cost), p(seeds), 1, None, None, None) == -1 and "null field" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field3(None, C.byref(_cfg(shape)), p(cost), p(seeds), 1, p(field), None, None) == -1 and "null handle" in L.tsl_last_error().decode()
    # the paths
    starts = np.array([[0, 0, 0]], np.int32)
    cells = np.full((1, 4, 3), 0x2B2B, np.int16)
    for word, cfg, f_, p_, s_, P, Lmax in (("L must", _cfg(shape), field, par, starts, 1, 0), ("L must", _cfg(shape), field, par, starts, 1, -3), ("null field", _cfg(shape), None, par, starts, 1, 4),
                                           ("null parent", _cfg(shape), field, None, starts, 1, 4), ("null starts", _cfg(shape), field, par, None, 1, 4),
                                           ("P must", _cfg(shape), field, par, starts, -1, 4), ("P must", _cfg(shape), field, par, starts, (1 << 20) + 1, 4),
                                           ("P * L", _cfg(shape), field, par, starts, 1 << 20, 257), ("H", _cfg(shape, H=0), field, par, starts, 1, 4),
                                           ("D", _cfg(shape, D=1025), field, par, starts, 1, 4)):
        assert L.tsl_tsdf_nav_field3_paths(g.h, C.byref(cfg), p(f_), p(p_), p(s_), P, Lmax, p(cells), None, None, None) == -1
        msg = L.tsl_last_error().decode()
        assert "nav_field3_paths:" in msg and word in msg and (cells == 0x2B2B).all(), (word, msg)
        assert L.tsl_tsdf_nav_field3_paths_dev(g.h, C.byref(cfg), p(f_), p(p_), p(s_), P, Lmax, p(cells), None, None, None, None) == -1
        assert "nav_field3_paths_dev:" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_nav_field3_paths(g.h, None, p(field), p(par), p(starts), 1, 4, p(cells), None, None, None) == -1 and "null cfg" in L.tsl_last_error().decode()
    with pytest.raises(ValueError):
        g.nav_field3d(cost.astype(np.int32), goals)
    with pytest.raises(ValueError):
        g.nav_field3d(cost[0], goals)
    with pytest.raises(ValueError):
        g.nav_field3d(cost, np.zeros((2, 5), np.int32))
    with pytest.raises(ValueError):
        g.nav_paths3d({"field": field}, starts, 4)
    with pytest.raises(_lib.TslError, match="neutral"):
        g.nav_field3d(cost, goals, neutral=0)
    with pytest.raises(_lib.TslError, match="L must"):
        g.nav_paths3d({"field": field, "parent": par}, starts, 0)
    _compare("random %d x %d x %d" % shape, cost, goals)

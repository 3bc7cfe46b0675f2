"""Free boxes and corridors on the GPU (tsl_nav_corridor.hip): nav_boxes and nav_corridor equal the restatement (tests/nav_corridor_ref.py) byte for byte on
the hand-built volumes of tests/nav_corridor_scenes.py -- partial words, boxes across bit 63 / 64, runs of up to five words, slabs of every kind of face
with more items than a wave (tests/test_nav_corridor_cpu.py counts them), every kind of seed -- in the host and the device forms; planes against per-plane calls; corridors fed from nav_paths and nav_paths3d; the device form behind
other work on its stream; one chain from the room map to a corridor in metres; the refusals; and two calls giving the same bytes."""
import ctypes as C

import numpy as np
import pytest

import nav_corridor_ref as ref
import nav_corridor_scenes as sc
from taichislam_amd import _lib
from util import SMALL, TALL

pytestmark = pytest.mark.gpu

_MAP = []
_REF = {}
BOX_SCENES = sc.box_scenes()
CORRIDOR_SCENES = sc.corridor_scenes()
KEYS = ("boxes", "seed", "link", "count", "status")


def _map():
    """one small handle for the whole module: it lends the device, the stream and scratch, its map is never read"""
    from taichislam_amd.mapping import DenseTSDF
    if not _MAP:
        _MAP.append(DenseTSDF(**TALL))
    return _MAP[0]


def _want_boxes(scene):
    """the restatement of a scene, computed once and shared"""
    name, cost, cells, free_below, ext = scene
    if name not in _REF:
        _REF[name] = ref.boxes(cost, cells, free_below, ext)
        for a in _REF[name]:
            a.setflags(write=False)
    return _REF[name]


def _want_corridor(scene):
    name, cost, cells, length, free_below, ext, Q = scene
    if name not in _REF:
        _REF[name] = ref.corridor(cost, cells, length, free_below, ext, Q)
        for a in _REF[name].values():
            a.setflags(write=False)
    return _REF[name]


def _host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def _same_boxes(got, want, what):
    b, f = _host(got["boxes"]), _host(got["flags"])
    assert b.dtype == np.int16 and f.dtype == np.uint8 and b.shape == want[0].shape and f.shape == want[1].shape, what
    bad = np.nonzero((b != want[0]).any(1) | (f != want[1]))[0]
    assert bad.size == 0, f"{what}: {len(bad)} boxes differ, first at seed {bad[0]}: {b[bad[0]].tolist()} / {f[bad[0]]} != {want[0][bad[0]].tolist()} / {want[1][bad[0]]}"


def _same_corridor(got, want, what):
    for k in KEYS:
        g = _host(got[k])
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k)
        bad = np.argwhere(g != want[k])
        assert bad.size == 0, f"{what}: {k} differs at {len(bad)} places, first {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[k][tuple(bad[0])]}"


@pytest.mark.parametrize("scene", BOX_SCENES, ids=[s[0] for s in BOX_SCENES])
def test_boxes_equal_the_restatement(hip_lib, scene):
    import torch
    name, cost, cells, free_below, ext = scene
    want = _want_boxes(scene)
    _same_boxes(_map().nav_boxes(cost, cells, free_below, ext), want, name)
    dev = _map().nav_boxes(torch.from_numpy(cost).cuda(), cells, free_below, ext)
    assert dev["boxes"].is_cuda and dev["flags"].is_cuda
    _same_boxes(dev, want, name + " (device)")
    _same_boxes(_map().nav_boxes(cost, cells, free_below, ext, device=True), want, name + " (device=True)")


def test_hand_worked_boxes(hip_lib):
    cost = sc.l_shape()
    for c, ext, want, flag in sc.L_SHAPE_CASES:
        got = _map().nav_boxes(cost, [c], sc.FREE_BELOW, ext)
        assert got["boxes"][0].tolist() == want and got["flags"][0] == flag, (c, ext)
    plane = _map().nav_boxes(cost[0], [[4, 0], [2, 0]], extent=4)    # [H, W] with [S, 2]: an int extent is (0, e, e)
    assert plane["boxes"].tolist() == [[0, 4, 0, 0, 4, 4], [0, 0, 0, 0, 4, 0]] and plane["flags"].tolist() == [0, 0]
    import torch
    dev_cells = _map().nav_boxes(torch.from_numpy(cost[0]).cuda(), torch.tensor([[4, 0], [2, 0], [9, 9]], dtype=torch.int64).cuda(), extent=4)      # cells on the device stay there
    assert dev_cells["boxes"].is_cuda and dev_cells["boxes"].cpu().tolist() == [[0, 4, 0, 0, 4, 4], [0, 0, 0, 0, 4, 0], [-1] * 6] and dev_cells["flags"].cpu().tolist() == [0, 0, 2]
    none = _map().nav_boxes(cost, np.zeros((0, 3), np.int32))       # S = 0 is no error
    assert none["boxes"].shape == (0, 6) and none["flags"].shape == (0,)


def test_planes_equal_per_plane_calls(hip_lib):
    B, H, W = 3, 21, 70
    cost = sc.random_volume(B, H, W, share=0.05, seed=21)
    rng = np.random.default_rng(4)
    cells = np.stack([rng.integers(0, B, 60), rng.integers(0, H, 60), rng.integers(0, W, 60)], 1).astype(np.int32)
    both = _map().nav_boxes(cost, cells, extent=(0, 6, 30))
    _same_boxes(both, ref.boxes(cost, cells, sc.FREE_BELOW, (0, 6, 30)), "planes")
    as_grid = _map().nav_boxes({"cost": cost, "cls": None}, cells, extent=30)      # the dict of nav_grid: an int extent stays in the plane
    _same_boxes(as_grid, ref.boxes(cost, cells, sc.FREE_BELOW, (0, 30, 30)), "planes, dict")
    as_volume = _map().nav_boxes({"cost": cost, "stride": 4}, cells, extent=2)     # the dict of flight_volume: it does not
    _same_boxes(as_volume, ref.boxes(cost, cells, sc.FREE_BELOW, (2, 2, 2)), "volume, dict")
    for b in range(B):
        rows = np.nonzero(cells[:, 0] == b)[0]
        one = _map().nav_boxes(cost[b], cells[rows, 1:], extent=(0, 6, 30))
        assert (one["boxes"][:, [0, 3]] == 0).all()
        assert one["boxes"][:, [1, 2, 4, 5]].tobytes() == both["boxes"][rows][:, [1, 2, 4, 5]].tobytes() and one["flags"].tobytes() == both["flags"][rows].tobytes()


@pytest.mark.parametrize("scene", CORRIDOR_SCENES, ids=[s[0] for s in CORRIDOR_SCENES])
def test_corridors_equal_the_restatement(hip_lib, scene):
    import torch
    name, cost, cells, length, free_below, ext, Q = scene
    want = _want_corridor(scene)
    got = _map().nav_corridor(cost, (cells, length), free_below, ext, Q)
    _same_corridor(got, want, name)
    assert got["free_below"] == free_below and got["extent"] == tuple(ext)
    dev = _map().nav_corridor(torch.from_numpy(cost).cuda(), (torch.from_numpy(cells).cuda(), torch.from_numpy(length).cuda()), free_below, ext, Q)
    assert all(dev[k].is_cuda for k in KEYS)
    _same_corridor(dev, want, name + " (device)")


def test_hand_worked_touch_only_link(hip_lib):
    _, cost, cells, length, fb, ext, Q = sc.touch_only()
    got = _map().nav_corridor(cost, (cells, length), fb, ext, Q)
    w = sc.TOUCH_ONLY_WANT
    assert got["boxes"][0, :2].tolist() == w["boxes"] and got["seed"][0, :2].tolist() == w["seed"] and got["link"][0, :2].tolist() == w["link"]
    assert got["count"][0] == w["count"] and got["status"][0] == w["status"] and (got["boxes"][0, 2:] == -1).all()


def _plane_scene():
    """two cost planes with walls and one goal each, for nav_field / nav_paths"""
    cost = sc.random_volume(2, 40, 70, share=0.12, seed=31)
    free = np.argwhere(cost < sc.FREE_BELOW)
    goals = np.array([free[free[:, 0] == 0][5], free[free[:, 0] == 1][-7]], np.int32)
    rng = np.random.default_rng(8)
    starts = free[rng.integers(0, len(free), 24)].astype(np.int32)
    return cost, goals, starts


def test_corridors_from_nav_paths_2d(hip_lib):
    cost, goals, starts = _plane_scene()
    g = _map()
    field = g.nav_field(cost, goals)
    paths = g.nav_paths(field, starts, 128)
    assert (paths["status"] == 0).sum() >= 12 and paths["cells"].shape == (24, 128, 2)
    got = g.nav_corridor(cost, paths, extent=(0, 9, 9), max_boxes=128, planes=starts[:, 0])      # (an int on a raw [B, H, W] array would reach across planes)
    assert got["extent"] == (0, 9, 9)
    cells3 = np.concatenate([np.broadcast_to(starts[:, 0].astype(np.int16)[:, None, None], (24, 128, 1)), paths["cells"]], 2)
    want = ref.corridor(cost, cells3, paths["length"], sc.FREE_BELOW, (0, 9, 9), 128)
    _same_corridor(got, want, "nav_paths")
    ok = paths["status"] == 0
    assert (got["status"][ok] == 0).all() and (got["link"][ok][:, 0] == 0).all() and ((got["link"][ok] & 4) == 0).sum() > 0
    # a margin: free_below under the field's lethal blocks some path cells
    tight = g.nav_corridor(cost, paths, free_below=150, extent=(0, 9, 9), max_boxes=128, planes=starts[:, 0])
    _same_corridor(tight, ref.corridor(cost, cells3, paths["length"], 150, (0, 9, 9), 128), "nav_paths, free_below 150")
    assert ((tight["link"] != ref.TAIL_LINK) & ((tight["link"] & 4) != 0)).any()
    one_plane = g.nav_corridor(cost[0], g.nav_paths(g.nav_field(cost[0], goals[:1]), starts[starts[:, 0] == 0], 128), extent=9)      # planes default to 0
    rows = np.nonzero(starts[:, 0] == 0)[0]
    want0 = ref.corridor(cost[:1], cells3[rows], paths["length"][rows], sc.FREE_BELOW, (0, 9, 9), 64)
    _same_corridor(one_plane, want0, "nav_paths, one plane")


def test_corridors_from_nav_paths3d_device_form_behind_other_work(hip_lib):
    import torch
    cost = sc.random_volume(*sc.RANDOM_SHAPE)
    free = np.argwhere(cost < sc.FREE_BELOW)
    goals = free[[100]].astype(np.int32)
    rng = np.random.default_rng(12)
    starts = free[rng.integers(0, len(free), 40)].astype(np.int32)
    g = _map()
    field = g.nav_field3d(cost, goals)
    paths = g.nav_paths3d(field, starts, 96)
    assert (paths["status"] == 0).sum() >= 20
    want = ref.corridor(cost, paths["cells"], paths["length"], sc.FREE_BELOW, sc.RANDOM_EXT, 32)
    host = g.nav_corridor(cost, paths, extent=sc.RANDOM_EXT, max_boxes=32)
    _same_corridor(host, want, "nav_paths3d")
    want_b = ref.boxes(cost, starts, sc.FREE_BELOW, sc.RANDOM_EXT)
    # the device form on a side stream, its inputs produced by work queued just before it on that stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), device="cuda")
        for _ in range(6):
            big = big @ big * 1e-4
        ct = torch.zeros(cost.shape, dtype=torch.uint8, device="cuda")
        ct += torch.from_numpy(cost).cuda() + (big[0, 0] * 0).to(torch.uint8)      # the cost depends on the work before it
        dfield = g.nav_field3d(ct, goals, rounds_fixed=field["rounds"] + 4)      # (rounds after the last one that changed anything visit no tile)
        dpaths = g.nav_paths3d(dfield, starts, 96)
        dev = g.nav_corridor(ct, dpaths, extent=sc.RANDOM_EXT, max_boxes=32)
        dev_b = g.nav_boxes(ct, starts, extent=sc.RANDOM_EXT)
        after = {k: dev[k].clone() for k in KEYS}                   # work queued behind the call sees its results
    side.synchronize()
    _same_corridor(dev, want, "nav_paths3d (device, side stream)")
    _same_corridor(after, want, "nav_paths3d (device, read by the stream)")
    _same_boxes(dev_b, want_b, "nav_boxes (device, side stream)")
    for k in KEYS:
        assert _host(dev[k]).tobytes() == host[k].tobytes(), k


def test_two_calls_give_identical_bytes_and_scratch_is_reused(hip_lib):
    big, small = CORRIDOR_SCENES[4], CORRIDOR_SCENES[0]
    a = _map().nav_corridor(big[1], (big[2], big[3]), big[4], big[5], big[6])
    s = _map().nav_corridor(small[1], (small[2], small[3]), small[4], small[5], small[6])      # a smaller problem in the same scratch
    b = _map().nav_corridor(big[1], (big[2], big[3]), big[4], big[5], big[6])
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    _same_corridor(s, _want_corridor(small), "small after big")
    scene = BOX_SCENES[-1]
    x, y = _map().nav_boxes(*scene[1:]), _map().nav_boxes(*scene[1:])
    assert x["boxes"].tobytes() == y["boxes"].tobytes() and x["flags"].tobytes() == y["flags"].tobytes()


ROOM_STRIDE, ROOM_MAX_DIST = 4, 2.0


def test_room_chain_from_the_map_to_a_corridor_in_metres(hip_lib):
    """update_esdf, flight_volume, nav_field3d, nav_paths3d from the reached frontier clusters, nav_corridor, corridor_metres"""
    import render_view_scenes as rv
    from taichislam_amd.mapping import DenseTSDF
    from taichislam_amd.utils import corridor_metres, flight_lut, frontier_reach3d
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.update_esdf(max_dist=ROOM_MAX_DIST)
    vs = float(m.voxel_scale)
    vol = m.flight_volume(stride=ROOM_STRIDE, lut=flight_lut(vs, 0.1 + ROOM_STRIDE * vs * np.sqrt(3.0) / 2.0, 0.8, scale=3.0))
    cost = vol["cost"]
    T0 = frames[0][1]
    cam = np.array([T0[2], T0[0], T0[1]], np.float64) / vs + np.array(vol["half"]) - np.array(vol["origin"])
    cand = np.argwhere(cost < 253)
    seed = cand[np.argmin(((cand * ROOM_STRIDE + ROOM_STRIDE // 2 - cam) ** 2).sum(1))]
    field = m.nav_field3d(vol, np.array([seed], np.int32))
    fr = m.extract_frontiers()
    reach = frontier_reach3d(fr, field, vol)
    hit = np.nonzero(reach["reached"])[0]
    assert len(hit) >= 1
    u = fr["indices"][reach["voxel"][hit]].astype(int)
    org, half = vol["origin"], vol["half"]
    starts = np.stack([(u[:, 2] + half[0] - org[0]) // ROOM_STRIDE, (u[:, 0] + half[1] - org[1]) // ROOM_STRIDE, (u[:, 1] + half[2] - org[2]) // ROOM_STRIDE], 1).astype(np.int32)
    paths = m.nav_paths3d(field, starts, 512)
    assert (paths["status"] == 0).all()
    got = m.nav_corridor(vol, paths, extent=8, max_boxes=512)                     # max_boxes = L: no path can be cut
    assert got["extent"] == (8, 8, 8)
    _same_corridor(got, ref.corridor(cost, paths["cells"], paths["length"], 253, (8, 8, 8), 512), "room")
    assert (got["status"] == 0).all()                               # every corridor is complete
    print(f"room: {len(hit)} paths of {paths['length'].min()} .. {paths['length'].max()} cells -> {got['count'].min()} .. {got['count'].max()} boxes; "
          f"links 1 / 2: {int(((got['link'] & 3) == 1).sum())} / {int(((got['link'] & 3) == 2).sum())}")
    metres = corridor_metres(got["boxes"], vol)
    assert metres.shape == got["boxes"].shape[:2] + (2, 3)
    free = cost < 253
    for p in range(len(hit)):
        n = int(got["count"][p])
        assert np.isnan(metres[p, n:]).all() and np.isfinite(metres[p, :n]).all()
        for q in range(n):
            b = got["boxes"][p, q].astype(int)
            assert free[b[0]:b[3] + 1, b[1]:b[4] + 1, b[2]:b[5] + 1].all(), (p, q)      # every box cell is free in the volume
            for corner in (b[:3], b[3:]):                           # the samples of the corner cells, as flight_volume places them, lie inside the metric box
                k, i, j = (corner * ROOM_STRIDE + ROOM_STRIDE // 2 + np.array(vol["origin"]) - np.array(vol["half"])).astype(np.float32) * np.float32(vs)
                xyz = np.array([i, j, k], np.float64)
                assert (metres[p, q, 0] < xyz).all() and (xyz < metres[p, q, 1]).all(), (p, q)
        # and the path's cells lie in the boxes of their corridor
        cells = paths["cells"][p, :paths["length"][p]].astype(int)
        bx = got["boxes"][p, :n].astype(int)
        assert all(((bx[:, :3] <= c) & (c <= bx[:, 3:])).all(1).any() for c in cells), p


def _cfg(shape, **kw):
    c = _lib.NavCorridorCfg()
    c.D, c.H, c.W = shape
    c.free_below, c.ext_k, c.ext_i, c.ext_j, c.max_boxes = 253, 2, 3, 4, 4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_refusals_leave_the_handle_usable(hip_lib):
    L, g = hip_lib, _map()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    cost = sc.random_volume(4, 9, 30, share=0.05, seed=2)
    shape = cost.shape
    cells = sc.probe_cells(shape, 8)
    S = len(cells)
    want = ref.boxes(cost, cells, 253, (2, 3, 4))

    def raw_boxes(cfg, cs, cl, n):
        boxes, flags = np.full((S, 6), 0x2B2B, np.int16), np.full(S, 0xAB, np.uint8)
        return L.tsl_tsdf_nav_boxes(g.h, None if cfg is None else C.byref(cfg), p(cs), p(cl), n, p(boxes), p(flags)), boxes, flags
    rc, b0, f0 = raw_boxes(_cfg(shape), cost, cells, S)
    assert rc == 0 and b0.tobytes() == want[0].tobytes() and f0.tobytes() == want[1].tobytes()
    bad = [("D", dict(D=0)), ("D", dict(D=4097)), ("H", dict(H=0)), ("H", dict(H=4097)), ("W", dict(W=-1)), ("W", dict(W=4097)), ("2^28", dict(D=4096, H=4096, W=17)),
           ("free_below", dict(free_below=0)), ("free_below", dict(free_below=256)), ("ext_k", dict(ext_k=-1)), ("ext_k", dict(ext_k=128)), ("ext_i", dict(ext_i=128)),
           ("ext_i", dict(ext_i=-2)), ("ext_j", dict(ext_j=128)), ("ext_j", dict(ext_j=-1))]
    cases = [(w, _cfg(shape, **kw), cost, cells, S) for w, kw in bad]
    cases += [("S must", _cfg(shape), cost, cells, -1), ("S must", _cfg(shape), cost, cells, (1 << 20) + 1), ("null cells", _cfg(shape), cost, None, 1),
              ("null cost", _cfg(shape), None, cells, S), ("null cfg", None, cost, cells, S)]
    for word, cfg, cs, cl, n in cases:
        rc, b, f = raw_boxes(cfg, cs, cl, n)
        msg = L.tsl_last_error().decode()
        assert rc == -1 and "nav_boxes:" in msg and word in msg, (word, msg)
        assert (b == 0x2B2B).all() and (f == 0xAB).all(), word      # nothing was written
        assert L.tsl_tsdf_nav_boxes_dev(g.h, None if cfg is None else C.byref(cfg), p(cs), p(cl), n, p(b), p(f), None) == -1      # (refused before any pointer is used)
        assert "nav_boxes_dev:" in L.tsl_last_error().decode()
        rc, b, f = raw_boxes(_cfg(shape), cost, cells, S)           # a good call still succeeds, with the same bytes
        assert rc == 0 and b.tobytes() == b0.tobytes() and f.tobytes() == f0.tobytes(), word
    assert L.tsl_tsdf_nav_boxes(None, C.byref(_cfg(shape)), p(cost), p(cells), S, None, None) == -1 and "null handle" in L.tsl_last_error().decode()
    assert raw_boxes(_cfg(shape, max_boxes=0), cost, cells, S)[0] == 0      # max_boxes is not read by the boxes forms
    assert L.tsl_tsdf_nav_boxes(g.h, C.byref(_cfg(shape)), p(cost), None, 0, None, None) == 0      # S = 0 with null cells; every output is nullable
    assert L.tsl_tsdf_nav_boxes(g.h, C.byref(_cfg(shape)), p(cost), p(cells), S, None, None) == 0
    only_flags = np.full(S, 0xAB, np.uint8)
    assert L.tsl_tsdf_nav_boxes(g.h, C.byref(_cfg(shape)), p(cost), p(cells), S, None, p(only_flags)) == 0 and only_flags.tobytes() == f0.tobytes()

    # the corridor forms
    _, _, pc, plen, _, _, _ = sc.short_paths()
    P, Lp = pc.shape[:2]
    wantc = ref.corridor(cost, pc, plen, 253, (2, 3, 4), 4)

    def raw_corridor(cfg, cs, cl, ln, np_, nl, Q=4):
        out = [np.full((P, Q, 6), 0x2B2B, np.int16), np.full((P, Q), 0x2B2B2B2B, np.int32), np.full((P, Q), 0xAB, np.uint8), np.full(P, 0x2B2B2B2B, np.int32),
               np.full(P, 0xAB, np.uint8)]
        return L.tsl_tsdf_nav_corridor(g.h, None if cfg is None else C.byref(cfg), p(cs), p(cl), p(ln), np_, nl, *[p(a) for a in out]), out
    rc, out0 = raw_corridor(_cfg(shape), cost, pc, plen, P, Lp)
    assert rc == 0 and all(a.tobytes() == wantc[k].tobytes() for a, k in zip(out0, KEYS))
    cases = [("P must", _cfg(shape), cost, pc, plen, -1, Lp), ("P must", _cfg(shape), cost, pc, plen, (1 << 16) + 1, 4), ("L must", _cfg(shape), cost, pc, plen, P, 0),
             ("L must", _cfg(shape), cost, pc, plen, P, 4097), ("P * L", _cfg(shape), cost, pc, plen, 1 << 16, 65), ("max_boxes", _cfg(shape, max_boxes=0), cost, pc, plen, P, Lp),
             ("max_boxes", _cfg(shape, max_boxes=Lp + 1), cost, pc, plen, P, Lp), ("null cells", _cfg(shape), cost, None, plen, P, Lp),
             ("null length", _cfg(shape), cost, pc, None, P, Lp), ("null cost", _cfg(shape), None, pc, plen, P, Lp), ("null cfg", None, cost, pc, plen, P, Lp),
             ("free_below", _cfg(shape, free_below=0), cost, pc, plen, P, Lp), ("ext_j", _cfg(shape, ext_j=200), cost, pc, plen, P, Lp), ("W", _cfg(shape, W=0), cost, pc, plen, P, Lp)]
    for word, cfg, cs, cl, ln, np_, nl in cases:
        rc, out = raw_corridor(cfg, cs, cl, ln, np_, nl)
        msg = L.tsl_last_error().decode()
        assert rc == -1 and "nav_corridor:" in msg and word in msg, (word, msg)
        assert (out[0] == 0x2B2B).all() and (out[1] == 0x2B2B2B2B).all() and (out[2] == 0xAB).all() and (out[3] == 0x2B2B2B2B).all() and (out[4] == 0xAB).all(), word
        assert L.tsl_tsdf_nav_corridor_dev(g.h, None if cfg is None else C.byref(cfg), p(cs), p(cl), p(ln), np_, nl, p(out[0]), None, None, None, None, None) == -1
        assert "nav_corridor_dev:" in L.tsl_last_error().decode()
        rc, out = raw_corridor(_cfg(shape), cost, pc, plen, P, Lp)
        assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(out, out0)), word
    assert L.tsl_tsdf_nav_corridor(g.h, C.byref(_cfg(shape)), p(cost), None, None, 0, Lp, None, None, None, None, None) == 0      # P = 0 is no error
    assert L.tsl_tsdf_nav_corridor(g.h, C.byref(_cfg(shape)), p(cost), p(pc), p(plen), P, Lp, None, None, None, None, None) == 0  # every output is nullable
    # the Python layer
    with pytest.raises(ValueError):
        g.nav_boxes(cost.astype(np.int32), cells)
    with pytest.raises(ValueError):
        g.nav_boxes(cost, cells[:, :2])                             # [S, 2] needs an [H, W] cost
    with pytest.raises(ValueError):
        g.nav_boxes(cost[0, 0], cells)
    with pytest.raises(ValueError):
        g.nav_boxes(cost, cells, extent=(1, 2))
    with pytest.raises(ValueError):
        g.nav_corridor(cost, (pc[:, :, :1], plen))
    with pytest.raises(_lib.TslError, match="ext_k"):
        g.nav_boxes(cost, cells, extent=128)                        # an int on a [D, H, W] array reaches along every axis: the layers are refused first
    with pytest.raises(_lib.TslError, match="ext_i"):
        g.nav_boxes(cost[0], cells[:, 1:], extent=128)              # on an [H, W] plane it is (0, e, e)
    with pytest.raises(_lib.TslError, match="max_boxes"):
        g.nav_corridor(cost, (pc, plen), max_boxes=Lp + 1)
    _same_boxes(g.nav_boxes(cost, cells, extent=(2, 3, 4)), want, "after the refusals")

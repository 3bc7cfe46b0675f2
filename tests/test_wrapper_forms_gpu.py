"""The two forms of every planner-facing wrapper of DenseTSDF -- numpy in / numpy out and torch device tensors in / out -- give the same bytes, for
batches of 0, 1 and 3 and with every optional output off and on.  One 2 m map of 0.1 m voxels, three synthetic frames, polylines of K = 5, images of
24 x 32: the cases the larger tests of each method leave out, small enough to run in well under a second each."""
import numpy as np
import pytest

from util import small_stream

pytestmark = pytest.mark.gpu

H, W, KP = 24, 32, 5
SIZES = (0, 1, 3)
_CACHE = {}


def _map():
    """the map, textured, with an ESDF; made once and only read by the tests"""
    if "g" not in _CACHE:
        from taichislam_amd.mapping import DenseTSDF
        K, frames = small_stream(3, H, W, radius=0.8, orbit=0.2)
        g = DenseTSDF(map_scale=[2.0, 2.0], voxel_scale=0.1, num_voxel_per_blk_axis=16, max_ray_length=2.0, min_ray_length=0.1, internal_voxels=4,
                      texture_enabled=True)
        g.set_dep_camera_intrinsic(K)
        g.set_color_camera_intrinsic(K)
        tex = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)
        for R, T, d in frames:
            g.recast_depth_to_map(R, T, d, tex)
        g.update_esdf(max_dist=0.5)
        _CACHE["g"], _CACHE["K"], _CACHE["pose"] = g, K, frames[1][:2]
    return _CACHE["g"]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(v):
    return v.cpu().numpy() if hasattr(v, "is_cuda") else v


def same(dev, host, what):
    """dev (tensors) and host (arrays) hold the same bytes in the same shapes; dicts and tuples member by member, None as None, the rest by =="""
    if isinstance(host, dict):
        assert set(dev) == set(host), (what, sorted(dev), sorted(host))
        for k in host:
            same(dev[k], host[k], f"{what}[{k}]")
    elif isinstance(host, (tuple, list)) and not all(isinstance(x, (int, float)) for x in host):
        assert len(dev) == len(host), what
        for i, (a, b) in enumerate(zip(dev, host)):
            same(a, b, f"{what}[{i}]")
    elif isinstance(host, np.ndarray):
        assert hasattr(dev, "is_cuda") and dev.is_cuda, f"{what}: the device form returned no device tensor"
        d = np.ascontiguousarray(_host(dev))
        assert d.shape == host.shape and d.dtype.itemsize == host.dtype.itemsize, (what, d.shape, d.dtype, host.shape, host.dtype)
        assert d.tobytes() == np.ascontiguousarray(host).tobytes(), what
    else:
        assert dev is host or dev == host, (what, dev, host)


def _points(n, seed=1):
    return np.random.default_rng(seed).uniform(-0.9, 0.9, (n, 3)).astype(np.float32)


def _lines(n, K=KP, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.5, 0.5, (n, 1, 3)) + np.cumsum(rng.normal(size=(n, K, 3)) * 0.08, axis=1)).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_point_and_ray_queries(hip_lib, n):
    g = _map()
    p = _points(n)
    for mode, param in ((0, 0), (1, 0), (2, 1)):
        same(g._query_points(mode, _t(p), param), g._query_points(mode, p, param), f"query_points mode {mode}")
    d = _points(n, 5)
    same(g.raycast(_t(p), _t(d), 1.5), g.raycast(p, d, 1.5), "raycast")
    if n == 3:
        assert g.raycast(p, d, 1.5)[0].dtype == bool and g.is_pos_unobserved(p).dtype == bool


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("colors", [False, True, None])
def test_render_view(hip_lib, normals, colors):
    g = _map()
    R, T = _CACHE["pose"]
    kw = dict(K=_CACHE["K"], shape=(H, W), normals=normals, colors=colors)
    host = g.render_view(R, T, **kw)
    same(g.render_view(R, T, device=True, **kw), host, "render_view")
    assert (host[1] is not None) == normals and (host[2] is not None) == (colors is not False) and (host[3] == 0).sum() > 100


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rays", [False, True])
def test_score_views(hip_lib, n, rays):
    from taichislam_amd.mapping.dense_tsdf import VIEW_GAIN_DTYPE
    g = _map()
    R, T = _CACHE["pose"]
    Rn, Tn = np.repeat(R[None], n, 0), np.repeat(T[None], n, 0) + np.arange(n)[:, None] * 0.05
    host = g.score_views(Rn, Tn, K=_CACHE["K"], shape=(H, W), rays=rays)
    dev = g.score_views(Rn, Tn, K=_CACHE["K"], shape=(H, W), rays=rays, device=True)
    assert set(dev) == {"records"} | ({"ray_unknown", "ray_status"} if rays else set()) and ("ray_status" in host) == rays
    rec = np.ascontiguousarray(dev["records"].cpu().numpy())
    assert rec.shape == (n, 16) and rec.dtype == np.int32
    rec = rec.reshape(-1).view(VIEW_GAIN_DTYPE)
    for k in VIEW_GAIN_DTYPE.names:
        assert np.array_equal(rec[k], host[k]), k
    for k in ("ray_unknown", "ray_status") if rays else ():
        same(dev[k], host[k], k)
    assert host["unknown_volume"].shape == (n,) and host["free_volume"].dtype == np.float64


@pytest.mark.parametrize("lut", [False, True])
@pytest.mark.parametrize("extras", [False, True])
def test_nav_grid_and_terrain(hip_lib, lut, extras):
    from taichislam_amd.utils.nav import inflation_lut
    g = _map()
    table = inflation_lut(0.1, 3, 0.1, 0.3) if lut else None
    kw = dict(bands=[(-2, 2), (0, 5)], radius=0.3, lut=table)
    host = g.nav_grid(counts=extras, span=extras, **kw)
    same(g.nav_grid(counts=extras, span=extras, device=True, **kw), host, "nav_grid")
    assert ("cost" in host) == lut and ("counts" in host) == extras and ("span" in host) == extras and (host["cls"] == 0).any()
    host = g.nav_terrain(clearance=0.3, **kw)
    same(g.nav_terrain(clearance=0.3, device=True, **kw), host, "nav_terrain")
    assert ("cost" in host) == lut and host["height"].shape == (2, g.N, g.N)


def _cost(shape, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 120, shape).astype(np.uint8)
    c[rng.random(shape) < 0.15] = 254
    return c


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("parent", [False, True])
@pytest.mark.parametrize("dims", [2, 3])
def test_nav_fields_and_paths(hip_lib, S, parent, dims):
    g = _map()
    cost = _cost((2, 16, 16) if dims == 2 else (4, 12, 12))
    free = np.argwhere(cost < 253)
    goals = free[:: max(1, len(free) // 3)][:S].astype(np.int64)
    field, paths = (g.nav_field, g.nav_paths) if dims == 2 else (g.nav_field3d, g.nav_paths3d)
    host = field(cost, goals, parent=parent)
    for how, dev in (("tensor", field(_t(cost), goals, parent=parent)), ("device=True", field(cost, goals, parent=parent, device=True)),
                     ("dict", field({"cost": _t(cost)}, goals, parent=parent, rounds_fixed=0))):
        same({k: v for k, v in dev.items() if k != "goals"}, {k: v for k, v in host.items() if k != "goals"}, f"field ({how})")
        assert np.array_equal(dev["goals"], host["goals"])
    assert ("parent" in host) == parent and host["goals"].shape == (S, 4) and host["n_bad_seeds"] == 0
    if not parent:
        with pytest.raises(ValueError):
            paths(host, free[:1], 8)
        return
    for P in SIZES:
        starts = free[5:: max(1, len(free) // 4)][:P]
        hp = paths(host, starts, 8)
        same(paths(dev, starts, 8), hp, f"paths P = {P}")
        assert hp["cells"].shape == (P, 8, dims) and hp["cost"].dtype == np.uint32


@pytest.mark.parametrize("S", SIZES)
def test_nav_boxes(hip_lib, S):
    g = _map()
    cost = _cost((3, 16, 16), 4)
    cells = np.argwhere(cost < 253)[3::97][:S]
    host = g.nav_boxes(cost, cells, extent=4)
    assert host["boxes"].shape == (S, 6) and host["flags"].shape == (S,)
    same(g.nav_boxes(_t(cost), cells, extent=4), host, "tensor cost")
    same(g.nav_boxes(cost, cells, extent=4, device=True), host, "device=True")
    same(g.nav_boxes(cost, _t(cells.reshape(-1, 3)), extent=4), host, "device cells")
    two = g.nav_boxes(cost[0], cells[:, 1:], extent=(0, 3, 3))
    same(g.nav_boxes(_t(cost[0]), _t(cells[:, 1:].reshape(-1, 2)), extent=(0, 3, 3)), two, "[H, W] cost, [S, 2] cells")


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("width", [2, 3])
def test_nav_corridor(hip_lib, P, width):
    g = _map()
    cost = _cost((3, 16, 16), 4)
    rng = np.random.default_rng(6)
    cells = np.cumsum(rng.integers(-1, 2, (P, 6, 3)), axis=1).astype(np.int16) + np.int16(6)
    cells[:, :, 0] = 1
    length = np.array([6, 1, 4], np.int32)[:P]
    planes = np.array([0, 2, 1], np.int16)[:P]
    c = cells if width == 3 else cells[:, :, 1:]
    for pl in ((None,) if width == 3 else (None, planes)):
        host = g.nav_corridor(cost, (c, length), extent=3, max_boxes=4, planes=pl)
        assert host["boxes"].shape == (P, 4, 6) and host["count"].shape == (P,)
        same(g.nav_corridor(_t(cost), (c, length), extent=3, max_boxes=4, planes=pl), host, "tensor cost")
        same(g.nav_corridor(cost, {"cells": _t(c), "length": _t(length)}, extent=3, max_boxes=4, planes=None if pl is None else _t(pl)), host, "tensor paths")


@pytest.mark.parametrize("n", SIZES)
def test_query_esdf(hip_lib, n):
    g = _map()
    p = _points(n)
    for interpolate, gradient in ((True, None), (True, False), (False, None)):
        for refresh in (False, True):
            kw = dict(interpolate=interpolate, gradient=gradient, unknown_value=-2.5, refresh=refresh)
            host = g.query_esdf(p, **kw)
            same(g.query_esdf(_t(p), **kw), host, f"query_esdf {kw}")
            assert (host[1] is not None) == (interpolate and gradient is None) and host[0].shape == (n,)
    if n == 3:
        dv = g.flight_volume(stride=4, device=True)
        hv = g.flight_volume(stride=4)
        same(dv, hv, "flight_volume")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("samples", [False, True])
def test_score_paths(hip_lib, n, samples):
    g = _map()
    w = _lines(n)
    lengths = np.array([5, 1, 3], np.int32)[:n]
    for ln in (None, lengths):
        kw = dict(margin=0.1, sub=3, samples=samples, unknown_value=-2.5, refresh=False)
        host = g.score_paths(w, 0.2, lengths=ln, **kw)
        same(g.score_paths(_t(w), 0.2, lengths=None if ln is None else _t(ln), **kw), host, "score_paths")
        assert ("sample_dist" in host) == samples and host["cost"].dtype == np.int64 and host["min_dist"].dtype == np.float32
    if n == 1:
        one = g.score_paths(w[0], 0.2, **kw)
        same(g.score_paths(_t(w[0]), 0.2, **kw), one, "one path")
        assert one["n_samples"].shape == (1,)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("extras", [False, True])
def test_trajectories(hip_lib, n, extras):
    g = _map()
    c = _lines(n, seed=7)
    lengths = np.array([5, 4, 4], np.int32)[:n]
    for ln in (None, lengths):
        lt = None if ln is None else _t(ln)
        host = g.traj_linearize(c, 0.3, sub=2, lengths=ln, gradients=extras, refresh=False)
        same(g.traj_linearize(_t(c), 0.3, sub=2, lengths=lt, gradients=extras, refresh=False), host, "traj_linearize")
        assert ("grad_collision" in host) == extras and host["cost_smooth"].dtype == np.int64
        kw = dict(sub=2, iters=3, fix_ends=1, history=extras, refresh=False)
        host = g.traj_optimize(c, 0.3, lengths=ln, **kw)
        same(g.traj_optimize(_t(c), 0.3, lengths=lt, **kw), host, "traj_optimize")
        assert ("history" in host) == extras and host["ctrl"].shape == (n, KP, 3) and (not extras or host["history"].shape == (n, 4, 2))
    if n == 1:
        one = g.traj_optimize(c[0], 0.3, **kw)
        same(g.traj_optimize(_t(c[0]), 0.3, **kw), one, "one trajectory")
        assert one["ctrl"].shape == (KP, 3) and one["iters_done"].shape == (1,)

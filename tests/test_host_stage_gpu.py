"""The host-pointer forms built on the staging helper (taichislam_amd/csrc/tsl_stage.hpp) against their _dev twins, on one map of 2 x 2 x 2 bricks with a
sphere in it: every converted entry point gives the same bytes through host pointers and through device pointers -- with every optional output, with each
optional output alone (a region in front is absent: the offsets move) and, where an entry point allows it, with none; at sizes that leave regions off a
16-byte boundary unless the helper rounds (1, 3 and 17 points, rays and waypoints; 3 paths of 5 cells; 3 seeds); one staging buffer serving one family
after another; and the refusals nav_grid and nav_terrain share, word for word."""
import ctypes as C

import numpy as np
import pytest

from taichislam_amd import _lib

pytestmark = pytest.mark.gpu

MAP = dict(map_scale=[1.28, 1.28], voxel_scale=0.04, num_voxel_per_blk_axis=16, max_submap_num=1, max_bricks=64)
N = 32                                  # voxels per side: 2 bricks
BANDS = [(-8, -1), (0, 7)]
R = 3                                   # radius of the distance transform in voxels
LUT = np.arange(R * R + 2, dtype=np.uint8) * 20
ODD = (1, 3, 17)
_SHARED = {}


def _fresh():
    """a map of 2 x 2 x 2 bricks holding a sphere of 10 voxels radius in a cube of 30^3 observed voxels, its ESDF up to date"""
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**MAP)
    assert (g.N, g.Nz) == (N, N)
    g.init_sphere(voxels=30, radius=0.4)
    g.update_esdf()
    return g


def _map():
    if "g" not in _SHARED:
        _SHARED["g"] = _fresh()
    return _SHARED["g"]


class In:
    """an input array; when = the output that needs it (None: always passed)"""
    def __init__(self, arr, when=None):
        self.arr, self.when = np.ascontiguousarray(arr), when


class Out:
    """an output plane; optional: the entry point takes NULL for it; group: optional outputs that come together"""
    def __init__(self, name, dtype, shape, optional=True, group=None, cast=None):
        self.name, self.dtype, self.shape, self.optional, self.group, self.cast = name, np.dtype(dtype), tuple(shape), optional, group or name, cast

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize


def _call(L, fn, args, want, dev):
    """one call of `fn` with the outputs named in `want` (the others NULL): {name: bytes}.  Output buffers start as 0xAB; the device form gets torch
    buffers and the NULL stream, which is the stream torch copies back on."""
    import torch
    keep, outs, argv = [], {}, []
    for a in args:
        if isinstance(a, In):
            if a.when is not None and a.when not in want:
                argv.append(None)
            elif dev:
                keep.append(torch.from_numpy(a.arr.view(np.uint8).reshape(-1).copy()).cuda())
                argv.append(keep[-1].data_ptr())
            else:
                argv.append(a.arr.ctypes.data_as(C.c_void_p))
        elif isinstance(a, Out):
            if a.name not in want:
                argv.append(None)
            elif dev:
                outs[a.name] = torch.full((a.nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
                argv.append(outs[a.name].data_ptr())
            else:
                outs[a.name] = np.full(a.nbytes, 0xAB, np.uint8)
                p = outs[a.name].ctypes.data_as(C.c_void_p)
                argv.append(C.cast(p, a.cast) if a.cast else p)
        else:
            argv.append(a)
    if dev:
        argv.append(None)
    rc = getattr(L, fn)(*argv)
    assert rc == 0, (fn, want, L.tsl_last_error().decode())
    return {k: (v.cpu().numpy() if dev else v).tobytes() for k, v in outs.items()}


def _variants(args, none_allowed=True):
    """every output; each optional group alone beside the required ones; the required ones alone"""
    outs = [a for a in args if isinstance(a, Out)]
    req = tuple(o.name for o in outs if not o.optional)
    v = [tuple(o.name for o in outs)]
    for grp in dict.fromkeys(o.group for o in outs if o.optional):
        v.append(req + tuple(o.name for o in outs if o.optional and o.group == grp))
    if req and none_allowed:
        v.append(req)
    return list(dict.fromkeys(v))


def _host_equals_dev(L, name, args, same=None, none_allowed=True):
    """the host form `name` against `name`_dev for every variant; same: {output: comparison} for an output that is not compared as bytes.  Returns the host
    result with every output."""
    full = None
    for want in _variants(args, none_allowed):
        host, dev = _call(L, name, args, want, False), _call(L, name + "_dev", args, want, True)
        assert set(host) == set(dev) == set(want), (name, want)
        for k in want:
            if same and k in same:
                same[k](host[k], dev[k], (name, want, k))
            else:
                assert host[k] == dev[k], f"{name} with outputs {want}: {k} differs between the host and the device form"
            assert host[k] != b"\xab" * len(host[k]) or len(host[k]) < 4, f"{name} with outputs {want}: {k} was not written"
        if full is None:
            full = host
        else:
            for k in want:
                if not (same and k in same):
                    assert host[k] == full[k], f"{name}: {k} with outputs {want} differs from the call with every output"
    return full


def _points(n, seed):
    """n points, most inside the volume (+-0.64 m), a few outside"""
    return np.random.default_rng(seed).uniform(-0.7, 0.7, (n, 3)).astype(np.float32)


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.55, 0.55, (n, 3)).astype(np.float32)
    pos[np.linalg.norm(pos, axis=1) < 0.45] *= np.float32(0.0)          # inside the sphere every ray hits at once: start those at the centre of it
    d = rng.normal(size=(n, 3))
    return pos, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# ---- the point, ray, path and view queries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ODD)
def test_query_points_and_raycast(hip_lib, n):
    g = _map()
    for mode, param in ((0, 0), (1, 0), (2, 1)):
        _host_equals_dev(hip_lib, "tsl_tsdf_query_points", [g.h, mode, param, In(_points(n, 1)), n, Out("out", np.uint8, (n,), optional=False)])
    pos, d = _rays(n, 2)
    _host_equals_dev(hip_lib, "tsl_tsdf_query_raycast", [g.h, In(pos), In(d), 1.0, n, Out("hit", np.uint8, (n,), optional=False),
                                                         Out("end", np.float32, (n, 3), optional=False), Out("len", np.float32, (n,), optional=False)])


@pytest.mark.parametrize("n", ODD)
def test_esdf_query_points(hip_lib, n):
    g = _map()
    _host_equals_dev(hip_lib, "tsl_esdf_query_points", [g.h, 1, float("nan"), In(_points(n, 3)), n, Out("dist", np.float32, (n,), optional=False),
                                                        Out("grad", np.float32, (n, 3)), Out("status", np.uint8, (n,), optional=False)])
    _host_equals_dev(hip_lib, "tsl_esdf_query_points", [g.h, 0, 7.5, In(_points(n, 4)), n, Out("dist", np.float32, (n,), optional=False), None,
                                                        Out("status", np.uint8, (n,), optional=False)])


@pytest.mark.parametrize("K", ODD)
def test_score_paths(hip_lib, K):
    g = _map()
    P, sub = 3, 2
    smax = (K - 1) * sub + 1
    wp = np.random.default_rng(5).uniform(-0.6, 0.6, (P, K, 3)).astype(np.float32)
    lengths = np.array([K, max(1, K - 1), 1], np.int32)
    for ln in (In(lengths), None):
        _host_equals_dev(hip_lib, "tsl_esdf_score_paths", [g.h, 1, float("nan"), In(wp), ln, P, K, sub, 0.05, 0.1, 6, Out("out", np.uint8, (P, 40), optional=False),
                                                           Out("sample_dist", np.float32, (P, smax)), Out("sample_status", np.uint8, (P, smax))])


def test_render_view_and_view_gain(hip_lib):
    g = _map()
    eye, T = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(0.0, 0.0, -0.6)
    v = _lib.ViewCfg()
    v.h, v.w, v.t_min, v.t_max = 5, 7, 0.05, 1.2
    v.K[0], v.K[4], v.K[2], v.K[5], v.K[8] = 4.0, 4.0, 3.0, 2.0, 1.0
    full = _host_equals_dev(hip_lib, "tsl_tsdf_render_view", [g.h, eye, T, C.byref(v), Out("depth", np.float32, (5, 7), optional=False), Out("normal", np.float32, (5, 7, 3)),
                                                              None, Out("status", np.uint8, (5, 7), optional=False)])      # (rgb needs a textured map)
    assert np.frombuffer(full["depth"], np.float32).max() > 0.0          # the camera looks at the sphere
    n = 3
    Rs, Ts = (C.c_double * (9 * n))(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * n)), (C.c_double * (3 * n))(0.0, 0.0, -0.6, 0.1, 0.0, -0.5, 0.5, 0.5, 0.5)
    c = _lib.GainCfg()
    c.h, c.w, c.t_min, c.t_max = 3, 5, 0.05, 1.2
    c.K[0], c.K[4], c.K[2], c.K[5], c.K[8] = 3.0, 3.0, 2.0, 1.0, 1.0
    _host_equals_dev(hip_lib, "tsl_tsdf_view_gain", [g.h, Rs, Ts, n, C.byref(c), Out("out", np.uint8, (n, 64), optional=False),
                                                     Out("ray_unknown", np.int32, (n, 3, 5), group="rays"), Out("ray_status", np.uint8, (n, 3, 5), group="rays")])


# ---- the navigation family --------------------------------------------------------------------------------------------------------------------
def _bands(cfg):
    cfg.n_bands = len(BANDS)
    for b, (k0, k1) in enumerate(BANDS):
        cfg.k_min[b], cfg.k_max[b] = k0, k1
    cfg.radius, cfg.cost_unknown = R, 200
    return cfg


def _terrain_cfg():
    cfg = _bands(_lib.NavTerrainCfg())
    cfg.clearance, cfg.free_run, cfg.pick, cfg.window, cfg.slope_base, cfg.max_step, cfg.min_support, cfg.max_slope2 = 3, 1, 0, 2, 1, 8, 1, 0xffffffff
    return cfg


def _nav_grid_args(g, cfg):
    B = len(BANDS)
    return [g.h, C.byref(cfg), In(LUT, when="cost"), Out("cls", np.uint8, (B, N, N)), Out("d2", np.uint16, (B, N, N)), Out("cost", np.uint8, (B, N, N)),
            Out("counts", np.uint16, (B, N, N, 3)), Out("span", np.int16, (B, N, N, 2))]


def _nav_terrain_args(g, cfg):
    B = len(BANDS)
    return [g.h, C.byref(cfg), In(LUT, when="cost"), Out("height", np.int16, (B, N, N)), Out("col", np.uint8, (B, N, N)), Out("step", np.uint16, (B, N, N)),
            Out("nsup", np.uint16, (B, N, N)), Out("slope2", np.uint32, (B, N, N)), Out("cls", np.uint8, (B, N, N)), Out("d2", np.uint16, (B, N, N)),
            Out("cost", np.uint8, (B, N, N))]


def _cost_planes():
    """the cost planes of nav_grid on the shared map, [2, 32, 32]: what the field, path, box and corridor calls below run on"""
    if "cost" not in _SHARED:
        got = _map().nav_grid(bands=BANDS, radius=R * MAP["voxel_scale"], lut=LUT, cost_unknown=200)
        _SHARED["cost"] = np.ascontiguousarray(got["cost"])
        _SHARED["cost"].setflags(write=False)
    return _SHARED["cost"]


def _seeds(cost, lethal=253):
    """3 seeds (leading index, row, col, value) on traversable cells: the first, the middle and the last of them"""
    cells = np.argwhere(cost < lethal)
    assert len(cells) >= 3
    pick = cells[[0, len(cells) // 2, len(cells) - 1]]
    return np.ascontiguousarray(np.concatenate([pick, [[0], [7], [3]]], 1).astype(np.int32))


def test_nav_grid_and_nav_terrain(hip_lib):
    g = _map()
    full = _host_equals_dev(hip_lib, "tsl_tsdf_nav_grid", _nav_grid_args(g, _bands(_lib.NavCfg())))
    assert len(set(full["cls"])) == 3                                    # free, occupied and unknown cells: the sphere, the cube around it, the rim
    _host_equals_dev(hip_lib, "tsl_tsdf_nav_terrain", _nav_terrain_args(g, _terrain_cfg()))


def test_nav_field_and_paths(hip_lib):
    g, L = _map(), hip_lib
    P, Lp = 3, 5
    starts_of = lambda shape: np.ascontiguousarray(np.array([[0, 2, 2], [shape[0] - 1, shape[1] // 2, 3], [0, shape[1] - 1, shape[2] - 1]], np.int32))
    # 2-D: one 32 x 32 tile per plane, so no tile meets a neighbour's write-back and the statistics are schedule-free too: bytes
    cost = _cost_planes()
    cfg = _lib.NavFieldCfg(2, N, N, 50, 253, 8, 0, 0, 0, 0)
    seeds = _seeds(cost)
    field_args = [g.h, C.byref(cfg), In(cost), In(seeds), len(seeds), Out("field", np.uint32, cost.shape, optional=False), Out("parent", np.uint8, cost.shape),
                  Out("stats", np.uint8, (24,), cast=C.POINTER(_lib.NavFieldStats))]
    f2 = _host_equals_dev(L, "tsl_tsdf_nav_field", field_args)
    assert (np.frombuffer(f2["field"], np.uint32) != _lib.NAV_UNREACHED).sum() > 3
    path_args = [g.h, C.byref(cfg), In(np.frombuffer(f2["field"], np.uint32)), In(np.frombuffer(f2["parent"], np.uint8)), In(starts_of(cost.shape)), P, Lp,
                 Out("cells", np.int16, (P, Lp, 2)), Out("length", np.int32, (P,)), Out("status", np.uint8, (P,)), Out("cost", np.uint32, (P,))]
    _host_equals_dev(L, "tsl_tsdf_nav_field_paths", path_args)
    # 3-D: 8 tiles of 16 x 8 x 8 cells; the header says the round count may depend on the schedule where tiles meet, so of the statistics only converged and
    # n_bad_seeds are compared (field and parent depend on no schedule)
    vol = np.ascontiguousarray(np.repeat(cost, 4, axis=0))             # [8, 32, 32]
    cfg3 = _lib.NavField3Cfg(8, N, N, 50, 253, 26, 0, 0, 0, 0)
    seeds3 = _seeds(vol)

    def same_stats(a, b, what):
        sa, sb = _lib.NavField3Stats.from_buffer_copy(a), _lib.NavField3Stats.from_buffer_copy(b)
        assert (sa.converged, sa.n_bad_seeds) == (sb.converged, sb.n_bad_seeds) == (1, 0) and sa.rounds > 0 and sb.rounds > 0, what

    f3 = _host_equals_dev(L, "tsl_tsdf_nav_field3", [g.h, C.byref(cfg3), In(vol), In(seeds3), len(seeds3), Out("field", np.uint32, vol.shape, optional=False),
                                                     Out("parent", np.uint8, vol.shape), Out("stats", np.uint8, (24,), cast=C.POINTER(_lib.NavField3Stats))],
                          same={"stats": same_stats})
    _host_equals_dev(L, "tsl_tsdf_nav_field3_paths", [g.h, C.byref(cfg3), In(np.frombuffer(f3["field"], np.uint32)), In(np.frombuffer(f3["parent"], np.uint8)),
                                                      In(starts_of(vol.shape)), P, Lp, Out("cells", np.int16, (P, Lp, 3)), Out("length", np.int32, (P,)),
                                                      Out("status", np.uint8, (P,)), Out("cost", np.uint32, (P,))])


def test_nav_boxes_and_corridor(hip_lib):
    g = _map()
    cost = _cost_planes()
    cfg = _lib.NavCorridorCfg(2, N, N, 253, 0, 6, 6, 3)
    cells = np.ascontiguousarray(_seeds(cost)[:, :3])
    _host_equals_dev(hip_lib, "tsl_tsdf_nav_boxes", [g.h, C.byref(cfg), In(cost), In(cells), 3, Out("boxes", np.int16, (3, 6)), Out("flags", np.uint8, (3,))])
    P, Lp, Q = 3, 5, 3
    rows = np.array([[[1, 2 + t, 2 + t] for t in range(Lp)], [[0, 16, 3 + t] for t in range(Lp)], [[1, 29 - t, 29] for t in range(Lp)]], np.int16)      # [P][L][3]
    length = np.array([5, 3, 4], np.int32)
    _host_equals_dev(hip_lib, "tsl_tsdf_nav_corridor", [g.h, C.byref(cfg), In(cost), In(rows), In(length), P, Lp, Out("boxes", np.int16, (P, Q, 6)),
                                                        Out("seed", np.int32, (P, Q)), Out("link", np.uint8, (P, Q)), Out("count", np.int32, (P,)),
                                                        Out("status", np.uint8, (P,))])


# ---- the topology graph, which stages in a buffer of its own ------------------------------------------------------------------------------------
def _octahedron(centre, r):
    """7 of the 8 faces of an octahedron: an odd count"""
    c = np.asarray(centre, np.float32)
    ax = [c + np.float32(r) * np.eye(3, dtype=np.float32)[a] * s for a in range(3) for s in (1, -1)]      # +x -x +y -y +z -z
    faces = [(ax[i], ax[2 + j], ax[4 + k]) for i in range(2) for j in range(2) for k in range(2)][:7]
    return np.ascontiguousarray(np.array(faces, np.float32).reshape(7, 9))


@pytest.mark.parametrize("n", ODD)
def test_topo_add_poly_and_rays(hip_lib, n):
    g, L = _map(), hip_lib
    t = C.c_void_p()
    assert L.tsl_topo_create(g.h, 8, 1.0, 1024, C.byref(t)) == 0
    try:
        centre = (0.45, 0.45, 0.45)                                      # free space between the sphere and the rim of the observed cube
        tris, nf = _octahedron(centre, 0.06), 7
        start = (C.c_float * 3)(*centre)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def add(want):
            assert L.tsl_topo_reset(t) == 0
            o = {"is_frontier": np.full(nf, 0xAB, np.uint8), "reason": np.full(nf, 0xAB, np.uint8), "neigh": np.full(nf, -1431655766, np.int32)}
            node = C.c_int32(-1)
            rc = L.tsl_topo_add_poly(t, p(tris), nf, start, 0.5, *[p(o[k]) if k in want else None for k in ("is_frontier", "reason", "neigh")], None, C.byref(node))
            assert rc == 0 and node.value == 0, L.tsl_last_error().decode()
            return {k: o[k].tobytes() for k in want}

        full = add(("is_frontier", "reason", "neigh"))                    # (there is no device form: each output alone against all three)
        for k in full:
            assert add((k,))[k] == full[k], k
        assert add(()) == {}
        pos = np.ascontiguousarray(np.tile(np.array(centre, np.float32), (n, 1)))
        d = _rays(n, 6)[1]
        skip = np.full(n, -1, np.int32)
        outs = [Out("hit", np.uint8, (n,)), Out("type", np.uint8, (n,)), Out("end", np.float32, (n, 3)), Out("len", np.float32, (n,)), Out("poly", np.int32, (n,))]
        for sk in (None, In(skip)):
            args = [t, In(pos), In(d), sk, n, 1.0, -0.01, 0] + outs
            every = tuple(o.name for o in outs)
            dev = _call(L, "tsl_topo_rays_dev", args, every, True)        # (the device form takes no NULL output)
            for want in _variants(args):
                host = _call(L, "tsl_topo_rays", args, want, False)
                for k in want:
                    assert host[k] == dev[k], f"topo_rays with outputs {want}: {k} differs from the device form"
            assert (np.frombuffer(dev["hit"], np.uint8) <= 1).all() and np.isfinite(np.frombuffer(dev["len"], np.float32)).all()      # written
    finally:
        L.tsl_topo_destroy(t)


# ---- one staging buffer, one family after another ---------------------------------------------------------------------------------------------
def _flat(v):
    """every array of a result, as bytes, in a fixed order"""
    if isinstance(v, dict):
        return [(k, b) for key in sorted(v) for k, b in [(f"{key}.{s}", b) for s, b in _flat(v[key])]]
    if isinstance(v, (tuple, list)):
        return [(f"{i}.{s}", b) for i, x in enumerate(v) for s, b in _flat(x)]
    return [("", np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())]


def test_reuse_across_families(hip_lib):
    """a large call, a small one, other families, and the large one again, through one buffer: each equals the call made alone on a fresh map (stale bytes,
    a grow that frees a buffer in use, a smaller call reading the old extent)"""
    pts, (pos, d) = _points(1000, 7), _rays(3, 8)
    cost = _cost_planes()
    seeds = _seeds(cost)[:, :3]
    starts = np.array([[0, 2, 2], [1, 16, 3], [0, 31, 31]], np.int32)
    steps = {
        "query_esdf": lambda g, r: g.query_esdf(pts),
        "raycast": lambda g, r: g.raycast(pos, d, 1.0),
        "nav_grid": lambda g, r: g.nav_grid(bands=BANDS, radius=R * MAP["voxel_scale"], lut=LUT, cost_unknown=200, counts=True, span=True),
        "nav_field": lambda g, r: g.nav_field(cost, seeds),
        "nav_paths": lambda g, r: g.nav_paths(r["nav_field"], starts, 5),
        "nav_boxes": lambda g, r: g.nav_boxes(cost, seeds, extent=6),
        "nav_corridor": lambda g, r: g.nav_corridor(cost, r["nav_paths"], extent=6, max_boxes=3, planes=starts[:, 0]),
    }
    alone = {}
    for name, step in steps.items():                                    # each call on a map that makes no other (nav_paths and nav_corridor read an earlier result)
        alone[name] = step(_fresh(), alone)
    g, seq = _fresh(), {}
    for name, step in steps.items():
        seq[name] = step(g, seq)
        assert _flat(seq[name]) == _flat(alone[name]), f"{name} behind the calls before it differs from {name} alone"
    again = steps["query_esdf"](g, seq)
    assert _flat(again) == _flat(seq["query_esdf"]) == _flat(alone["query_esdf"])
    assert np.isfinite(again[0]).sum() > 100 and (np.asarray(seq["nav_paths"]["length"]) > 0).any()


# ---- the refusals of the shared band check ----------------------------------------------------------------------------------------------------------
def test_shared_refusals_read_the_same(hip_lib):
    g, L = _map(), hip_lib
    cls = np.zeros((2, N, N), np.uint8)
    p = cls.ctypes.data_as(C.c_void_p)

    def both(change, cost=None):
        msgs = []
        for who, cfg, call in (("nav_grid", _bands(_lib.NavCfg()), lambda c, sfx: getattr(L, "tsl_tsdf_nav_grid" + sfx)(g.h, C.byref(c), None, p, None, cost, None, None, *([None] if sfx else []))),
                               ("nav_terrain", _terrain_cfg(), lambda c, sfx: getattr(L, "tsl_tsdf_nav_terrain" + sfx)(g.h, C.byref(c), None, None, None, None, None, None, p, None, cost, *([None] if sfx else [])))):
            change(cfg)
            for sfx in ("", "_dev"):                                     # (refused before any pointer is used: host memory does for the device form)
                assert call(cfg, sfx) == -1
                head, _, text = L.tsl_last_error().decode().partition(": ")
                assert head == who + sfx, head
                msgs.append(text)
        assert len(set(msgs)) == 1, msgs
        assert (cls == 0).all()
        return msgs[0]

    def empty(c): c.k_min[0], c.k_max[0] = 3, 2
    def leaves(c): c.k_max[1] = N // 2
    def radius(c): c.radius = 255
    assert both(empty) == "band 0 is empty (k_min > k_max) or leaves the volume"
    assert both(leaves) == "band 1 is empty (k_min > k_max) or leaves the volume"
    assert both(radius) == "radius must be 0 .. 254 voxels"
    assert both(lambda c: None, cost=p) == "cost and lut come together or not at all"

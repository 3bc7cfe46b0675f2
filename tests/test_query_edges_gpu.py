"""The map queries (tsl_query.hip) and the TSDF's point insert on bad input and at the walls, against the CPU oracle, exactly, on the cubic SMALL volume and on
SLAB.  A coordinate that is not finite, or whose cell index does not fit an int, lies outside every map (include/taichislam_hip.h): a query there reads
"outside", a ray "hits" there, a cloud point there is gated.  Every ray is cast with max_dist <= 4 m; a negative or non-finite max_dist is refused."""
import ctypes as C

import numpy as np
import pytest

import octomap_limit_scenes as sc
from util import SLAB, SMALL, assert_export_equal, make_pair

pytestmark = pytest.mark.gpu
CFGS = {"small": SMALL, "slab": SLAB}
STAT_KEYS = ("p_used", "p_valid", "p_oob", "v_pcl", "v_skipped", "steps", "steps_oob", "unique", "bricks")


@pytest.fixture(scope="module", params=["small", "slab"])
def scene(request, hip_lib):
    """(HIP map, oracle, frames, lo, hi) of one volume: the frames of query_scene and its blocks at the walls, in both; shared by the tests and not changed"""
    from oracle import BATCHED
    cfg = CFGS[request.param]
    K, frames, blocks, lo, hi = sc.query_scene(cfg)
    g, o = make_pair(cfg, K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None); o.integrate_depth(R, T, d, mode=BATCHED)
    g.load_numpy(0, blocks["indices"], blocks["TSDF"], blocks["W_TSDF"], blocks["occupy"], np.array([]))
    o.import_sparse(0, blocks["indices"], blocks["TSDF"], blocks["W_TSDF"], blocks["occupy"])
    origin = np.zeros((1, 3), np.float32)
    assert not o.query_points(0, origin)[0] and not o.query_points(1, origin)[0], "voxel (0, 0, 0) must be observed and free"
    return g, o, frames, lo, hi, cfg["voxel_scale"]


def _query(g, mode, pts, param, device):
    if device:
        import torch
        out = g._query_points(mode, torch.from_numpy(pts).cuda(), param)
        return out.cpu().numpy()
    return g._query_points(mode, pts, param)


# ---- 9. bad points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_query_points_read_outside(scene, device):
    """NaN, +-inf, +-1e12, 3e38 and points 10 m out read as outside (occupied and unobserved), not as voxel (0, 0, 0), which is observed and free here"""
    g, o, _, _, _, _ = scene
    pts, is_special, n_special = sc.query_bad_points()
    n_out = sc.BAD_POINTS.shape[0]
    for mode, param in ((0, 0), (1, 0), (2, 2), (2, 1)):
        want = o.query_points(mode, pts, param)
        special = want[is_special]
        assert special[:n_out].all(), f"mode {mode}: the oracle reads a bad point as inside"
        if mode < 2:
            assert special[-8:].all() and not special[[n_out, n_out + 1, n_out + 3]].any()        # 10 m out: outside; -0.0, 0.01 and the origin: cell 0, observed and free
        assert want[~is_special].any() and not want[~is_special].all()
        got = _query(g, mode, pts, param, device)
        assert np.array_equal(got, want), f"mode {mode} param {param}: {np.nonzero(got != want)[0][:10]} of {pts[got != want][:5]}"


# ---- 10. walls and halves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_walls_corners_and_exact_halves(scene, device):
    from taichislam_amd._lib import TslError
    g, o, _, lo, hi, vs = scene
    walls, cells = sc.wall_points(lo, hi, vs)
    inside = np.all((cells >= lo) & (cells < hi), axis=1)
    halves = sc.half_points(vs)
    for mode in (0, 1):
        want = o.query_points(mode, walls)
        assert want[~inside].all() and not want[inside].all(), "the last cell inside must read differently from the first outside"
        assert np.array_equal(_query(g, mode, walls, 0, device), want), f"walls, mode {mode}"
        want = o.query_points(mode, halves)
        assert np.array_equal(_query(g, mode, halves, 0, device), want), f"halves, mode {mode}"
    assert o.query_points(0, halves).any() and not o.query_points(0, halves).all()
    pts = np.concatenate([walls, halves])
    assert not _query(g, 2, pts, 0, device).any() and not o.query_points(2, pts, 0).any()          # param 0: no voxel is looked at
    for param in (1, 2):
        want = o.query_points(2, pts, param)
        assert np.array_equal(_query(g, 2, pts, param, device), want), f"mode 2 param {param}"
    few = np.concatenate([walls[:6], walls[-6:], sc.BAD_POINTS[:5]])                               # a wall, a corner and bad points: 32^3 voxels each
    want = o.query_points(2, few, 16)
    assert np.array_equal(_query(g, 2, few, 16, device), want)
    with pytest.raises(TslError, match="error -1"):
        _query(g, 2, few, 17, device)


# ---- 11. rays -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rays(scene):
    """the ray set of the scene and the oracle's answers for max_dist 0, less than a voxel and 4 m, computed once"""
    g, o, frames, lo, hi, vs = scene
    pos, d, finite = sc.ray_set(frames, lo, hi, vs)
    return pos, d, finite, {md: o.raycast(pos, d, md) for md in (0.0, 0.03, 4.0)}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rays_from_everywhere(scene, rays, device):
    """2000 rays from free space, from the unobserved region, from the surface, from outside the volume and from NaN; hit, end and len bit for bit"""
    g, o, _, lo, hi, vs = scene
    pos, d, finite, want = rays
    free = finite & ~o.query_points(0, pos) & ~o.query_points(1, pos)
    oh = want[4.0][0]
    assert free.sum() > 300 and oh[free].any() and not oh[free].all(), "hits and misses among the finite rays that start in free space"
    assert (~finite).sum() > 100 and oh[~finite].all() and np.isnan(want[4.0][1][~finite]).any()
    assert o.query_points(1, pos[finite]).any() and np.any(np.all(d == 0, axis=1) & free)
    for md, (wh, we, wl) in want.items():
        if device:
            import torch
            gh, ge, gl = (t.cpu().numpy() for t in g.raycast(torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda(), md))
        else:
            gh, ge, gl = g.raycast(pos, d, md)
        assert np.array_equal(gh, wh), f"max_dist {md}: hit differs at {np.nonzero(gh != wh)[0][:10]}"
        assert np.array_equal(ge.view(np.uint32), we.view(np.uint32)), f"max_dist {md}: end differs at {np.nonzero((ge.view(np.uint32) != we.view(np.uint32)).any(1))[0][:10]}"
        assert np.array_equal(gl.view(np.uint32), wl.view(np.uint32)), f"max_dist {md}: len"
        if md < vs:
            assert not wh.any() and not we.any() and not wl.any()                       # no step at all


@pytest.mark.parametrize("max_dist", [-1.0, -0.0001, float("nan"), float("inf"), float("-inf")])
def test_raycast_refuses_a_bad_max_dist(scene, max_dist):
    """(int)(inf / voxel) steps would never end: both forms return TSL_ERR_ARG before any launch and leave the output buffers alone"""
    import torch
    from taichislam_amd._lib import TslError
    g, _, _, _, _, _ = scene
    L = g.L
    n = 64
    pos = np.zeros((n, 3), np.float32); d = np.tile(np.float32([1, 0, 0]), (n, 1))
    hit = np.full(n, 0xAB, np.uint8); end = np.full((n, 3), 7.5, np.float32); ln = np.full(n, 7.5, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.tsl_tsdf_query_raycast(g.h, vp(pos), vp(d), max_dist, n, vp(hit), vp(end), vp(ln)) == -1
    assert (hit == 0xAB).all() and (end == 7.5).all() and (ln == 7.5).all()
    tp, td = torch.from_numpy(pos).cuda(), torch.from_numpy(d).cuda()
    th, te, tl = torch.from_numpy(hit).cuda(), torch.from_numpy(end).cuda(), torch.from_numpy(ln).cuda()
    assert L.tsl_tsdf_query_raycast_dev(g.h, tp.data_ptr(), td.data_ptr(), max_dist, n, th.data_ptr(), te.data_ptr(), tl.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream) == -1
    torch.cuda.synchronize()
    assert (th.cpu().numpy() == 0xAB).all() and (te.cpu().numpy() == 7.5).all() and (tl.cpu().numpy() == 7.5).all()
    with pytest.raises(TslError, match="error -1"):
        g.raycast(pos, d, max_dist)


# ---- 12. bad points in a TSDF cloud ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,group", [("batched", 1), ("batched", 0), ("sequential", 1)])
def test_tsdf_point_insert_gates_bad_points(hip_lib, mode, group):
    """recast_pcl_to_map gates a point by `len < max_ray_length`, which is false for NaN and inf: the bad points count in p_used only, and the map is the map of
    the same cloud without them.  (The sequential semantics need the hash grouping: group 0 exists in the batched mode only.)"""
    from oracle import BATCHED, FAITHFUL
    from taichislam_amd.utils import synthetic as syn
    xyz, is_bad = sc.bad_cloud(n_valid=6000, span=2.5)
    R, T = syn.camera_pose(3)
    omode = FAITHFUL if mode == "sequential" else BATCHED
    g, o = make_pair(SMALL, syn.K_DEPTH)
    g2, o2 = make_pair(SMALL, syn.K_DEPTH)
    for m in (g, g2):
        if mode == "sequential":
            m.set_option("semantics", 1)
        else:
            m.set_option("group", group)
        assert m.get_option("group") == group
    g.recast_pcl_to_map(R, T, xyz, np.array([])); so = o.integrate_points(R, T, xyz, None, mode=omode)
    g2.recast_pcl_to_map(R, T, xyz[~is_bad], np.array([])); so2 = o2.integrate_points(R, T, xyz[~is_bad], None, mode=omode)
    sg, sg2 = g.last_frame_stats(), g2.last_frame_stats()
    assert {k: sg[k] for k in STAT_KEYS} == {k: so[k] for k in STAT_KEYS} and {k: sg2[k] for k in STAT_KEYS} == {k: so2[k] for k in STAT_KEYS}
    assert so["p_used"] - so2["p_used"] == int(is_bad.sum()) and so["p_valid"] > 1000
    assert {k: so[k] for k in STAT_KEYS if k != "p_used"} == {k: so2[k] for k in STAT_KEYS if k != "p_used"}
    assert_export_equal(g.export_submap(), o.export_sparse(), "cloud with bad points")
    assert_export_equal(g.export_submap(), g2.export_submap(), "the same cloud without them")

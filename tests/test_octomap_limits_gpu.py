"""The Octomap (tsl_octo.hip) at its limits and on bad input, against the CPU oracle, exactly: arities 3 and 4, the edges of the tree's lopsided extent,
coordinates that are not finite, a brick pool that fills, the ring of statistics slots, lane groups of 64 and of 1, the depth gate at its bounds and the clamp
of the exports.  The scenes are in octomap_limit_scenes.py; every test asserts from the oracle's output that its scene reaches the path it is about."""
import numpy as np
import pytest

import octomap_limit_scenes as sc
from octomap_limit_scenes import leaves, run_gpu, run_oracle, stats3
from util import small_stream, sorted_rows

pytestmark = pytest.mark.gpu
BRICKS = 4096          # the default pool of 65536 bricks is 1 GiB of counts (7 GiB textured): none of these scenes needs a tenth of this


def _pair(cfg, **gpu_kw):
    from oracle import OracleOctomap
    from taichislam_amd.mapping import Octomap
    gpu_kw.setdefault("max_bricks", BRICKS)
    return Octomap(**cfg, **gpu_kw), OracleOctomap(**cfg)


def _play(g, o, ops, what=""):
    """both sides play `ops`; every insert's statistics are equal.  Returns the oracle's statistics."""
    so = run_oracle(o, ops)
    sg = run_gpu(g, ops)
    for n, s in sg.items():
        assert stats3(s) == stats3(so[n]), f"{what}: statistics of operation {n} ({ops[n][0]})"
    return so


def _assert_leaves(g, o, what, color=False, min_rows=1):
    a, b = leaves(g, color), leaves(o, color)
    assert b.shape[0] >= min_rows, f"{what}: the oracle has {b.shape[0]} leaves"
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: leaves differ ({a.shape[0]} vs {b.shape[0]})"
    return b


def _assert_levels(g, o, levels, what):
    """get_occupy_voxels(level) of both sides for every level; returns the oracle's counts"""
    counts = []
    for level in levels:
        gx, _ = g.get_occupy_voxels(level)
        ox, on = o.occupied_voxels(level)
        assert gx.shape[0] == on and np.array_equal(sorted_rows(gx), sorted_rows(ox)), f"{what}: level {level}"
        counts.append(on)
    return counts


# ---- 1. arity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,map_scale,dims", sc.ARITY_CASES)
def test_arity_3_and_4(hip_lib, K, map_scale, dims):
    """K = 3 (odd N: hN = N / 2 truncates and bricks lie partly outside the tree) and K = 4, cubic and with Rz < Rxy: depth frames from host and device
    images, point clouds, two submaps and their fusion; leaves, statistics and every level of get_occupy_voxels."""
    cfg = sc.arity_cfg(K, map_scale)
    g, o = _pair(cfg)
    assert (g.N, g.Nz, g.Rxy, g.Rz) == (o.N, o.Nz, o.Rxy, o.Rz) == dims
    Kd, subs, bases = sc.arity_ops()
    g.set_dep_camera_intrinsic(Kd); o.set_intrinsics(Kd)
    levels = range(0, dims[2] + 3)
    for sid, ops in enumerate(subs):
        so = _play(g, o, ops, f"submap {sid}")
        if map_scale[1] < map_scale[0]:
            assert so[-1]["p_oob"] > 0, "the flat tree must cut the cloud"
        _assert_leaves(g, o, f"submap {sid}", min_rows=1000)
        counts = _assert_levels(g, o, levels, f"submap {sid}")
        assert len({c for c in counts if c > 0}) >= 3, f"levels of submap {sid}: {counts}"
        g.switch_to_next_submap(); o.set_active_submap(sid + 1)
    gg, og = _pair(dict(cfg, is_global_map=True))
    for sid, (R, T) in enumerate(bases):
        gg.set_base_pose_submap(sid, R, T); og.set_base_pose_submap(sid, R, T)
    gg.fuse_submaps(g); og.fuse_submaps(o)
    _assert_leaves(gg, og, "fused", min_rows=1000)
    counts = _assert_levels(gg, og, levels, "fused")
    assert len({c for c in counts if c > 0}) >= 3 and counts[-1] == counts[-2], f"levels of the fused map: {counts}"      # (the r < 0 break: no level above the root)


# ---- 2. tree edges -----------------------------------------------------------------------------------------------------------------
def test_tree_edges(hip_lib):
    """Cells live in [-hN, ext - hN) with ext = K^(R+1) (for z: K^(1 + min(Rxy, Rz))), not in [-hN, N - hN): points in the last cell inside and the first
    outside on every axis, and the frames of a room larger than the tree."""
    g, o = _pair(sc.EDGE_CFG)
    d = sc.EDGE_DIMS
    assert (g.N, g.Nz, g.Rxy, g.Rz) == (o.N, o.Nz, o.Rxy, o.Rz) == (d["N"], d["Nz"], d["Rxy"], d["Rz"])
    xyz, cells, inside = sc.edge_cloud()
    Kd, frames = small_stream(3)
    g.set_dep_camera_intrinsic(Kd); o.set_intrinsics(Kd)
    ops = [("points", sc.I3, sc.Z3, xyz, None, False)]
    so = _play(g, o, ops, "edge cloud")
    assert stats3(so[0]) == (xyz.shape[0], int(inside.sum()), int((~inside).sum())) and so[0]["p_oob"] > 0
    b = _assert_leaves(g, o, "edge cloud")
    assert np.array_equal(b[:, :3].min(0), [-d["hN"], -d["hN"], -d["hNz"]])
    assert np.array_equal(b[:, :3].max(0), [d["ext_xy"] - d["hN"] - 1, d["ext_xy"] - d["hN"] - 1, d["ext_z"] - d["hNz"] - 1])
    assert b[:, :3].max(0)[0] >= d["N"] - d["hN"] and b[:, :3].max(0)[2] >= d["Nz"] - d["hNz"]              # beyond the nominal N, Nz: the extent is what counts
    ops = [("depth", R, T, dep, None, f == 1) for f, (R, T, dep) in enumerate(frames)] + [("points", sc.I3, sc.Z3, xyz, None, True)]
    so = _play(g, o, ops, "room larger than the tree")
    assert all(s["p_oob"] > 0 and s["p_valid"] > 0 for s in so)
    _assert_leaves(g, o, "room larger than the tree", min_rows=1000)
    _assert_levels(g, o, range(0, d["Rxy"] + 3), "edges")


# ---- 3. coordinates that are not finite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("textured", [False, True], ids=["plain", "textured"])
def test_bad_points_touch_no_leaf(hip_lib, textured, device):
    """NaN, +-inf, +-1e12 and 3e38 in a cloud count in p_oob and touch no leaf (v_cvt_i32_f32 turns NaN into 0: unguarded, each NaN point is a phantom
    hit in leaf (0, 0, 0)); -0.0 is an ordinary point of cell 0."""
    cfg = dict(sc.POOL_CFG, texture_enabled=textured)
    g, o = _pair(cfg)
    xyz, is_bad = sc.bad_cloud()
    rgb = np.random.default_rng(8).integers(0, 256, size=(xyz.shape[0], 3)).astype(np.uint8) if textured else None
    so = _play(g, o, [("points", sc.I3, sc.Z3, xyz, rgb, device)], "bad cloud")
    assert stats3(so[0]) == (xyz.shape[0], int((~is_bad).sum()), int(is_bad.sum()))                  # the valid points all lie inside this tree
    b = _assert_leaves(g, o, "bad cloud", color=textured, min_rows=1000)
    in_zero = int(np.all(sc.cell_of(xyz[~is_bad], 0.05) == 0, axis=1).sum())
    zero = b[np.all(b[:, :3] == 0, axis=1)]
    assert in_zero >= sc.ZERO_POINTS.shape[0] and zero.shape[0] == 1 and zero[0, 3] == in_zero
    ga = leaves(g, textured)
    assert ga[np.all(ga[:, :3] == 0, axis=1)][0, 3] == in_zero, "leaf (0, 0, 0) holds more than its valid points"
    if textured:
        gx, gcol = g.get_occupy_voxels(0)
        ox, ocol, on = o.occupied_voxels(0, with_color=True)
        assert gx.shape[0] == on and np.array_equal(sorted_rows(np.concatenate([gx, gcol], 1)), sorted_rows(np.concatenate([ox, ocol], 1)))


def test_fusion_moves_leaves_out_of_the_tree(hip_lib):
    """a base pose whose translation carries part of a submap over the edge of the global tree (cells [-128, 384)): those leaves are dropped, the rest lands
    where the oracle puts it; the second submap's pose carries all of it far beyond any int cell index"""
    cfg = dict(sc.POOL_CFG, max_submap_num=4)
    g, o = _pair(cfg)
    xyz, _ = sc.bad_cloud()
    ops = [("points", sc.I3, sc.Z3, xyz, None, False), ("next",), ("points", sc.I3, sc.Z3, xyz[::2], None, True), ("next",)]
    _play(g, o, ops, "submaps")
    gg, og = _pair(dict(cfg, is_global_map=True))
    th = np.deg2rad(20.0)
    Rb = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    for m in (gg, og):
        m.set_base_pose_submap(0, Rb, np.array([-5.0, 18.0, 0.3]))
        m.set_base_pose_submap(1, sc.I3, np.array([0.0, 1e12, 0.0]))
    gg.fuse_submaps(g); og.fuse_submaps(o)
    b = _assert_leaves(gg, og, "fused over the edge", min_rows=100)
    o.set_active_submap(0)
    src = leaves(o)
    assert 0 < b[:, 3].sum() < src[:, 3].sum(), "the pose must move some, not all, of submap 0 out of the tree"
    assert b[:, 0].min() == -128 or b[:, 1].max() == 383


# ---- 4. a pool that fills ------------------------------------------------------------------------------------------------------------
def _assert_partial(g, o_full, total, what):
    """what does not depend on which four bricks got in: the statistics raise the capacity error once; the exported leaves span exactly four bricks and are the
    oracle's leaves inside those, with its counts; p_valid is their sum and p_valid + p_oob the oracle's"""
    from taichislam_amd._lib import TslError
    with pytest.raises(TslError, match="error -3"):
        g.last_frame_stats()
    s = g.last_frame_stats()                                                         # the flag was cleared by the first read
    a, b = leaves(g), leaves(o_full)
    got = sc.bricks_of(a[:, :3], sc.POOL_HN, sc.POOL_HN)
    assert got.shape[0] == 4 and sc.bricks_of(b[:, :3], sc.POOL_HN, sc.POOL_HN).shape[0] > 16, what
    u = (b[:, :3].astype(np.int64) + sc.POOL_HN) >> 4
    keep = np.zeros(b.shape[0], bool)
    for br in got:
        keep |= np.all(u == br, axis=1)
    assert np.array_equal(a, b[keep]), f"{what}: the leaves inside the four bricks"
    assert s["p_valid"] == a[:, 3].sum() > 0 and s["p_valid"] + s["p_oob"] == total, what


def test_full_pool_points_and_queued_depth(hip_lib):
    from oracle import OracleOctomap
    g, o = _pair(sc.POOL_CFG, max_bricks=4)
    wide = sc.wide_cloud()
    of = OracleOctomap(**sc.POOL_CFG)
    so = of.integrate_points(sc.I3, sc.Z3, wide)
    g.recast_pcl_to_map(sc.I3, sc.Z3, wide, None)
    _assert_partial(g, of, so["p_valid"] + so["p_oob"], "cloud")
    g.reset()
    _play(g, o, [("points", sc.I3, sc.Z3, sc.four_brick_cloud(), None, False)], "after reset")       # raises nothing: the pool holds exactly these four
    b = _assert_leaves(g, o, "after reset", min_rows=1000)
    assert sc.bricks_of(b[:, :3], sc.POOL_HN, sc.POOL_HN).shape[0] == 4
    # the same on the queued depth path (k_octo_depth_batch), from a device image
    g.reset(); o.reset()
    Kd, frames = small_stream(1)
    of = OracleOctomap(**sc.POOL_CFG); of.set_intrinsics(Kd)
    so = of.integrate_depth(*frames[0])
    g.set_dep_camera_intrinsic(Kd)
    run_gpu(g, [("depth", *frames[0], None, True)], read=())
    _assert_partial(g, of, so["p_valid"] + so["p_oob"], "queued frame")
    g.reset()
    g.set_dep_camera_intrinsic(sc.FOUR_BRICK_K); o.set_intrinsics(sc.FOUR_BRICK_K)
    R, T, d = sc.four_brick_frame()
    _play(g, o, [("depth", R, T, d, None, True), ("depth", R, T, d, None, False)], "four-brick frames after reset")
    b = _assert_leaves(g, o, "four-brick frames after reset", min_rows=400)
    assert sc.bricks_of(b[:, :3], sc.POOL_HN, sc.POOL_HN).shape[0] == 4


def test_full_pool_in_fusion(hip_lib):
    from taichislam_amd._lib import TslError
    g, o = _pair(sc.POOL_CFG)
    _play(g, o, [("points", sc.I3, sc.Z3, sc.wide_cloud(), None, False), ("next",)], "wide submap")
    gs, os_ = _pair(sc.POOL_CFG)
    _play(gs, os_, [("points", sc.I3, sc.Z3, sc.four_brick_cloud(), None, False), ("next",)], "small submap")
    gg, og = _pair(dict(sc.POOL_CFG, is_global_map=True), max_bricks=4)
    with pytest.raises(TslError, match="error -3"):
        gg.fuse_submaps(g)
    a = leaves(gg)
    og.fuse_submaps(o)
    b = leaves(og)
    got = sc.bricks_of(a[:, :3], sc.POOL_HN, sc.POOL_HN)
    u = (b[:, :3].astype(np.int64) + sc.POOL_HN) >> 4
    keep = np.zeros(b.shape[0], bool)
    for br in got:
        keep |= np.all(u == br, axis=1)
    assert got.shape[0] == 4 and np.array_equal(a, b[keep])
    gg.reset()
    assert leaves(gg).shape[0] == 0
    gg.fuse_submaps(gs); og.fuse_submaps(os_)                                       # usable again, and raises nothing
    _assert_leaves(gg, og, "fusion after the reset", min_rows=1000)


# ---- 5. statistics ring ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring():
    """the stream of test_statistics_ring and what the oracle makes of it, computed once"""
    from oracle import OracleOctomap
    Kd, ops = sc.ring_ops()
    o = OracleOctomap(**sc.RING_CFG); o.set_intrinsics(Kd)
    so = run_oracle(o, ops)
    return Kd, ops, so, leaves(o, True)


@pytest.mark.parametrize("reads", [None, sc.RING_READS_2], ids=["every_frame", "every_8th"])
def test_statistics_ring(hip_lib, ring, reads):
    """140 frames through the ring of 64 statistics slots (the index wraps twice, each half is cleared when it is entered, by octo_next_stats or by the queued
    path's own code): every statistics read, after every frame or after every 8th and around the two seams, is the oracle's for that frame"""
    from taichislam_amd.mapping import Octomap
    Kd, ops, so, want = ring
    assert len(ops) == sc.RING_FRAMES and all(s["p_oob"] > 0 and s["p_valid"] > 0 for s in so)
    assert len({stats3(s) for s in so}) > sc.RING_FRAMES // 2                      # the frames differ: a stale slot would show
    g = Octomap(**sc.RING_CFG, max_bricks=1024)
    g.set_dep_camera_intrinsic(Kd); g.set_color_camera_intrinsic(Kd)
    sg = run_gpu(g, ops, read=reads)
    assert len(sg) == (len(ops) if reads is None else len(reads))
    for n, s in sg.items():
        assert stats3(s) == stats3(so[n]), f"statistics read after operation {n}"
    a = leaves(g, True)
    assert a.shape == want.shape and np.array_equal(a, want)


# ---- 6. group sizes --------------------------------------------------------------------------------------------------------------------
def test_lane_groups_of_64_and_of_1(hip_lib):
    """k_octo_depth_batch groups the lanes of a wave by leaf and adds the group's size: 0.5 m voxels put whole waves into one leaf, 5 mm voxels leave every
    pixel alone in its leaf"""
    Kd, frames = small_stream(2)
    g, o = _pair(sc.COARSE_CFG)
    g.set_dep_camera_intrinsic(Kd); o.set_intrinsics(Kd)
    Kw, R, T, wall = sc.wall_frame()
    tiles = sc.wave_tiles(Kw, wall, sc.COARSE_CFG["recast_step"], 0.5)
    assert sum(t.shape[0] == 64 and np.unique(t, axis=0).shape[0] == 1 for t in tiles) >= 4, "no wave falls into one leaf"
    assert any(np.unique(t, axis=0).shape[0] >= 3 for t in tiles), "no wave is split over three leaves"
    _play(g, o, [("depth", R, T, wall, None, True)], "0.5 m wall")
    b = _assert_leaves(g, o, "0.5 m wall")
    assert b[:, 3].max() >= 64 and b[:, 3].sum() == wall.size
    g.reset(); o.reset()
    _play(g, o, [("depth", *frames[0], None, True)], "0.5 m")
    b = _assert_leaves(g, o, "0.5 m")
    assert b[:, 3].max() >= 64 and b[:, 3].min() >= 1                               # some leaf gains a wave's worth from one frame
    _play(g, o, [("depth", *frames[1], None, False), ("depth", *frames[0], None, True)], "0.5 m")
    a = leaves(g)
    assert np.array_equal(a, leaves(o)) and np.array_equal(a[:, 3], np.round(a[:, 3]))
    g, o = _pair(sc.FINE_CFG, max_bricks=8192)
    g.set_dep_camera_intrinsic(Kd); o.set_intrinsics(Kd)
    so = _play(g, o, [("depth", *frames[0], None, True)], "5 mm")
    b = _assert_leaves(g, o, "5 mm", min_rows=1000)
    assert b[:, 3].max() == 1 and b.shape[0] == so[0]["p_valid"]


# ---- 7. depth gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["queued", "textured"])
def test_depth_gate_at_its_bounds(hip_lib, kernel):
    """d != 0 and thr_min <= d <= thr_max with thr_max = 3333.3 (no whole number of millimetres): 299 and 3334 are gated, 300 and 3333 are not"""
    textured = kernel == "textured"
    g, o = _pair(dict(sc.GATE_CFG, texture_enabled=textured))
    Kd, R, T, d = sc.gate_frame()
    g.set_dep_camera_intrinsic(Kd); g.set_color_camera_intrinsic(Kd); o.set_intrinsics(Kd)
    sampled = d[::2, ::2]
    assert all((sampled == v).sum() > 50 for v in sc.GATE_VALUES)
    tex = np.random.default_rng(2).integers(0, 256, size=d.shape + (3,)).astype(np.uint8) if textured else None
    so = _play(g, o, [("depth", R, T, d, tex, not textured), ("depth", R, T, d, tex, False)], kernel)
    assert so[0]["p_valid"] == int(np.isin(sampled, sc.GATE_PASS).sum()) and so[0]["p_oob"] == 0 and so[0]["p_used"] == sampled.size
    _assert_leaves(g, o, kernel, color=textured, min_rows=50)


# ---- 8. export clamp ---------------------------------------------------------------------------------------------------------------------
def _rows_in(rows, pool):
    """every row of `rows` is a row of `pool`, and no two are the same row"""
    have = {r.tobytes() for r in np.ascontiguousarray(pool, dtype=np.float32)}
    mine = [r.tobytes() for r in np.ascontiguousarray(rows, dtype=np.float32)]
    return len(set(mine)) == len(mine) and all(r in have for r in mine)


def test_exports_clamped_at_max_disp_particles(hip_lib):
    """more occupied voxels than max_disp_particles: the counter counts them all, the buffer holds the first max_disp_particles of them; and
    cvt_occupy_voxels_to appends another map's voxels to the same buffers"""
    Kd, frames = small_stream(2)
    _, other = small_stream(2, start_deg=120.0)                                     # looks elsewhere: the two maps share no voxel
    cfg = dict(sc.POOL_CFG)
    a, oa = _pair(cfg, max_disp_particles=100)
    b, ob = _pair(cfg, max_disp_particles=100)
    for m, o, fr in ((a, oa, frames), (b, ob, other)):
        m.set_dep_camera_intrinsic(Kd); o.set_intrinsics(Kd)
        _play(m, o, [("depth", *f, None, False) for f in fr], "frames")
    xa, na = oa.occupied_voxels(0)
    xb, nb = ob.occupied_voxels(0)
    assert na > 1000 and nb > 1000 and not ({r.tobytes() for r in xa} & {r.tobytes() for r in xb})
    a.cvt_occupy_to_voxels(0)
    assert a.num_export_particles[None] == na
    rows = a.export_x.to_numpy(a.num_export_particles[None])
    assert rows.shape == (100, 3) and _rows_in(rows, xa)
    pc = a.pointcloud2()
    assert pc["width"] == 100 and pc["point_step"] == 12 and pc["data"] == rows.tobytes()
    b.cvt_occupy_voxels_to(0, a.num_export_particles, a.max_disp_particles, a.export_x, a.export_color)
    assert a.num_export_particles[None] == na + nb                                  # the counter continues; nothing is written beyond the buffer
    assert np.array_equal(a.export_x.to_numpy(100), rows)
    # a buffer that ends inside the second map's voxels
    c, oc = _pair(cfg, max_disp_particles=na + 50)
    c.set_dep_camera_intrinsic(Kd)
    run_gpu(c, [("depth", *f, None, False) for f in frames], read=())
    c.cvt_occupy_to_voxels(0)
    b.cvt_occupy_voxels_to(0, c.num_export_particles, c.max_disp_particles, c.export_x, c.export_color)
    assert c.num_export_particles[None] == na + nb
    rows = c.export_x.to_numpy(na + nb)
    assert rows.shape == (na + 50, 3) and np.array_equal(sorted_rows(rows[:na]), sorted_rows(xa)) and _rows_in(rows[na:], xb)

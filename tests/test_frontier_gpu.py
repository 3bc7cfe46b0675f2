"""Frontier extraction on the GPU (tsl_frontier.hip): voxels, masks, cluster rows and cluster records equal the numpy restatement
(tests/frontier_ref.py) over the oracle's export exactly -- on the hand-built scenes of tests/frontier_scenes.py, on three geometries, and on the
room maps -- plus ordering behind queued frames, the device form, repeatability, an empty map and the refusals."""
import ctypes as C

import numpy as np
import pytest

import frontier_ref as ref
import frontier_scenes as fs
import render_view_scenes as rv
from taichislam_amd import _lib
from util import SLAB, SMALL, make_pair, small_stream

pytestmark = pytest.mark.gpu

VS = SMALL["voxel_scale"]
_MAPS = {}


def _map(geo, hip_lib):
    """one GPU map per geometry for the whole module, reset before every use"""
    from taichislam_amd.mapping import DenseTSDF
    if geo not in _MAPS:
        _MAPS[geo] = DenseTSDF(**fs.GEOMETRIES[geo]["cfg"])
    g = _MAPS[geo]
    g.reset()
    g.active_submap_id[None] = 0
    return g


def _oracle(geo):
    from oracle import OracleTSDF
    return OracleTSDF(**fs.GEOMETRIES[geo]["cfg"])


def _loaded(geo, sc, hip_lib, sid=0):
    g, o = _map(geo, hip_lib), _oracle(geo)
    fs.load_pair(g, o, fs.place(sc, geo), sid)
    return g, o


def _compare(g, o, what, **kw):
    """extract_frontiers against the restatement over the oracle's export; the keywords are those of extract_frontiers (z_range in voxel layers)"""
    kr = kw.pop("k_range", None)
    want = ref.extract(o.export_sparse(), o.N, o.Nz, VS, k_range=kr, **kw)
    if kr is not None:
        kw["z_range"] = (kr[0] * VS - 0.25 * VS, kr[1] * VS + 0.25 * VS)
    got = g.extract_frontiers(**kw)
    ref.assert_equal(got, want, what)
    assert np.array_equal(got["xyz"], got["indices"].astype(np.float32) * np.float32(VS))
    return got, want


SCENE_NAMES = sorted(fs.SCENES) + ["wall"]


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scenes_equal_the_restatement(hip_lib, geo, name):
    sc = fs.wall(geo) if name == "wall" else fs.SCENES[name]()
    g, o = _loaded(geo, sc, hip_lib)
    for conn in (26, 6):
        for clear in (False, True):
            got, _ = _compare(g, o, f"{name} on {geo}, connectivity {conn}, clear {clear}", connectivity=conn, clear_of_occupied=clear)
            if not clear:
                assert got["indices"].shape[0] > 0
    if name == "shell" and geo == "SMALL":
        assert got["indices"].shape[0] == fs.SHELL_VOXELS and got["clusters"].shape[0] == 1
    if name in ("tube", "spiral"):
        assert got["clusters"].shape[0] == 1                      # also under 6-connectivity: chained unions and the convergence in LDS


def test_options_equal_the_restatement(hip_lib):
    g, o = _loaded("SMALL", fs.shell(), hip_lib)
    for mu, n in ((2, fs.SHELL_EDGES_CORNERS), (3, fs.SHELL_CORNERS), (6, 0)):
        got, _ = _compare(g, o, f"min_unknown {mu}", min_unknown=mu)
        assert got["indices"].shape[0] == n
    got, _ = _compare(g, o, "z_range", k_range=(0, 3))
    assert got["indices"][:, 2].min() == 0 and got["indices"][:, 2].max() == 3
    _compare(g, o, "z_range of one layer", k_range=(-10, -10), connectivity=18)
    g, o = _loaded("SMALL", fs.diagonal(), hip_lib)
    for conn, n in fs.DIAGONAL_CLUSTERS.items():
        got, _ = _compare(g, o, f"diagonal, connectivity {conn}", connectivity=conn)
        assert got["clusters"].shape[0] == n
        got, _ = _compare(g, o, f"diagonal, connectivity {conn}, min_cluster 9", connectivity=conn, min_cluster=9)
        assert got["clusters"].shape[0] == (n if conn == 26 else 1 if conn == 18 else 0)
    g, o = _loaded("SMALL", fs.two_values(), hip_lib)
    a, _ = _compare(g, o, "default threshold")
    b, _ = _compare(g, o, "free_thres 0.2", free_thres=0.2)
    assert b["indices"].shape[0] < a["indices"].shape[0] and b["indices"][:, 2].min() == 0
    g, o = _loaded("SMALL", fs.plate(), hip_lib)
    a, _ = _compare(g, o, "plate")
    b, _ = _compare(g, o, "plate, clear_of_occupied", clear_of_occupied=True)
    assert b["indices"].shape[0] < a["indices"].shape[0]


def test_more_frontier_bricks_than_the_first_allocation_holds(hip_lib):
    """343 lone voxels, one per brick: the per-brick arrays start at 256 bricks and must grow; then a small scene on the grown arrays"""
    r = np.arange(-3, 4) * 16 + 8
    lone = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    g, o = _loaded("SMALL", fs.scene([(lone, fs.FREE_T)]), hip_lib)
    got, _ = _compare(g, o, "scatter")
    assert got["indices"].shape[0] == 343 and got["clusters"].shape[0] == 343 and (got["mask"] == 63).all()
    centroid, normal = got["centroid"], got["normal"]
    assert np.allclose(centroid, got["indices"].astype(np.float64) * VS) and not normal.any()
    g, o = _loaded("SMALL", fs.diagonal(), hip_lib)
    _compare(g, o, "diagonal after the scatter")


def test_submap_slot_one_with_other_content_in_slot_zero(hip_lib):
    g, o = _map("SMALL", hip_lib), _oracle("SMALL")
    fs.load_pair(g, o, fs.place(fs.diagonal(), "SMALL"), 0)
    fs.load_pair(g, o, fs.place(fs.shell(), "SMALL"), 1)
    g.active_submap_id[None] = 1
    o.set_active_submap(1)
    got, _ = _compare(g, o, "slot 1")
    assert got["indices"].shape[0] == fs.SHELL_VOXELS and got["clusters"].shape[0] == 1
    g.active_submap_id[None] = 0
    o.set_active_submap(0)
    got, _ = _compare(g, o, "slot 0")
    assert got["indices"].shape[0] == 32


_ROOMS = {}


def _room(geo):
    """(GPU map, oracle) of the room scene: four 320 x 240 frames, built once per geometry"""
    from oracle import BATCHED
    if geo not in _ROOMS:
        K, frames = rv.room_scene()
        g, o = make_pair({"SMALL": SMALL, "SLAB": SLAB}[geo], K)
        for R, T, d in frames:
            g.recast_depth_to_map(R, T, d, None)
            o.integrate_depth(R, T, d, mode=BATCHED)
        _ROOMS[geo] = (g, o)
    return _ROOMS[geo]


@pytest.mark.parametrize("geo", ["SMALL", "SLAB"])
@pytest.mark.parametrize("conn", [26, 6])
@pytest.mark.parametrize("clear", [False, True])
def test_room_equals_the_restatement(hip_lib, geo, conn, clear):
    g, o = _room(geo)
    got, want = _compare(g, o, f"room on {geo}, connectivity {conn}, clear {clear}", connectivity=conn, clear_of_occupied=clear)
    nv, nc, nb = ref.room_quantities(got, o.N, o.Nz)
    print(f"room on {geo}, connectivity {conn}, clear {clear}: {nv} frontier voxels, {nc} clusters, largest in {nb} bricks")
    if conn == 26 and not clear:
        assert nv >= 1000 and nc >= 10 and nb >= 8
        c, n = got["centroid"], got["normal"]
        assert c.shape == (nc, 3) and np.allclose(c, got["clusters"]["sum"] / got["clusters"]["count"][:, None] * VS)
        ln = np.linalg.norm(n, axis=1)
        assert (np.isclose(ln, 1.0) | (ln == 0.0)).all()


def test_extraction_runs_behind_the_queued_frames(hip_lib):
    """extract_frontiers straight after recast_depth_to_map of a fifth frame, nothing waited for: the result is the one of five frames, not of four"""
    from oracle import BATCHED
    K, frames = small_stream(5, h=240, w=320)
    g, o = make_pair(SMALL, K)
    for R, T, d in frames[:4]:
        g.recast_depth_to_map(R, T, d, None)
        o.integrate_depth(R, T, d, mode=BATCHED)
    four = g.extract_frontiers()
    ref.assert_equal(four, ref.extract(o.export_sparse(), o.N, o.Nz, VS), "four frames")
    R, T, d = frames[4]
    g.recast_depth_to_map(R, T, d, None)
    five = g.extract_frontiers()
    o.integrate_depth(R, T, d, mode=BATCHED)
    ref.assert_equal(five, ref.extract(o.export_sparse(), o.N, o.Nz, VS), "five frames")
    assert five["indices"].shape != four["indices"].shape or not np.array_equal(five["indices"], four["indices"])


def test_device_form_equals_the_host_form(hip_lib):
    import torch
    g, o = _room("SMALL")
    host = g.extract_frontiers()
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            dev = g.extract_frontiers(device=True)
            got = {k: dev[k].clone() for k in ("indices", "xyz", "mask", "cluster", "clusters_dev")}
        torch.cuda.synchronize()
        assert all(v.is_cuda for v in got.values())
        for k in ("indices", "xyz", "mask", "cluster"):
            assert np.array_equal(got[k].cpu().numpy(), host[k]), k
        assert np.array_equal(got["clusters_dev"].cpu().numpy().view(np.uint8).reshape(-1), host["clusters"].view(np.uint8).reshape(-1))
        assert np.array_equal(dev["clusters"].view(np.uint8), host["clusters"].view(np.uint8))
        assert np.array_equal(dev["centroid"], host["centroid"]) and np.array_equal(dev["normal"], host["normal"])


def test_second_call_returns_the_same_bytes_and_a_reset_map_nothing(hip_lib):
    g, o = _loaded("SMALL", fs.tube(), hip_lib)
    a, b = g.extract_frontiers(), g.extract_frontiers()
    for k in ("indices", "xyz", "mask", "cluster", "clusters"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["indices"].shape[0] > 0
    g.reset()
    e = g.extract_frontiers()
    assert e["indices"].shape == (0, 3) and e["mask"].shape == (0,) and e["cluster"].shape == (0,) and e["clusters"].shape == (0,)
    assert e["centroid"].shape == (0, 3) and e["normal"].shape == (0, 3)
    import torch
    d = g.extract_frontiers(device=True)
    assert d["indices"].shape == (0, 3) and d["indices"].is_cuda and d["clusters"].shape == (0,)
    torch.cuda.synchronize()


def test_refusals_leave_the_handle_usable(hip_lib):
    g, o = _loaded("SMALL", fs.diagonal(), hip_lib)
    L = hip_lib
    nv, nc = C.c_int32(), C.c_int32()

    def cfg(**kw):
        c = _lib.FrontierCfg(0.0, 1, 0, 1, 26, 1, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    bad = [("connectivity", dict(connectivity=7)), ("connectivity", dict(connectivity=-6)), ("min_unknown", dict(min_unknown=7)), ("min_unknown", dict(min_unknown=-1)),
           ("min_cluster", dict(min_cluster=-1)), ("free_thres", dict(free_thres=float("nan")))]
    for word, kw in bad:
        assert L.tsl_tsdf_frontier_extract(g.h, C.byref(cfg(**kw)), C.byref(nv), C.byref(nc)) == -1, kw
        msg = L.tsl_last_error().decode()
        assert "frontier_extract" in msg and word in msg, msg
        p = [C.c_void_p() for _ in range(4)]
        assert L.tsl_tsdf_frontier_dev(g.h, C.byref(cfg(**kw)), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3]), C.byref(nv), C.byref(nc), None) == -1
        assert "frontier_dev" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_frontier_extract(g.h, None, C.byref(nv), C.byref(nc)) == -1 and "null cfg" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_frontier_extract(None, C.byref(cfg()), C.byref(nv), C.byref(nc)) == -1 and "null handle" in L.tsl_last_error().decode()
    with pytest.raises(_lib.TslError, match="connectivity"):
        g.extract_frontiers(connectivity=8)
    with pytest.raises(ValueError):
        g.extract_frontiers(z_range=(0.01, 0.02))
    assert L.tsl_tsdf_frontier_extract(g.h, C.byref(cfg()), C.byref(nv), C.byref(nc)) == 0 and nv.value == 32 and nc.value == 2
    idx = np.zeros((32, 3), np.int16)
    assert L.tsl_tsdf_frontier_read(g.h, idx.ctypes.data_as(C.c_void_p), None, None, None, -1, 0) == -1 and "negative" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_frontier_read(g.h, idx.ctypes.data_as(C.c_void_p), None, None, None, 33, 0) == -1 and "more rows" in L.tsl_last_error().decode()
    assert L.tsl_tsdf_frontier_read(g.h, idx.ctypes.data_as(C.c_void_p), None, None, None, 32, 0) == 0 and idx.any()
    _compare(g, o, "after the refusals")                                    # the handle is still usable


def test_too_large_a_volume_is_refused(hip_lib):
    """N * N * Nz >= 2^31: 2048 x 2048 x 512 voxels (a sparse map: only the brick table is that large)"""
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(map_scale=[81.92, 20.48], voxel_scale=0.04, num_voxel_per_blk_axis=16, max_submap_num=1, max_bricks=64)
    assert (g.N, g.Nz) == (2048, 512)
    with pytest.raises(_lib.TslError, match="too large"):
        g.extract_frontiers()
    assert g.count_active() == 0

"""The indexed marching-cubes mesh on the GPU (tsl_mesh_indexed.hip): counts, vertices, normals, colours, edge records and triangles equal the numpy
restatement (tests/mesh_indexed_ref.py) over the oracle's export bit for bit and row for row, nothing sorted -- on the hand-built scenes of
tests/mesh_indexed_scenes.py on three geometries and on integrated streams -- plus the relation to the soup, load-order independence, capacities,
ordering behind queued frames, the device form, an empty map, the refusals, the soup path left as it was, and NaN map values under the soup's tile
kernel, which shares the indexed mesh's tile normal."""
import ctypes as C

import numpy as np
import pytest

import mesh_indexed_ref as ref
import mesh_indexed_scenes as ms
from frontier_scenes import GEOMETRIES
from taichislam_amd import _lib
from util import SLAB, SMALL, make_pair, small_stream, sorted_rows

pytestmark = pytest.mark.gpu

VS = SMALL["voxel_scale"]
CAP = 60000
POOL = dict(max_bricks=2048)          # every map here fits a small brick pool: the module keeps several alive, and the suite shares one device
_MAPS = {}
_STREAMS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_maps():
    """the maps this module keeps are freed when it is done, not at the end of the session"""
    yield
    import gc
    _MAPS.clear()
    _STREAMS.clear()
    gc.collect()


def _map(geo, hip_lib):
    """one GPU map per geometry for the whole module, reset before every use"""
    from taichislam_amd.mapping import DenseTSDF
    if geo not in _MAPS:
        _MAPS[geo] = DenseTSDF(**GEOMETRIES[geo]["cfg"], **POOL)
    g = _MAPS[geo]
    g.reset()
    g.active_submap_id[None] = 0
    return g


def _oracle(geo):
    from oracle import OracleTSDF
    return OracleTSDF(**GEOMETRIES[geo]["cfg"])


def _mesher(g, thres, cap=CAP):
    from taichislam_amd.mapping import MarchingCubeMesher
    return MarchingCubeMesher(g, max_triangles=cap, tsdf_surface_thres=thres)


def _indexed(g, thres, **kw):
    m = _mesher(g, thres)
    m.generate_indexed_mesh(**kw)
    return m, m.get_indexed_mesh()


def _want(o, thres, texture=False):
    return ref.extract(o.export_sparse(), o.N, o.Nz, VS, thres, texture=texture)


def _bytes(mesh):
    return [mesh[k].tobytes() for k in ("vertices", "normals", "edges", "triangles")] + [mesh["num_vertices"], mesh["num_triangles"]]


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
@pytest.mark.parametrize("name", ms.SCENE_NAMES)
def test_scenes_equal_the_restatement(hip_lib, geo, name):
    g, o = _map(geo, hip_lib), _oracle(geo)
    sc = ms.build(name, geo)
    ms.load_pair(g, o, sc)
    m, got = _indexed(g, sc["thres"])
    want = _want(o, sc["thres"])
    ref.assert_equal(got, want, f"{name} on {geo}")
    assert got["num_triangles"] > 0 and got["colors"] is None
    if name == "cases":
        assert got["num_triangles"] == ms.CASES_TRIANGLES
    if name == "ball":
        ref.manifold(got["triangles"], got["num_vertices"], f"ball on {geo}")


def _stream(geo):
    """(GPU map, oracle) after small_stream(3), built once per geometry"""
    from oracle import BATCHED
    if geo not in _STREAMS:
        K, frames = small_stream(3)
        g, o = make_pair({"SMALL": SMALL, "SLAB": SLAB}[geo], K, **POOL)
        for R, T, d in frames:
            g.recast_depth_to_map(R, T, d, None)
            o.integrate_depth(R, T, d, mode=BATCHED)
        _STREAMS[geo] = (g, o)
    return _STREAMS[geo]


@pytest.mark.parametrize("geo", ["SMALL", "SLAB"])
def test_streams_equal_the_restatement_and_relate_to_the_soup(hip_lib, geo):
    g, o = _stream(geo)
    thres = 5 * VS
    m, got = _indexed(g, thres)
    want = _want(o, thres)
    ref.assert_equal(got, want, f"stream on {geo}")
    assert got["num_triangles"] > (5000 if geo == "SMALL" else 100)
    m.generate_mesh(1)
    assert m.num_facelets[None] == got["num_triangles"]
    v, nr, _ = m.get_mesh()
    ref.soup_relation(v, dict(got, keys=want["keys"]), o.N, o.Nz, VS, f"GPU soup against GPU indexed mesh, {geo}")


def test_textured_map_colours_equal_the_restatement(hip_lib):
    from oracle import BATCHED
    from test_texture_gpu import TEX, _texture
    K, frames = small_stream(2)
    g, o = make_pair(TEX, K, **POOL)
    for f, (R, T, d) in enumerate(frames):
        tex = _texture(d.shape[0], d.shape[1], f)
        g.recast_depth_to_map(R, T, d, tex)
        o.integrate_depth(R, T, d, tex, mode=BATCHED)
    m, got = _indexed(g, 5 * VS)
    want = _want(o, 5 * VS, texture=True)
    ref.assert_equal(got, want, "textured")
    assert got["colors"].shape == got["vertices"].shape and (got["colors"] > 0).mean() > 0.5


def test_load_order_and_repetition_do_not_change_a_byte(hip_lib):
    parts = [ms.placed(p, "SMALL") for p in ms.ball_parts()]
    out = []
    for order in (range(8), reversed(range(8))):
        g = _map("SMALL", hip_lib)
        for n in order:
            p = parts[n]
            g.load_numpy(0, p["indices"], p["TSDF"], p["W_TSDF"], p["occupy"], None)
        m, a = _indexed(g, ms.BALL_THRES)
        m.generate_indexed_mesh()
        b = m.get_indexed_mesh()
        assert _bytes(a) == _bytes(b), "two consecutive calls differ"
        out.append(a)
    assert out[0]["num_triangles"] > 0 and _bytes(out[0]) == _bytes(out[1]), "the load order shows in the mesh"


def test_capacity_truncates_to_the_prefix_and_writes_nothing_behind_it(hip_lib):
    import torch
    from taichislam_amd.mapping.fields import device_view
    g, o = _map("SMALL", hip_lib), _oracle("SMALL")
    ms.load_pair(g, o, ms.build("ball", "SMALL"))
    m, full = _indexed(g, ms.BALL_THRES)
    nv, nt = full["num_vertices"], full["num_triangles"]
    p = m._indexed_dev()
    views = [device_view(p[0], (CAP, 3), "<f4", keep=m), device_view(p[1], (CAP, 3), "<f4", keep=m), device_view(p[3], (CAP, 4), "<i2", keep=m),
             device_view(p[4], (CAP, 3), "<i4", keep=m)]
    fills = [-7.25, -7.25, 0x5a5a, 0x5a5a5a5a]
    for v, f in zip(views, fills):
        v.fill_(f)
    torch.cuda.synchronize()
    mv, mt = nv // 3, nt // 3
    with pytest.raises(_lib.TslError, match="capacities"):
        m.generate_indexed_mesh(max_vertices=mv, max_triangles=mt)
    assert m.generate_indexed_mesh(max_vertices=mv, max_triangles=mt, allow_truncated=True) == (nv, nt)
    assert m._indexed_dev() == p, "a smaller capacity moved the buffers"
    part = m.get_indexed_mesh()
    assert (part["num_vertices"], part["num_triangles"]) == (nv, nt)
    assert part["vertices"].shape == (mv, 3) and part["triangles"].shape == (mt, 3)
    for k, rows in (("vertices", mv), ("normals", mv), ("edges", mv), ("triangles", mt)):
        assert ref._same(part[k], full[k][:rows]), k
    assert part["triangles"].max() >= mv                                     # a stored triangle names a vertex row that is not stored
    for v, f, rows in zip(views, fills, (mv, mv, mv, mt)):
        head, tail = v[:rows].cpu().numpy(), v[rows:].cpu().numpy()
        assert (tail == np.asarray(f, tail.dtype)).all(), "a row beyond the capacity was written"
        assert not (head == np.asarray(f, head.dtype)).all(1).any(), "a row below the capacity was not written"


def test_mesh_runs_behind_the_queued_frames(hip_lib):
    from oracle import BATCHED
    K, frames = small_stream(3)
    g, o = make_pair(SMALL, K, **POOL)
    for R, T, d in frames[:2]:
        g.recast_depth_to_map(R, T, d, None)
        o.integrate_depth(R, T, d, mode=BATCHED)
    two = _indexed(g, 5 * VS)[1]
    R, T, d = frames[2]
    g.recast_depth_to_map(R, T, d, None)
    m, three = _indexed(g, 5 * VS)                                           # nothing waited for
    g.sync()
    m.generate_indexed_mesh()
    after = m.get_indexed_mesh()
    o.integrate_depth(R, T, d, mode=BATCHED)
    ref.assert_equal(three, _want(o, 5 * VS), "three frames, no sync")
    assert _bytes(three) == _bytes(after) and _bytes(three) != _bytes(two)


def test_device_form_equals_the_host_form(hip_lib):
    import torch
    g, o = _stream("SMALL")
    m, host = _indexed(g, 5 * VS)
    dev = {"vertices": m.indexed_vertices.to_torch(), "normals": m.indexed_normals.to_torch(), "edges": m.indexed_edges.to_torch(),
           "triangles": m.indexed_triangles.to_torch()}
    torch.cuda.synchronize()
    for k, t in dev.items():
        assert t.is_cuda and tuple(t.shape) == host[k].shape, k
        assert ref._same(t.cpu().numpy(), host[k]), k
    assert dev["edges"].dtype == torch.int16 and dev["triangles"].dtype == torch.int32
    assert m.indexed_vertices.shape == host["vertices"].shape and m.indexed_triangles.to_numpy(5).shape == (5, 3)
    with pytest.raises(ValueError):
        m.indexed_colors.to_torch()                                          # an untextured map has no such buffer


def test_empty_map_gives_no_rows(hip_lib):
    import torch
    g = _map("SMALL", hip_lib)
    m = _mesher(g, 0.1)
    assert m.indexed_vertices.to_numpy().shape == (0, 3) and m.num_indexed_vertices[None] == 0          # before the first call
    assert m.generate_indexed_mesh() == (0, 0)
    e = m.get_indexed_mesh()
    assert e["vertices"].shape == (0, 3) and e["edges"].shape == (0, 4) and e["triangles"].shape == (0, 3) and e["num_vertices"] == 0
    t = m.indexed_triangles.to_torch()
    assert tuple(t.shape) == (0, 3) and t.is_cuda and t.dtype == torch.int32


def test_refusals_report_and_leave_the_handle_usable(hip_lib):
    L = hip_lib
    g, o = _map("SMALL", hip_lib), _oracle("SMALL")
    sc = ms.build("orphan", "SMALL")
    ms.load_pair(g, o, sc)
    nv, nt = C.c_int64(), C.c_int64()
    assert L.tsl_mesh_generate_indexed(None, 0.1, 10, 10, C.byref(nv), C.byref(nt)) == -1 and "null handle" in L.tsl_last_error().decode()
    assert L.tsl_mesh_read_indexed(None, None, None, None, None, None, 0, 0) == -1 and "null handle" in L.tsl_last_error().decode()
    assert L.tsl_mesh_indexed_dev(None, None, None, None, None, None, None, None) == -1 and "null handle" in L.tsl_last_error().decode()
    for mv, mt in ((0, 10), (10, 0), (-1, 10), (10, -5)):
        assert L.tsl_mesh_generate_indexed(g.h, 0.1, mv, mt, C.byref(nv), C.byref(nt)) == -1, (mv, mt)
        assert "must be positive" in L.tsl_last_error().decode()
    m = _mesher(g, sc["thres"])
    with pytest.raises(_lib.TslError, match="positive"):
        m.generate_indexed_mesh(max_vertices=0)
    a, b = m.generate_indexed_mesh()
    assert a > 0 and b > 0
    buf = np.zeros((a + 1, 3), np.float32)
    idx = np.zeros((b + 1, 3), np.int32)
    assert L.tsl_mesh_read_indexed(g.h, buf.ctypes.data_as(C.c_void_p), None, None, None, None, a + 1, 0) == -1 and "more rows" in L.tsl_last_error().decode()
    assert L.tsl_mesh_read_indexed(g.h, None, None, None, None, idx.ctypes.data_as(C.c_void_p), 0, b + 1) == -1 and "more rows" in L.tsl_last_error().decode()
    assert L.tsl_mesh_read_indexed(g.h, None, None, None, None, None, -1, 0) == -1 and "negative" in L.tsl_last_error().decode()
    assert L.tsl_mesh_read_indexed(g.h, buf.ctypes.data_as(C.c_void_p), None, None, None, idx.ctypes.data_as(C.c_void_p), a, b) == 0 and buf.any() and idx.any()
    with pytest.raises(_lib.TslError, match="step"):
        m.generate_indexed_mesh(step=2)
    ref.assert_equal(_indexed(g, sc["thres"])[1], _want(o, sc["thres"]), "after the refusals")


def test_soup_path_is_untouched_by_an_indexed_call(hip_lib):
    g, o = _stream("SMALL")
    m, got = _indexed(g, 5 * VS)
    m.generate_mesh(1)
    assert m.mesh_indices is None
    v, nr, col = m.get_mesh()
    ov, onr, _, on = o.generate_mesh(1, 5 * VS, CAP)
    assert m.num_facelets[None] == on and col is None
    assert np.array_equal(sorted_rows(np.concatenate([v.reshape(-1, 9), nr.reshape(-1, 9)], 1)), sorted_rows(np.concatenate([ov.reshape(-1, 9), onr.reshape(-1, 9)], 1)))
    m.generate_indexed_mesh()                                                # ... and the soup's device view still counts the soup's rows
    assert tuple(m.mesh_vertices.to_torch().shape) == (3 * on, 3)
    assert ref._same(m.mesh_vertices.to_torch().cpu().numpy(), v)


def _soup_rows(m):
    """the soup of the last generate_mesh as uint32 rows [positions 9 | normals 9], sorted: the order of the rows is the arrival order of the bricks"""
    v, nr, _ = m.get_mesh()
    rows = np.ascontiguousarray(np.concatenate([v.reshape(-1, 9), nr.reshape(-1, 9)], axis=1), np.float32).view(np.uint32)
    return rows[np.lexsort(rows.T[::-1])]


def test_nan_map_values_keep_the_soup_normal_inside_its_tile(hip_lib):
    """A NaN map value (load_numpy stores what it is given) makes a NaN vertex, whose nearest voxel is anything: the tile kernel clamps the voxel of
    the normal to its tile, as the indexed mesh does (tsl_mc.hpp, mc_tile_normal).  A flat surface between z = -1 and z = 0 across eight bricks, every
    voxel observed, NaN in the voxel at brick-local (0, 0, 0) above it and in the one at brick-local (15, 7, 15) below it.  The tile kernel gives
    the same rows twice (compared as sorted rows of bits: bricks reserve their rows by an atomic, so the order of the rows is not defined) and as
    many triangles as the indexed mesh; where a triangle's positions are finite it is the gather kernel's triangle, normals included."""
    idx = ms.box((-10, -10, -4), (9, 9, 3))
    val = ((idx[:, 2] + 0.5) * 0.04).astype(np.float16)
    for nan_voxel in ((0, 0, 0), (-1, 7, -1)):
        val[(idx == np.array(nan_voxel)).all(1)] = np.nan
    assert np.isnan(val).sum() == 2
    sc = ms.placed(ms.scene(idx, val, 1.0), "SMALL")
    g = _map("SMALL", hip_lib)
    g.load_numpy(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], None)
    m, got = _indexed(g, sc["thres"])
    tile = []
    for _ in range(2):
        m.generate_mesh(1)
        assert m.num_facelets[None] == got["num_triangles"] > 0
        tile.append(_soup_rows(m))
    assert tile[0].tobytes() == tile[1].tobytes(), "two meshes of one map by the tile kernel differ"
    g.set_option("mesh_gather", 1)
    try:
        m.generate_mesh(1)
        gather = _soup_rows(m)
    finally:
        g.set_option("mesh_gather", 0)
    a, b = (r[np.isfinite(r[:, :9].view(np.float32)).all(1)].view(np.float32) for r in (tile[0], gather))
    assert 0 < a.shape[0] < tile[0].shape[0], "the map has no NaN vertex, or nothing else"
    assert a.shape == b.shape and np.array_equal(a[:, :9], b[:, :9]), "the triangles with finite positions differ between the tile and the gather kernel"
    assert np.array_equal(np.isnan(a[:, 9:]), np.isnan(b[:, 9:])), "a normal is NaN in one kernel only"
    assert np.isnan(a[:, 9:]).any() and np.array_equal(np.nan_to_num(a[:, 9:]), np.nan_to_num(b[:, 9:])), "normals differ"

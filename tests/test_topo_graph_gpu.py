"""TopoGraphGen on the HIP back end (csrc/tsl_topo.hip, mapping/topo_graph.py) against the sequential restatement (tests/topo_graph_ref.py) on the hand-built
cases and scenes of tests/topo_graph_scenes.py: every output bit for bit, there is no tolerance in this file.  tests/test_topo_graph_cpu.py shows with the
restatement alone that each case has the property it is here for."""
import ctypes as C
import gc

import numpy as np
import pytest

import topo_graph_scenes as ts
from taichislam_amd import _lib
from taichislam_amd.mapping import DenseTSDF, TopoGraphGen
from topo_graph_ref import F32, RefTopo, bits, uniform_sample_points

pytestmark = pytest.mark.gpu

POOL = dict(max_submap_num=2, max_bricks=1024)          # the scenes use a few hundred bricks
_KEEP = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _KEEP.clear()
    gc.collect()


def _pair(cfg, sc):
    from oracle import OracleTSDF
    g, o = DenseTSDF(**cfg, **POOL), OracleTSDF(**cfg)
    g.load_numpy(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], None)
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    return g, o


def hand(hip_lib):
    """(map, oracle, graph with max_raycast_dist 1.0) on hand_map(), once per module"""
    if "hand" not in _KEEP:
        g, o = _pair(ts.HAND_CFG, ts.hand_map())
        _KEEP["hand"] = (g, o, TopoGraphGen(g, coll_det_num=32, max_raycast_dist=1.0))
    return _KEEP["hand"]


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    if a.dtype == np.float32 or b.dtype == np.float32:
        a, b = bits(a), bits(b)
    bad = np.argwhere(np.atleast_1d(a != b))
    assert bad.size == 0, f"{what}: {bad.shape[0]} differ, first at {bad[0]}: {a[tuple(bad[0])] if a.ndim else a} != {b[tuple(bad[0])] if b.ndim else b}"


def same_rays(got, want, what):
    for name, a, b in zip(("hit", "type", "position", "length", "poly"), got, want):
        same(a, b, f"{what}: {name}")


def test_empty_store_equals_query_raycast(hip_lib):
    g, o, t = hand(hip_lib)
    t.reset()
    rng = np.random.default_rng(7)
    pos = rng.uniform(-1.2, 1.2, (257, 3)).astype(F32)
    pos[:, 0] = rng.uniform(-2.2, 5.2, 257)
    d = rng.normal(size=(257, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    for max_dist in (1.5, 4.0, 0.03):
        hit, typ, end, ln, poly = t.rays(pos, d, max_dist)
        h0, e0, l0 = g.raycast(pos, d, max_dist)                        # tsl_tsdf_query_raycast: existing code is the yardstick
        same(hit, h0, "hit"); same(end, e0, "end"); same(ln, l0, "len")
        assert (typ == 0).all() and (poly == -1).all()
        assert max_dist < 0.05 or (hit.any() and not hit.all())


@pytest.mark.parametrize("name", list(ts.hand_cases()))
def test_hand_case(hip_lib, name):
    g, o, t = hand(hip_lib)
    t.reset()
    case = ts.hand_cases()[name]
    r = RefTopo(o, coll_det_num=32, max_raycast_dist=1.0)
    for k, (tris, start) in enumerate(case["polys"]):
        node, centre, fr, why, nb = t.add_poly(tris, start)
        rnode, rcentre, rfr, rwhy, rnb = r.add_poly(tris, start)
        assert node == rnode == k
        same(centre, rcentre, "node centre"); same(fr, rfr, "is_frontier"); same(why, rwhy, "reason"); same(nb, rnb, "neighbour poly")
    if case["polys"]:
        got, want = t.read_facelets(), r.facelets()
        for a, b in (("tri_vertices", "tri"), ("v0", "v0"), ("edge1", "edge1"), ("edge2", "edge2"), ("normal", "normal"), ("center", "center"), ("poly_idx", "poly")):
            same(got[a], want[b], f"facelet {a}")
        same(t.tri_vertices.to_numpy(), want["tri"].reshape(-1, 3), "tri_vertices")
    for i, q in enumerate(case["rays"]):
        got = t.rays(q["pos"], q["dir"], q["max_dist"], q["skip"], q["backward"], q["facelets_only"])
        want = r.rays(q["pos"], q["dir"], q["max_dist"], q["skip"], q["backward"], q["facelets_only"])
        same_rays(got, want, f"{name} ray set {i}")


def test_device_form_and_views(hip_lib):
    import torch
    g, o, t = hand(hip_lib)
    t.reset()
    case = ts.hand_cases()["count65"]
    for tris, start in case["polys"]:
        t.add_poly(tris, start)
    dev = torch.device(f"cuda:{g.device}")
    for q in case["rays"]:
        want = t.rays(q["pos"], q["dir"], q["max_dist"], q["skip"], q["backward"], q["facelets_only"])
        got = t.rays_dev(torch.from_numpy(q["pos"]).to(dev), torch.from_numpy(q["dir"]).to(dev), q["max_dist"], None, q["backward"], q["facelets_only"])
        same_rays([x.cpu().numpy() for x in got], want, "rays_dev")
    same(t.tri_vertices.to_torch().cpu().numpy(), t.tri_vertices.to_numpy(), "tri_vertices.to_torch")
    assert t.tri_vertices.to_numpy().shape == (390, 3)


def test_collide_compacts_in_ray_order(hip_lib):
    g, o, t = hand(hip_lib)
    t.reset()
    r = RefTopo(o, coll_det_num=32, max_raycast_dist=1.0)
    same(t.sample_dirs, r.dirs, "sample directions"); same(t.sample_dirs, uniform_sample_points(32), "sample directions")
    for tris, start in ts.hand_cases()["count64"]["polys"]:
        t.add_poly(tris, start); r.add_poly(tris, start)
    for start in ((0.0, 0.1, 0.0), (0.4, 0.3, 0.1), (2.0, 0.0, 0.0), (0.55, -0.75, 0.0)):
        got, want = t.detect_collisions(start), r.collide(start)
        assert got[0] == want[0] and got[4] == want[4], start
        for k, what in ((1, "black positions"), (2, "black directions"), (3, "black lengths")):
            same(got[k], want[k], f"{what} at {start}")
        same(np.array([got[5]], F32), np.array([want[5]], F32), "node_size")
    assert not t.detect_collisions((2.0, 0.0, 0.0))[0] and np.isnan(t.detect_collisions((2.0, 0.0, 0.0))[5])          # nothing within 1 m: no black ray, 0 / 0


def _compare_graph(t, r, what):
    assert len(t.nodes()["master_idx"]) == len(r.node_fl), what
    for k, v in r.nodes().items():
        same(t.nodes()[k], v, f"{what}: node {k}")
    got, want = t.read_facelets(), r.facelets()
    for a, b in (("tri_vertices", "tri"), ("v0", "v0"), ("edge1", "edge1"), ("edge2", "edge2"), ("normal", "normal"), ("center", "center"), ("poly_idx", "poly")):
        same(got[a], want[b], f"{what}: facelet {a}")
    same(np.concatenate(t._frontier_flags), want["is_frontier"], f"{what}: is_frontier")
    assert t.num_frontiers[None] == len(r.frontier) and t.search_frontiers_idx[None] == r.search_idx, what
    for k, v in r.frontiers().items():
        same(t.frontiers()[k], v, f"{what}: frontier {k}")
    same(t.edges.to_numpy(), np.array(r.edges, F32).reshape(-1, 3), f"{what}: edges")
    same(t.edge_index(), np.array(r.edge_idx, np.int32).reshape(-1, 2), f"{what}: edge_index")
    assert t.edge_num[None] == 2 * len(r.edge_idx) and t.num_nodes[None] == len(r.node_fl) and t.num_facelets[None] == r.nfacelets
    assert t.stats == r.count, what


@pytest.mark.parametrize("cdn", [32, 64])
def test_whole_graph(hip_lib, cdn):
    sc = ts.graph_scene()
    if "graph" not in _KEEP:
        _KEEP["graph"] = _pair(ts.GRAPH_CFG, sc) + (DenseTSDF(**ts.GRAPH_CFG, **POOL),)
        s2 = ts.reordered(sc)
        _KEEP["graph"][2].load_numpy(0, s2["indices"], s2["TSDF"], s2["W_TSDF"], s2["occupy"], None)
    g, o, g2 = _KEEP["graph"]
    r = RefTopo(o, coll_det_num=cdn, **ts.GRAPH_PARAMS)
    r.generate_topo_graph(ts.GRAPH_START, ts.GRAPH_MAX_FRONTIERS)
    t = TopoGraphGen(g, coll_det_num=cdn, **ts.GRAPH_PARAMS)
    assert t.generate_topo_graph(ts.GRAPH_START, max_nodes=ts.GRAPH_MAX_FRONTIERS) == len(r.node_fl) >= 3
    _compare_graph(t, r, "first run")
    col = t.tri_colors.to_numpy()
    assert col.shape == (3 * r.nfacelets, 4) and col.dtype == np.float32
    fr = np.repeat(r.facelets()["is_frontier"], 3)
    assert (col[fr, 3] == F32(0.6)).all() and (col[~fr, 3] == F32(0.7)).all() and fr.any() and not fr.all()
    t.reset()
    assert t.num_nodes[None] == 0 and t.num_facelets[None] == 0 and t.edge_num[None] == 0
    t.generate_topo_graph(ts.GRAPH_START, max_nodes=ts.GRAPH_MAX_FRONTIERS)
    _compare_graph(t, r, "after reset()")
    t2 = TopoGraphGen(g2, coll_det_num=cdn, **ts.GRAPH_PARAMS)
    t2.generate_topo_graph(ts.GRAPH_START, max_nodes=ts.GRAPH_MAX_FRONTIERS)
    _compare_graph(t2, r, "another brick order")


def test_refusals_leave_nothing_changed(hip_lib):
    g, o, t = hand(hip_lib)
    L = hip_lib
    for cdn in (3, 513, 0, -1):
        with pytest.raises(_lib.TslError, match="coll_det_num"):
            TopoGraphGen(g, coll_det_num=cdn)
    t.reset()
    sq = ts.square(0.5)
    t.add_poly(sq, ts.ORIGIN)
    pos, d = np.array([[0.0, 0.1, 0.0]], F32), np.array([[1.0, 0.0, 0.0]], F32)
    before = t.rays(pos, d, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), -0.0001):
        hit, ln = np.full(1, 77, np.uint8), np.full(1, 77.0, F32)
        rc = L.tsl_topo_rays(t.h, pos.ctypes.data, d.ctypes.data, None, 1, bad, -0.01, 0, hit.ctypes.data, None, None, ln.ctypes.data, None)
        assert rc == -1 and b"max_dist" in L.tsl_last_error() and hit[0] == 77 and ln[0] == 77.0
        fr = np.full(2, 77, np.uint8)
        assert L.tsl_topo_add_poly(t.h, sq.ctypes.data, 2, pos.ctypes.data, bad, fr.ctypes.data, None, None, None, None) == -1 and fr[0] == 77
    nf, nn = C.c_int64(), C.c_int32()
    L.tsl_topo_counts(t.h, C.byref(nf), C.byref(nn))
    assert (nf.value, nn.value) == (2, 1)
    same_rays(t.rays(pos, d, 1.0), before, "after the refusals")
    # a store at max_facelets
    small = TopoGraphGen(g, coll_det_num=32, max_raycast_dist=1.0, max_facelets=3)
    small.add_poly(sq, ts.ORIGIN)
    fr = np.full(2, 77, np.uint8)
    rc = L.tsl_topo_add_poly(small.h, sq.ctypes.data, 2, pos.ctypes.data, 0.5, fr.ctypes.data, None, None, None, None)
    assert rc == -3 and b"max_facelets" in L.tsl_last_error() and fr[0] == 77
    L.tsl_topo_counts(small.h, C.byref(nf), C.byref(nn))
    assert (nf.value, nn.value) == (2, 1)
    small.add_poly(sq[:1], ts.ORIGIN)                                    # one more still fits
    same_rays(small.rays(pos, d, 1.0), before, "the full store")
    # a destroyed map
    gone = DenseTSDF(**ts.HAND_CFG, **POOL)
    orphan = TopoGraphGen(gone, coll_det_num=32)
    gone.__del__()
    assert gone.h is None
    with pytest.raises(_lib.TslError, match="destroyed"):
        orphan.rays(pos, d, 1.0)
    with pytest.raises(_lib.TslError, match="destroyed"):
        orphan.add_poly(sq, ts.ORIGIN)
    with pytest.raises(_lib.TslError, match="destroyed"):
        orphan.reset()
    del orphan                                                           # tsl_topo_destroy of an orphan is fine
    gc.collect()

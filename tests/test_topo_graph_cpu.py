"""CPU side of the topology graph: the boundary declares and binds the entry points, and the sequential restatement (tests/topo_graph_ref.py)
-- the yardstick of tests/test_topo_graph_gpu.py -- gives the hand-worked answers on the hand-built cases and a graph that is not vacuous on the scene."""
import functools
import os
import re

import numpy as np
import pytest

import topo_graph_scenes as ts
from topo_graph_ref import F32, RefTopo, bits, ray_triangles, uniform_sample_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("tsl_topo_create", "tsl_topo_destroy", "tsl_topo_reset", "tsl_topo_rays", "tsl_topo_rays_dev", "tsl_topo_collide", "tsl_topo_add_poly",
                "tsl_topo_buffers_dev")
VS = F32(ts.HAND_VS)


def test_abi_declares_binds_and_exports_the_entry_points():
    from taichislam_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taichislam_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tsl_topo_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
        assert hasattr(L, name), f"{name} is not exported"
    import taichislam_amd.mapping as mapping
    assert hasattr(mapping, "TopoGraphGen")


def test_refusals_that_need_no_device():
    import ctypes as C
    from taichislam_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.tsl_topo_create(None, 64, 1.0, 1024, C.byref(h)) == -1 and not h.value and b"topo_create" in L.tsl_last_error()
    assert L.tsl_topo_rays(None, None, None, None, 0, 1.0, -0.01, 0, None, None, None, None, None) == -1 and b"topo_rays" in L.tsl_last_error()
    assert L.tsl_topo_reset(None) == -1
    L.tsl_topo_destroy(None)                                   # a no-op


@functools.lru_cache(maxsize=None)
def hand_oracle():
    from oracle import OracleTSDF
    o = OracleTSDF(**ts.HAND_CFG)
    sc = ts.hand_map()
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    return o


def run_case(name):
    """[(hit, type, position, length, poly)] of the case's ray sets, and the restatement that holds its store"""
    case = ts.hand_cases()[name]
    r = RefTopo(hand_oracle(), coll_det_num=32, max_raycast_dist=1.0)
    added = [r.add_poly(tris, start) for tris, start in case["polys"]]
    out = [r.rays(q["pos"], q["dir"], q["max_dist"], q["skip"], q["backward"], q["facelets_only"]) for q in case["rays"]]
    return out, r, added


def test_the_sample_directions_are_the_fibonacci_sphere():
    d = uniform_sample_points(32)
    assert d.dtype == np.float32 and d.shape == (32, 3)
    assert np.array_equal(d[0], np.array([0.0, 1.0, 0.0], F32)) and np.array_equal(d[31, 1], F32(-1.0))
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.allclose(d[1:, 1] - d[:-1, 1], -2.0 / 31, atol=1e-6)


def test_ray_against_one_triangle_by_hand():
    # the triangle (0.5, -1, -1), (0.5, 1, -1), (0.5, 1, 1), a ray from (0, 0.5, 0) along +x: q = w x e2 = (0, -2, 2), a = e1 . q = -4, s = (P - v0) / a =
    # (0.125, -0.375, -0.25), r = s x e1 = (0.5, 0, 0.25), b0 = s . q = 0.25, b1 = r . w = 0.5, b2 = 0.25, t = e2 . r = 0.5: every number exact in f32
    v0, e1, e2 = np.array([[0.5, -1, -1]], F32), np.array([[0, 2, 0]], F32), np.array([[0, 2, 2]], F32)
    ok, t = ray_triangles(v0, e1, e2, np.array([0, 0.5, 0], F32), np.array([1, 0, 0], F32))
    assert ok[0] and t[0] == F32(0.5)
    ok, t = ray_triangles(v0, e1, e2, np.array([0, -0.5, 0.5], F32), np.array([1, 0, 0], F32))          # outside: b1 = r . w < 0
    assert not ok[0]
    ok, t = ray_triangles(v0, e1, e2, np.array([0, np.nan, 0], F32), np.array([1, 0, 0], F32))          # NaN: succ stays set, t is NaN and loses every comparison
    assert np.isnan(t[0]) and not (F32(-0.01) < t[0]) and not (t[0] < F32(1.0))


def test_facelet_by_hand():
    # one triangle wound so that cross(e1, e2) points at the start: the normal is turned away from it
    tri = np.array([[[0.5, -1, -1], [0.5, 1, 1], [0.5, 1, -1]]], F32)
    r = RefTopo(hand_oracle(), coll_det_num=32, max_raycast_dist=1.0)
    node, centre, is_frontier, reason, neigh = r.add_poly(tri, (0, 0, 0))
    fl = r.facelets()
    assert node == 0 and np.array_equal(fl["normal"][0], np.array([1, 0, 0], F32)) and np.array_equal(fl["edge1"][0], np.array([0, 2, 2], F32))
    third = (F32(-1) + F32(1) + F32(1)) / F32(3)
    assert np.array_equal(bits(fl["center"][0]), bits(np.array([0.5, third, -third], F32)))
    assert np.array_equal(bits(centre), bits(fl["center"][0]))          # one facelet: the node centre is ((v0 + v1) + v2) / 3 as well
    assert is_frontier[0] and reason[0] == 0 and neigh[0] == -1          # observed free space, nothing within 0.5 m in front of it


def covered(n, y, z, y0, y1, z0=-1.0, z1=1.0):
    """whether (y, z) lies in strip(n, ., y0, y1): whole cells of two triangles, and the lower right half of the last cell when n is odd"""
    cells = (n + 1) // 2
    w = (y1 - y0) / cells
    c = np.clip(np.floor((y - y0) / w), 0, cells - 1).astype(int)
    inside = (y >= y0) & (y <= y1)
    half = (z - z0) <= (y - (y0 + c * w)) * (z1 - z0) / w
    return inside & ((2 * c + 1 < n) | half)


@pytest.mark.parametrize("n", ts.COUNTS)
def test_counts_by_hand(n):
    out, r, added = run_case(f"count{n}")
    assert r.nfacelets == 2 * n and len(r.node_fl) == 2
    y = ts.hand_cases()[f"count{n}"]["rays"][0]["pos"][:, 1].astype(np.float64)
    near, far = covered(n, y, 0.1, 0.0, 1.0), covered(n, y, 0.1, -1.0, 1.0)      # the nearer strip (node 1, x = 0.3) lies in front of y >= 0
    assert near.sum() >= (8 if n > 1 else 1) and (far & ~near).sum() >= (8 if n > 1 else 1)
    hit, typ, x, ln, poly = out[0]                                       # along +x
    assert np.array_equal(hit & (typ == 1), far | near) and np.array_equal(poly, np.where(near, 1, np.where(far, 0, -1)))
    assert np.allclose(ln[near], 0.3, atol=1e-6) and np.allclose(ln[far & ~near], 0.5, atol=1e-6) and np.allclose(x[far | near, 0], ln[far | near], atol=1e-6)
    hit, typ, x, ln, poly = out[3]                                       # max_dist 0.4: the far strip is out of range, the map is free for 8 steps
    assert np.array_equal(hit, near) and np.array_equal(bits(ln[~near]), bits(np.full((~near).sum(), F32(7) * VS, F32)))
    # the facelets of node 1 look at node 0, 0.2 m ahead: reason 3 through a type-1 hit, and the neighbour is node 0.  (Not all of them: the odd one at the end
    # of a strip may look past node 0, and a centre can fall on a diagonal of node 0's and slip between its two triangles.)  Node 0 looks into free space or,
    # in the rows where it is 0.1 m away, at the wall: reason 3 through the map, no neighbour.
    _, _, fr1, why1, nb1 = added[1]
    assert np.isin(why1, (0, 3)).all() and (why1 == 3).sum() >= max(1, n // 2) and np.array_equal(nb1, np.where(why1 == 3, 0, -1)) and np.array_equal(fr1, why1 == 0)
    _, _, fr0, why0, nb0 = added[0]
    assert np.isin(why0, (0, 3)).all() and (nb0 == -1).all() and np.array_equal(fr0, why0 == 0) and (n == 1 or ((why0 == 0).any() and (why0 == 3).any()))


def test_ties_windows_and_culling_by_hand():
    out, _, _ = run_case("tie")
    for hit, typ, x, ln, poly in out:
        # three rays through the shared edge: node 0's triangle wins; then one through node 1's triangle alone and one through node 0's alone
        assert hit.all() and (typ == 1).all() and poly.tolist() == [0, 0, 0, 1, 0] and np.array_equal(bits(ln), bits(np.full(5, 0.5, F32)))
    out, _, _ = run_case("parallel")
    assert out[0][0].tolist() == [False, False, True] and abs(out[0][3][2]) < 1e-3 and out[0][4].tolist() == [-1, -1, 0]
    assert np.array_equal(bits(out[0][3][:2]), bits(np.full(2, 1.0, F32)))          # no hit: t = max_dist
    out, _, _ = run_case("backward")
    assert out[0][0].tolist() == [True, True, False, False] and out[1][0].tolist() == [True, True, False, False] and out[2][0].tolist() == [True, True, False, False]
    assert (out[0][3][:2] < 0).all() and (out[0][1][:2] == 1).all()                 # a negative length leaves no step to the map: the facelet stands
    out, _, _ = run_case("skip")
    assert out[0][4].tolist() == [0, -1, 0] and out[1][0].tolist() == [True, False, True] and out[0][1].tolist() == [1, 0, 1] and out[0][0].tolist() == [True, False, True]
    y_in, y_out = ts.cull_ys()
    assert np.nextafter(y_in, F32(np.inf)) == y_out and abs(float(y_in) - 3.75 ** 0.5) < 1e-6
    out, _, _ = run_case("cull")
    assert out[0][0].tolist() == [True, False, True, False] and out[0][4].tolist() == [0, -1, 0, -1]
    assert out[1][4].tolist() == [0, -1, 0, -1] and (out[1][1] == 0).all() and (out[1][3] == 0).all()      # the origins are in unobserved space: the map wins at step 0


def test_map_against_facelets_by_hand():
    wall = F32(12) * VS
    for name, typ, ln in (("map_nearer", 0, wall), ("facelet_nearer", 1, None), ("equal_len", 1, wall), ("one_step_more", 0, wall), ("cut_short", 1, None)):
        (hit, t, x, l, poly), = run_case(name)[0]
        assert hit.all() and (t == typ).all() and (poly == 0).all(), name          # poly is the facelet hit's node even when the map wins
        if ln is not None:
            assert np.array_equal(bits(l), bits(np.full(3, ln, F32))), name
    assert np.allclose(run_case("facelet_nearer")[0][0][3], 0.4, atol=1e-6)
    # the patch at 0.62 m lies behind the step that finds the wall (0.6 m), and still wins: the walk is cut to int(0.62 / voxel) = 12 steps, 0 .. 11
    assert np.allclose(run_case("cut_short")[0][0][3], 0.62, atol=1e-6) and F32(0.62) > wall


def test_step_counts_by_hand():
    out, _, _ = run_case("steps")
    rows = ["wall12", "wall63", "wall64", "open"]
    want = {0.0: [None] * 4, 0.04: [None] * 4, 3.16: [(1, 12), (0, 62), (0, 62), (0, 62)], 3.21: [(1, 12), (1, 63), (0, 63), (0, 63)],
            3.26: [(1, 12), (1, 63), (1, 64), (0, 64)], 4.01: [(1, 12), (1, 63), (1, 64), (0, 79)]}
    for q, (hit, typ, x, ln, poly) in zip(ts.hand_cases()["steps"]["rays"], out):
        for i, row in enumerate(rows):
            w = want[q["max_dist"]][i]
            if w is None:                                       # no step: no hit, length 0, and the position is (0, 0, 0), not the origin
                assert not hit[i] and ln[i] == 0 and not x[i].any()
            else:
                assert bool(hit[i]) == bool(w[0]) and bits(ln[i:i + 1])[0] == bits(np.array([F32(w[1]) * VS]))[0], (q["max_dist"], row)
                assert np.array_equal(bits(x[i]), bits(np.array([F32(w[1]) * VS * F32(1.0) + F32(0.0), ts.HAND_Y[row], 0.0], F32)))
        assert (typ == 0).all() and (poly == -1).all()


def test_odd_origins_by_hand():
    for name in ("odd_empty", "odd_store"):
        hit, typ, x, ln, poly = run_case(name)[0][0]
        assert hit.all() and (typ == 0).all() and (ln == 0).all() and (poly == -1).all(), name      # outside / not finite reads as occupied: a hit at step 0
        assert bits(x[1])[0] == 0x7fc00000 and bits(x[2])[1] == 0x7fc00000 and np.array_equal(x[0], np.array([100, 0, 0], F32))
        assert bits(x[4]).tolist() == [0x7fc00000, bits(np.array([0.1], F32))[0], 0] and bits(x[5])[0] == 0x7fc00000      # NaN * 0 + 0 and inf * 0 + 0 on the x axis
    hit, typ, x, ln, poly = run_case("odd_store")[0][1]         # facelets only: a NaN t never wins, and a NaN distance is not inside the reach
    assert hit.tolist() == [False, False, False, False, False, False, False] and (poly == -1).all()


@functools.lru_cache(maxsize=None)
def graph(cdn, reorder=False):
    from oracle import OracleTSDF
    o = OracleTSDF(**ts.GRAPH_CFG)
    sc = ts.reordered(ts.graph_scene()) if reorder else ts.graph_scene()
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    r = RefTopo(o, coll_det_num=cdn, **ts.GRAPH_PARAMS)
    r.generate_topo_graph(ts.GRAPH_START, ts.GRAPH_MAX_FRONTIERS)
    return r


@pytest.mark.parametrize("cdn", [32, 64])
def test_the_scene_is_not_vacuous(cdn):
    r = graph(cdn)
    assert len(r.node_fl) >= 3
    assert r.count["frontiers_valid"] >= 1 and r.count["frontiers_invalid"] >= 1
    assert r.count["refused_by_collisions"] >= 1
    assert r.search_idx == ts.GRAPH_MAX_FRONTIERS and len(r.frontier) > ts.GRAPH_MAX_FRONTIERS          # max_nodes bounds the frontiers examined
    reasons = np.bincount(r.facelets()["reason"], minlength=4)
    assert (reasons > 0).all(), reasons                         # frontier facelets, and facelets that are none for each of the three reasons
    nd = r.nodes()
    assert nd["master_idx"][0] == -1 and (nd["master_idx"][1:] >= 0).all() and np.array_equal(nd["start_facelet_idx"][1:], nd["end_facelet_idx"][:-1])
    assert len(r.edge_idx) >= len(r.node_fl) - 1 and len(r.edges) == 2 * len(r.edge_idx)


def test_the_scene_has_a_neighbour_edge_through_a_type_1_hit():
    r = graph(32)
    nd = r.nodes()
    extra = [(a, b) for a, b in r.edge_idx if nd["master_idx"][b] != a]
    assert extra, "no edge beside the master edges"


def test_the_graph_repeats_after_reset_and_for_another_voxel_order():
    a, b = graph(32), graph(32, True)
    fa, fb = a.facelets(), b.facelets()
    assert all(np.array_equal(fa[k], fb[k]) for k in fa) and a.edge_idx == b.edge_idx
    a2 = RefTopo(a.o, coll_det_num=32, **ts.GRAPH_PARAMS)
    a2.generate_topo_graph(ts.GRAPH_START, ts.GRAPH_MAX_FRONTIERS)
    a2.reset()
    a2.generate_topo_graph(ts.GRAPH_START, ts.GRAPH_MAX_FRONTIERS)
    f2 = a2.facelets()
    assert all(np.array_equal(bits(fa[k]) if fa[k].dtype == np.float32 else fa[k], bits(f2[k]) if f2[k].dtype == np.float32 else f2[k]) for k in fa)

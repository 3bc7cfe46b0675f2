"""The pose-graph kernel (taichislam_amd/csrc/tsl_pose_graph.hip) against its numpy restatement (tests/pose_graph_ref.py), bit for bit: every output of
linearize and solve, through the host form and through the device form, on the smallest graphs at which the kernel takes another path."""
import functools

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_scenes as sc

pytestmark = pytest.mark.gpu

QUICK = dict(iters=2, pcg_max=40)           # the long chains: the restatement stays quick, every loop of the kernel still runs


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _star():
    """a hub (pose 0, free) with 70 edges in both directions; leaf 1 is fixed"""
    return sc.random_graph(71, [(i, 0) if i % 3 else (0, i) for i in range(1, 71)], seed=21, fixed=(1,))


def _mask65():
    """30 poses, 65 edges: the chain and 36 closures; edge 64 (a closure) is the only one disabled: the second mask word holds one bit, and it is 0"""
    G = sc.random_graph(30, sc.chain_edges(30, [((7 * k) % 30, (7 * k + 3 + k % 5) % 30) for k in range(36)]), seed=22)
    rows = np.ones((1, 65), bool)
    rows[0, 64] = False
    return dict(G, masks=ref.make_masks(rows))


def _b3():
    """a chain of 6 and one closure measured half a turn wrong (edge 6).  Variant 0 leaves it out: solvable.  Variant 1 also cuts the chain: status 4.
    Variant 2 has every edge: the wrong one is flipped at the start, status 5."""
    G = sc.random_graph(6, sc.chain_edges(6, [(5, 0), (4, 1)]), seed=23)
    G["Z"][6, :9] = (G["Z"][6, :9].reshape(3, 3) @ sc.rodrigues([0, 0, np.pi])).reshape(9)
    rows = np.ones((3, 7), bool)
    rows[0, 6] = False
    rows[1, [6, 2, 5]] = False
    return dict(G, masks=ref.make_masks(rows))


CASES = {
    "pair": lambda: (sc.random_graph(2, [(1, 0)], seed=20), {}),
    "triangle": lambda: (sc.random_graph(3, [(1, 0), (2, 1), (0, 2)], seed=24), {}),
    "star70": lambda: (_star(), dict(iters=4)),
    "chain257": lambda: (sc.loop(257, seed=25), QUICK),
    "chain1025": lambda: (sc.loop(1025, seed=26), QUICK),          # above 1024 poses p leaves LDS for the workspace
    "mask65": lambda: (_mask65(), dict(iters=6)),
    "double_edge": lambda: (sc.random_graph(3, [(1, 0), (1, 0), (2, 1), (0, 1)], seed=27), {}),
    "fixed_middle": lambda: (sc.random_graph(9, sc.chain_edges(9, [(8, 0)]), seed=28, fixed=(4,)), {}),
    "one_free": lambda: (sc.random_graph(6, [(3, 0), (1, 3), (3, 5), (2, 1), (4, 5)], seed=29, fixed=(0, 1, 2, 4, 5)), {}),
    "b3": lambda: (_b3(), {}),
    "huber": lambda: (sc.loop(40, seed=30, wrong=(2, 0.8)), dict(huber=3.0, iters=8)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, solver keywords, the restatement's variants, its linearisation under the first mask); computed once, shared, never written"""
    G, kw = CASES[name]()
    masks = G.get("masks")
    return G, kw, ref.solve(*sc.args(G), masks=masks, **kw), ref.linearize(*sc.args(G), mask=None if masks is None else masks[0], huber=kw.get("huber", 0.0))


@functools.lru_cache(maxsize=None)
def solver():
    from taichislam_amd.mapping import PoseGraph
    return PoseGraph(1100, 1200, 4)


def _check_solve(name, got, want, where):
    rep = got["report"]
    for v, w in enumerate(want):
        tag = f"{name} {where} variant {v}"
        assert int(rep["status"][v]) == w["status"] and int(rep["iterations"][v]) == w["iterations"], (tag, rep["status"][v], rep["iterations"][v], w["status"], w["iterations"])
        for k, wk in (("R", "R"), ("T", "T"), ("r", "r"), ("edge_cost", "edge_cost")):
            assert np.array_equal(_bits(got[k][v]), _bits(w[wk])), (tag, k, np.abs(np.asarray(got[k][v]) - w[wk]).max())
        assert _bits(rep["cost"][v]) == _bits(w["cost"]), (tag, "cost", rep["cost"][v], w["cost"])
        it = rep["it"][v]
        for n, q in enumerate(w["records"]):
            have = (it["cost_before"][n], it["cost_after"][n], it["max_step"][n], it["damping"][n])
            assert np.array_equal(_bits(have), _bits(q[:4])) and (int(it["pcg_iters"][n]), int(it["accepted"][n])) == (q[4], q[5]), (tag, "record", n, have, it["pcg_iters"][n], q)
        assert not np.ascontiguousarray(it[len(w["records"]):]).view(np.uint8).any(), (tag, "the records behind the last are not zero")


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_solve_equals_the_restatement(hip_lib, name):
    from taichislam_amd.mapping import PoseGraph
    from taichislam_amd.mapping.pose_graph import pack_information
    G, kw, want, _ = case(name)
    print(name, "statuses", [w["status"] for w in want], "iterations", [w["iterations"] for w in want], "pcg", [[q[4] for q in w["records"]] for w in want])
    pg = solver()
    got = pg.solve(*sc.args(G), masks=G.get("masks"), **kw)
    _check_solve(name, got, want, "host form")
    dev = pg.solve(_device(G["R"]), _device(G["T"]), G["fixed"], G["ij"], _device(G["Z"]), _device(pack_information(G["L"])), masks=G.get("masks"), **kw)
    host = {k: dev[k].cpu().numpy() for k in ("R", "T", "r", "edge_cost")}
    host["report"] = PoseGraph.decode(dev["report"])
    _check_solve(name, host, want, "device form")


@pytest.mark.parametrize("name", ["pair", "star70", "chain1025", "mask65", "double_edge", "one_free", "huber"])
def test_linearize_equals_the_restatement(hip_lib, name):
    from taichislam_amd.mapping.pose_graph import pack_information
    G, kw, _, want = case(name)
    pg, mask, huber = solver(), None if G.get("masks") is None else G["masks"][0], kw.get("huber", 0.0)
    got = pg.linearize(*sc.args(G), mask=mask, huber=huber)
    dev = pg.linearize(_device(G["R"]), _device(G["T"]), G["fixed"], G["ij"], _device(G["Z"]), _device(pack_information(G["L"])), mask=mask, huber=huber)
    for where, out in (("host form", got), ("device form", {k: v.cpu().numpy() for k, v in dev.items()})):
        for k in ("r", "cost", "Hd", "g"):
            assert np.array_equal(_bits(out[k]), _bits(want[k])), (name, where, k, np.abs(out[k] - want[k]).max())
        assert np.array_equal(out["flipped"], want["flipped"]), (name, where)
    assert not got["Hd"][G["fixed"] != 0].any() and not got["g"][G["fixed"] != 0].any()


def test_statuses_beside_each_other(hip_lib):
    G, _, want, _ = case("b3")
    assert [w["status"] for w in want] == [0, 4, 5]
    got = solver().solve(*sc.args(G), masks=G["masks"])
    assert list(got["report"]["status"]) == [0, 4, 5]
    for v in (1, 2):                                                 # not solved: the poses as given
        assert np.array_equal(_bits(got["R"][v]), _bits(G["R"])) and np.array_equal(_bits(got["T"][v]), _bits(G["T"]))


def test_the_same_call_twice_gives_the_same_bytes(hip_lib):
    G, kw, _, _ = case("huber")
    a, b = solver().solve(*sc.args(G), **kw), solver().solve(*sc.args(G), **kw)
    for k in a:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def test_leave_one_out_ranks_the_wrong_closure_last(hip_lib):
    """the condition tests/test_pose_graph_cpu.py checks on the restatement, on the GPU: 8 variants in one launch"""
    from taichislam_amd.mapping import PoseGraph
    from test_pose_graph_cpu import loo_scene
    G, edges, wrong = loo_scene()
    out = PoseGraph(64, 128, 8).leave_one_out(*sc.args(G), edges, huber=3.0)
    print("statuses", list(out["report"]["status"]), "leave-one-out", out["loo_cost"], "with every edge", out["full_cost"])
    assert np.argmax(out["loo_cost"]) == wrong and out["loo_cost"][wrong] > 10 * np.delete(out["loo_cost"], wrong).max()


def test_capacities(hip_lib):
    from taichislam_amd import _lib
    from taichislam_amd.mapping import PoseGraph
    for n, e, b in ((4096, 32768, 1), (1024, 8192, 256)):
        PoseGraph(n, e, b)
    for n, e, b in ((8193, 16, 1), (16, 131073, 1), (16, 16, 1025), (8192, 131072, 1024), (0, 1, 1)):
        with pytest.raises(_lib.TslError, match="tsl_pgo_create"):
            PoseGraph(n, e, b)


def test_bad_arguments_are_refused(hip_lib):
    import ctypes as C
    from taichislam_amd import _lib
    from taichislam_amd.mapping import PoseGraph
    G, _, _, _ = case("triangle")
    pg = PoseGraph(8, 8, 2)
    R, T, fixed, ij, Z, L = sc.args(G)

    def refused(who="tsl_pgo_solve", **change):
        a = dict(R=R, T=T, fixed=fixed, ij=ij, Z=Z, L=L)
        kw = {k: change.pop(k) for k in list(change) if k not in a}
        a.update(change)
        with pytest.raises(_lib.TslError, match=who):
            pg.solve(a["R"], a["T"], a["fixed"], a["ij"], a["Z"], a["L"], **kw)
    bad = ij.copy(); bad[1] = (2, 2)
    refused(ij=bad)
    bad = ij.copy(); bad[0, 0] = 3
    refused(ij=bad)
    bad = ij.copy(); bad[2, 1] = -1
    refused(ij=bad)
    for k, a in (("R", R), ("T", T), ("Z", Z), ("L", L)):
        for v in (np.nan, np.inf):
            bad = np.array(a, np.float64); bad.reshape(-1)[1] = v
            refused(**{k: bad})
    bad = L.copy(); bad[1, 6] = -1.0
    refused(L=bad)
    refused(fixed=np.zeros(3, np.uint8))
    for k in ("damping", "damping_up", "damping_down", "damping_min", "damping_max", "pcg_tol", "min_step", "rel_tol", "huber"):
        refused(**{k: -1.0})
        refused(**{k: np.nan})
    refused(iters=65); refused(iters=-1); refused(pcg_max=-1); refused(damping_down=0.0)
    refused(masks=np.full((3, 1), 7, np.uint64))                      # three variants, room for two
    big = sc.random_graph(9, sc.chain_edges(9), seed=1)
    with pytest.raises(_lib.TslError, match="tsl_pgo_solve"):
        pg.solve(*sc.args(big))
    with pytest.raises(_lib.TslError, match="tsl_pgo_linearize"):
        pg.linearize(*sc.args(big))
    with pytest.raises(_lib.TslError, match="tsl_pgo_linearize"):
        pg.linearize(R, T, fixed, ij, Z, L, huber=-1.0)
    # null pointers, straight at the library
    Lb, out, cfg = _lib.lib(), np.zeros(4096), _lib.PgoCfg(1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Lp = np.ascontiguousarray(L)
    assert Lb.tsl_pgo_solve(None, 3, p(R), p(T), p(fixed), 3, p(ij), p(Z), p(Lp), 1, None, C.byref(cfg), p(out), p(out), p(out), p(out), p(out)) == -1
    assert b"tsl_pgo_solve" in Lb.tsl_last_error()
    assert Lb.tsl_pgo_solve(pg.h, 3, None, p(T), p(fixed), 3, p(ij), p(Z), p(Lp), 1, None, C.byref(cfg), p(out), p(out), p(out), p(out), p(out)) == -1
    assert Lb.tsl_pgo_solve(pg.h, 3, p(R), p(T), p(fixed), 3, p(ij), p(Z), p(Lp), 1, None, None, p(out), p(out), p(out), p(out), p(out)) == -1
    assert Lb.tsl_pgo_solve(pg.h, 3, p(R), p(T), p(fixed), 3, p(ij), p(Z), p(Lp), 1, None, C.byref(cfg), p(out), None, p(out), p(out), p(out)) == -1
    assert Lb.tsl_pgo_solve_dev(pg.h, 3, p(R), p(T), None, 3, p(ij), p(Z), p(Lp), 1, None, C.byref(cfg), p(out), p(out), p(out), p(out), p(out), None) == -1
    assert b"tsl_pgo_solve_dev" in Lb.tsl_last_error()
    assert Lb.tsl_pgo_linearize_dev(pg.h, 3, p(R), p(T), None, 3, p(ij), p(Z), p(Lp), None, 0.0, None, p(out), p(out), p(out), p(out), None) == -1
    assert b"tsl_pgo_linearize_dev" in Lb.tsl_last_error()
    # and the graph still solves after all that
    _check_solve("triangle", pg.solve(R, T, fixed, ij, Z, L), case("triangle")[2], "after the refusals")

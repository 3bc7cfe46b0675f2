"""The numpy restatement of the pose graph (tests/pose_graph_ref.py) checked on its own, without a GPU: hand-worked residuals and adjoints, difference
quotients of the cost, an independent dense Gauss-Newton, a drifted loop, every status, and the leave-one-out ranking the GPU tests rely on."""
import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_scenes as sc

I3 = np.eye(3)
RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _two(Ra, Ta, Rb, Tb, Rz=I3, Tz=(0, 0, 0)):
    R, T = np.stack([Ra, Rb]).astype(np.float64), np.array([Ta, Tb], np.float64)
    Z = np.concatenate([np.asarray(Rz, np.float64).reshape(9), np.asarray(Tz, np.float64)])[None]
    return R, T, np.array([[0, 1]], np.int32), Z


def test_residual_of_a_pure_translation_by_hand():
    R, T, ij, Z = _two(I3, (1, 2, 3), I3, (0.5, 0, 0))
    r, den = ref.residual(R[[0]], T[[0]], R[[1]], T[[1]], Z)
    assert np.array_equal(r[0], [0.5, 2.0, 3.0, 0.0, 0.0, 0.0]) and den[0] == 4.0
    # A = Ad(P_b^-1) with P_b^-1 = (I, (-0.5, 0, 0)): A (v, w) = (v + t x w, w); t x e_z = (-0.5, 0, 0) x (0, 0, 1) = (0, 0.5, 0)
    ti = ref.tinv(R[[1]], T[[1]])
    assert np.array_equal(ti[0], [-0.5, 0.0, 0.0])
    assert np.array_equal(ref.adj(R[[1]], ti, np.array([[1.0, 0, 0, 0, 0, 1.0]]))[0], [1.0, 0.5, 0.0, 0.0, 0.0, 1.0])
    # A^T m = (m_v, m_w - t x m_v): m = (0, 1, 0, 0, 0, 0) -> t x m_v = (-0.5, 0, 0) x (0, 1, 0) = (0, 0, -0.5)
    assert np.array_equal(ref.adj_t(R[[1]], ti, np.array([[0, 1.0, 0, 0, 0, 0]]))[0], [0.0, 1.0, 0.0, 0.0, 0.0, 0.5])


def test_residual_of_a_quarter_turn_by_hand():
    # R_D = Rz(90 deg): den = 1 + tr = 2, vee(R_D - R_D^T) = (0, 0, 2), omega = 2 * 2 / 2 = 2 = 2 tan(45 deg): the Cayley twist of a quarter turn
    R, T, ij, Z = _two(RZ90, (0, 0, 0), I3, (0, 0, 0))
    r, den = ref.residual(R[[0]], T[[0]], R[[1]], T[[1]], Z)
    assert np.array_equal(r[0], [0, 0, 0, 0, 0, 2.0]) and den[0] == 2.0
    Rr, Tr = ref.retract(r, I3[None], np.zeros((1, 3)))
    assert np.array_equal(Rr[0], RZ90) and np.array_equal(Tr[0], [0, 0, 0])
    # b turned instead: A = Ad(P_b^-1) = (Rz90^T, 0): A (e_x, e_x) = (Rz90^T e_x) twice = (0, -1, 0)
    ti = ref.tinv(RZ90[None], np.zeros((1, 3)))
    assert np.array_equal(ref.adj(RZ90[None], ti, np.array([[1.0, 0, 0, 1.0, 0, 0]]))[0], [0, -1.0, 0, 0, -1.0, 0])


def test_flipped_above_120_degrees():
    for deg, want in ((119.0, False), (121.0, True)):
        R, T, ij, Z = _two(sc.rodrigues([0, 0, np.radians(deg)]), (0, 0, 0), I3, (0, 0, 0))
        assert bool(ref.linearize(R, T, None, ij, Z, sc.information(1))["flipped"][0]) is want


def test_zero_residual_at_consistent_poses_and_retraction_reproduces_the_error():
    G = sc.random_graph(12, sc.chain_edges(12, [(11, 0), (7, 2)]), seed=3)
    rng = np.random.default_rng(0)
    Z = sc.measure(G["R_true"], G["T_true"], G["ij"], rng)
    a, b = G["ij"][:, 0], G["ij"][:, 1]
    r, _ = ref.residual(G["R_true"][a], G["T_true"][a], G["R_true"][b], G["T_true"][b], Z)
    print("largest residual at consistent poses", np.abs(r).max())
    assert np.abs(r).max() < 1e-14                                    # a few roundings of numbers of size <= 10
    r, _ = ref.residual(G["R"][a], G["T"][a], G["R"][b], G["T"][b], G["Z"])
    Rr, Tr = ref.retract(r, np.tile(I3, (len(a), 1, 1)), np.zeros((len(a), 3)))
    for e in range(len(a)):                                           # D = (P_b^-1 P_a) Z^-1
        Rz, Tz = G["Z"][e, :9].reshape(3, 3), G["Z"][e, 9:]
        Rx, Tx = G["R"][b[e]].T @ G["R"][a[e]], G["R"][b[e]].T @ (G["T"][a[e]] - G["T"][b[e]])
        RD = Rx @ Rz.T
        assert np.abs(Rr[e] - RD).max() < 1e-14 and np.abs(Tr[e] - (Tx - RD @ Tz)).max() < 1e-14


def _cost_at(G, Z, xi):
    """half the plain cost with every pose retracted by its twist"""
    R, T = ref.retract(xi, G["R_true"], G["T_true"])
    return 0.5 * ref.linearize(R, T, None, G["ij"], Z, G["L"])["cost"].sum()


def test_blocks_against_difference_quotients():
    N = 6
    G = sc.random_graph(N, [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (5, 0), (3, 0), (3, 0)], seed=5)
    rng = np.random.default_rng(1)
    # Hd: at consistent poses the cost's Hessian IS sum A^T L A (r = 0: no second-order term, the Jacobian of the inverse retraction is the identity)
    Z = sc.measure(G["R_true"], G["T_true"], G["ij"], rng)
    Hd = ref.full(ref.linearize(G["R_true"], G["T_true"], None, G["ij"], Z, G["L"])["Hd"], 1.0)
    h, worst = 1e-4, 0.0
    for i in range(N):
        for k in range(6):
            for l in range(k, 6):
                def c(sk, sl):
                    xi = np.zeros((N, 6)); xi[i, k] += sk * h; xi[i, l] += sl * h
                    return _cost_at(G, Z, xi)
                fd = (c(1, 1) - c(1, -1) - c(-1, 1) + c(-1, -1)) / (4 * h * h) if k != l else (c(0.5, 0.5) - 2 * c(0, 0) + c(-0.5, -0.5)) / (h * h)
                worst = max(worst, abs(fd - Hd[i, k, l]))
    print("Hd against second differences: gap", worst, "of", np.abs(Hd).max(), "=", worst / np.abs(Hd).max())
    assert worst / np.abs(Hd).max() < sc.FD_HESSIAN_BOUND
    # g: residuals of about 1e-3
    Z = sc.measure(G["R_true"], G["T_true"], G["ij"], rng, 1e-3, 1e-3)
    g = ref.linearize(G["R_true"], G["T_true"], None, G["ij"], Z, G["L"])["g"]
    h, worst = 1e-6, 0.0
    for i in range(N):
        for k in range(6):
            xi = np.zeros((N, 6)); xi[i, k] = h
            worst = max(worst, abs((_cost_at(G, Z, xi) - _cost_at(G, Z, -xi)) / (2 * h) - g[i, k]))
    print("g against first differences: gap", worst, "of", np.abs(g).max(), "=", worst / np.abs(g).max())
    assert worst / np.abs(g).max() < sc.FD_GRADIENT_BOUND


def dense_gauss_newton(G, min_step=1e-9, iters=50):
    """an independent solver: plain Gauss-Newton on the assembled 6 N x 6 N matrix, numpy's own matrix products and np.linalg.solve"""
    R, T = G["R"].copy(), G["T"].copy()
    N, ij = len(R), G["ij"]
    free = np.flatnonzero(np.repeat(G["fixed"] == 0, 6))
    Lf = ref.full(G["L"], 1.0)

    def hat(t):
        return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    for _ in range(iters):
        H, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
        for e, (a, b) in enumerate(ij):
            Rz, Tz = G["Z"][e, :9].reshape(3, 3), G["Z"][e, 9:]
            RD = R[b].T @ R[a] @ Rz.T
            TD = R[b].T @ (T[a] - T[b]) - RD @ Tz
            S = RD - RD.T
            r = np.concatenate([TD, 2 * np.array([S[2, 1], S[0, 2], S[1, 0]]) / (1 + np.trace(RD))])
            Ri, ti = R[b].T, -R[b].T @ T[b]
            A = np.block([[Ri, hat(ti) @ Ri], [np.zeros((3, 3)), Ri]])
            J = np.zeros((6, 6 * N))
            J[:, 6 * a:6 * a + 6], J[:, 6 * b:6 * b + 6] = A, -A
            H += J.T @ Lf[e] @ J
            g += J.T @ Lf[e] @ r
        x = np.zeros(6 * N)
        x[free] = np.linalg.solve(H[np.ix_(free, free)], -g[free])
        x = x.reshape(N, 6)
        R, T = ref.retract(x, R, T)
        if np.sqrt((x * x).sum(axis=1).max()) < min_step:
            break
    return R, T


def test_converges_where_a_dense_gauss_newton_does():
    G = sc.random_graph(10, sc.chain_edges(10, [(9, 0), (6, 1), (8, 3)]), seed=11, fixed=(4,))
    out = ref.solve(*sc.args(G), iters=50, pcg_tol=1e-8, min_step=1e-9, rel_tol=0.0)[0]
    Rd, Td = dense_gauss_newton(G, min_step=1e-9)
    gap = max(np.abs(out["T"] - Td).max(), np.abs(out["R"] - Rd).max())
    print("status", out["status"], "iterations", out["iterations"], "gap to the dense Gauss-Newton", gap)
    assert out["status"] == 0 and gap < sc.DENSE_GN_BOUND


def test_drifted_loop_ends_closer_to_the_truth():
    G = sc.loop(40, seed=7)
    out = ref.solve(*sc.args(G))[0]
    before, after = sc.pose_error(G["R"], G["T"], G), sc.pose_error(out["R"], out["T"], G)
    first = out["records"][0][0]
    print("loop of 40: status", out["status"], "iterations", out["iterations"], "pcg", [q[4] for q in out["records"]], "cost", first, "->", out["cost"], "error", before, "->", after)
    assert out["status"] == 0 and out["cost"] < first and after[0] < before[0] and after[1] < before[1]
    assert np.array_equal(out["R"][0], G["R"][0]) and np.array_equal(out["T"][0], G["T"][0])      # the fixed pose stays


def test_every_status():
    G = sc.random_graph(8, sc.chain_edges(8, [(7, 0)]), seed=2)
    A = sc.args(G)
    assert ref.solve(*A)[0]["status"] == 0
    assert ref.solve(*A, iters=1, min_step=0.0, rel_tol=0.0)[0]["status"] == 1
    # 2: without a conjugate-gradient iteration the step is 0 and the trial costs what the poses cost: rejected until 1e-6 * 10^13 passes damping_max
    out = ref.solve(*A, iters=20, pcg_max=0)[0]
    assert out["status"] == 2 and out["iterations"] == 13 and not any(q[5] for q in out["records"])
    # 3: pose 7 has no information on any of its edges
    L = G["L"].copy(); L[[6, 7]] = 0.0
    assert ref.solve(G["R"], G["T"], G["fixed"], G["ij"], G["Z"], L)[0]["status"] == 3
    # 4: a chain cut in two by the mask; and a pose left without an edge
    H = sc.random_graph(8, sc.chain_edges(8), seed=2)
    rows = np.ones((3, 7), bool); rows[1, 3] = False; rows[2, 6] = False
    assert [o["status"] for o in ref.solve(*sc.args(H), masks=ref.make_masks(rows))] == [0, 4, 4]
    # 5: pose 3 starts half a turn away
    R = G["R"].copy(); R[3] = sc.rodrigues([0, 0, np.pi]) @ R[3]
    out = ref.solve(R, G["T"], G["fixed"], G["ij"], G["Z"], G["L"])[0]
    assert out["status"] == 5 and out["iterations"] == 0 and np.array_equal(out["R"], R)


def loo_scene():
    """a loop of 60 whose closure 2 is a quarter turn wrong: the graph, the indices of its closures, the wrong one"""
    G = sc.loop(60, seed=9, wrong=(2, np.pi / 2))
    return G, np.arange(G["n_odometry"], len(G["ij"])), 2


def loo_masks(G, edges):
    rows = np.ones((1 + len(edges), len(G["ij"])), bool)
    rows[1 + np.arange(len(edges)), edges] = False
    return rows


def test_a_wrong_closure_costs_more_left_out_than_every_sound_one():
    G, edges, wrong = loo_scene()
    outs = ref.solve(*sc.args(G), masks=ref.make_masks(loo_masks(G, edges)), huber=3.0)
    loo = np.array([outs[1 + k]["edge_cost"][e] for k, e in enumerate(edges)])
    print("statuses", [o["status"] for o in outs], "leave-one-out costs", loo)
    assert all(o["status"] in (0, 1) for o in outs)
    assert np.argmax(loo) == wrong and loo[wrong] > 10 * np.delete(loo, wrong).max()


def test_room_chain():
    """the three registrations of the room's submaps and their pose graph, restatements over the oracle's maps: the figures the GPU run is held to"""
    import pose_graph_room as room
    c = room.chain()
    print("room chain: registrations", [(k[0], k[1], k[5]) for k in c["constraints"]], "graph status", c["status"], "iterations", c["iterations"], "errors", c["errors"],
          "from", room.errors(room.start()))
    assert all(k[5] == 0 for k in c["constraints"]) and c["status"] == 0
    assert abs(c["errors"][0] - room.MEASURED_M) < 1e-6 and abs(c["errors"][1] - room.MEASURED_DEG) < 1e-6
    assert room.errors(room.start())[0] > 0.029                       # and the start was 3 cm off


def test_room_wrong_constraint_costs_most_left_out():
    """the condition tests/test_pose_graph_submaps_gpu.py relies on: with a fourth constraint 25 degrees wrong, the leave-one-out cost ranks it last"""
    import pose_graph_room as room
    c = room.chain()
    fa, fb, R, T = room.wrong_constraint()
    cons = list(c["constraints"]) + [(fa, fb, R, T, c["constraints"][1][4], 0)]
    A = room.graph(cons, room.start())
    rows = np.ones((5, 6), bool)
    rows[1 + np.arange(4), 2 + np.arange(4)] = False
    outs = ref.solve(*A, masks=ref.make_masks(rows), huber=3.0, **room.SOLVER)
    loo = np.array([outs[1 + k]["edge_cost"][2 + k] for k in range(4)])
    print("room, a wrong fourth constraint: statuses", [o["status"] for o in outs], "leave-one-out", loo)
    assert np.argmax(loo) == 3 and loo[3] > 10 * loo[:3].max()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_class_sum_is_a_sum(n):
    t = np.random.default_rng(n).normal(size=n)
    assert abs(ref.class_sum(t) - np.sum(t)) < 1e-12 and ref.class_sum(t, np.arange(n) % 2 == 0) == ref.class_sum(np.where(np.arange(n) % 2 == 0, t, 0.0))

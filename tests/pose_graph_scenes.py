"""Seeded pose graphs for the pose-graph tests, their truth, and the bounds measured on them (tests/test_pose_graph_cpu.py measures, the GPU tests
rely on them).  Everything is generated from a seed; nothing here calls the library."""
import numpy as np

# ---- measured bounds -------------------------------------------------------------------------------------------------------------------------------
# test_blocks_against_difference_quotients.  Hd against the second central differences of the cost at consistent poses, h = 1e-4: the gap measured
# 1.8e-9 of the largest entry of Hd.  A central second difference is off by h^2 / 12 times the fourth derivative (1e-8 times a ratio of derivatives of
# order 1 to 10 for poses a few metres apart) plus eps * cost / h^2 of rounding (4e-11 here), so the bound is 1e-7.
FD_HESSIAN_BOUND = 1e-7
# g against the first central differences of cost / 2, h = 1e-6, with measurement noise of 1e-3 (metres and radians): the gap measured 4.0e-4 of the
# largest entry of g.  This one is not rounding: the Jacobian of the inverse retraction is taken as the identity where it is I + ad(r) / 2 + ..., an
# error of |r| / 2 per unit of g, and |r| reaches 3 sigma = 3e-3 here (two noisy measurements can meet in one pose), so the bound is 3e-3.
FD_GRADIENT_BOUND = 3e-3
# test_converges_where_a_dense_gauss_newton_does: the largest difference (metres, and rotation-matrix entries) between the poses the restatement
# converges to with pcg_tol = 1e-8 and those of an independent dense Gauss-Newton (np.linalg.solve on the assembled matrix) run to the same min_step =
# 1e-9 measured 8.8e-10; the bound is twice that, as REGISTER_BOUND_M is made.
DENSE_GN_GAP = 8.8e-10
DENSE_GN_BOUND = 2 * DENSE_GN_GAP


def rodrigues(w):
    """the rotation matrix of the rotation vector w (scene construction only: the library has no trigonometry)"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def measure(Rt, Tt, ij, rng, sigma_t=0.0, sigma_r=0.0):
    """Z [E, 12] of the edges ij at the poses (Rt, Tt): P_b^-1 P_a, the translation off by N(0, sigma_t) and the rotation by a vector N(0, sigma_r)"""
    Z = np.zeros((len(ij), 12))
    for e, (a, b) in enumerate(ij):
        Rz = Rt[b].T @ Rt[a] @ rodrigues(rng.normal(0, sigma_r, 3) if sigma_r else np.zeros(3))
        Tz = Rt[b].T @ (Tt[a] - Tt[b]) + (rng.normal(0, sigma_t, 3) if sigma_t else 0.0)
        Z[e, :9], Z[e, 9:] = Rz.reshape(9), Tz
    return Z


def information(E, sigma_t=0.02, sigma_r=0.01, rng=None):
    """L [E, 21]: diag(1 / sigma_t^2 x 3, 1 / sigma_r^2 x 3), or with rng a dense positive definite matrix of that scale per edge"""
    L = np.zeros((E, 6, 6))
    d = np.array([1 / sigma_t ** 2] * 3 + [1 / sigma_r ** 2] * 3)
    for e in range(E):
        if rng is None:
            L[e] = np.diag(d)
        else:
            Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
            M = Q @ np.diag(rng.uniform(0.5, 2.0, 6)) @ Q.T
            L[e] = np.sqrt(d)[:, None] * ((M + M.T) / 2) * np.sqrt(d)[None, :]
    return np.stack([L[:, a, c] for a in range(6) for c in range(a, 6)], axis=-1)


def random_graph(N, ij, seed, fixed=(0,), spread=3.0, angle=0.5, start_t=0.05, start_r=0.03, sigma_t=0.01, sigma_r=0.005, dense_information=True):
    """N random poses (rotation vectors of N(0, angle) per axis), edges ij measured with noise, start = the truth moved by N(0, start_t) metres and N(0,
    start_r) radians except at the fixed poses"""
    rng = np.random.default_rng(seed)
    Rt = np.stack([rodrigues(rng.normal(0, angle, 3)) for _ in range(N)])
    Tt = rng.uniform(-spread, spread, (N, 3))
    fx = np.zeros(N, np.uint8)
    fx[list(fixed)] = 1
    R0, T0 = Rt.copy(), Tt.copy()
    for i in range(N):
        if not fx[i]:
            R0[i] = rodrigues(rng.normal(0, start_r, 3)) @ Rt[i]
            T0[i] = Tt[i] + rng.normal(0, start_t, 3)
    ij = np.asarray(ij, np.int32).reshape(-1, 2)
    return {"R": R0, "T": T0, "fixed": fx, "ij": ij, "Z": measure(Rt, Tt, ij, rng, sigma_t, sigma_r),
            "L": information(len(ij), rng=rng if dense_information else None), "R_true": Rt, "T_true": Tt}


def chain_edges(n, closures=()):
    """odometry edges (i + 1 -> i) and then the closures (a, b)"""
    return [(i + 1, i) for i in range(n - 1)] + [tuple(c) for c in closures]


def loop(n, seed, closures=None, radius=5.0, odo_t=0.02, odo_r=0.01, clo_t=0.01, clo_r=0.005, wrong=None):
    """A robot drives n poses round a circle, yawing with it and bobbing a little.  The odometry edges are noisy, the start poses are the odometry integrated
    from pose 0 (fixed), so they drift; the closures (default: the ends of the loop, and every tenth pose to the pose a quarter turn on) are measured
    with less noise.  wrong = (k, angle): closure k is measured with its rotation off by `angle` radians about z.  Returns the graph and n_odometry."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    Rt = np.stack([rodrigues([0.05 * np.sin(3 * a), 0.05 * np.cos(2 * a), a]) for a in ang])
    Tt = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.3 * np.sin(2 * ang)], axis=1)
    if closures is None:
        closures = [(n - 1, 0)] + [(i, (i + n // 4) % n) for i in range(0, n, 10)]
    ij = np.asarray(chain_edges(n, closures), np.int32)
    n_odo = n - 1
    Z = np.concatenate([measure(Rt, Tt, ij[:n_odo], rng, odo_t, odo_r), measure(Rt, Tt, ij[n_odo:], rng, clo_t, clo_r)])
    if wrong is not None:
        k, angle = wrong
        Z[n_odo + k, :9] = (Z[n_odo + k, :9].reshape(3, 3) @ rodrigues([0, 0, angle])).reshape(9)
    R0, T0 = Rt.copy(), Tt.copy()
    for i in range(1, n):                                            # P_i = P_(i-1) Z_i: the edge (i, i - 1) measures P_(i-1)^-1 P_i
        Rz, Tz = Z[i - 1, :9].reshape(3, 3), Z[i - 1, 9:]
        R0[i], T0[i] = R0[i - 1] @ Rz, R0[i - 1] @ Tz + T0[i - 1]
    fx = np.zeros(n, np.uint8)
    fx[0] = 1
    L = np.concatenate([information(n_odo, odo_t, odo_r), information(len(ij) - n_odo, clo_t, clo_r)])
    return {"R": R0, "T": T0, "fixed": fx, "ij": ij, "Z": Z, "L": L, "R_true": Rt, "T_true": Tt, "n_odometry": n_odo}


def pose_error(R, T, G):
    """the largest translation error in metres and the largest rotation-matrix entry error against the truth"""
    return float(np.abs(T - G["T_true"]).max()), float(np.abs(R - G["R_true"]).max())


def args(G):
    return G["R"], G["T"], G["fixed"], G["ij"], G["Z"], G["L"]

"""The pose graph of include/taichislam_hip.h ("pose graph") restated in float64 numpy, bit for bit: every expression below has the
operand order of the header, and every sum over a summed axis is written out term by term -- no np.sum, np.dot, @ or einsum on a summed axis, which
re-associate.  Vectorised only ACROSS edges or poses, where the elements do not meet.  tests/test_pose_graph_cpu.py checks this file against hand-worked
cases, difference quotients and an independent dense Gauss-Newton; tests/test_pose_graph_gpu.py holds the kernel to it."""
import numpy as np

STATUS = ("converged", "iterations", "stalled", "singular", "unanchored", "flipped")
DIAG = (0, 6, 11, 15, 18, 20)            # the diagonal among the 21 upper-triangle entries
DEFAULTS = dict(iters=20, damping=1e-6, damping_up=10.0, damping_down=10.0, damping_min=1e-12, damping_max=1e6, pcg_tol=1e-3, pcg_max=1000, min_step=1e-6,
                rel_tol=1e-9, huber=0.0)


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def dot6(a, b):
    return ((((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]) + a[..., 4] * b[..., 4]) + a[..., 5] * b[..., 5]


def upper_index(a, c):
    return a * 6 - (a * (a - 1)) // 2 + (c - a)


def full(L21, w):
    """[M, 21] (times w [M]) -> the symmetric [M, 6, 6]"""
    Lf = np.zeros(L21.shape[:-1] + (6, 6))
    k = 0
    for a in range(6):
        for c in range(a, 6):
            x = w * L21[..., k]
            Lf[..., a, c] = x
            Lf[..., c, a] = x
            k += 1
    return Lf


def pack_upper(M):
    """a symmetric [.., 6, 6] -> its 21 upper-triangle entries (what the library takes as L)"""
    M = np.asarray(M, np.float64)
    return np.stack([M[..., a, c] for a in range(6) for c in range(a, 6)], axis=-1)


def matvec(Lf, v):
    return np.stack([dot6(Lf[..., i, :], v) for i in range(6)], axis=-1)


def residual(Ra, Ta, Rb, Tb, Z):
    """r [M, 6] and den [M] of edges with poses Ra [M, 3, 3] .. and measurements Z [M, 12]"""
    Rz, Tz = Z[:, :9].reshape(-1, 3, 3), Z[:, 9:]
    d = Ta - Tb
    Rx = np.zeros_like(Ra)
    RD = np.zeros_like(Ra)
    Tx = np.zeros_like(Ta)
    for i in range(3):
        for j in range(3):
            Rx[:, i, j] = dot3(Rb[:, 0, i], Ra[:, 0, j], Rb[:, 1, i], Ra[:, 1, j], Rb[:, 2, i], Ra[:, 2, j])
        Tx[:, i] = dot3(Rb[:, 0, i], d[:, 0], Rb[:, 1, i], d[:, 1], Rb[:, 2, i], d[:, 2])
    for i in range(3):
        for j in range(3):
            RD[:, i, j] = dot3(Rx[:, i, 0], Rz[:, j, 0], Rx[:, i, 1], Rz[:, j, 1], Rx[:, i, 2], Rz[:, j, 2])
    r = np.zeros((Ra.shape[0], 6))
    for i in range(3):
        r[:, i] = Tx[:, i] - dot3(RD[:, i, 0], Tz[:, 0], RD[:, i, 1], Tz[:, 1], RD[:, i, 2], Tz[:, 2])
    den = 1.0 + ((RD[:, 0, 0] + RD[:, 1, 1]) + RD[:, 2, 2])
    with np.errstate(all="ignore"):
        r[:, 3] = (2.0 * (RD[:, 2, 1] - RD[:, 1, 2])) / den
        r[:, 4] = (2.0 * (RD[:, 0, 2] - RD[:, 2, 0])) / den
        r[:, 5] = (2.0 * (RD[:, 1, 0] - RD[:, 0, 1])) / den
    return r, den


def tinv(Rb, Tb):
    return np.stack([-dot3(Rb[:, 0, i], Tb[:, 0], Rb[:, 1, i], Tb[:, 1], Rb[:, 2, i], Tb[:, 2]) for i in range(3)], axis=-1)


def adj(Rb, ti, d):
    """A d, A = Ad(P_b^-1)"""
    Rv = [dot3(Rb[:, 0, i], d[:, 0], Rb[:, 1, i], d[:, 1], Rb[:, 2, i], d[:, 2]) for i in range(3)]
    Rw = [dot3(Rb[:, 0, i], d[:, 3], Rb[:, 1, i], d[:, 4], Rb[:, 2, i], d[:, 5]) for i in range(3)]
    return np.stack([Rv[0] + (ti[:, 1] * Rw[2] - ti[:, 2] * Rw[1]), Rv[1] + (ti[:, 2] * Rw[0] - ti[:, 0] * Rw[2]), Rv[2] + (ti[:, 0] * Rw[1] - ti[:, 1] * Rw[0]),
                     Rw[0], Rw[1], Rw[2]], axis=-1)


def adj_t(Rb, ti, m):
    """A^T m"""
    s = [m[:, 3] - (ti[:, 1] * m[:, 2] - ti[:, 2] * m[:, 1]), m[:, 4] - (ti[:, 2] * m[:, 0] - ti[:, 0] * m[:, 2]), m[:, 5] - (ti[:, 0] * m[:, 1] - ti[:, 1] * m[:, 0])]
    return np.stack([dot3(Rb[:, i, 0], m[:, 0], Rb[:, i, 1], m[:, 1], Rb[:, i, 2], m[:, 2]) for i in range(3)] +
                    [dot3(Rb[:, i, 0], s[0], Rb[:, i, 1], s[1], Rb[:, i, 2], s[2]) for i in range(3)], axis=-1)


def class_sum(terms, on=None):
    """the 256-class sum of the header; on: the terms that take part"""
    s = np.zeros(256)
    n = terms.shape[0]
    for lo in range(0, n, 256):
        c = terms[lo:lo + 256]
        k = c.shape[0]
        s[:k] = s[:k] + c if on is None else np.where(on[lo:lo + 256], s[:k] + c, s[:k])
    h = 128
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def mask_bits(mask, E):
    """uint64 words [ceil(E / 64)] (None: every edge) -> bool [E]"""
    if mask is None:
        return np.ones(E, bool)
    w = np.asarray(mask, np.uint64).reshape(-1)
    e = np.arange(E)
    return ((w[e >> 6] >> (e & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def make_masks(rows):
    """bool [B, E] -> uint64 [B, ceil(E / 64)]"""
    rows = np.atleast_2d(np.asarray(rows, bool))
    B, E = rows.shape
    out = np.zeros((B, (E + 63) // 64), np.uint64)
    for e in range(E):
        out[:, e >> 6] |= rows[:, e].astype(np.uint64) << np.uint64(e & 63)
    return out


class Graph:
    """the arrays of a call as float64 / int32, and the incidence lists as rounds: round k holds, for every pose with more than k incident edges, the
    k-th of them in ascending edge index"""

    def __init__(self, fixed, ij, Z, L):
        self.ij = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
        self.Z = np.ascontiguousarray(Z, np.float64).reshape(-1, 12)
        self.L = np.ascontiguousarray(L, np.float64).reshape(-1, 21)
        self.E = self.ij.shape[0]
        self.fixed = np.asarray(fixed).astype(bool)
        self.N = self.fixed.shape[0]
        self.free = ~self.fixed
        lists = [[] for _ in range(self.N)]
        for e in range(self.E):
            lists[self.ij[e, 0]].append(2 * e)
            lists[self.ij[e, 1]].append(2 * e + 1)
        self.rounds = []
        k = 0
        while True:
            idx = np.array([i for i in range(self.N) if len(lists[i]) > k and self.free[i]], np.int64)
            if idx.size == 0:
                break
            code = np.array([lists[i][k] for i in idx], np.int64)
            self.rounds.append((idx, code >> 1, (code & 1).astype(bool)))
            k += 1

    def gather(self, per_edge, on, start=None):
        """per free pose: start (or 0) + / - the rows of per_edge over its enabled incident edges in ascending index; 0 for fixed poses"""
        out = np.zeros((self.N,) + per_edge.shape[1:]) if start is None else start.copy()
        for idx, e, is_b in self.rounds:
            cur = out[idx]
            sel = on[e].reshape((-1,) + (1,) * (per_edge.ndim - 1))
            nxt = np.where(is_b.reshape(sel.shape), cur - per_edge[e], cur + per_edge[e])
            out[idx] = np.where(sel, nxt, cur)
        return out

    def gather_plus(self, per_edge, on):
        out = np.zeros((self.N,) + per_edge.shape[1:])
        for idx, e, _ in self.rounds:
            cur = out[idx]
            out[idx] = np.where(on[e][:, None], cur + per_edge[e], cur)
        return out


def edges(G, R, T, on, huber):
    """one pass over the edges: r, c = r^T L r, wgt, flipped, and the cost over the enabled edges"""
    a, b = G.ij[:, 0], G.ij[:, 1]
    r, den = residual(R[a], T[a], R[b], T[b], G.Z)
    with np.errstate(all="ignore"):
        c = dot6(r, matvec(full(G.L, 1.0), r))
        rho, w = c.copy(), np.ones(G.E)
        if huber > 0.0:
            chi = np.sqrt(c)
            out = chi > huber
            w = np.where(out, huber / chi, 1.0)
            rho = np.where(out, (2.0 * huber) * chi - huber * huber, c)
        flipped = den < 1.0
        return r, c, w, flipped, class_sum(rho, on)


def blocks(G, R, T, on, r, w):
    """Hd [N, 21] and g [N, 6]"""
    b = G.ij[:, 1]
    Rb, ti = R[b], tinv(R[b], T[b])
    Lw = full(G.L, w)
    q = adj_t(Rb, ti, matvec(Lw, r))
    W = np.zeros((G.E, 21))
    for j in range(6):
        ej = np.zeros((G.E, 6))
        ej[:, j] = 1.0
        wj = adj_t(Rb, ti, matvec(Lw, adj(Rb, ti, ej)))
        for a in range(j + 1):
            W[:, upper_index(a, j)] = wj[:, a]
    return G.gather_plus(W, on), G.gather(q, on)


def linearize(R, T, fixed, ij, Z, L, mask=None, huber=0.0):
    R, T = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(T, np.float64).reshape(-1, 3)
    G = Graph(np.zeros(R.shape[0], bool) if fixed is None else fixed, ij, Z, L)
    on = mask_bits(mask, G.E)
    r, c, w, flipped, _ = edges(G, R, T, on, huber)
    Hd, g = blocks(G, R, T, on, r, w)
    return {"r": r, "cost": c, "flipped": flipped.astype(np.uint8), "Hd": Hd, "g": g}


def cholesky(Hm):
    """[M, 6, 6] -> the lower factor and singular [M], in al_cholesky's order"""
    M = Hm.shape[0]
    Lm = np.zeros((M, 6, 6))
    bad = np.zeros(M, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = Hm[:, j, j].copy()
            for k in range(j):
                d = d - Lm[:, j, k] * Lm[:, j, k]
            bad |= ~(d > 0.0) | ~np.isfinite(d)
            Lm[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                t = Hm[:, i, j].copy()
                for k in range(j):
                    t = t - Lm[:, i, k] * Lm[:, j, k]
                Lm[:, i, j] = t / Lm[:, j, j]
    return Lm, bad


def cholesky_solve(Lm, c):
    y = np.zeros_like(c)
    x = np.zeros_like(c)
    for i in range(6):
        t = c[:, i].copy()
        for k in range(i):
            t = t - Lm[:, i, k] * y[:, k]
        y[:, i] = t / Lm[:, i, i]
    for i in range(5, -1, -1):
        t = y[:, i].copy()
        for k in range(i + 1, 6):
            t = t - Lm[:, k, i] * x[:, k]
        x[:, i] = t / Lm[:, i, i]
    return x


def retract(xi, R, T):
    """al_retract over [M] poses"""
    a = xi[:, 3:] * 0.5
    aa = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    den = 1.0 + aa
    zero = np.zeros_like(aa)
    S = [[zero, -a[:, 2], a[:, 1]], [a[:, 2], zero, -a[:, 0]], [-a[:, 1], a[:, 0], zero]]
    Cm = [[((((1.0 - aa) if i == j else zero) + (2.0 * a[:, i]) * a[:, j]) + 2.0 * S[i][j]) / den for j in range(3)] for i in range(3)]
    Rn, Tn = np.zeros_like(R), np.zeros_like(T)
    for i in range(3):
        for j in range(3):
            Rn[:, i, j] = (Cm[i][0] * R[:, 0, j] + Cm[i][1] * R[:, 1, j]) + Cm[i][2] * R[:, 2, j]
        Tn[:, i] = ((Cm[i][0] * T[:, 0] + Cm[i][1] * T[:, 1]) + Cm[i][2] * T[:, 2]) + xi[:, i]
    return Rn, Tn


def unanchored(G, on):
    """status 4: some component of the enabled edges holds a free pose and no fixed one"""
    root = list(range(G.N))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i
    for e in range(G.E):
        if on[e]:
            a, b = find(int(G.ij[e, 0])), find(int(G.ij[e, 1]))
            if a != b:
                root[max(a, b)] = min(a, b)
    has = {find(i) for i in range(G.N) if G.fixed[i]}
    return any(find(i) not in has for i in range(G.N) if G.free[i])


def _solve_one(G, R0, T0, on, o):
    R, T = R0.copy(), T0.copy()
    N, f = G.N, G.free
    records = []
    status = 4 if unanchored(G, on) else 0
    damping = float(o["damping"])
    tol2 = o["pcg_tol"] * o["pcg_tol"]
    if status == 0 and np.any(edges(G, R, T, on, o["huber"])[3] & on):
        status = 5
    if status == 0:
        status = 1
        for _ in range(int(o["iters"])):
            r, _, w, _, cost = edges(G, R, T, on, o["huber"])
            Hd, g = blocks(G, R, T, on, r, w)
            Hm = full(Hd[f], 1.0)
            for a in range(6):
                Hm[:, a, a] = Hm[:, a, a] + damping * Hm[:, a, a]
            Lm, bad = cholesky(Hm)
            if bad.any():
                records.append((cost, cost, 0.0, damping, 0, 0))
                status = 3
                break
            b = G.ij[:, 1]
            Rb, ti, Lw = R[b], tinv(R[b], T[b]), full(G.L, w)
            dg = Hd[:, DIAG]
            x, rr, z = np.zeros((N, 6)), np.zeros((N, 6)), np.zeros((N, 6))
            rr[f] = -g[f]
            z[f] = cholesky_solve(Lm, rr[f])
            p = z.copy()
            rz = class_sum(dot6(rr, z))
            rz0 = rz
            n_pcg = 0
            with np.errstate(all="ignore"):
                while n_pcg < int(o["pcg_max"]) and not rz <= tol2 * rz0:
                    u = adj_t(Rb, ti, matvec(Lw, adj(Rb, ti, p[G.ij[:, 0]] - p[b])))
                    start = np.zeros((N, 6))
                    start[f] = (damping * dg[f]) * p[f]
                    y = G.gather(u, on, start)
                    pAp = class_sum(dot6(p, y))
                    if not pAp > 0.0:
                        break
                    alpha = rz / pAp
                    x = x + alpha * p
                    rr = rr - alpha * y
                    z = np.zeros((N, 6))
                    z[f] = cholesky_solve(Lm, rr[f])
                    rz_new = class_sum(dot6(rr, z))
                    beta = rz_new / rz
                    p = z + beta * p
                    rz = rz_new
                    n_pcg += 1
                Rt, Tt = R.copy(), T.copy()
                Rt[f], Tt[f] = retract(x[f], R[f], T[f])
                n2 = dot6(x[f], x[f])
                n2max = 0.0
                for v in n2:                                # max is order-free unless a NaN takes part; the kernel keeps the larger by `>`
                    n2max = v if v > n2max else n2max
                step = np.sqrt(n2max)
                _, _, _, fl, trial = edges(G, Rt, Tt, on, o["huber"])
                accept = bool(not np.any(fl & on) and np.isfinite(trial) and trial < cost)
            records.append((cost, trial, step, damping, n_pcg, int(accept)))
            if accept:
                R, T = Rt, Tt
                d = damping / o["damping_down"]
                damping = d if d > o["damping_min"] else o["damping_min"]
                if step < o["min_step"] or cost - trial <= o["rel_tol"] * cost:
                    status = 0
                    break
            else:
                damping = damping * o["damping_up"]
                if damping > o["damping_max"]:
                    status = 2
                    break
    r, c, _, _, cost = edges(G, R, T, on, o["huber"])
    return {"R": R, "T": T, "r": r, "edge_cost": c, "cost": cost, "status": status, "iterations": len(records), "records": records}


def solve(R, T, fixed, ij, Z, L, masks=None, **kw):
    """the variants one after the other: a list of {"R", "T", "r", "edge_cost", "cost", "status", "iterations", "records": [(cost_before, cost_after,
    max_step, damping, pcg_iters, accepted)]}"""
    o = dict(DEFAULTS)
    o.update(kw)
    R, T = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(T, np.float64).reshape(-1, 3)
    G = Graph(fixed, ij, Z, L)
    rows = [None] if masks is None else list(np.asarray(masks, np.uint64).reshape(-1, (G.E + 63) // 64))
    return [_solve_one(G, R, T, mask_bits(m, G.E), o) for m in rows]

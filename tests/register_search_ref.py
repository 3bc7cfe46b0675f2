"""numpy restatement of the pose search for the registration (taichislam_amd/csrc/tsl_register_search.hip).  score: e, n_used,
n_unknown, n_far and n_grad of register_ref.linearize for every pose, which the GPU must equal; gate: the pose-independent counts and index sums;
candidates, cost and search: the lattice, the integer cost and the ranking in float64 / int64 in the written order, the refinement by
register_ref.register.  Sources and grids are those of register_ref."""
import numpy as np

import register_ref as rr
import render_view_ref as rv
import track_ref as tr

F32 = np.float32
FIELDS = ("e", "n_used", "n_unknown", "n_far", "n_grad")
_SLOT = dict(e=tr.I_E, n_used=tr.I_USED, n_unknown=tr.I_UNKNOWN, n_far=tr.I_FAR, n_grad=tr.I_GRAD)
MAX_CANDIDATES = 65536


def _gated(src, stride, w_min, band):
    """(lattice mask, pass mask over the lattice voxels) as register_ref.linearize forms them"""
    idx, t, w = src
    lattice = ((idx % stride) == 0).all(1)
    with np.errstate(invalid="ignore"):
        gate = ~((w[lattice] >= F32(w_min)) & (np.abs(t[lattice]) <= F32(band)))
    return lattice, ~gate


def gate(src, stride, w_min, band, **_):
    """tsl_register_gate as a dict: n_gate, n_pass and the integer sums of the passing voxels' indices"""
    lattice, ok = _gated(src, stride, w_min, band)
    idx = src[0][lattice][ok]
    return dict(n_gate=int((~ok).sum()), n_pass=int(ok.sum()), sum_i=int(idx[:, 0].sum()), sum_j=int(idx[:, 1].sum()), sum_k=int(idx[:, 2].sum()))


def score_slow(src, R, T, stride, vs, grid, counts_only=False, **gates):
    """the definition: register_ref.linearize per pose"""
    R, T = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(T, np.float64).reshape(-1, 3)
    out = {f: np.zeros(R.shape[0], np.int64) for f in FIELDS}
    for k in range(R.shape[0]):
        s = rr.linearize(src, R[k], T[k], stride, vs, grid, **gates)
        for f in FIELDS:
            out[f][k] = s[_SLOT[f]]
    if counts_only:
        out["e"][:] = 0
    return out


def score(src, R, T, stride, vs, grid, w_min, band, r_max, g_max, huber=0.0, counts_only=False, chunk=256):
    """The fast path: the same f32 expressions in the same order as register_ref.linearize, over chunks of poses at once, without H and b.
    tests/test_register_search_cpu.py checks it against score_slow.  Returns a dict of int64 arrays [n]."""
    assert stride in rr.STRIDES
    R = np.asarray(R, np.float64).reshape(-1, 3, 3).astype(F32)
    T = np.asarray(T, np.float64).reshape(-1, 3).astype(F32)
    n = R.shape[0]
    val, known, lo = grid
    vs, r_max, g_max, huber = F32(vs), F32(r_max), F32(g_max), F32(huber)
    gm2 = g_max * g_max
    lattice, ok = _gated(src, stride, w_min, band)
    idx, t = src[0][lattice][ok], src[1][lattice][ok]
    m = idx.shape[0]
    q = idx.astype(F32) * vs
    out = {f: np.zeros(n, np.int64) for f in FIELDS}
    if m == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a0 in range(0, n, chunk):
            Rc, Tc = R[a0:a0 + chunk], T[a0:a0 + chunk]
            c = Rc.shape[0]
            p = np.stack([((Rc[:, a, 0, None] * q[None, :, 0] + Rc[:, a, 1, None] * q[None, :, 1]) + Rc[:, a, 2, None] * q[None, :, 2]) + Tc[:, a, None]
                          for a in range(3)], 2).astype(F32).reshape(c * m, 3)
            s, kn, g = rv.sample(p, vs, val, known, lo)
            g = (g / vs).astype(F32)
            far = kn & ~(np.abs(s) <= r_max)
            gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            bad = kn & ~far & ~((gg > 0) & (gg <= gm2))
            used = kn & ~far & ~bad
            r = np.where(used, s - np.tile(t, c), F32(0)).astype(F32)      # only a used sample's residual reaches fix()
            e = np.where(used, tr.fix((tr.robust_weight(r, huber) * r) * r), 0)
            sl = slice(a0, a0 + c)
            out["e"][sl] = e.reshape(c, m).sum(1)
            out["n_used"][sl] = used.reshape(c, m).sum(1)
            out["n_unknown"][sl] = (~kn).reshape(c, m).sum(1)
            out["n_far"][sl] = far.reshape(c, m).sum(1)
            out["n_grad"][sl] = bad.reshape(c, m).sum(1)
    if counts_only:
        out["e"][:] = 0
    return out


def half_counts(window, step):
    """round(window / step) per axis, as DenseTSDF.register_search forms them; a step may be a scalar"""
    step = np.broadcast_to(np.asarray(step, np.float64), (3,))
    return tuple(int(round(float(w) / float(s))) if float(w) != 0.0 else 0 for w, s in zip(window, step)), tuple(float(s) for s in step)


def candidates(R0, T0, pivot, n_t, step_t, n_r, step_r):
    """(R [n, 3, 3], T [n, 3]) float64: k runs over (r0, r1, r2, t0, t1, t2), the last fastest; an offset is (index - n) * step.  Tp = T0 - pivot;
    (R, Tp) <- retract((0, 0, 0, omega), R0, Tp); T = (Tp + pivot) + v.  The candidate with every offset zero is the guess itself."""
    R0, T0 = np.array(R0, np.float64).reshape(3, 3), np.array(T0, np.float64).reshape(3)
    pivot = np.array(pivot, np.float64).reshape(3)
    nn = [int(v) for v in n_r] + [int(v) for v in n_t]
    st = [float(v) for v in step_r] + [float(v) for v in step_t]
    total = 1
    for v in nn:
        assert v >= 0
        total *= 2 * v + 1
    assert total <= MAX_CANDIDATES
    Rs, Ts = np.empty((total, 3, 3), np.float64), np.empty((total, 3), np.float64)
    cache = {}                                                     # the rotation part depends on (r0, r1, r2) alone
    for k, ix in enumerate(np.ndindex(*[2 * v + 1 for v in nn])):
        off = [float(ix[a] - nn[a]) * st[a] for a in range(6)]
        if all(ix[a] == nn[a] for a in range(6)):
            Rs[k], Ts[k] = R0, T0
            continue
        if ix[:3] not in cache:
            cache[ix[:3]] = tr.retract([0.0, 0.0, 0.0, off[0], off[1], off[2]], R0, T0 - pivot)
        Rk, Tp = cache[ix[:3]]
        Rs[k] = Rk
        Ts[k] = (Tp + pivot) + np.array(off[3:], np.float64)
    return Rs, Ts


def cost(sc, r_max, miss):
    """J = e + F n_far + U (n_unknown + n_grad) as int64; r_max after its default, miss 0 = r_max"""
    r_max = F32(r_max)
    miss = F32(miss) if miss else r_max
    F, U = int(tr.fix(r_max * r_max)), int(tr.fix(miss * miss))
    return sc["e"] + F * sc["n_far"] + U * (sc["n_unknown"] + sc["n_grad"])


def auto_pivot(src, R0, T0, stride, voxel_scale, **gates):
    """(pivot or None, gate dict): R0 qbar + T0, qbar the centroid of the gated source voxels; None when nothing passes the gate"""
    g = gate(src, stride, **gates)
    if g["n_pass"] == 0:
        return None, g
    R0, T0 = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(T0, np.float64).reshape(3)
    qb = [(float(g[s]) / float(g["n_pass"])) * float(voxel_scale) for s in ("sum_i", "sum_j", "sum_k")]
    return np.array([((R0[a, 0] * qb[0] + R0[a, 1] * qb[1]) + R0[a, 2] * qb[2]) + T0[a] for a in range(3)], np.float64), g


def search(src, R0, T0, vs, grid, voxel_scale, n_t, step_t, n_r, step_r, pivot=None, stride=4, miss=0.0, min_used=6, score_fn=score, register_kw=None, **gates):
    """(R, T, info) of tsl_tsdf_register_search.  info: register_ref.register's (status, iterations, records) and `search` = dict(status, n_candidates,
    n_valid, best, J_best, score_best, pivot, R_best, T_best, gate, scores).  gates: the values after the defaults."""
    R0, T0 = np.array(R0, np.float64).reshape(3, 3), np.array(T0, np.float64).reshape(3)
    g = gate(src, stride, **gates)
    n = 1
    for v in list(n_r) + list(n_t):
        n *= 2 * int(v) + 1
    rep = dict(status=2, n_candidates=n, n_valid=0, best=-1, J_best=0, score_best=None, pivot=None, R_best=R0.copy(), T_best=T0.copy(), gate=g, scores=None)
    lost = dict(status=2, iterations=0, records=[], search=rep)
    if pivot is None:
        pivot, _ = auto_pivot(src, R0, T0, stride, voxel_scale, **gates)
        if pivot is None:
            return R0, T0, lost
    rep["pivot"] = np.array(pivot, np.float64).reshape(3)
    Rs, Ts = candidates(R0, T0, rep["pivot"], n_t, step_t, n_r, step_r)
    sc = score_fn(src, Rs, Ts, stride, vs, grid, **gates)
    rep["scores"] = sc
    J = cost(sc, gates["r_max"], miss)
    valid = sc["n_used"] >= (min_used if min_used else 6)
    rep["n_valid"] = int(valid.sum())
    if not valid.any():
        return R0, T0, lost
    best = int(np.flatnonzero(valid)[np.argmin(J[valid])])          # argmin returns the first of equal values: ties go to the least k
    rep.update(best=best, J_best=int(J[best]), score_best={f: int(sc[f][best]) for f in FIELDS}, R_best=Rs[best].copy(), T_best=Ts[best].copy())
    R, T, info = rr.register(src, Rs[best], Ts[best], vs, grid, **(register_kw or {}), **gates)
    rep["status"] = info["status"]
    info["search"] = rep
    return R, T, info

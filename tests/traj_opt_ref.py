"""numpy float32 restatement of the B-spline trajectory linearisation and descent (taichislam_amd/csrc/tsl_traj_opt.hip, DESIGN.md section 4.22,
include/taichislam_hip.h): the GPU records, gradient planes, control points and histories must equal it bit for bit.  The values and gradients come from
esdf_query_ref.query (mode 1); the map is a dense grid as there.  A voxel whose TSDF is NaN counts as unknown: pass it with known = False, as for
path_score_ref.  Vectorised over the trajectories; the descent loops over the iterations on the host."""
import numpy as np

import esdf_query_ref as qref
from path_score_ref import NONE, key, unkey

F32 = np.float32
FIELDS = ("n_samples", "n_pen", "n_unknown", "n_outside", "argmin", "min_dist", "short_update", "iters_done", "cost_collision", "cost_smooth")
ONE = F32(1048576.0)             # 2^20: the fixed point
INV = F32(9.5367431640625e-07)   # 2^-20
BOUND = F32(1024.0)
STOP_FREE = 1


def basis(sub):
    """f32 [sub + 1, 4]: w_i = b_i / 6 at u = (float)m / (float)sub, m = 0 .. sub"""
    u = (np.arange(sub + 1).astype(F32) / F32(sub)).astype(F32)
    v = F32(1.0) - u
    u2 = u * u
    u3 = u2 * u
    b0 = (v * v) * v
    b1 = (F32(3.0) * u3 - F32(6.0) * u2) + F32(4.0)
    b2 = ((F32(3.0) * u2 - F32(3.0) * u3) + F32(3.0) * u) + F32(1.0)
    return (np.stack([b0, b1, b2, u3], 1) / F32(6.0)).astype(F32)


def clamp(t, b=BOUND):
    """fminf(fmaxf(t, -b), b): a NaN comes out as -b"""
    return np.fmin(np.fmax(np.asarray(t, F32), -F32(b)), F32(b)).astype(F32)


def q(t):
    """(int64)(int32)(clamp(t) * 2^20), truncated toward zero"""
    return np.trunc(clamp(t) * ONE).astype(np.int64)


def sq_cost(x):
    """(int64)((x * x) * 2^20) of f32 x with |x| <= 1024, truncated"""
    x = np.asarray(x, F32)
    return np.trunc((x * x).astype(F32) * ONE).astype(np.int64)


def _lengths(n, K, lengths):
    L = np.full(n, K, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    assert L.shape == (n,) and K >= 4 and (n == 0 or ((L >= 4) & (L <= K)).all())
    return L


def sample_points(ctrl, sub, lengths=None):
    """(p f32 [n, S_max, 3], valid bool [n, S_max], seg int [n, S_max], w f32 [n, S_max, 4]); the entries that are not valid repeat the last sample"""
    c = np.asarray(ctrl, F32)
    n, K = c.shape[:2]
    L = _lengths(n, K, lengths)
    S = (L - 3) * sub + 1
    j = np.arange((K - 3) * sub + 1)[None, :]
    valid = j < S[:, None]
    jj = np.minimum(j, S[:, None] - 1)
    seg = np.minimum(jj // sub, (L - 4)[:, None])
    w = basis(sub)[jj - seg * sub]
    r = np.arange(n)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        p = ((w[..., 0:1] * c[r, seg] + w[..., 1:2] * c[r, seg + 1]) + w[..., 2:3] * c[r, seg + 2]) + w[..., 3:4] * c[r, seg + 3]
    return p.astype(F32), valid, seg, w


def sample_values(ctrl, sub, lengths, vs, val, known, lo, unknown=np.nan):
    """(d f32 [n, S_max], g f32 [n, S_max, 3], st u8 [n, S_max] (0xff where not valid), valid, seg, w): the query's answer per sample; a status-0 sample
    whose value or gradient is not finite is unknown"""
    p, valid, seg, w = sample_points(ctrl, sub, lengths)
    d = np.full(valid.shape, F32(unknown), F32)
    g = np.zeros(valid.shape + (3,), F32)
    st = np.full(valid.shape, 0xff, np.uint8)
    qd, qg, qs = qref.query(p[valid], 1, vs, val, known, lo, unknown=unknown)
    bad = (qs == 0) & ~(np.isfinite(qd) & np.isfinite(qg).all(1))
    qd[bad], qg[bad], qs[bad] = F32(unknown), 0.0, 1
    d[valid], g[valid], st[valid] = qd, qg, qs
    return d, g, st, valid, seg, w


def smooth_terms(c, L):
    """(a f32 [n, K - 2, 3], counted bool [n, K - 2, 3]): the second differences of the terms 0 .. L - 3 and which of them are finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = ((c[:, :-2] - (c[:, 1:-1] + c[:, 1:-1])) + c[:, 2:]).astype(F32)
    counted = (np.arange(c.shape[1] - 2)[None, :] <= (L - 3)[:, None])[:, :, None] & np.isfinite(a)
    return a, counted


def linearize(ctrl, clearance, sub, lengths, vs, val, known, lo, unknown=np.nan):
    """(record dict FIELDS, grad_collision int64 [n, K, 3], grad_smooth int64 [n, K, 3]) of tsl_esdf_traj_linearize"""
    c = np.asarray(ctrl, F32)
    if c.ndim == 2:
        c = c[None]
    n, K = c.shape[:2]
    L = _lengths(n, K, lengths)
    d, g, st, valid, seg, w = sample_values(c, sub, L, vs, val, known, lo, unknown)
    ok = valid & (st == 0)
    with np.errstate(invalid="ignore", over="ignore"):
        cl = np.where(ok, np.minimum(F32(clearance) - d, BOUND), F32(0.0)).astype(F32)
        pen = ok & (cl > 0)
        Gp = -((F32(2.0) * cl)[..., None] * g).astype(F32)
        gc = np.zeros((n, K, 3), np.int64)
        r = np.broadcast_to(np.arange(n)[:, None], seg.shape)
        for i in range(4):
            t = (w[..., i:i + 1] * Gp).astype(F32)
            np.add.at(gc, (r, seg + i), np.where(pen[..., None], q(t), 0))
        a, counted = smooth_terms(c, L)
        gs = np.zeros((n, K, 3), np.int64)
        gs[:, :-2] += np.where(counted, q(F32(2.0) * a), 0)
        gs[:, 1:-1] += np.where(counted, q(F32(-4.0) * a), 0)
        gs[:, 2:] += np.where(counted, q(F32(2.0) * a), 0)
        cost_s = np.where(counted, sq_cost(clamp(np.where(counted, a, F32(0.0)))), 0).sum((1, 2))
    j = np.arange(valid.shape[1])[None, :]
    kv = np.where(ok, (key(d).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64), NONE)
    best = kv.min(1) if kv.shape[1] else np.full(n, NONE)
    has = best != NONE
    rec = {
        "n_samples": valid.sum(1).astype(np.int32), "n_pen": pen.sum(1).astype(np.int32), "n_unknown": (valid & (st == 1)).sum(1).astype(np.int32),
        "n_outside": (valid & (st == 2)).sum(1).astype(np.int32),
        "argmin": np.where(has, (best & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32),
        "min_dist": np.where(has, unkey((best >> np.uint64(32)).astype(np.uint32)), F32(np.inf)).astype(F32),
        "short_update": np.zeros(n, np.int32), "iters_done": np.zeros(n, np.int32),
        "cost_collision": np.where(pen, sq_cost(cl), 0).sum(1).astype(np.int64), "cost_smooth": cost_s.astype(np.int64),
    }
    return rec, gc, gs


def optimize(ctrl, clearance, sub, iters, lengths, vs, val, known, lo, w_collision=1.0, w_smooth=1.0, step=0.05, momentum=0.8, max_move=None, fix_head=3,
             fix_tail=3, flags=0, unknown=np.nan):
    """(ctrl_out f32 [n, K, 3], record dict, history int64 [n, iters + 1, 2], n_clamped int [n]) of tsl_esdf_traj_optimize; n_clamped counts the
    velocity components the max_move clamp changed (for the tests: it is not an output of the kernel)"""
    c = np.array(ctrl, F32)
    if c.ndim == 2:
        c = c[None]
    n, K = c.shape[:2]
    L = _lengths(n, K, lengths)
    mm = F32(0.5) * F32(vs) if max_move is None else F32(max_move)
    wc, ws, step, mom = F32(w_collision), F32(w_smooth), F32(step), F32(momentum)
    i = np.arange(K)[None, :]
    moves = ((i >= fix_head) & (i <= (L - 1 - fix_tail)[:, None]))[:, :, None]
    v = np.zeros_like(c)
    live = np.ones(n, bool)
    rec = {k: np.zeros(n, np.float32 if k == "min_dist" else np.int64 if k.startswith("cost") else np.int32) for k in FIELDS}
    hist = np.full((n, iters + 1, 2), -1, np.int64)
    n_clamped = np.zeros(n, np.int64)
    for k in range(iters + 1):
        at = np.nonzero(live)[0]
        if at.size == 0:
            break
        r, gc, gs = linearize(c[at], clearance, sub, L[at], vs, val, known, lo, unknown)
        for f in FIELDS:
            rec[f][at] = r[f]
        rec["iters_done"][at] = k
        hist[at, k, 0], hist[at, k, 1] = r["cost_collision"], r["cost_smooth"]
        if k == iters:
            break
        if flags & STOP_FREE:
            keep = r["n_pen"] > 0
            live[at[~keep]] = False
            at, gc, gs = at[keep], gc[keep], gs[keep]
        with np.errstate(invalid="ignore", over="ignore"):
            gr = (wc * (gc.astype(F32) * INV) + ws * (gs.astype(F32) * INV)).astype(F32)
            nv = (mom * v[at] - step * gr).astype(F32)
            nv[~np.isfinite(nv)] = F32(0.0)
            cv = clamp(nv, mm)
            n_clamped[at] += ((cv != nv) & moves[at]).sum((1, 2))
            v[at] = np.where(moves[at], cv, v[at])
            c[at] = np.where(moves[at], (c[at] + v[at]).astype(F32), c[at])
    return c, rec, hist, n_clamped


def assert_equal(got, want, what):
    """every record field as integers / bits"""
    for k in FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "min_dist":
            g, w = np.ascontiguousarray(g, F32).view(np.uint32), np.ascontiguousarray(w, F32).view(np.uint32)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} trajectories, first {bad[:5]}: {g[bad[:5]]} / {w[bad[:5]]}"


def assert_bits(got, want, what):
    """two arrays of the same shape, equal as bits (NaN equals NaN of the same payload)"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.shape} {g.dtype} / {w.shape} {w.dtype}"
    gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
    bad = np.argwhere(gv != wv)
    assert bad.size == 0, f"{what}: differs at {len(bad)} entries, first {bad[:3].tolist()}: {g[tuple(bad[0])]} / {w[tuple(bad[0])]}"

"""numpy float32 restatement of the path scoring (taichislam_amd/csrc/tsl_path_score.hip, DESIGN.md section 4.13, include/taichislam_hip.h): the GPU
records and per-sample rows must equal it bit for bit.  The values come from esdf_query_ref.query; the map is a dense grid as there.  A voxel whose TSDF
is NaN counts as unknown here although the point query reports a value for it (0: the sign of a NaN times the magnitude): pass it with known = False."""
import numpy as np

import esdf_query_ref as qref

F32 = np.float32
STOP, UNKNOWN_BLOCKS, OUTSIDE_BLOCKS = 1, 2, 4
FIELDS = ("n_samples", "first_stop", "n_hit", "n_unknown", "n_outside", "argmin", "min_dist", "short_update", "cost")
NONE = np.uint64(0xffffffffffffffff)


def key(d):
    """the monotone uint32 image of a float's bits: -0.0 sorts before +0.0"""
    b = np.ascontiguousarray(d, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def sample_points(waypoints, sub, lengths=None):
    """(p f32 [n, S_max, 3], valid bool [n, S_max]): sample j of a path is waypoint j / sub itself when j % sub == 0, else lerp(a, b, (float)m / (float)sub)"""
    w = np.asarray(waypoints, F32)
    n, K = w.shape[:2]
    smax = (K - 1) * sub + 1
    j = np.arange(smax)
    seg, m = j // sub, j % sub
    a, b = w[:, seg], w[:, np.minimum(seg + 1, K - 1)]
    t = (m.astype(F32) / F32(sub)).astype(F32)[None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        p = qref.lerp(a, b, t).astype(F32)
    p = np.where((m == 0)[None, :, None], a, p)
    L = np.full(n, K, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    assert ((L >= 1) & (L <= K)).all()
    valid = j[None, :] < ((L - 1) * sub + 1)[:, None]
    return p, valid


def sample_values(waypoints, sub, lengths, mode, vs, val, known, lo, unknown=np.nan):
    """(d f32 [n, S_max], st u8 [n, S_max], valid, p): the query's answer per sample; a NaN value of status 0 is unknown.  Entries that are not valid hold
    unknown / 0xff."""
    p, valid = sample_points(waypoints, sub, lengths)
    d = np.full(valid.shape, F32(unknown), F32)
    st = np.full(valid.shape, 0xff, np.uint8)
    qd, _, qs = qref.query(p[valid], mode, vs, val, known, lo, unknown=unknown)
    nan = (qs == 0) & np.isnan(qd)
    qd[nan] = F32(unknown)
    qs[nan] = 1
    d[valid], st[valid] = qd, qs
    return d, st, valid, p


def records(d, st, valid, radius, margin, flags, unknown=np.nan):
    """the records (dict of arrays, FIELDS) and the per-sample rows (sample_dist, sample_status) from the sample values"""
    n, smax = d.shape
    radius, rm = F32(radius), F32(F32(radius) + F32(margin))
    j = np.arange(smax)[None, :]
    ok = valid & (st == 0)
    with np.errstate(invalid="ignore"):
        hit = ok & (d < radius)
    unk, outs = valid & (st == 1), valid & (st == 2)
    blocks = hit | (unk & bool(flags & UNKNOWN_BLOCKS)) | (outs & bool(flags & OUTSIDE_BLOCKS))
    first = np.where(blocks.any(1), blocks.argmax(1), -1).astype(np.int32)
    counted = valid.copy()
    if flags & STOP:
        counted &= (first[:, None] < 0) | (j <= first[:, None])
    ok &= counted
    kv = np.where(ok, (key(d).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64), NONE)
    best = kv.min(1)
    has = best != NONE
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.minimum(rm - d, F32(1024.0)).astype(F32)
        term = np.where(ok & (c > 0), np.trunc(np.nan_to_num(c * F32(1048576.0), nan=0.0, posinf=0.0, neginf=0.0)), 0.0).astype(np.int64)
    rec = {
        "n_samples": counted.sum(1).astype(np.int32), "first_stop": first,
        "n_hit": (hit & counted).sum(1).astype(np.int32), "n_unknown": (unk & counted).sum(1).astype(np.int32),
        "n_outside": (outs & counted).sum(1).astype(np.int32),
        "argmin": np.where(has, (best & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32),
        "min_dist": np.where(has, unkey((best >> np.uint64(32)).astype(np.uint32)), F32(np.inf)).astype(F32),
        "short_update": np.zeros(n, np.int32), "cost": term.sum(1),
    }
    return rec, np.where(counted, d, F32(unknown)).astype(F32), np.where(counted, st, 0xff).astype(np.uint8)


def score(waypoints, radius, margin, sub, lengths, mode, flags, vs, val, known, lo, unknown=np.nan):
    """(records, sample_dist, sample_status) of tsl_esdf_score_paths"""
    w = np.asarray(waypoints, F32)
    if w.ndim == 2:
        w = w[None]
    d, st, valid, _ = sample_values(w, sub, lengths, mode, vs, val, known, lo, unknown)
    return records(d, st, valid, radius, margin, flags, unknown)


def assert_equal(got, want, what, rows=None):
    """every record field as integers / bits; rows = (sample_dist, sample_status) pairs (got, want) when given"""
    for k in FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "min_dist":
            g, w = np.ascontiguousarray(g, F32).view(np.uint32), np.ascontiguousarray(w, F32).view(np.uint32)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} paths, first {bad[:5]}: {g[bad[:5]]} / {w[bad[:5]]}"
    if rows is not None:
        (gd, gs), (wd, ws) = rows
        assert np.array_equal(gs, ws), f"{what}: sample_status differs at {(gs != ws).sum()} samples"
        assert np.array_equal(np.ascontiguousarray(gd, F32).view(np.uint32), np.ascontiguousarray(wd, F32).view(np.uint32)), f"{what}: sample_dist differs"

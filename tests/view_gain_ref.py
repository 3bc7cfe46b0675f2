"""numpy f32 restatement of the view gain (include/taichislam_hip.h "view gain") over the class array of tests/frontier_ref.py:
vectorised over the rays of all poses, a loop over the samples, every sample evaluated (no skipping).  Every integer of the ABI must equal it."""
import numpy as np

import frontier_ref as fref

F32 = np.float32
OUT, UNKNOWN, FREE, OCC = fref.OUT, fref.UNKNOWN, fref.FREE, fref.OCC
HIT, RANGE, CUT, FRONTIER = 0, 1, 2, 0x10
RECORD_DTYPE = np.dtype({"names": ["n_unknown", "n_free", "vol_unknown", "vol_free", "n_hit", "n_range", "n_cut", "n_frontier"],
                         "formats": [np.int64, np.int64, np.int64, np.int64, np.int32, np.int32, np.int32, np.int32],
                         "offsets": [0, 8, 16, 24, 32, 36, 40, 44], "itemsize": 64})
CLAMP = F32(16777216.0)


def rnd_i(x):
    """the project's rnd_i on f32: (int)(x + copysign(0.49999997f, x)), the conversion truncating"""
    x = np.asarray(x, F32)
    return np.trunc(x + np.copysign(F32(0.49999997), x)).astype(np.int64)


def voxel_of(u):
    """rnd_i(clamp(u)): the clamp keeps the conversion inside an int, a NaN lands on it"""
    return rnd_i(np.fmax(np.fmin(np.asarray(u, F32), CLAMP), -CLAMP))


def weight(t):
    t = F32(t)
    return int(rnd_i((t * t) * F32(1024.0)))


def sample_count(t_min, t_max, dt):
    return int((F32(t_max) - F32(t_min)) / F32(dt)) + 1


def default_step(vs):
    return F32(0.75) * F32(vs)


def scaled_K(K, stride):
    """the float64 scaling of DenseTSDF.score_views: fx / stride, (cx + 0.5) / stride - 0.5"""
    k = np.asarray(K, np.float64).reshape(-1).copy()
    s = float(stride)
    k[0], k[4] = k[0] / s, k[4] / s
    k[2], k[5] = (k[2] + 0.5) / s - 0.5, (k[5] + 0.5) / s - 0.5
    return k


def ray_dirs(R, K, h, w):
    """d = R dc per ray, f32 [h * w, 3]: rows summed left to right, not normalised (k_render_view's rays)"""
    K = np.asarray(K, np.float64).reshape(-1)
    fx, fy, cx, cy = F32(K[0]), F32(K[4]), F32(K[2]), F32(K[5])
    R = np.asarray(R, np.float64).reshape(9).astype(F32)
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dc0 = (uu.ravel().astype(F32) - cx) / fx
    dc1 = (vv.ravel().astype(F32) - cy) / fy
    dc2 = np.ones(h * w, F32)
    return np.stack([(R[r * 3] * dc0 + R[r * 3 + 1] * dc1) + R[r * 3 + 2] * dc2 for r in range(3)], 1)


def brick_set(e, N, Nz):
    """bool [N / 16, N / 16, Nz / 16]: the bricks the export implies are allocated (those that hold an exported voxel)"""
    b = np.zeros((N // 16, N // 16, Nz // 16), bool)
    u = (np.asarray(e["indices"]).astype(np.int64).reshape(-1, 3) + np.array([N // 2, N // 2, Nz // 2])) >> 4
    b[u[:, 0], u[:, 1], u[:, 2]] = True
    return b


def score(c, bricks, N, Nz, vs, R, T, K, h, w, t_min, t_max, dt, unknown_run=0):
    """The result of tsl_tsdf_view_gain.  c: frontier_ref.class_array (padded), bricks: brick_set, R [n, 3, 3], T [n, 3] float64 (rounded to f32 here, once),
    K the fan's intrinsics, t_min / t_max / dt the effective f32 values.  Returns {records RECORD_DTYPE [n], ray_unknown int32 [n, h, w], ray_status u8
    [n, h, w], and the diagnostics: n_absent / n_unobserved (counted unknown samples in absent / allocated bricks), n_outside (OUTSIDE samples met before the
    ray ended), cut_in_absent (rays whose cutting sample lay in an absent brick), status (rays per status [3])}."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3)
    n = R.shape[0]
    vs, t_min, dt = F32(vs), F32(t_min), F32(dt)
    S = sample_count(t_min, t_max, dt)
    d = np.concatenate([ray_dirs(R[k], K, h, w) for k in range(n)]) if n else np.zeros((0, 3), F32)
    o = np.repeat(T.astype(F32), h * w, axis=0)
    m = d.shape[0]
    half = np.array([N // 2, N // 2, Nz // 2])
    size = np.array([N, N, Nz])
    alive = np.ones(m, bool)
    status = np.full(m, RANGE, np.uint8)
    front = np.zeros(m, bool)
    pfree = np.zeros(m, bool)
    run = np.zeros(m, np.int64)
    nu, nf, wu, wf = (np.zeros(m, np.int64) for _ in range(4))
    diag = {"n_absent": 0, "n_unobserved": 0, "n_outside": 0, "cut_in_absent": 0}
    with np.errstate(all="ignore"):
        for s in range(S):
            if not alive.any():
                break
            t = t_min + F32(s) * dt
            wgt = weight(t)
            p = o + t * d
            v = voxel_of(p / vs)
            ui = v + half
            inside = np.isfinite(p).all(1) & (ui >= 0).all(1) & (ui < size).all(1)
            uc = np.where(inside[:, None], ui, 0)
            cls = np.where(inside, c[uc[:, 0] + 1, uc[:, 1] + 1, uc[:, 2] + 1], OUT)
            absent = ~bricks[uc[:, 0] >> 4, uc[:, 1] >> 4, uc[:, 2] >> 4]
            diag["n_outside"] += int((alive & (cls == OUT)).sum())
            hit = alive & (cls == OCC)
            status[hit] = HIT
            alive &= ~hit
            fr = alive & (cls == FREE)
            nf[fr] += 1; wf[fr] += wgt; run[fr] = 0; pfree[fr] = True
            un = alive & (cls == UNKNOWN)
            front |= un & pfree
            pfree[un] = False
            nu[un] += 1; wu[un] += wgt; run[un] += 1
            diag["n_absent"] += int((un & absent).sum()); diag["n_unobserved"] += int((un & ~absent).sum())
            if unknown_run > 0:
                cut = un & (run >= unknown_run)
                status[cut] = CUT
                diag["cut_in_absent"] += int((cut & absent).sum())
                alive &= ~cut
    rec = np.zeros(n, RECORD_DTYPE)
    per = lambda a: a.reshape(n, h * w)
    rec["n_unknown"], rec["n_free"], rec["vol_unknown"], rec["vol_free"] = per(nu).sum(1), per(nf).sum(1), per(wu).sum(1), per(wf).sum(1)
    rec["n_hit"], rec["n_range"], rec["n_cut"] = (per(status) == HIT).sum(1), (per(status) == RANGE).sum(1), (per(status) == CUT).sum(1)
    rec["n_frontier"] = per(front).sum(1)
    diag["status"] = [int((status == k).sum()) for k in (HIT, RANGE, CUT)]
    out = {"records": rec, "ray_unknown": nu.astype(np.int32).reshape(n, h, w),
           "ray_status": (status | np.where(front, FRONTIER, 0).astype(np.uint8)).reshape(n, h, w)}
    out.update(diag)
    return out


def score_export(e, N, Nz, vs, R, T, K, h, w, t_min, t_max, dt=None, unknown_run=0, free_thres=None):
    """score() over an export_sparse dictionary"""
    thres = fref.surf_thres(vs) if free_thres is None else F32(free_thres)
    return score(fref.class_array(e, N, Nz, thres), brick_set(e, N, Nz), N, Nz, vs, R, T, K, h, w, t_min, t_max, default_step(vs) if dt is None else dt, unknown_run)


def volume(vol, dt, K):
    """cubic metres of a weight sum: sum(w) / 1024 * dt / (fx * fy), float64 of the f32 values"""
    K = np.asarray(K, np.float64).reshape(-1)
    return np.asarray(vol, np.float64) / 1024.0 * float(F32(dt)) / (float(F32(K[0])) * float(F32(K[4])))


def assert_equal(got, want, what=""):
    """the records of DenseTSDF.score_views (a dict of arrays per pose) and, where given, both per-ray arrays, exactly"""
    for k in RECORD_DTYPE.names:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), want["records"][k].astype(np.int64)), \
            f"{what}: {k} differs: {np.asarray(got[k]).tolist()} vs {want['records'][k].tolist()}"
    if "ray_unknown" in got:
        for k in ("ray_unknown", "ray_status"):
            bad = np.argwhere(np.asarray(got[k]) != want[k])
            assert bad.shape[0] == 0, f"{what}: {k} differs at {bad.shape[0]} rays, first {bad[0].tolist()}: {np.asarray(got[k])[tuple(bad[0])]} vs {want[k][tuple(bad[0])]}"

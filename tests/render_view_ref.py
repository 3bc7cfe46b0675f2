"""numpy float32 restatement of the view renderer (taichislam_amd/csrc/tsl_render.hip): the GPU image must equal it bit for
bit.  The map is given as a dense grid: val / known [N][N][Nz] (and col [N][N][Nz][3]) indexed by voxel index - lo.  Every sample of every ray is
evaluated: no skipping."""
import numpy as np

from esdf_query_ref import CLAMP, HALF_DOWN, lerp

F32 = np.float32
HIT, MISS, BACK, NO_NORMAL = 0, 1, 2, 0x40
CORNERS = np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)], np.int64)      # corner c = p << 2 | q << 1 | r


def grid_from_export(idx, tsdf, N, Nz, color=None):
    """(val f32, known, lo[, col f16]) dense grids of a map N x N x Nz from a sparse export: int16 indices [n, 3], f16 TSDF [n], f16 colour [n, 3]."""
    lo = np.array([-(N // 2), -(N // 2), -(Nz // 2)], np.int64)
    g = np.zeros((N, N, Nz), F32)
    k = np.zeros((N, N, Nz), bool)
    i = idx.astype(np.int64) - lo
    g[i[:, 0], i[:, 1], i[:, 2]] = np.asarray(tsdf).astype(F32)
    k[i[:, 0], i[:, 1], i[:, 2]] = True
    if color is None:
        return g, k, lo
    c = np.zeros((N, N, Nz, 3), np.float16)
    c[i[:, 0], i[:, 1], i[:, 2]] = np.asarray(color).view(np.float16).reshape(-1, 3)
    return g, k, lo, c


def sample(p, vs, val, known, lo):
    """p f32 [n, 3] -> (value f32 [n], known [n], gradient per cell f32 [n, 3]) of the trilinear interpolant; value and gradient of an unknown
    sample mean nothing."""
    shape = np.array(val.shape, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(p).all(1)
        u = p / vs
        fl = np.floor(u)
        fl = np.where(np.isnan(fl), CLAMP, np.clip(fl, -CLAMP, CLAMP)).astype(F32)       # cell_floor
        b = fl.astype(np.int64) - lo
        f = (u - fl).astype(F32)
        ins = fin & (b >= 0).all(1) & ((b + 1) < shape).all(1)
        bb = np.where(ins[:, None], b, 0)
        c = []
        kn = ins.copy()
        for cc in range(8):
            o = bb + CORNERS[cc]
            c.append(val[o[:, 0], o[:, 1], o[:, 2]])
            kn &= known[o[:, 0], o[:, 1], o[:, 2]]
        c000, c001, c010, c011, c100, c101, c110, c111 = c
        f0, f1, f2 = f[:, 0], f[:, 1], f[:, 2]
        d = lerp(lerp(lerp(c000, c100, f0), lerp(c010, c110, f0), f1), lerp(lerp(c001, c101, f0), lerp(c011, c111, f0), f1), f2)
        g0 = lerp(lerp(c100 - c000, c110 - c010, f1), lerp(c101 - c001, c111 - c011, f1), f2)
        g1 = lerp(lerp(c010 - c000, c110 - c100, f0), lerp(c011 - c001, c111 - c101, f0), f2)
        g2 = lerp(lerp(c001 - c000, c101 - c100, f0), lerp(c011 - c010, c111 - c110, f0), f1)
    return d.astype(F32), kn, np.stack([g0, g1, g2], 1).astype(F32)


def nearest_colour(p, vs, known, lo, col):
    """colour f32 [n, 3] of the voxel rnd_i(p / vs); 0 where that voxel is unknown"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = p / vs
        r = u + np.copysign(HALF_DOWN, u)
        b = np.trunc(np.clip(np.nan_to_num(r, nan=0.0), -CLAMP, CLAMP)).astype(np.int64) - lo
    ok = np.isfinite(p).all(1) & (b >= 0).all(1) & (b < np.array(known.shape, np.int64)).all(1)
    bb = np.where(ok[:, None], b, 0)
    ok &= known[bb[:, 0], bb[:, 1], bb[:, 2]]
    return np.where(ok[:, None], col[bb[:, 0], bb[:, 1], bb[:, 2]].astype(F32), F32(0))


def rays(R, K, h, w):
    """(dc, d) f32 [h * w, 3]: the pixel's direction in the camera (z = 1) and in the map frame, not normalised"""
    R = np.asarray(R, np.float64).reshape(3, 3).astype(F32)
    K = np.asarray(K, np.float64).reshape(-1)
    fx, fy, cx, cy = (F32(K[i]) for i in (0, 4, 2, 5))
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dc = np.stack([(uu.ravel().astype(F32) - cx) / fx, (vv.ravel().astype(F32) - cy) / fy, np.ones(h * w, F32)], 1)
        d = np.stack([(R[r, 0] * dc[:, 0] + R[r, 1] * dc[:, 1]) + R[r, 2] * dc[:, 2] for r in range(3)], 1)
    return dc, d.astype(F32)


def render(R, T, K, h, w, tmin, tmax, dt, vs, val, known, lo, col=None):
    """(depth f32 [h, w], normal f32 [h, w, 3], rgb f32 [h, w, 3] or None, status u8 [h, w]) of tsl_tsdf_render_view"""
    T = np.asarray(T, np.float64).reshape(3).astype(F32)
    _, d = rays(R, K, h, w)
    tmin, tmax, dt, vs = F32(tmin), F32(tmax), F32(dt), F32(vs)
    S = int((tmax - tmin) / dt) + 1
    n = h * w
    st = np.full(n, MISS, np.uint8)
    depth = np.zeros(n, F32)
    nrm = np.zeros((n, 3), F32)
    rgb = None if col is None else np.zeros((n, 3), F32)
    live = np.arange(n)                                  # rays still walking
    pk = np.zeros(n, bool)
    ps = np.zeros(n, F32)
    pt = F32(0)
    for i in range(S):
        if live.size == 0:
            break
        t = tmin + F32(i) * dt
        dl = d[live]
        with np.errstate(invalid="ignore", over="ignore"):
            s, kn, _ = sample(T[None, :] + t * dl, vs, val, known, lo)
        both = pk[live] & kn
        psl = ps[live]
        hit = both & (psl > 0) & (s <= 0)
        back = both & (psl <= 0) & (s > 0)
        if hit.any():
            hi = live[hit]
            ts = pt + dt * (psl[hit] / (psl[hit] - s[hit]))
            depth[hi] = ts
            pstar = T[None, :] + ts[:, None] * dl[hit]
            _, k2, g = sample(pstar, vs, val, known, lo)
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            ok = k2 & (ln > 0)
            nrm[hi] = np.where(ok[:, None], g / np.where(ok, ln, F32(1))[:, None], F32(0))
            st[hi] = np.where(ok, HIT, NO_NORMAL)
            if rgb is not None:
                rgb[hi] = nearest_colour(pstar, vs, known, lo, col)
        st[live[back]] = BACK
        pk[live], ps[live], pt = kn, s, t
        live = live[~(hit | back)]
    return depth.reshape(h, w), nrm.reshape(h, w, 3), None if rgb is None else rgb.reshape(h, w, 3), st.reshape(h, w)


def depth_to_mm(depth):
    return np.clip(np.rint(F32(1000.0) * np.asarray(depth, F32)), 0, 65535).astype(np.uint16)

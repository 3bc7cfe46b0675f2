"""DenseTSDF: drop-in for taichi_slam.mapping.DenseTSDF (reference taichi_slam/mapping/dense_tsdf.py:12-516)
running on hand-written HIP kernels for MI355X through include/taichislam_hip.h.

Same constructor keywords, methods and attribute names as the reference; numpy in / numpy out.  Depth images
and point clouds may also be torch CUDA tensors (their device pointer is handed to the *_dev entry points)."""
import ctypes as C
import os
import math
import time

import numpy as np

from .. import _lib
from ._sides import HOST, _is_device_tensor, _torch, _vp, device_dtypes, device_side, record_columns
from .fields import DeviceArrayField, MapFieldRef, ScalarField
from .mapping_common import BaseMap, _dptr, jet_colormap

Wmax = 1000


def _DEPTH_DTYPES(torch, _cache=[]):
    if not _cache:
        _cache.append((torch.int16, device_dtypes(torch)["u2"]))
    return _cache[0]


def _f64(a, n):
    """`a` as a C-contiguous float64 array of n values; the array itself when it already is one (the common case)."""
    if type(a) is np.ndarray and a.dtype == np.float64 and a.size == n and a.flags.c_contiguous:
        return a
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


def view_config(K=None, shape=(480, 640), t_min=None, t_max=None, step=None, skip=True):
    """The tsl_view_cfg of DenseTSDF.render_view; None = the map's default (passed as 0).  Raises ValueError for values no view can have."""
    cfg = _lib.ViewCfg()
    if K is not None:
        k = np.asarray(K, dtype=np.float64).reshape(-1)
        if k.size != 9 or not np.isfinite(k).all() or not k.any():
            raise ValueError("render_view: K must hold 9 finite values, not all zero")
        cfg.K[:] = k.tolist()
    h, w = (int(x) for x in shape)
    if h <= 0 or w <= 0:
        raise ValueError("render_view: shape must be (h, w) with h, w > 0")
    cfg.h, cfg.w = h, w
    for name, v in (("t_min", t_min), ("t_max", t_max), ("dt", step)):
        if v is None:
            continue
        v = float(v)
        if not math.isfinite(v) or (v <= 0.0 and name != "t_min") or v == 0.0:
            raise ValueError(f"render_view: {name if name != 'dt' else 'step'} must be finite" + (" and positive" if name != "t_min" else " and not 0 (0 stands for the default)"))
        setattr(cfg, name, v)
    cfg.flags = 0 if skip else 1
    return cfg


def depth_to_mm(depth):
    """A rendered depth image as the uint16 millimetre image recast_depth_to_map takes: rint(1000 * depth), 0 where there is no hit."""
    if _is_device_tensor(depth):
        torch = _torch()
        return torch.clamp(torch.round(depth * 1000.0), 0, 65535).to(torch.int32).to(_DEPTH_DTYPES(torch)[1])
    d = np.asarray(depth, dtype=np.float32)
    return np.clip(np.rint(np.float32(1000.0) * d), 0, 65535).astype(np.uint16)


def align_config(K=None, shape=(480, 640), stride=1, d_min=None, d_max=None, r_max=None, g_max=None, huber=0.0, counts_only=False):
    """The tsl_align_cfg of DenseTSDF.align_linearize / track_depth; None = the map's default (passed as 0).  The library checks the values."""
    cfg = _lib.AlignCfg()
    if K is not None:
        k = np.asarray(K, dtype=np.float64).reshape(-1)
        if k.size != 9:
            raise ValueError("align: K must hold 9 values")
        cfg.K[:] = k.tolist()
    cfg.h, cfg.w, cfg.stride = int(shape[0]), int(shape[1]), int(stride)
    for name, v in (("d_min", d_min), ("d_max", d_max), ("r_max", r_max), ("g_max", g_max), ("huber", huber)):
        if v is not None:
            setattr(cfg, name, float(v))
    cfg.flags = 1 if counts_only else 0
    return cfg


def align_points_config(stride=1, d_min=None, d_max=None, r_max=None, g_max=None, huber=0.0, counts_only=False):
    """The tsl_align_points_cfg of DenseTSDF.align_points_linearize / track_points; None = the map's default (passed as 0).  The library checks the values."""
    cfg = _lib.AlignPointsCfg()
    cfg.stride = int(stride)
    for name, v in (("d_min", d_min), ("d_max", d_max), ("r_max", r_max), ("g_max", g_max), ("huber", huber)):
        if v is not None:
            setattr(cfg, name, float(v))
    cfg.flags = 1 if counts_only else 0
    return cfg


def _point_cloud(xyz):
    """(pointer, n, keep-alive, is_device) of a cloud f32 [n, 3]: a numpy array or a torch CUDA tensor, the forms recast_pcl_to_map accepts"""
    if _is_device_tensor(xyz):
        x = xyz.reshape(-1, 3).contiguous().float()
        return C.c_void_p(x.data_ptr()), int(x.shape[0]), x, True
    x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    return _vp(x), int(x.shape[0]), x, False


def _points_f32(xyz):
    """(points f32 [n, 3] contiguous, their side) of the point queries: a numpy array, or a torch CUDA tensor that stays where it is"""
    if _is_device_tensor(xyz):
        return xyz.reshape(-1, 3).contiguous().float(), device_side(xyz.device)
    return np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3)), HOST


ALIGN_SCALE = 2.0 ** -20       # the sums of tsl_align_sums are 2^-20 fixed point


def align_sums_dict(v):
    """The 33 integers of tsl_align_sums (H[21] upper triangle row-major, b[6], e, five counts) as the dict align_linearize returns."""
    v = np.asarray(v, dtype=np.int64).reshape(-1)[:33]
    H = np.zeros((6, 6), np.int64)
    iu = np.triu_indices(6)
    H[iu] = v[:21]
    H[(iu[1], iu[0])] = v[:21]
    out = {"H": H, "b": v[21:27].copy(), "e": int(v[27]), "H_f": H.astype(np.float64) * ALIGN_SCALE, "b_f": v[21:27].astype(np.float64) * ALIGN_SCALE,
           "e_f": float(v[27]) * ALIGN_SCALE, "sums": v.copy()}
    for i, n in enumerate(("n_used", "n_gate", "n_unknown", "n_far", "n_grad")):
        out[n] = int(v[28 + i])
    return out


def align_rgbd_config(K=None, shape=(480, 640), stride=1, d_min=None, d_max=None, r_max=None, g_max=None, huber=0.0, rc_max=None, gc_max=None, huber_c=0.0,
                      counts_only=False):
    """The tsl_align_rgbd_cfg of DenseTSDF.align_rgbd_linearize / track_rgbd: align_config and the colour gates; None = the default (passed as 0)."""
    cfg = _lib.AlignRgbdCfg()
    cfg.a = align_config(K, shape, stride, d_min, d_max, r_max, g_max, huber, counts_only)
    for name, v in (("rc_max", rc_max), ("gc_max", gc_max), ("huber_c", huber_c)):
        if v is not None:
            setattr(cfg, name, float(v))
    return cfg


def align_rgbd_sums_dict(sums):
    """{"geo", "col"}: the two dicts of align_linearize from a tsl_align_rgbd_sums"""
    v = np.frombuffer(sums, dtype=np.int64)
    return {"geo": align_sums_dict(v[:33]), "col": align_sums_dict(v[33:66])}


def _rgbd_images(who, depth, rgb, host=False):
    """(depth pointer, rgb pointer, (h, w), keep-alive, side) of a uint16 [h, w] depth image and the uint8 [h, w, 3] colour image registered to it: two
    numpy arrays or two torch CUDA tensors.  host: tensors are copied to the host (a host-form call)."""
    ptr, shape, keep, on_dev = _depth_image(depth)
    if on_dev != _is_device_tensor(rgb):
        raise ValueError(f"{who}: depth and rgb must both be numpy arrays or both torch CUDA tensors")
    if on_dev and not host:
        if not (rgb.dim() == 3 and rgb.is_contiguous() and rgb.dtype == _torch().uint8 and tuple(rgb.shape) == (shape[0], shape[1], 3) and rgb.device == keep.device):
            raise ValueError(f"{who}: rgb must be a contiguous uint8 [h, w, 3] tensor on the depth image's device")
        return ptr, C.c_void_p(rgb.data_ptr()), shape, (keep, rgb), device_side(keep.device)
    if on_dev:
        keep, rgb = keep.cpu().numpy().view(np.uint16), rgb.cpu().numpy()
        ptr = _vp(keep)
    c = np.ascontiguousarray(np.asarray(rgb, dtype=np.uint8))
    if c.shape != (shape[0], shape[1], 3):
        raise ValueError(f"{who}: rgb must be uint8 [h, w, 3] with the depth image's h and w")
    return ptr, _vp(c), shape, (keep, c), HOST


REGISTER_LEVELS = ((4, 4), (2, 4), (1, 6))      # (stride, iterations) of DenseTSDF.register_submap


def register_config(stride=1, w_min=0, band=0, r_max=0, g_max=0, huber=0, counts_only=False):
    """The tsl_register_cfg of DenseTSDF.register_linearize / register_submap; 0 = the default.  The library checks the values."""
    cfg = _lib.RegisterCfg()
    cfg.stride = int(stride)
    cfg.w_min, cfg.band, cfg.r_max, cfg.g_max, cfg.huber = float(w_min), float(band), float(r_max), float(g_max), float(huber)
    cfg.flags = 1 if counts_only else 0
    return cfg


def _track_config(levels, min_step, damping, min_used):
    """The tsl_track_cfg of track_depth / register_submap; the library checks the values (a fifth level is counted, not stored)."""
    levels = [(int(a), int(b)) for a, b in levels]
    tc = _lib.TrackCfg()
    tc.n_levels = len(levels)
    for i, (st, it) in enumerate(levels[:4]):
        tc.stride[i], tc.iters[i] = st, it
    tc.min_used, tc.min_step, tc.damping = (0 if min_used is None else int(min_used)), float(min_step), float(damping)
    return tc


def _sid(sid):
    """A submap id as the library takes it: -1 = the active submap"""
    return -1 if sid is None else int(sid)


def _pose_out():
    """(R [9], T [3], their pointers): the float64 arrays a call writes its pose into"""
    Ro, To = np.empty(9, np.float64), np.empty(3, np.float64)
    return Ro, To, Ro.ctypes.data_as(_lib.dp), To.ctypes.data_as(_lib.dp)


def _track_info(rep):
    """The info dict of track_depth / register_submap from a tsl_track_report"""
    records = []
    for i in range(rep.iterations):
        it = rep.it[i]
        rec = align_sums_dict(np.frombuffer(it.sums, dtype=np.int64))
        rec.update(R=np.array(it.R[:], np.float64).reshape(3, 3), T=np.array(it.T[:], np.float64), xi=np.array(it.xi[:], np.float64))
        records.append(rec)
    return {"status": int(rep.status), "iterations": int(rep.iterations), "records": records}


_SCORE_DTYPE = np.dtype([("e", np.int64), ("n_used", np.int32), ("n_unknown", np.int32), ("n_far", np.int32), ("n_grad", np.int32)])      # tsl_register_score


def _scores_dict(a):
    """The dict of DenseTSDF.register_score from an array of tsl_register_score"""
    out = {n: a[n].astype(np.int64) for n in _SCORE_DTYPE.names}
    out["e_f"] = out["e"].astype(np.float64) * ALIGN_SCALE
    return out


def _half_counts(window, step):
    """(half-counts, steps) of three axes of DenseTSDF.register_search's lattice: round(window / step), 0 for a window of 0; a step may be a scalar.
    A step that is not positive on an axis with a window is passed on with a half-count of 1, for the library to refuse by name."""
    steps = [float(s) for s in np.broadcast_to(np.asarray(step, np.float64), (3,))]
    counts = []
    for w, s in zip(window, steps):
        w = float(w)
        if not np.isfinite(w):
            raise ValueError("register_search: a window is not finite")
        counts.append(0 if w == 0.0 else int(round(w / s)) if s > 0.0 and np.isfinite(s) else 1)
    return counts, steps


# tsl_frontier_cluster (include/taichislam_hip.h): 64 bytes at fixed offsets
FRONTIER_CLUSTER_DTYPE = np.dtype({"names": ["key", "count", "sum", "nsum", "lo", "hi"],
                                   "formats": [np.int32, np.int32, (np.int64, 3), (np.int32, 3), (np.int16, 3), (np.int16, 3)],
                                   "offsets": [0, 4, 8, 32, 44, 50], "itemsize": 64})


def frontier_cluster_geometry(clusters, voxel_scale):
    """(centroid f64 [m, 3] in metres, unit normal f64 [m, 3] pointing into the unknown; 0 where the signed face counts cancel) of frontier cluster records"""
    cnt = np.maximum(clusters["count"].astype(np.float64), 1.0)[:, None]
    centroid = clusters["sum"].astype(np.float64) / cnt * float(voxel_scale)
    ns = clusters["nsum"].astype(np.float64)
    ln = np.sqrt((ns * ns).sum(1))[:, None]
    normal = np.divide(ns, ln, out=np.zeros_like(ns), where=ln > 0)
    return centroid.reshape(-1, 3), normal.reshape(-1, 3)


NAV_FREE, NAV_OCCUPIED, NAV_UNKNOWN = 0, 1, 2          # cell classes of DenseTSDF.nav_grid (TSL_NAV_* of include/taichislam_hip.h)
NAV_UNREACHED = 0xffffffff                             # DenseTSDF.nav_field: the cell reaches no goal (TSL_NAV_UNREACHED)
TERRAIN_NO_HEIGHT, TERRAIN_NO_STAT, TERRAIN_NO_SLOPE = 32767, 65535, 0xffffffff      # DenseTSDF.nav_terrain: no support / no window statistics / no valid slope

# tsl_path_score (include/taichislam_hip.h): 40 bytes per path
PATH_SCORE_DTYPE = np.dtype({"names": ["n_samples", "first_stop", "n_hit", "n_unknown", "n_outside", "argmin", "min_dist", "short_update", "cost"],
                             "formats": [np.int32, np.int32, np.int32, np.int32, np.int32, np.int32, np.float32, np.int32, np.int64],
                             "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32], "itemsize": 40})

# tsl_traj_score (include/taichislam_hip.h): 48 bytes per trajectory
TRAJ_SCORE_DTYPE = np.dtype({"names": ["n_samples", "n_pen", "n_unknown", "n_outside", "argmin", "min_dist", "short_update", "iters_done", "cost_collision",
                                       "cost_smooth"],
                             "formats": [np.int32, np.int32, np.int32, np.int32, np.int32, np.float32, np.int32, np.int32, np.int64, np.int64],
                             "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 40], "itemsize": 48})

# tsl_view_gain (include/taichislam_hip.h): 64 bytes per pose at fixed offsets
VIEW_GAIN_DTYPE = np.dtype({"names": ["n_unknown", "n_free", "vol_unknown", "vol_free", "n_hit", "n_range", "n_cut", "n_frontier"],
                            "formats": [np.int64, np.int64, np.int64, np.int64, np.int32, np.int32, np.int32, np.int32],
                            "offsets": [0, 8, 16, 24, 32, 36, 40, 44], "itemsize": 64})


def gain_intrinsics(K, stride):
    """Row-major K [9] of the fan that takes every stride-th pixel of the image K describes: fx / stride, (cx + 0.5) / stride - 0.5, the same for y, in float64"""
    k = np.asarray(K, dtype=np.float64).reshape(-1).copy()
    if k.size != 9 or not np.isfinite(k).all() or not k.any():
        raise ValueError("score_views: K must hold 9 finite values, not all zero")
    s = float(stride)
    k[0], k[4] = k[0] / s, k[4] / s
    k[2], k[5] = (k[2] + 0.5) / s - 0.5, (k[5] + 0.5) / s - 0.5
    return k


def gain_config(K=None, shape=(60, 80), stride=1, t_min=None, t_max=None, step=None, free_thres=None, unknown_run=0, skip=True):
    """The tsl_gain_cfg of DenseTSDF.score_views; None = the map's default (passed as 0).  The fan is every stride-th pixel of the `shape` image:
    ceil(h / stride) x ceil(w / stride) rays (a stride > 1 needs K).  Raises ValueError for values no fan can have."""
    cfg = _lib.GainCfg()
    stride = int(stride)
    if stride < 1:
        raise ValueError("score_views: stride must be at least 1")
    if K is not None:
        cfg.K[:] = gain_intrinsics(K, stride).tolist()
    elif stride > 1:
        raise ValueError("score_views: a stride needs the intrinsics it scales")
    h, w = (int(x) for x in shape)
    if h <= 0 or w <= 0:
        raise ValueError("score_views: shape must be (h, w) with h, w > 0")
    cfg.h, cfg.w = -(-h // stride), -(-w // stride)
    if cfg.h > 4096 or cfg.w > 4096:
        raise ValueError("score_views: at most 4096 rays per side")
    for name, v in (("t_min", t_min), ("t_max", t_max), ("dt", step), ("free_thres", free_thres)):
        if v is None:
            continue
        v = float(v)
        if not math.isfinite(v) or (v <= 0.0 and name != "t_min") or v == 0.0:
            raise ValueError(f"score_views: {name if name != 'dt' else 'step'} must be finite" + (" and positive" if name != "t_min" else " and not 0 (0 stands for the default)"))
        setattr(cfg, name, v)
    if int(unknown_run) < 0:
        raise ValueError("score_views: unknown_run must not be negative")
    cfg.unknown_run = int(unknown_run)
    cfg.flags = 0 if skip else 1
    return cfg


def gain_poses(R, T):
    """(R float64 [n, 9], T float64 [n, 3]) of the poses of DenseTSDF.score_views: R [n, 3, 3] or [3, 3], T [n, 3] or [3]"""
    R, T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)
    if R.ndim == 2 and R.shape == (3, 3) and T.shape == (3,):
        R, T = R[None], T[None]
    if R.ndim != 3 or R.shape[1:] != (3, 3) or T.ndim != 2 or T.shape != (R.shape[0], 3):
        raise ValueError("score_views: R must be [n, 3, 3] or [3, 3] and T [n, 3] or [3], the same n")
    if R.shape[0] > 65536:
        raise ValueError("score_views: at most 65536 poses")
    if not (np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("score_views: a pose is not finite")
    return np.ascontiguousarray(R.reshape(-1, 9)), np.ascontiguousarray(T)


def gain_volume(vol, step, fx, fy):
    """Cubic metres of a weight sum of tsl_view_gain: sum(w) / 1024 * dt / (fx * fy), float64 (step, fx, fy: the f32 values the library used)"""
    return np.asarray(vol, dtype=np.float64) / 1024.0 * float(np.float32(step)) / (float(np.float32(fx)) * float(np.float32(fy)))


def frontier_view_candidates(frontiers, standoff, yaws=1, up=(0.0, 0.0, 1.0)):
    """Candidate camera poses from the `centroid` / `normal` arrays of DenseTSDF.extract_frontiers: per cluster a camera `standoff` metres back from the
    centroid, against the cluster's direction into the unknown, looking along it (optical convention: x right, y down, z forward; y as close to -up as the
    direction allows).  yaws > 1 places that many headings per cluster, the direction turned about `up` by 2 pi j / yaws, each camera still `standoff` metres
    from the centroid and looking at it.  Clusters whose normal is 0 are skipped.  Returns (R float64 [m, 3, 3], T float64 [m, 3]), cluster-major,
    camera-to-map in the frame of extract_frontiers: what DenseTSDF.score_views takes."""
    c = np.asarray(frontiers["centroid"], dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(frontiers["normal"], dtype=np.float64).reshape(-1, 3)
    yaws = int(yaws)
    if yaws < 1:
        raise ValueError("frontier_view_candidates: yaws must be at least 1")
    standoff = float(standoff)
    if not math.isfinite(standoff):
        raise ValueError("frontier_view_candidates: standoff is not finite")
    upv = np.asarray(up, dtype=np.float64).reshape(3)
    ul = np.linalg.norm(upv)
    if not ul > 0.0:
        raise ValueError("frontier_view_candidates: up must not be 0")
    upv = upv / ul
    Rs, Ts = [], []
    for ci, ni in zip(c, nrm):
        ln = np.linalg.norm(ni)
        if not ln > 0.0:
            continue
        z0 = ni / ln
        for j in range(yaws):
            if j == 0:
                z = z0
            else:                                                      # Rodrigues: z0 turned about up by 2 pi j / yaws
                a = 2.0 * math.pi * j / yaws
                z = z0 * math.cos(a) + np.cross(upv, z0) * math.sin(a) + upv * float(upv @ z0) * (1.0 - math.cos(a))
            x = np.cross(z, upv)
            if np.linalg.norm(x) < 1e-9:                               # looking along up: any horizontal axis serves
                x = np.cross(z, np.array([1.0, 0.0, 0.0]) if abs(upv[0]) < 0.9 else np.array([0.0, 1.0, 0.0]))
            x = x / np.linalg.norm(x)
            y = np.cross(z, x)
            Rs.append(np.stack([x, y, z], 1))
            Ts.append(ci - standoff * z)
    if not Rs:
        return np.zeros((0, 3, 3)), np.zeros((0, 3))
    return np.stack(Rs), np.stack(Ts)


BRICK = 16                       # voxels per brick axis: the granule of DenseTSDF.evict / restore_bricks
BRICK_VOXELS = BRICK ** 3


def metric_box_to_voxels(lo, hi, voxel_scale):
    """The inclusive voxel box of a box in metres in the map's own frame: voxel i belongs to it iff lo <= i * voxel_scale <= hi, per axis, computed in
    float64 as i_lo = ceil(lo / voxel_scale), i_hi = floor(hi / voxel_scale) and then moved by the one step the rounded quotient can be off: a face
    that is the float64 product i * voxel_scale includes voxel i (fl(fl(i * vs) / vs) is not always i: 1286 of the 10 000 i around 0 miss at 0.04).
    Returns (i_lo, i_hi) as int64 [3]; i_lo > i_hi where the box holds no voxel centre on that axis."""
    vs = float(voxel_scale)
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and vs > 0.0):
        raise ValueError("metric_box_to_voxels: the box is not finite")
    lim = float(2 ** 30)
    i_lo, i_hi = np.clip(np.ceil(lo / vs), -lim, lim), np.clip(np.floor(hi / vs), -lim, lim)
    for _ in range(2):
        i_lo = i_lo - ((i_lo - 1.0) * vs >= lo) + (i_lo * vs < lo)
        i_hi = i_hi + ((i_hi + 1.0) * vs <= hi) - (i_hi * vs > hi)
    return i_lo.astype(np.int64), i_hi.astype(np.int64)


def brick_key_ijk(keys, block_num_xy, block_num_z):
    """(sid, bi, bj, bk) of brick keys: key = sid * nb3 + (bi * nbx + bj) * nbz + bk with nbx = block_num_xy, nbz = block_num_z, nb3 = nbx * nbx * nbz.
    Brick (bi, bj, bk) holds the voxels 16 * bi - N / 2 .. 16 * bi + 15 - N / 2 of export_submap's `indices` (k with Nz / 2)."""
    k = np.asarray(keys, np.int64)
    nbx, nbz = int(block_num_xy), int(block_num_z)
    b = k % (nbx * nbx * nbz)
    return k // (nbx * nbx * nbz), b // (nbz * nbx), (b // nbz) % nbx, b % nbz


def _depth_image(depth):
    """(pointer, (h, w), keep-alive, is_device) of a uint16 millimetre image: a numpy array or a torch CUDA tensor, the forms recast_depth_to_map accepts"""
    if _is_device_tensor(depth):
        torch = _torch()
        assert depth.dim() == 2 and depth.is_contiguous() and depth.dtype in _DEPTH_DTYPES(torch), \
            "device depth must be a contiguous [h,w] uint16 tensor of millimetres (int16 = the same bits)"
        return C.c_void_p(depth.data_ptr()), (int(depth.shape[0]), int(depth.shape[1])), depth, True
    d = np.ascontiguousarray(np.asarray(depth, dtype=np.uint16))
    if d.ndim != 2:
        raise ValueError("depth must be a 2-d uint16 array")
    return _vp(d), d.shape, d, False


def _polylines(who, arr, lengths, min_len, noun, name):
    """(array f32 [n, K, 3] contiguous, lengths int32 [n] or None, side, was it one [K, 3] polyline?) of a batch of polylines -- the paths of score_paths, the
    control points of traj_* -- a numpy array or a torch device tensor; `name` and `noun`: the argument and one of its rows, in messages.  The range of
    the lengths, min_len .. K, is checked on the host side only: the device form reads no values (the library clamps them)."""
    if _is_device_tensor(arr):
        side, a = device_side(arr.device), arr
    else:
        side, a = HOST, np.asarray(arr, dtype=np.float32)
    one = a.ndim == 2
    if one:
        a = a[None]
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{who}: {name} must be [n, K, 3] or [K, 3]")
    a = np.ascontiguousarray(a) if side is HOST else a.contiguous().float()
    n, K = int(a.shape[0]), int(a.shape[1])
    ln = lengths
    if ln is not None and side is HOST:
        ln = np.asarray(ln)
        if not np.issubdtype(ln.dtype, np.integer):
            raise TypeError(f"{who}: lengths must be integers")
    elif ln is not None:
        if not _is_device_tensor(ln) or ln.dtype != _torch().int32:
            raise TypeError(f"{who}: with torch {name}, lengths must be a torch.int32 tensor on the same device")
        ln = ln.reshape(-1).contiguous()
    if ln is not None and tuple(ln.shape) != (n,):
        raise ValueError(f"{who}: one length per {noun}")
    if ln is not None and side is HOST:
        if n and (ln.min() < min_len or ln.max() > K):
            raise ValueError(f"{who}: a length outside {min_len} .. K")
        ln = np.ascontiguousarray(ln, dtype=np.int32)
    return a, ln, side, one


def _index_rows(x, widths, message, clip=None):
    """Rows of cell indices (goals, starts, cells: an array, a list or a tensor, which is read back) as int32 [S, w] with w among `widths`: the leading
    `clip` columns (None = all) clipped to int32's range, so that the library sees a far index as outside, the rest keeping their low 32 bits.  An empty
    input becomes [0, widths[-1]]; any other shape raises ValueError(message)."""
    x = x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)
    if x.size == 0:
        x = np.zeros((0, widths[-1]), np.int32)
    if x.ndim != 2 or x.shape[1] not in widths:
        raise ValueError(message)
    x = x.astype(np.int64)
    rows = np.ascontiguousarray((x & 0xffffffff).astype(np.uint32).view(np.int32))
    rows[:, :clip] = np.clip(x[:, :clip], -(1 << 31), (1 << 31) - 1)
    return rows


class DenseTSDF(BaseMap):
    _prefix = "tsl_tsdf"

    def __init__(self, map_scale=[10, 10], voxel_scale=0.05, texture_enabled=False,
                 max_disp_particles=1024 * 1024, num_voxel_per_blk_axis=16, max_ray_length=10, min_ray_length=0.3,
                 internal_voxels=10, max_submap_num=1024, is_global_map=False,
                 disp_ceiling=1.8, disp_floor=-0.3, recast_step=2, color_same_proj=True,
                 # legacy keywords still passed by tests/marching_cube_test.py:12-16 and TaichiSLAM_demo.py:147-152
                 min_occupy_thres=None, enable_esdf=None,
                 # backend knobs (not in the reference)
                 device=0, max_bricks=0, max_frame_bricks=0, max_points=0):
        super(DenseTSDF, self).__init__(voxel_scale)
        self.num_voxel_per_blk_axis = num_voxel_per_blk_axis
        self.voxel_scale = voxel_scale
        self.N = math.ceil(map_scale[0] / voxel_scale / num_voxel_per_blk_axis) * num_voxel_per_blk_axis
        self.Nz = math.ceil(map_scale[1] / voxel_scale / num_voxel_per_blk_axis) * num_voxel_per_blk_axis
        self.block_num_xy = math.ceil(map_scale[0] / voxel_scale / num_voxel_per_blk_axis)
        self.block_num_z = math.ceil(map_scale[1] / voxel_scale / num_voxel_per_blk_axis)
        self.map_size_xy = voxel_scale * self.N
        self.map_size_z = voxel_scale * self.Nz
        self.max_disp_particles = max_disp_particles
        self.enable_texture = texture_enabled
        self.max_ray_length = max_ray_length
        self.min_ray_length = min_ray_length
        self.tsdf_surface_thres = self.voxel_scale * 1.8
        self.internal_voxels = internal_voxels
        self.max_submap_num = max_submap_num
        self.is_global_map = is_global_map
        self.disp_ceiling = disp_ceiling
        self.disp_floor = disp_floor
        self.recast_step = recast_step
        self.color_same_proj = color_same_proj
        self.clear_last_TSDF_exporting = False
        self.device = device
        self._held, self._pending_inputs = [], None
        self._c_total, self._c_done, self._c_stream = C.c_int64(), C.c_int64(), C.c_void_p()
        self._ref_total, self._ref_done = C.byref(self._c_total), C.byref(self._c_done)
        self._integrate_depth_stream = self.L.tsl_tsdf_integrate_depth_stream
        self._integrate_depth_host = _lib.integrate_depth_host_fn()
        self.mem_per_voxel = 2 + 2 + 1 + 1 + (6 if texture_enabled else 0)

        cfg = _lib.TsdfCfg(float(map_scale[0]), float(map_scale[1]), float(voxel_scale), int(num_voxel_per_blk_axis),
                           float(max_ray_length), float(min_ray_length), int(internal_voxels), int(max_submap_num),
                           int(bool(is_global_map)), int(bool(texture_enabled)), float(disp_ceiling), float(disp_floor),
                           int(recast_step), int(bool(color_same_proj)), int(max_disp_particles),
                           int(max_bricks), int(max_frame_bricks), int(max_points))
        h = C.c_void_p()
        _lib.check(self.L.tsl_tsdf_create(C.byref(cfg), int(device), C.byref(h)))
        self.h = h
        n, nz = C.c_int32(), C.c_int32()
        self._call("get_dims", C.byref(n), C.byref(nz), None, None)
        assert (n.value, nz.value) == (self.N, self.Nz), "host/device extent mismatch"
        self.initialize_fields()
        if os.environ.get("TSL_ESDF_MODE"):          # developer / test aid: the form of the incremental ESDF update for handles made from here on (set_option("esdf_mode", ...))
            self.set_option("esdf_mode", int(os.environ["TSL_ESDF_MODE"]))
        print(f"TSDF map initialized blocks {self.block_num_xy}x{self.block_num_xy}x{self.block_num_z}")

    # ---- fields (dense_tsdf.py:52-106) -------------------------------------------------------------------
    def initialize_fields(self):
        self.num_TSDF_particles = ScalarField(self._get_num_particles, self._set_num_particles, "num_TSDF_particles")
        self.num_export_particles = ScalarField(lambda: 0, None, "num_export_particles")
        md = self.max_disp_particles
        self.num_export_ESDF_particles = ScalarField(lambda: self._esdf_slice_n, None, "num_export_ESDF_particles")
        self._esdf_slice_n = 0
        self.export_TSDF_xyz = DeviceArrayField(self, lambda n: self._read_exports(n)[0], md, 3, "export_TSDF_xyz",
                                                writer=lambda row, v: self._call("set_export_row", 0, row, _vp(np.ascontiguousarray(v[:3], np.float32))),
                                                dev=lambda: self._exports_dev(0))
        self.export_color = DeviceArrayField(self, lambda n: self._read_exports(n)[1], md, 3, "export_color",
                                             writer=lambda row, v: self._call("set_export_row", 1, row, _vp(np.ascontiguousarray(v[:3], np.float32))),
                                             dev=lambda: self._exports_dev(1))
        self.export_TSDF = DeviceArrayField(self, lambda n: self._read_exports(n)[2], md, 1, "export_TSDF", dev=lambda: self._exports_dev(2))
        # dense_esdf.py:112-113 (legacy module): the ESDF slice exports
        self.export_ESDF_xyz = DeviceArrayField(self, lambda n: self._read_esdf_slice(n)[0], md, 3, "export_ESDF_xyz", dev=lambda: self._esdf_slice_dev(0))
        self.export_ESDF = DeviceArrayField(self, lambda n: self._read_esdf_slice(n)[1], md, 1, "export_ESDF", dev=lambda: self._esdf_slice_dev(1))
        self.export_x = self.export_TSDF_xyz
        self.TSDF = MapFieldRef(self, "TSDF")
        self.W_TSDF = MapFieldRef(self, "W_TSDF")
        self.TSDF_observed = MapFieldRef(self, "TSDF_observed")
        self.occupy = MapFieldRef(self, "occupy")
        self.color = MapFieldRef(self, "color") if self.enable_texture else None
        self.colormap = jet_colormap()
        self._call("set_colormap", _vp(self.colormap))
        self.initialize_submap_fields(self.max_submap_num)

    def _get_num_particles(self):
        v = C.c_int32()
        self._call("num_particles", C.byref(v))
        return v.value

    def _set_num_particles(self, n):
        self._call("set_num_particles", int(n))

    def _read_exports(self, n):
        n = int(max(0, min(n, self.max_disp_particles)))
        xyz = np.empty((n, 3), np.float32)
        rgb = np.empty((n, 3), np.float32)
        val = np.empty(n, np.float32)
        self._call("read_exports", _vp(xyz), _vp(rgb), _vp(val), n)
        return xyz, rgb, val

    def _exports_dev(self, which):
        """(device pointer of export_TSDF_xyz / export_color / export_TSDF, particles of the last cvt_* call)"""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        n = C.c_int32()
        self._call("exports_dev", C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(n))
        return p[which].value, max(0, min(n.value, self.max_disp_particles))

    def _read_esdf_slice(self, n):
        n = int(max(0, min(n, self.max_disp_particles, self._esdf_slice_n)))
        xyz = np.empty((n, 3), np.float32)
        val = np.empty(n, np.float32)
        _lib.check(self.L.tsl_esdf_read_slice(self.h, _vp(xyz), _vp(val), n))
        return xyz, val

    def _esdf_slice_dev(self, which):
        p = [C.c_void_p(), C.c_void_p()]
        n = C.c_int32()
        _lib.check(self.L.tsl_esdf_slice_dev(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(n)))
        return p[which].value, max(0, min(n.value, self.max_disp_particles))

    # ---- backend knobs ---------------------------------------------------------------------------------
    def set_option(self, name, value):
        self._call("set_option", name.encode(), int(value))

    def get_option(self, name):
        v = C.c_int()
        self._call("get_option", name.encode(), C.byref(v))
        return v.value

    def enable_profiling(self, on=True, only=None):
        """HIP-event timing of the per-frame kernels; `only` = iterable of kernel ids restricts it (less host overhead)."""
        if on and only is not None:
            mask = 0
            for k in only:
                mask |= 1 << int(k)
            self._call("prof_enable", 2 * mask)
        else:
            self._call("prof_enable", int(bool(on)))

    def kernel_time(self, kernel_id):
        """(total_ms, launches) recorded by HIP events since the last query; synchronises."""
        ms, n = C.c_double(), C.c_int64()
        self._call("prof_query", int(kernel_id), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def last_frame_stats(self):
        st = _lib.FrameStats()
        self._call("last_frame_stats", C.byref(st))
        return st.as_dict()

    def memory_bytes(self):
        v = C.c_int64()
        self._call("memory_bytes", C.byref(v))
        return v.value

    def bricks_in_use(self):
        v = C.c_int32()
        self._call("bricks_in_use", C.byref(v))
        return v.value

    # ---- integration (dense_tsdf.py:157-165) -----------------------------------------------------------------
    def _adopt_device_inputs(self, points, *tensors):
        """The reference's recast_* calls are synchronous; here a frame is only queued and its kernels are enqueued later (when
        its batch is full, or when anything else needs the map) on the library's own streams.  For torch tensors the
        shim therefore (1) has the stream that will read the frame wait for the work already queued on torch's current
        stream (the tensor may still be being produced; tsl_tsdf_input_stream) and (2) keeps the tensors referenced until the
        device has read them (tsl_tsdf_frames_consumed; the library never lets the host run more than eight batches ahead,
        so at most ~72 frames are held), so a tensor the caller drops right after the call is not recycled by torch's
        caching allocator under a queued frame.  No torch stream / event queries: they cost ~100 us each while the GPU is busy."""
        import torch
        cur = torch.cuda.current_stream(tensors[0].device)
        self._call("input_stream", int(points), 1, C.c_void_p(cur.cuda_stream), C.byref(self._c_stream))
        self._pending_inputs = tensors

    def _release_device_inputs(self, force=False):
        """Drop the references to input tensors whose frames have been read (called right after the frame was queued)."""
        if force:
            self._held.clear(); self._pending_inputs = None
            return
        total, done = self._c_total, self._c_done                             # preallocated: no per-frame garbage for the cyclic GC
        self._call("frames_consumed", C.byref(total), C.byref(done))          # host-side counters only: no device query
        if self._pending_inputs is not None:
            self._held.append((total.value - 1, self._pending_inputs))       # index of the frame just queued
            self._pending_inputs = None
        while self._held and self._held[0][0] < done.value:
            self._held.pop(0)

    def sync(self):
        super().sync()
        self._release_device_inputs(force=True)

    def __del__(self):
        try:
            if self.h is not None and (self._held or self._pending_inputs is not None):
                super().sync()                                  # nothing may still read the tensors when they are released
            self._held.clear(); self._pending_inputs = None
        except Exception:
            pass
        super().__del__()

    def recast_pcl_to_map(self, R, T, xyz_array, rgb_array=None, n=None):
        """recast_pcl_to_map(R, T, xyz_array, rgb_array); the third positional `n` of the stale demo
        (TaichiSLAM_demo.py:52) is tolerated and ignored."""
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        if _is_device_tensor(xyz_array):
            import torch
            x = xyz_array.reshape(-1, 3).contiguous().float()
            ins, rgb_ptr = [x], None
            if self.enable_texture and rgb_array is not None and _is_device_tensor(rgb_array) and rgb_array.numel():
                c = rgb_array.reshape(-1, 3).contiguous().to(torch.uint8)
                assert c.shape[0] == x.shape[0], "rgb_array must hold one colour per point"
                ins.append(c)
                rgb_ptr = C.c_void_p(c.data_ptr())
            self._adopt_device_inputs(1, *ins)
            self._call("integrate_points_dev", r, t, C.c_void_p(x.data_ptr()), rgb_ptr, int(x.shape[0]))
            self._release_device_inputs()
            return
        xyz = np.ascontiguousarray(np.asarray(xyz_array, dtype=np.float32).reshape(-1, 3))
        rgb = None
        if self.enable_texture and rgb_array is not None and getattr(rgb_array, "size", 0):
            rgb = np.ascontiguousarray(np.asarray(rgb_array, dtype=np.uint8).reshape(-1, 3))
        self._call("integrate_points", r, t, _vp(xyz), _vp(rgb), int(xyz.shape[0]))

    def recast_depth_to_map(self, R, T, depthmap, texture=None):
        if _is_device_tensor(depthmap):
            # the per-frame path of a device-resident stream: ONE crossing into the library (input ordering against torch's current
            # stream + queueing + the consumed-frames count), no numpy / ctypes temporaries for poses that already are float64 arrays
            torch = _torch()
            assert depthmap.dim() == 2 and depthmap.is_contiguous() and depthmap.dtype in _DEPTH_DTYPES(torch), \
                "device depth must be a contiguous [h,w] uint16 tensor of millimetres (int16 = the same bits)"
            ins, tex_ptr, th, tw = (depthmap,), None, 0, 0
            if self.enable_texture and texture is not None and _is_device_tensor(texture):
                assert texture.dtype == torch.uint8 and texture.is_contiguous() and texture.dim() == 3 and texture.shape[2] == 3
                ins = (depthmap, texture)
                tex_ptr, th, tw = texture.data_ptr(), int(texture.shape[0]), int(texture.shape[1])
            Ra, Ta = _f64(R, 9), _f64(T, 3)
            total, done = self._c_total, self._c_done                         # preallocated: no per-frame garbage for the cyclic GC
            shape = depthmap.shape
            _lib.check(self._integrate_depth_stream(self.h, Ra.ctypes.data, Ta.ctypes.data, depthmap.data_ptr(), shape[0], shape[1],
                                                    tex_ptr, th, tw, torch.cuda.current_stream(depthmap.device).cuda_stream,
                                                    self._ref_total, self._ref_done))
            # keep the tensors referenced until the device has read them (see _adopt_device_inputs)
            held = self._held
            held.append((total.value - 1, ins))
            d = done.value
            while held and held[0][0] < d:
                held.pop(0)
            return
        if type(depthmap) is np.ndarray and depthmap.dtype == np.uint16 and depthmap.ndim == 2 and depthmap.flags.c_contiguous and (texture is None or not self.enable_texture):
            # the reference node's calling convention (taichislam_node.py:381-382: a uint16 numpy image per frame) without numpy / ctypes temporaries:
            # pointers as plain integers, one crossing into the library (the host side of a 25 k frames/s stream has ~40 us per call)
            Ra, Ta = _f64(R, 9), _f64(T, 3)
            rc = self._integrate_depth_host(self.h, Ra.ctypes.data, Ta.ctypes.data, depthmap.ctypes.data, depthmap.shape[0], depthmap.shape[1], None, 0, 0)
            if rc:
                _lib.check(rc)
            return
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        depth = np.ascontiguousarray(np.asarray(depthmap, dtype=np.uint16))
        if depth.ndim != 2:
            raise ValueError("depthmap must be a 2-d uint16 array")
        tex, th, tw = None, 0, 0
        if self.enable_texture and texture is not None and getattr(texture, "size", 0):
            tex = np.ascontiguousarray(np.asarray(texture, dtype=np.uint8))
            th, tw = tex.shape[:2]
        self._call("integrate_depth", r, t, _vp(depth), depth.shape[0], depth.shape[1], _vp(tex), th, tw)

    # north-star alias (BASELINE.json says "integrate"; the reference method is recast_depth_to_map)
    integrate = recast_depth_to_map

    # ---- fusion (dense_tsdf.py:309-318) -------------------------------------------------------------------------
    def reset(self):
        self._call("reset")

    def fuse_submaps(self, submaps):
        t = time.time()
        # the kernel reads the global map's pose table (dense_tsdf.py:286-293): make sure the handle has it
        _lib.check(self.L.tsl_tsdf_fuse_submaps(self.h, submaps.h))
        print(f"[DenseTSDF] Fuse submaps {(time.time() - t) * 1000:.1f}ms, active local: "
              f"{submaps.active_submap_id[None]} remote: {submaps.remote_submap_num[None]}")

    # multi-GPU merge (include/taichislam_hip.h; taichislam_amd.distributed.allreduce_merge drives these)
    def allreduce_merge(self, submaps, comm=None):
        """One native call: splat `submaps`, all-reduce over `comm` (taichislam_amd.distributed.Communicator, None = this rank
        alone), finalise.  Returns the bytes all-reduced."""
        n = C.c_int64()
        _lib.check(self.L.tsl_tsdf_allreduce_merge(self.h, submaps.h, comm.handle if comm is not None else None, C.byref(n)))
        return n.value

    def merge_begin(self, submaps):
        """Step 1: reset this global map, splat `submaps` into the per-brick sums; returns the touched-brick byte mask (torch CUDA)."""
        import torch
        nb = C.c_int64()
        self._call("merge_mask_bytes", C.byref(nb))
        mask = torch.zeros(nb.value, dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.current_stream(mask.device).synchronize()
        _lib.check(self.L.tsl_tsdf_merge_begin(self.h, submaps.h, C.c_void_p(mask.data_ptr()), nb.value))
        return mask

    def empty_merge_mask(self):
        """An all-zero brick mask: what a rank that could not splat its submaps contributes to the exchange (distributed.allreduce_merge)."""
        import torch
        nb = C.c_int64()
        self._call("merge_mask_bytes", C.byref(nb))
        return torch.zeros(nb.value, dtype=torch.uint8, device=f"cuda:{self.device}")

    def merge_pack(self, mask):
        """Step 2 (after the MAX all-reduce of the mask): packed sums of the union bricks, (int64 [n,4096,2], int32 [n,4096])."""
        import torch
        n = C.c_int32()
        self._call("merge_union", C.c_void_p(mask.data_ptr()), C.byref(n))
        acc = torch.empty((n.value, 4096, 2), dtype=torch.int64, device=mask.device)
        cnt = torch.empty((n.value, 4096), dtype=torch.int32, device=mask.device)
        torch.cuda.current_stream(mask.device).synchronize()
        self._call("merge_pack", C.c_void_p(acc.data_ptr()) if n.value else None, C.c_void_p(cnt.data_ptr()) if n.value else None)
        return acc, cnt

    def merge_finish(self, acc, cnt):
        """Step 3 (after the SUM all-reduce of both): write the global map."""
        self._call("merge_finish", C.c_void_p(acc.data_ptr()) if len(acc) else None, C.c_void_p(cnt.data_ptr()) if len(cnt) else None)

    MERGE_RECORD_BYTES = 4096 * 4 + 4096 + 4096 // 8          # tsl_tsdf_merge_record_bytes

    def merge_finalize_slice(self, acc, cnt):
        """Reduce-scatter form, step 3: the union bricks whose reduced sums this rank holds (int64 [k,4096,2], int32 [k,4096]) as finalised records, uint8 [k, 20992]."""
        import torch
        k = int(acc.shape[0])
        rec = torch.empty((k, self.MERGE_RECORD_BYTES), dtype=torch.uint8, device=acc.device)
        torch.cuda.current_stream(acc.device).synchronize()
        _lib.check(self.L.tsl_tsdf_merge_finalize_slice(self.h, C.c_void_p(acc.data_ptr()) if k else None, C.c_void_p(cnt.data_ptr()) if k else None, k,
                                                        C.c_void_p(rec.data_ptr()) if k else None))
        return rec

    def merge_finish_records(self, rec):
        """Reduce-scatter form, step 4 (after the all-gather): write the global map from the records of all union bricks (those behind the union are padding)."""
        import torch
        torch.cuda.current_stream(rec.device).synchronize()
        _lib.check(self.L.tsl_tsdf_merge_finish_records(self.h, C.c_void_p(rec.data_ptr()) if len(rec) else None))

    # ---- visualisation exports (dense_tsdf.py:320-404) --------------------------------------------------------------
    def cvt_occupy_to_voxels(self):
        self.cvt_TSDF_surface_to_voxels()

    def cvt_TSDF_surface_to_voxels(self):
        n = C.c_int32()
        self._call("surface_voxels", None, 0, C.byref(n))

    def cvt_TSDF_surface_to_voxels_to(self, num_TSDF_particles, max_disp_particles, export_TSDF_xyz, export_color):
        """Append this map's surface voxels to another map's export buffers (submap_mapping.py:212-213)."""
        dst = export_TSDF_xyz._owner
        n = C.c_int32()
        self._call("surface_voxels", dst.h, 1, C.byref(n))

    def cvt_TSDF_to_voxels_slice(self, z, dz=0.5, clear_last=True):
        n = C.c_int32()
        self._call("slice_voxels", float(z), float(dz), int(bool(clear_last)), C.byref(n))

    def pointcloud2(self, n=None, has_rgb=None):
        """The first `n` exported particles (default: all of the last cvt_* call) as a sensor_msgs/PointCloud2 payload -- what
        scripts/taichislam_node.py:420-425 + utils/ros_pcl_transfer.py:96-136 assemble from numpy copies -- interleaved on the device.
        See taichislam_amd.utils.ros_adapters for the message fields."""
        from ..utils import ros_adapters
        n = self.num_TSDF_particles[None] if n is None else int(n)
        n = max(0, min(n, self.max_disp_particles))
        has_rgb = self.enable_texture if has_rgb is None else bool(has_rgb)
        data = np.empty((n, 6 if has_rgb else 3), np.float32)
        self._call("pack_pointcloud2", int(has_rgb), n, _vp(data))
        return ros_adapters.pointcloud2_payload(data, has_rgb)

    def get_voxels_TSDF_surface(self):
        self.cvt_TSDF_surface_to_voxels()
        n = self.num_TSDF_particles[None]
        xyz, rgb, val = self._read_exports(n)
        return xyz, val, (rgb if self.enable_texture else None)

    def get_voxels_TSDF_slice(self, z):
        self.cvt_TSDF_to_voxels_slice(z)
        xyz, _, val = self._read_exports(self.num_TSDF_particles[None])
        return xyz, val

    def get_voxels_occupy(self):
        self.cvt_occupy_to_voxels()
        xyz, rgb, _ = self._read_exports(self.num_TSDF_particles[None])
        return xyz, rgb

    # ---- sparse export / import (dense_tsdf.py:412-515) ----------------------------------------------------------------
    def count_active(self):
        v = C.c_int64()
        self._call("count_active", C.byref(v))
        return v.value

    def to_numpy(self, data_indices, data_tsdf, data_wtsdf, data_occ, data_color):
        n = C.c_int64()
        col = data_color if (self.enable_texture and getattr(data_color, "size", 0)) else None
        self._call("export_sparse", _vp(data_indices), _vp(data_tsdf), _vp(data_wtsdf), _vp(data_occ), _vp(col),
                   int(data_tsdf.shape[0]), C.byref(n))
        return n.value

    def load_numpy(self, submap_id, data_indices, data_tsdf, data_wtsdf, data_occ, data_color):
        idx = np.ascontiguousarray(data_indices, dtype=np.int16)
        t = np.ascontiguousarray(data_tsdf, dtype=np.float16)
        w = np.ascontiguousarray(data_wtsdf, dtype=np.float16)
        occ = np.ascontiguousarray(data_occ, dtype=np.int8)
        col = None
        if self.enable_texture and data_color is not None and getattr(data_color, "size", 0):
            col = np.ascontiguousarray(data_color, dtype=np.float16)
        self._call("import_sparse", int(submap_id), _vp(idx), _vp(t), _vp(w), _vp(occ), _vp(col), int(t.shape[0]))

    def export_submap(self):
        s = time.time()
        num = self.count_active()
        indices = np.zeros((num, 3), np.int16)
        tsdf = np.zeros((num), np.float16)
        w_tsdf = np.zeros((num), np.float16)
        occupy = np.zeros((num), np.int8)
        color = np.zeros((num, 3), np.float16) if self.enable_texture else np.array([])
        self.to_numpy(indices, tsdf, w_tsdf, occupy, color)
        obj = {
            'indices': indices, 'TSDF': tsdf, 'W_TSDF': w_tsdf, 'color': color, 'occupy': occupy,
            "map_scale": [self.map_size_xy, self.map_size_z], "voxel_scale": self.voxel_scale,
            "texture_enabled": self.enable_texture, "num_voxel_per_blk_axis": self.num_voxel_per_blk_axis,
        }
        print(f"Export submap {self.active_submap_id[None]} to numpy, voxels {num / 1024:.1f}k, "
              f"time: {1000 * (time.time() - s):.1f}ms")
        return obj

    def export_occupied(self):
        """(indices int16[n,3], occupy int8[n]) of voxels with occupy != 0 (backend extra, used by parity tests)."""
        n = C.c_int64()
        self._call("export_occupied", None, None, 0, C.byref(n))
        idx = np.zeros((n.value, 3), np.int16)
        occ = np.zeros(n.value, np.int8)
        self._call("export_occupied", _vp(idx), _vp(occ), n.value, C.byref(n))
        return idx, occ

    # ---- evict / snapshot / restore bricks (tsl_evict.hip, DESIGN.md "Evict and restore bricks") ---------------------------------
    def brick_keys(self, device=False):
        """The keys of the bricks in use, int32 [bricks_in_use()], in pool order (brick_key_ijk decodes them)."""
        side = device_side(self.device) if device else HOST
        n = C.c_int32()
        self._call("brick_keys", None, 0, C.byref(n))
        keys = side.out(n.value, "i4")
        if n.value:
            side.call(self.L.tsl_tsdf_brick_keys, self.L.tsl_tsdf_brick_keys_dev, self.h, side.ptr(keys), n.value, C.byref(n))
        return keys

    def brick_key_ijk(self, keys):
        """(sid, bi, bj, bk) of brick keys of this map (the module-level brick_key_ijk with this map's brick counts)"""
        return brick_key_ijk(keys, self.block_num_xy, self.block_num_z)

    def _payload_head(self):
        return {"N": int(self.N), "Nz": int(self.Nz), "brick": BRICK, "texture_enabled": bool(self.enable_texture), "voxel_scale": float(self.voxel_scale)}

    def _evict(self, who, release, keep_box, clear_box, keys, sid, metres, payload, device):
        if sum(r is not None for r in (keep_box, clear_box, keys)) != 1:
            raise ValueError(f"{who}: give exactly one of keep_box, clear_box and keys")
        side = device_side(self.device) if device else HOST
        cfg = _lib.EvictCfg()
        cfg.release = 1 if release else 0
        kin, nk = None, 0
        if keys is not None:
            cfg.rule, cfg.sid = _lib.EVICT_KEYS, -1
            if _is_device_tensor(keys):
                if not device:
                    raise ValueError(f"{who}: keys on the device need device=True")
                kin = keys.reshape(-1).to(_torch().int32).contiguous()
            else:
                k = np.asarray(keys).reshape(-1)
                if k.size and (k.dtype.kind not in "iu" or int(k.min()) < -2 ** 31 or int(k.max()) >= 2 ** 31):
                    raise ValueError(f"{who}: keys must be 32-bit integers")
                kin = side.put(np.ascontiguousarray(k, np.int32))
            nk = int(kin.shape[0])
        else:
            lo, hi = keep_box if keep_box is not None else clear_box
            if metres:
                lo, hi = metric_box_to_voxels(lo, hi, self.voxel_scale)
            lo, hi = np.asarray(lo).reshape(3), np.asarray(hi).reshape(3)
            if (lo > hi).any():
                raise ValueError(f"{who}: the box is empty (lo > hi)")
            lim = 2 ** 30
            cfg.rule = _lib.EVICT_KEEP_BOX if keep_box is not None else _lib.EVICT_CLEAR_BOX
            cfg.sid = int(self.active_submap_id[None]) if sid is None else int(sid)
            for a in range(3):
                cfg.lo[a], cfg.hi[a] = int(max(-lim, min(lim, lo[a]))), int(max(-lim, min(lim, hi[a])))
        st = _lib.EvictStats()
        fn, fn_dev = self.L.tsl_tsdf_evict, self.L.tsl_tsdf_evict_dev
        out = self._payload_head()
        if payload:
            # the selection is counted first (all planes null, nothing released): the planes then hold exactly its rows
            count = _lib.EvictCfg.from_buffer_copy(cfg)
            count.release = 0
            side.call(fn, fn_dev, self.h, C.byref(count), side.ptr(kin), nk, None, None, None, None, None, 0, C.byref(st))
            n = st.selected
            out["keys"], out["tw"] = side.out(n, "i4"), side.out((n, BRICK_VOXELS), "u4")
            out["obs"], out["occ"] = side.out((n, BRICK_VOXELS), "i1"), side.out((n, BRICK_VOXELS), "i1")
            if self.enable_texture:
                out["col"] = side.out((n, BRICK_VOXELS, 4), "u2")
            if n:
                side.call(fn, fn_dev, self.h, C.byref(cfg), side.ptr(kin), nk, *(side.ptr(out[k]) if n else None for k in ("keys", "tw", "obs", "occ")),
                          side.ptr(out["col"]) if n and self.enable_texture else None, n, C.byref(st))
        else:
            side.call(fn, fn_dev, self.h, C.byref(cfg), side.ptr(kin), nk, None, None, None, None, None, 0, C.byref(st))
        out["stats"] = st.as_dict()
        return out

    def evict(self, keep_box=None, clear_box=None, keys=None, sid=None, metres=False, payload=True, device=False):
        """Give bricks back to the pool and return their content.  Exactly one rule selects 16^3 bricks: keep_box = (lo, hi) evicts every brick of the
        chosen slots whose voxels do not intersect the inclusive box, clear_box = (lo, hi) every brick that lies wholly inside it (a brick the box cuts
        through stays under both), keys = an int32 list of brick keys (duplicates count once, a key without a brick counts in stats `missing`, a key out
        of range is an error).  Boxes are voxel indices, the `indices` of export_submap, or with metres=True metres in the map's own frame
        (metric_box_to_voxels).  sid: the submap slot of a box rule, None = the active submap, -1 = every slot.  Returns the payload -- `keys` int32 [n]
        ascending, `tw` uint32 [n, 4096] (TSDF f16 bits | weight f16 bits << 16), `obs` int8 [n, 4096], `occ` int8 [n, 4096], on textured maps `col`
        uint16 [n, 4096, 4], the geometry it belongs to -- and `stats` (selected, missing, moved, bricks_before, bricks_after).  Voxel (li, lj, lk) of a
        brick is element li * 256 + lj * 16 + lk of its row.  payload=False discards the content (clearing a region).  device=True returns torch tensors on
        the map's device, ordered with torch.cuda.current_stream; otherwise numpy arrays, a dict mapping.wire.pack takes as it is.  Queued frames are
        integrated first; with a brick evicted the ESDF needs an update_esdf before the next query."""
        return self._evict("evict", True, keep_box, clear_box, keys, sid, metres, payload, device)

    def snapshot_bricks(self, keep_box=None, clear_box=None, keys=None, sid=None, metres=False, payload=True, device=False):
        """The payload evict() would return for the same selection; the map is untouched.  No rule at all = every brick of the map."""
        if keep_box is None and clear_box is None and keys is None:
            h = 2 ** 29
            clear_box, sid = ((-h, -h, -h), (h, h, h)), -1
        return self._evict("snapshot_bricks", False, keep_box, clear_box, keys, sid, metres, payload, device)

    def restore_bricks(self, payload, sid=None, on_conflict="skip"):
        """Put the rows of a payload (evict / snapshot_bricks, of this or another map of the same N, Nz, brick size and texture setting; numpy arrays or
        torch tensors on this map's device) back into the map: every row under its own key, or with sid all rows into that submap slot.  A row whose
        brick exists again is dropped and counted (on_conflict="skip") or replaces the brick ("overwrite").  All or nothing: when the new bricks do not
        fit max_bricks the call raises and the map is unchanged.  Returns the stats (restored, skipped, bricks_before, bricks_after)."""
        if on_conflict not in ("skip", "overwrite"):
            raise ValueError('restore_bricks: on_conflict must be "skip" or "overwrite"')
        head = self._payload_head()
        for k in ("N", "Nz", "brick", "texture_enabled"):
            if k not in payload or payload[k] != head[k]:
                raise ValueError(f"restore_bricks: the payload's {k} is {payload.get(k)!r}, this map's is {head[k]!r}")
        names = ("keys", "tw", "obs", "occ") + (("col",) if self.enable_texture else ())
        kinds = {"keys": "i4", "tw": "u4", "obs": "i1", "occ": "i1", "col": "u2"}
        device = _is_device_tensor(payload["keys"])
        side = device_side(self.device) if device else HOST
        n = int(payload["keys"].shape[0])
        planes = {}
        for k in names:
            a = payload[k]
            if _is_device_tensor(a) != device:
                raise ValueError("restore_bricks: the payload mixes host and device arrays")
            shape = (n,) if k == "keys" else (n, BRICK_VOXELS, 4) if k == "col" else (n, BRICK_VOXELS)
            if tuple(a.shape) != shape:
                raise ValueError(f"restore_bricks: {k} has shape {tuple(a.shape)}, not {shape}")
            if device:
                if a.dtype != side._kinds[kinds[k]] or a.device.index != side.dev.index:
                    raise ValueError(f"restore_bricks: {k} must be {side._kinds[kinds[k]]} on this map's device")
                planes[k] = a.contiguous()
            else:
                planes[k] = np.ascontiguousarray(a, np.dtype(kinds[k]))
        st = _lib.EvictStats()
        if n:
            side.call(self.L.tsl_tsdf_restore_bricks, self.L.tsl_tsdf_restore_bricks_dev, self.h, *(side.ptr(planes[k]) for k in ("keys", "tw", "obs", "occ")),
                      side.ptr(planes.get("col")), n, -1 if sid is None else int(sid), _lib.RESTORE_OVERWRITE if on_conflict == "overwrite" else _lib.RESTORE_SKIP,
                      C.byref(st))
        else:
            st.bricks_before = st.bricks_after = self.bricks_in_use()
        return st.as_dict()

    def saveMap(self, filename):
        np.save(filename, self.export_submap())

    @staticmethod
    def loadMap(filename, **backend_opts):
        obj = np.load(filename, allow_pickle=True).item()
        mapping = DenseTSDF(map_scale=obj['map_scale'], voxel_scale=obj['voxel_scale'],
                            texture_enabled=obj['texture_enabled'],
                            num_voxel_per_blk_axis=obj['num_voxel_per_blk_axis'], is_global_map=True, **backend_opts)
        mapping.load_numpy(0, obj['indices'], obj['TSDF'], obj['W_TSDF'], obj['occupy'], obj['color'])
        print(f"[SubmapMapping] Loaded {obj['TSDF'].shape[0]} voxels from {filename}")
        return mapping

    def input_remote_submap(self, submap):
        # remote submaps are stored from the top of the submap axis downwards (dense_tsdf.py:500-515)
        self.remote_submap_num[None] = self.remote_submap_num[None] + 1
        idx = self.max_submap_num - self.remote_submap_num[None]
        R, T = submap['pose']
        color = submap['color'] if self.enable_texture else np.array([])
        self.load_numpy(idx, submap['indices'], submap['TSDF'], submap['W_TSDF'], submap['occupy'], color)
        self.set_base_pose_submap(idx, R, T)
        return idx

    # ---- batched map queries (mapping_common.py:165-204; the reference exposes them as ti.funcs for TopoGraphGen) ----
    def _query_points(self, mode, xyz, param=0):
        # device tensors in, device tensor out, nothing waited for: the query runs on the map's stream behind every queued frame and
        # torch's current stream is ordered after it (tsl_tsdf_query_points_dev)
        x, side = _points_f32(xyz)
        out = side.out(x.shape[0], "u1")
        side.call(self.L.tsl_tsdf_query_points, self.L.tsl_tsdf_query_points_dev, self.h, mode, int(param), side.ptr(x), x.shape[0], side.ptr(out))
        return out.astype(bool) if side is HOST else out.bool()

    def is_pos_occupy(self, xyz):
        return self._query_points(0, xyz)

    def is_pos_unobserved(self, xyz):
        return self._query_points(1, xyz)

    def is_near_pos_occupy(self, xyz, voxel):
        return self._query_points(2, xyz, voxel)

    def raycast(self, pos, dir, max_dist):
        """Batched BaseMap.raycast: returns (hit bool[n], end xyz f32[n,3], length f32[n]); torch CUDA tensors in -> torch CUDA tensors
        out, asynchronously (the planner's 64-128 rays per node expansion, topo_graph.py:444-507, without a host round trip)."""
        (p, side), (d, side_d) = _points_f32(pos), _points_f32(dir)
        assert p.shape == d.shape and (side is HOST) == (side_d is HOST)
        n = p.shape[0]
        hit, end, ln = side.out(n, "u1"), side.out((n, 3), "f4"), side.out(n, "f4")
        side.call(self.L.tsl_tsdf_query_raycast, self.L.tsl_tsdf_query_raycast_dev, self.h, side.ptr(p), side.ptr(d), float(max_dist), n, side.ptr(hit),
                  side.ptr(end), side.ptr(ln))
        return (hit.astype(bool) if side is HOST else hit.bool()), end, ln

    # ---- view rendering (tsl_render.hip; beside BaseMap.raycast, mapping_common.py:165-178) ----------
    def render_view(self, R, T, K=None, shape=(480, 640), t_min=None, t_max=None, step=None, normals=True, colors=None, device=False, skip=True):
        """What a camera at the camera-to-map pose (R, T) -- in the frame of is_pos_occupy / raycast: the active submap's, submap 0 on a global
        map -- would see of the TSDF: returns (depth f32 [h, w], normal f32 [h, w, 3] or None, rgb f32 [h, w, 3] or None, status u8 [h, w]).
        depth is the optical-axis depth of the first front face along the pixel's ray (the unit of the depth images; 0 where there is none), found
        by sampling the trilinear interpolant of the TSDF every `step` metres of depth between t_min and t_max and refining the zero crossing
        linearly; the normal is the normalised gradient of the interpolant there (map frame, pointing into free space), rgb the colour of the
        nearest voxel.  status: 0 hit, 1 miss, 2 the ray met a surface from behind (depth 0), | 0x40 a hit without a normal (it touches
        unobserved voxels).  K: row-major intrinsics of the view (default: the map's depth intrinsics); t_min / t_max default to the map's
        min / max_ray_length, step to 0.75 voxel; colors=None means "if the map is textured".  skip=False evaluates every sample instead of
        jumping over unallocated bricks: the same image bit for bit, slower (the A/B switch).  device=True returns torch tensors on the map's
        device, asynchronously, ordered with torch.cuda.current_stream (tsl_tsdf_render_view_dev); otherwise numpy arrays."""
        cfg = view_config(K, shape, t_min, t_max, step, skip)
        colors = bool(self.enable_texture) if colors is None else bool(colors)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        h, w = cfg.h, cfg.w
        side = device_side(self.device) if device else HOST
        depth = side.out((h, w), "f4")
        normal = side.out((h, w, 3), "f4") if normals else None
        rgb = side.out((h, w, 3), "f4") if colors else None
        status = side.out((h, w), "u1")
        side.call(self.L.tsl_tsdf_render_view, self.L.tsl_tsdf_render_view_dev, self.h, r, t, C.byref(cfg), side.ptr(depth), side.ptr(normal), side.ptr(rgb),
                  side.ptr(status))
        return depth, normal, rgb, status

    # ---- view gain (tsl_view_gain.hip) --------------------------------------------------------------
    def score_views(self, R, T, K=None, shape=(60, 80), stride=1, t_min=None, t_max=None, step=None, free_thres=None, unknown_run=0, rays=False,
                    device=False, skip=True):
        """Scores candidate camera poses by the unobserved space a sensor there would see: R [n, 3, 3] (or [3, 3]), T [n, 3] (or [3]) camera-to-map in the
        frame of is_pos_occupy / render_view.  Per pose a pinhole fan -- every stride-th pixel of the `shape` image with intrinsics K (default: the map's
        depth intrinsics) -- is walked every `step` metres of depth (default 0.75 voxel) from t_min to t_max (default: the map's min / max_ray_length);
        a sample has the class extract_frontiers gives its nearest voxel (free_thres as there), samples outside the volume count nothing, the first
        occupied sample ends the ray; with unknown_run > 0 so do that many unknown samples in a row (unknown space may hide a wall).  Returns a dict of
        arrays per pose: n_unknown, n_free (samples), vol_unknown, vol_free (the same weighted by rnd(t^2 * 1024)), n_hit, n_range, n_cut (rays per
        status), n_frontier (rays on which an unknown sample follows a free one), and unknown_volume / free_volume, float64 cubic metres
        (vol / 1024 * step / (fx * fy)); with rays=True also ray_unknown int32 [n, h, w] and ray_status u8 [n, h, w] (0 hit, 1 range, 2 cut, | 0x10
        through a frontier).  Every integer is exact and independent of the schedule.  skip=False evaluates every sample instead of jumping over the
        outside and over unallocated bricks: the same result, slower (the A/B switch).  device=True returns torch tensors on the map's device,
        asynchronously, ordered with torch.cuda.current_stream: `records` int32 [n, 16] (the tsl_view_gain records) and the per-ray arrays."""
        Kuse = K
        if K is None and self.K_cam_dep is not None:
            Kuse = self.K_cam_dep                                    # the values the library holds: passed so that the stride can scale them
        if Kuse is None:
            raise ValueError("score_views: the map has no depth intrinsics; pass K")
        cfg = gain_config(Kuse, shape, stride, t_min, t_max, step, free_thres, unknown_run, skip)
        Rn, Tn = gain_poses(R, T)
        n, h, w = Rn.shape[0], cfg.h, cfg.w
        r, t = Rn.ctypes.data_as(_lib.dp), Tn.ctypes.data_as(_lib.dp)
        side = device_side(self.device) if device else HOST
        rec = side.out((n, 16), "i4", zero=True)
        ru = side.out((n, h, w), "i4", zero=True) if rays else None
        rs = side.out((n, h, w), "u1", zero=True) if rays else None
        if n or side is HOST:                                        # the device form of an empty batch is its zeroed tensors
            side.call(self.L.tsl_tsdf_view_gain, self.L.tsl_tsdf_view_gain_dev, self.h, r, t, n, C.byref(cfg), side.ptr(rec), side.ptr(ru), side.ptr(rs))
        if side is HOST:
            rec = rec.view(VIEW_GAIN_DTYPE).reshape(n)
            out = {k: rec[k].copy() for k in VIEW_GAIN_DTYPE.names}
            dt = np.float32(cfg.dt) if cfg.dt != 0.0 else np.float32(0.75) * np.float32(self.voxel_scale)
            out["unknown_volume"] = gain_volume(out["vol_unknown"], dt, cfg.K[0], cfg.K[4])
            out["free_volume"] = gain_volume(out["vol_free"], dt, cfg.K[0], cfg.K[4])
        else:
            out = {"records": rec}
        if rays:
            out["ray_unknown"], out["ray_status"] = ru, rs
        return out

    # ---- exploration frontiers (tsl_frontier.hip) ---------------------------------------------------
    def extract_frontiers(self, free_thres=None, z_range=None, min_unknown=1, connectivity=26, min_cluster=1, clear_of_occupied=False, device=False):
        """Where the known map ends: the free voxels of the submap the point queries read (the active one; submap 0 on a global map) that have at
        least `min_unknown` of their six face neighbours unknown, grouped into connected clusters (connectivity 6, 18 or 26) -- the targets of an
        exploration planner.  A voxel is unknown when its brick is absent or it was never observed, occupied when its TSDF is below `free_thres`
        (default: the surface threshold of is_pos_occupy), free otherwise; the space outside the volume is not unknown.  z_range = (z0, z1) in metres
        keeps the voxel layers with z0 <= k * voxel <= z1; clear_of_occupied drops voxels with an occupied voxel among their 26 neighbours; clusters
        of fewer than min_cluster voxels are dropped with their voxels.  Returns a dict: `indices` int16 [n, 3], `xyz` f32 [n, 3] = indices * voxel
        (the frame of is_pos_occupy), `mask` u8 [n] (bit 0 .. 5: the neighbour at -x, +x, -y, +y, -z, +z is unknown), `cluster` int32 [n] (row of
        `clusters`), voxels sorted by key ((i + N / 2) * N + j + N / 2) * Nz + k + Nz / 2; `clusters`, a structured array (FRONTIER_CLUSTER_DTYPE:
        key = least voxel key, count, sum int64 [3], nsum int32 [3], lo / hi int16 [3]) sorted by key; `centroid` f64 [m, 3] = sum / count * voxel
        and `normal` f64 [m, 3] = nsum / |nsum| (0 where nsum is 0), the direction from the cluster into the unknown.  device=True returns indices,
        xyz, mask and cluster as torch tensors on the map's device -- zero-copy views of the handle's result buffers, valid until the next call, ordered
        with torch.cuda.current_stream -- and `clusters_dev`, the records as int32 [m, 16]; clusters, centroid and normal stay numpy (they are small)."""
        cfg = _lib.FrontierCfg()
        cfg.free_thres = 0.0 if free_thres is None else float(free_thres)
        if free_thres is not None and not float(free_thres) > 0.0:
            raise ValueError("extract_frontiers: free_thres must be positive")
        cfg.k_min, cfg.k_max = 1, 0                                      # no height limit
        if z_range is not None:
            z0, z1 = float(z_range[0]), float(z_range[1])
            if not (math.isfinite(z0) and math.isfinite(z1)):
                raise ValueError("extract_frontiers: z_range is not finite")
            k0 = max(-32768, min(32767, math.ceil(z0 / float(self.voxel_scale))))
            k1 = max(-32768, min(32767, math.floor(z1 / float(self.voxel_scale))))
            if k0 > k1:
                raise ValueError("extract_frontiers: z_range holds no voxel layer")
            cfg.k_min, cfg.k_max = k0, k1
        cfg.min_unknown, cfg.connectivity, cfg.min_cluster = int(min_unknown), int(connectivity), int(min_cluster)
        cfg.flags = 1 if clear_of_occupied else 0
        nv, nc = C.c_int32(), C.c_int32()
        vs = np.float32(self.voxel_scale)
        if device:
            torch = _torch()
            from .fields import device_view
            dev = torch.device(f"cuda:{self.device}")
            p = [C.c_void_p() for _ in range(4)]
            _lib.check(self.L.tsl_tsdf_frontier_dev(self.h, C.byref(cfg), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3]), C.byref(nv), C.byref(nc),
                                                    torch.cuda.current_stream(dev).cuda_stream))
            n, m = nv.value, nc.value
            if n:
                idx = device_view(p[0].value, (n, 3), "<i2", self, self.device); mask = device_view(p[1].value, (n,), "|u1", self, self.device)
                cl = device_view(p[2].value, (n,), "<i4", self, self.device); cdev = device_view(p[3].value, (m, 16), "<i4", self, self.device)
            else:
                idx = torch.empty((0, 3), dtype=torch.int16, device=dev); mask = torch.empty(0, dtype=torch.uint8, device=dev)
                cl = torch.empty(0, dtype=torch.int32, device=dev); cdev = torch.empty((0, 16), dtype=torch.int32, device=dev)
            out = {"indices": idx, "xyz": idx.float() * float(vs), "mask": mask, "cluster": cl, "clusters_dev": cdev}
            clusters = np.zeros(m, FRONTIER_CLUSTER_DTYPE)
            _lib.check(self.L.tsl_tsdf_frontier_read(self.h, None, None, None, _vp(clusters), 0, m))
        else:
            _lib.check(self.L.tsl_tsdf_frontier_extract(self.h, C.byref(cfg), C.byref(nv), C.byref(nc)))
            n, m = nv.value, nc.value
            idx = np.zeros((n, 3), np.int16); mask = np.zeros(n, np.uint8); cl = np.zeros(n, np.int32)
            clusters = np.zeros(m, FRONTIER_CLUSTER_DTYPE)
            _lib.check(self.L.tsl_tsdf_frontier_read(self.h, _vp(idx), _vp(mask), _vp(cl), _vp(clusters), n, m))
            out = {"indices": idx, "xyz": idx.astype(np.float32) * vs, "mask": mask, "cluster": cl}
        out["clusters"] = clusters
        out["centroid"], out["normal"] = frontier_cluster_geometry(clusters, float(self.voxel_scale))
        return out

    # ---- navigation grids (tsl_nav_grid.hip) ---------------------------------------------------------
    def _nav_bands(self, bands, z_range):
        """[(k_min, k_max)] of nav_grid: `bands` as given (voxel layers; the library checks them), else z_range -- one (z0, z1) in metres or a list of them --
        turned into layers the way extract_frontiers does and clamped to the volume, else the whole height"""
        if bands is not None and z_range is not None:
            raise ValueError("nav_grid: give bands or z_range, not both")
        lo, hi = -(self.Nz // 2), self.Nz // 2 - 1
        if bands is not None:
            out = [(int(a), int(b)) for a, b in bands]
        elif z_range is None:
            out = [(lo, hi)]
        else:
            zr = list(z_range)
            if len(zr) == 2 and not hasattr(zr[0], "__len__"):
                zr = [zr]
            out = []
            for z in zr:
                z0, z1 = float(z[0]), float(z[1])
                if not (math.isfinite(z0) and math.isfinite(z1)):
                    raise ValueError("nav_grid: z_range is not finite")
                k0 = max(lo, math.ceil(z0 / float(self.voxel_scale)))
                k1 = min(hi, math.floor(z1 / float(self.voxel_scale)))
                if k0 > k1:
                    raise ValueError("nav_grid: a z_range holds no voxel layer of the volume")
                out.append((k0, k1))
        if not 1 <= len(out) <= 16:
            raise ValueError("nav_grid: 1 .. 16 bands")
        return out

    @staticmethod
    def _nav_head(who, cfg, bl, free_thres, R, unknown_is_obstacle, wall_is_obstacle, cost_unknown, lut):
        """Fills what NavCfg and NavTerrainCfg share -- the bands, free_thres, the radius in voxels, the flags, cost_unknown -- and returns the lut as the
        u8 array of R * R + 2 costs the library reads, or None"""
        if free_thres is not None and not float(free_thres) > 0.0:
            raise ValueError(f"{who}: free_thres must be positive")
        cfg.n_bands = len(bl)
        for b, (k0, k1) in enumerate(bl):
            cfg.k_min[b], cfg.k_max[b] = k0, k1
        cfg.free_thres = 0.0 if free_thres is None else float(free_thres)
        cfg.radius = R
        cfg.flags = (1 if unknown_is_obstacle else 0) | (2 if wall_is_obstacle else 0)
        cfg.cost_unknown = int(cost_unknown) & 0xff
        if lut is not None:
            lut = np.ascontiguousarray(np.asarray(lut, dtype=np.uint8).reshape(-1))
            if lut.size != R * R + 2:
                raise ValueError(f"{who}: lut must hold R * R + 2 = {R * R + 2} entries, not {lut.size}")
        return lut

    def nav_grid(self, bands=None, z_range=None, radius=1.0, free_thres=None, min_occ=1, min_free=1, max_unknown=None, unknown_is_obstacle=False,
                 wall_is_obstacle=False, lut=None, cost_unknown=255, counts=False, span=False, device=False):
        """Height bands of the submap the point queries read (the active one; submap 0 on a global map) as 2-D navigation grids: what a 2-D planner or a
        costmap layer consumes.  bands: [(k_min, k_max)] voxel layers, both ends inclusive, or z_range: (z0, z1) in metres or a list of them (the layers
        with z0 <= k * voxel <= z1, clamped to the volume; an empty band raises); neither = the whole height; at most 16.  Per band and (x, y) column the
        voxels are classed as extract_frontiers does (free_thres as there; an observed NaN counts as unknown) and counted; the cell is occupied
        (NAV_OCCUPIED = 1) when at least min_occ are occupied, else free (NAV_FREE = 0) when at least min_free are free and at most max_unknown unknown
        (None = no limit), else unknown (NAV_UNKNOWN = 2).  d2 is the exact squared distance in voxels to the nearest obstacle cell -- occupied cells,
        with unknown_is_obstacle the unknown ones too, with wall_is_obstacle the positions just outside the grid -- up to `radius` (metres, rounded to
        voxels, at most 254 voxels): R * R + 1 beyond it.  lut: a u8 table of R * R + 2 costs (utils.inflation_lut); cost = cost_unknown for an unknown
        cell, else lut[d2].  Returns a dict: `cls` u8 [B, N, N], `d2` uint16 [B, N, N], with lut `cost` u8 [B, N, N], with counts=True `counts` uint16
        [B, N, N, 3] (occupied, free, unknown voxels), with span=True `span` int16 [B, N, N, 2] (lowest / highest occupied layer; 32767 / -32768 when
        none) -- every plane indexed [b][i + N / 2][j + N / 2] -- and `voxel`, `origin_xy` = (-(N / 2) - 0.5) * voxel (the corner of cell 0, 0),
        `bands`, `radius_vox`.  device=True returns the planes as torch tensors on the map's device, asynchronously, ordered with
        torch.cuda.current_stream (tsl_tsdf_nav_grid_dev); otherwise numpy arrays."""
        bl = self._nav_bands(bands, z_range)
        radius = float(radius)
        if not math.isfinite(radius) or radius < 0.0:
            raise ValueError("nav_grid: radius must be finite and not negative")
        R = int(round(radius / float(self.voxel_scale)))
        cfg = _lib.NavCfg()
        lut = self._nav_head("nav_grid", cfg, bl, free_thres, R, unknown_is_obstacle, wall_is_obstacle, cost_unknown, lut)
        cfg.min_occ, cfg.min_free = int(min_occ), int(min_free)
        cfg.max_unknown = -1 if max_unknown is None else max(0, int(max_unknown))
        B, N = len(bl), self.N
        out = {"voxel": float(self.voxel_scale), "origin_xy": (-(N // 2) - 0.5) * float(self.voxel_scale), "bands": bl, "radius_vox": R}
        side = device_side(self.device) if device else HOST
        cls, d2 = side.out((B, N, N), "u1"), side.out((B, N, N), "u2")
        cost = side.out((B, N, N), "u1") if lut is not None else None
        cnt = side.out((B, N, N, 3), "u2") if counts else None
        sp = side.out((B, N, N, 2), "i2") if span else None
        lut = None if lut is None else side.put(lut)
        side.call(self.L.tsl_tsdf_nav_grid, self.L.tsl_tsdf_nav_grid_dev, self.h, C.byref(cfg), side.ptr(lut), side.ptr(cls), side.ptr(d2), side.ptr(cost),
                  side.ptr(cnt), side.ptr(sp))
        out["cls"], out["d2"] = cls, d2
        for k, v in (("cost", cost), ("counts", cnt), ("span", sp)):
            if v is not None:
                out[k] = v
        return out

    # ---- cost-to-go fields and paths: the one body of nav_field / nav_field3d and of nav_paths / nav_paths3d ----------------------
    def _cost_u8(self, who, cost, device):
        """A uint8 cost array, or the dict that holds one, on the host or on the device -> (contiguous array or tensor, its side): a tensor, or
        device=True, gives the device side, on the map's device"""
        if isinstance(cost, dict):
            cost = cost["cost"]
        on_dev = hasattr(cost, "is_cuda")
        if not (on_dev or device):
            cost = np.asarray(cost)
            if cost.dtype != np.uint8:
                raise ValueError(f"{who}: cost must be uint8")
            return np.ascontiguousarray(cost), HOST
        torch, side = _torch(), device_side(self.device)
        ct = cost if on_dev else torch.from_numpy(np.ascontiguousarray(np.asarray(cost, dtype=np.uint8)))
        if ct.dtype != torch.uint8:
            raise ValueError(f"{who}: cost must be uint8")
        return ct.to(side.dev).contiguous(), side

    def _nav_field_call(self, who, shape_rule, shape_text, cfg_cls, stats_cls, fn_host, fn_dev, cost, goals, neutral, lethal, connectivity, parent, max_rounds,
                        rounds_fixed, check_every, device):
        """who: the name in messages; shape_rule: the cost's shape -> the three extents, or None for one that is refused with shape_text; cfg_cls,
        stats_cls: the ctypes forms of the entry points fn_host (numpy) and fn_dev (torch)."""
        cost, side = self._cost_u8(who, cost, device)
        shape = shape_rule(tuple(cost.shape))
        if shape is None:
            raise ValueError(f"{who}: cost must be {shape_text}")
        g = _index_rows(goals, (3, 4), f"{who}: goals must be [S, 3] or [S, 4]", clip=3)
        seeds = np.zeros((g.shape[0], 4), np.int32)                 # [S, 3]: the start value is 0
        seeds[:, :g.shape[1]] = g
        cfg = cfg_cls(*shape)                                       # the three extents lead both structs
        cfg.neutral, cfg.lethal, cfg.connectivity = int(neutral), int(lethal), int(connectivity)
        cfg.max_rounds = 0 if max_rounds is None else int(max_rounds)
        if max_rounds is not None and int(max_rounds) == 0:
            raise ValueError(f"{who}: max_rounds must be at least 1")
        cfg.rounds_fixed = int(rounds_fixed)
        cfg.check_every = 0 if check_every is None else int(check_every)
        S = seeds.shape[0]
        st = stats_cls()
        field = side.out(shape, "u4")
        par = side.out(shape, "u1") if parent else None
        sd = side.put(seeds) if S else None
        std = None if side is HOST else side.out(6, "i4", zero=True)         # the statistics: a struct on the host side, six words on the device
        side.call(fn_host, fn_dev, self.h, C.byref(cfg), side.ptr(cost), side.ptr(sd), S, side.ptr(field), side.ptr(par),
                  C.byref(st) if std is None else side.ptr(std))
        if std is not None:
            sv = std.cpu().numpy()
            st.converged, st.rounds, st.n_bad_seeds = int(sv[0]), int(sv[1]), int(sv[4])
            st.tile_visits = int(sv[2:4].view(np.int64)[0])
        out = {"field": field, "converged": int(st.converged), "rounds": int(st.rounds), "tile_visits": int(st.tile_visits), "n_bad_seeds": int(st.n_bad_seeds),
               "goals": seeds, "neutral": int(neutral), "lethal": int(lethal), "connectivity": int(connectivity)}
        if par is not None:
            out["parent"] = par
        return out

    def _nav_paths_call(self, who, field_who, shape_text, cfg_cls, fn_host, fn_dev, width, field_result, starts, max_len):
        """who, field_who: the names of the method and of the one that makes its fields, in messages; shape_text: the refusal of a field that does not
        have three axes, or None; width: the components of a path cell."""
        if "parent" not in field_result:
            raise ValueError(f"{who}: the field was computed without parents ({field_who}(parent=True))")
        field, par = field_result["field"], field_result["parent"]
        s = _index_rows(starts, (3,), f"{who}: starts must be [P, 3]")
        P, L = s.shape[0], int(max_len)
        if shape_text is not None and len(field.shape) != 3:
            raise ValueError(f"{who}: the field must be {shape_text}")
        d0, d1, d2 = tuple(field.shape)
        cfg = cfg_cls(d0, d1, d2)
        Lc = max(L, 0)
        if hasattr(field, "is_cuda"):
            side = device_side(field.device)
        else:
            side, field, par = HOST, np.ascontiguousarray(field, dtype=np.uint32), np.ascontiguousarray(par, dtype=np.uint8)
        cells, length, status, cost = side.out((P, Lc, width), "i2"), side.out(P, "i4"), side.out(P, "u1"), side.out(P, "u4")
        sd = side.put(s) if P else None
        side.call(fn_host, fn_dev, self.h, C.byref(cfg), side.ptr(field), side.ptr(par), side.ptr(sd), P, L, side.ptr(cells), side.ptr(length),
                  side.ptr(status), side.ptr(cost))
        return {"cells": cells, "length": length, "status": status, "cost": cost}

    # ---- cost-to-go fields and paths (tsl_nav_field.hip) ------------------------------------------------
    def nav_field(self, cost, goals, neutral=50, lethal=253, connectivity=8, parent=True, max_rounds=None, rounds_fixed=0, check_every=None, device=False):
        """The cost-to-go field over 2-D cost planes: for every cell the least cost of getting to a goal, and which cells reach none.  cost: the `cost`
        array of nav_grid, or the dict nav_grid returns (its cost plane is used), or any uint8 array [H, W] or [B, H, W] (1 <= H, W <= 4096, B <= 16):
        the map is not read.  A cell is traversable when cost < lethal; moves go to the 4 or 8 neighbours (`connectivity`), a diagonal one only between
        two traversable cells; leaving a cell costs (neutral + its cost) times 5 along an axis and 7 along a diagonal.  goals: [S, 3] = plane, row, col
        (value 0) or [S, 4] with a start value (read as uint32); goals outside or on a wall are counted in n_bad_seeds.  Returns a dict: `field` uint32
        [B, H, W] (NAV_UNREACHED = 2^32 - 1 where no goal is reached, sums clipped to 2^32 - 2), with parent=True `parent` u8 [B, H, W] (255 unreached,
        8 a goal cell, else the direction code 0 .. 7 of (di, dj) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1) of the next cell), `converged`,
        `rounds`, `tile_visits`, `n_bad_seeds`, and `goals` (int32 [S, 4]) and the parameters, for nav_paths.  The rounds stop when one changes nothing
        (the host looks every `check_every` rounds) or at max_rounds (None = 4 * tiles of a plane + 64): then converged is 0 and the field holds upper
        bounds.  rounds_fixed > 0 runs exactly that many rounds and reads nothing in between.  numpy in gives numpy out; torch device tensors in (or
        device=True) give tensors out, ordered with torch.cuda.current_stream (tsl_tsdf_nav_field_dev: asynchronous with rounds_fixed > 0, and the
        statistics are then read, which waits)."""
        return self._nav_field_call("nav_field", lambda s: (1,) + s if len(s) == 2 else (s if len(s) == 3 else None), "[H, W] or [B, H, W]", _lib.NavFieldCfg,
                                    _lib.NavFieldStats, self.L.tsl_tsdf_nav_field, self.L.tsl_tsdf_nav_field_dev, cost, goals, neutral, lethal, connectivity, parent,
                                    max_rounds, rounds_fixed, check_every, device)

    def nav_paths(self, field_result, starts, max_len):
        """The cheapest way to a goal from every start, along the parents of a nav_field result (computed with parent=True).  starts: [P, 3] = plane, row,
        col.  One lane per start follows the parents for at most max_len cells.  Returns a dict: `cells` int16 [P, max_len, 2] = (row, col) from the
        start on, -1 past the end; `length` int32 [P]; `status` u8 [P] (0 = ended on a goal, 1 = truncated at max_len, 2 = the start is unreached or a
        wall, 3 = the start is outside); `cost` uint32 [P] = the field at the start.  A result of torch tensors gives tensors, asynchronously on
        torch.cuda.current_stream (tsl_tsdf_nav_field_paths_dev); otherwise numpy arrays."""
        return self._nav_paths_call("nav_paths", "nav_field", None, _lib.NavFieldCfg, self.L.tsl_tsdf_nav_field_paths, self.L.tsl_tsdf_nav_field_paths_dev, 2,
                                    field_result, starts, max_len)

    # ---- 3-D cost-to-go fields and paths over flight volumes (tsl_nav_field3.hip) -----------------------
    def nav_field3d(self, cost, goals, neutral=50, lethal=253, connectivity=26, parent=True, max_rounds=None, rounds_fixed=0, check_every=None, device=False):
        """nav_field in 3-D: the cost-to-go field over a cost volume, for platforms that fly.  cost: a uint8 array [D, H, W] (layer k = z, row i = x,
        column j = y; 1 <= D, H, W <= 1024, at most 2^27 cells) or the dict flight_volume returns: the map is not read.  A cell is traversable when
        cost < lethal; moves go to the 6, 18 or 26 neighbours (`connectivity`), a diagonal one only when every cell of the square or cube it spans is
        traversable; leaving a cell costs (neutral + its cost) times 5, 7 or 9 for a move with one, two or three non-zero components.  goals: [S, 3] =
        layer, row, col (value 0) or [S, 4] with a start value (read as uint32); goals outside or on a wall are counted in n_bad_seeds.  Returns a dict
        like nav_field's: `field` uint32 [D, H, W] (NAV_UNREACHED where no goal is reached, sums clipped to 2^32 - 2), with parent=True `parent` u8
        [D, H, W] (255 unreached, 26 = _lib.NAV3_SEED a goal cell, else the direction code 0 .. 25 of the next cell: 0 .. 7 nav_field's (di, dj) with
        dk = 0, 8 = up, 9 .. 16 the same eight with dk = 1, 17 = down, 18 .. 25 with dk = -1), `converged`, `rounds`, `tile_visits`, `n_bad_seeds`, and
        `goals` (int32 [S, 4]) and the parameters, for nav_paths3d.  Rounds, max_rounds (None = min(4 * tiles + 64, 65536)), rounds_fixed, check_every
        and the numpy / torch forms are nav_field's."""
        return self._nav_field_call("nav_field3d", lambda s: s if len(s) == 3 else None, "[D, H, W]", _lib.NavField3Cfg, _lib.NavField3Stats,
                                    self.L.tsl_tsdf_nav_field3, self.L.tsl_tsdf_nav_field3_dev, cost, goals, neutral, lethal, connectivity, parent, max_rounds,
                                    rounds_fixed, check_every, device)

    def nav_paths3d(self, field_result, starts, max_len):
        """nav_paths in 3-D: the cheapest way to a goal from every start, along the parents of a nav_field3d result (computed with parent=True).
        starts: [P, 3] = layer, row, col.  Returns a dict: `cells` int16 [P, max_len, 3] = (layer, row, col) from the start on, -1 past the end;
        `length` int32 [P]; `status` u8 [P] (0 = ended on a goal, 1 = truncated at max_len, 2 = the start is unreached or a wall, 3 = the start is
        outside); `cost` uint32 [P] = the field at the start.  A result of torch tensors gives tensors, asynchronously on torch.cuda.current_stream
        (tsl_tsdf_nav_field3_paths_dev); otherwise numpy arrays."""
        return self._nav_paths_call("nav_paths3d", "nav_field3d", "[D, H, W]", _lib.NavField3Cfg, self.L.tsl_tsdf_nav_field3_paths,
                                    self.L.tsl_tsdf_nav_field3_paths_dev, 3, field_result, starts, max_len)

    # ---- safe corridors: free boxes around cells and along paths (tsl_nav_corridor.hip) -----------------
    def _nav_corridor_cost(self, who, cost, extent, free_below, device):
        """the cost of nav_boxes / nav_corridor -> (array or tensor [D, H, W], its side, whether it had two axes, the filled NavCorridorCfg)"""
        planes = isinstance(cost, dict) and "stride" not in cost    # an int extent reaches along the leading axis only in a volume (flight_volume's dict)
        cost, side = self._cost_u8(who, cost, device)
        shape = tuple(cost.shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"{who}: cost must be [H, W], [B, H, W] or [D, H, W]")
        two = len(shape) == 2
        if two:
            cost = cost.reshape((1,) + shape)
        if isinstance(extent, (int, np.integer)):
            e = int(extent)
            ext = (0, e, e) if (two or planes) else (e, e, e)
        else:
            ext = tuple(int(e) for e in extent)
            if len(ext) != 3:
                raise ValueError(f"{who}: extent must be an int or (e_k, e_i, e_j)")
        cfg = _lib.NavCorridorCfg(*cost.shape)
        cfg.free_below = int(free_below)
        cfg.ext_k, cfg.ext_i, cfg.ext_j = ext
        cfg.max_boxes = 1
        return cost, side, two, cfg

    def nav_boxes(self, cost, cells, free_below=253, extent=16, device=False):
        """The free box around every cell of a list: an axis-aligned box of free cells that contains the cell, grown face by face in the fixed order -j, +j,
        -i, +i, -k, +k until no face can move (include/taichislam_hip.h states the rule; it is the one box that order gives, not the largest free box).
        cost: a uint8 array [H, W],
        [B, H, W] or [D, H, W] (1 <= D, H, W <= 4096, at most 2^28 cells), the dict of nav_grid or nav_terrain (its cost plane is used) or the dict of
        flight_volume: the map is not read.  A cell is free when cost < free_below (1 .. 255).  cells: [S, 3] = layer, row, col ([S, 2] = row, col with
        an [H, W] cost).  extent: the most a box may reach from its cell, in cells, 0 .. 127: an int or (e_k, e_i, e_j); an int on a 2-D cost or on
        the dict of nav_grid / nav_terrain means (0, e, e) -- the planes are independent.  Returns {"boxes": int16 [S, 6] = (k0, i0, j0, k1, i1, j1),
        both ends inclusive, "flags": u8 [S]}: flag _lib.BOX_BLOCKED = 1 for a cell that is not free (the box is the cell), _lib.BOX_OUTSIDE = 2 for a
        cell outside (the box is six times -1).  numpy in gives numpy out; torch device tensors in (or device=True) give tensors out, asynchronously,
        ordered with torch.cuda.current_stream (tsl_tsdf_nav_boxes_dev); cells that are a device tensor are prepared on the device and not read by the
        host (the call still waits where the handle's scratch has to grow: the first call and any larger one)."""
        cost, side, two, cfg = self._nav_corridor_cost("nav_boxes", cost, extent, free_below, device or _is_device_tensor(cells))
        width_ok = (2, 3) if two else (3,)
        bad_cells = "nav_boxes: cells must be [S, 3]" + (" or [S, 2]" if two else "")
        if _is_device_tensor(cells):
            # cells already on a device stay there: clipped, widened and made int32 by torch on the current stream, so the call does not wait
            torch = _torch()
            if cells.dim() != 2 or cells.shape[1] not in width_ok:
                raise ValueError(bad_cells)
            c = cells.to(side.dev).clamp(-(1 << 31), (1 << 31) - 1).to(torch.int32)
            if c.shape[1] == 2:
                c = torch.cat([torch.zeros((c.shape[0], 1), dtype=torch.int32, device=c.device), c], 1)
            c = c.contiguous()
        else:
            c = _index_rows(cells, width_ok, bad_cells)
            if c.shape[1] == 2:
                c = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
            c = side.put(np.ascontiguousarray(c))
        S = c.shape[0]
        boxes, flags = side.out((S, 6), "i2"), side.out(S, "u1")
        side.call(self.L.tsl_tsdf_nav_boxes, self.L.tsl_tsdf_nav_boxes_dev, self.h, C.byref(cfg), side.ptr(cost), side.ptr(c) if S else None, S,
                  side.ptr(boxes), side.ptr(flags))
        return {"boxes": boxes, "flags": flags}

    def nav_corridor(self, cost, paths, free_below=253, extent=16, max_boxes=64, planes=None):
        """The safe corridor of every path: a short chain of free boxes (nav_boxes) that contains the path, the form corridor-based trajectory optimisers
        take.  cost, free_below and extent as in nav_boxes.  paths: the dict of nav_paths or nav_paths3d, or (cells, length) with cells [P, L, 3] or
        [P, L, 2]; cells of width 2 get their plane from `planes` ([P], default 0) in front.  The walk: the first box is the box of the path's first
        cell; the next box is seeded at the last path cell the current box still holds (the cell after the seed when it holds none further), until a
        box holds the path's last cell (status 0) or max_boxes boxes (1 .. L) are out (status 1); an empty path has status 2.  Returns a dict: `boxes` int16
        [P, max_boxes, 6], `seed` int32 [P, max_boxes] (the index of each box's cell in its path), `link` u8 [P, max_boxes] (0 the first box, 1 the box
        shares a cell with the one before, 2 it shares none -- the two only touch --, plus 4 when its seed is not free or outside), `count` int32 [P],
        `status` u8 [P], and `free_below` and `extent` (e_k, e_i, e_j).  Rows past count hold -1 (link 255).  Tensors in (the cost or the paths) give
        tensors out, asynchronously on torch.cuda.current_stream (tsl_tsdf_nav_corridor_dev); otherwise numpy arrays."""
        cells, length = (paths["cells"], paths["length"]) if isinstance(paths, dict) else paths
        want_dev = hasattr(cells, "is_cuda") or hasattr(cost, "is_cuda") or (isinstance(cost, dict) and hasattr(cost["cost"], "is_cuda"))
        cost, side, two, cfg = self._nav_corridor_cost("nav_corridor", cost, extent, free_below, want_dev)
        if len(cells.shape) != 3 or cells.shape[2] not in (2, 3):
            raise ValueError("nav_corridor: cells must be [P, L, 3] or [P, L, 2]")
        P, L, width = (int(v) for v in cells.shape)
        if tuple(length.shape) != (P,):
            raise ValueError("nav_corridor: length must be [P]")
        Q = int(max_boxes)
        cfg.max_boxes = Q
        if side is HOST:
            cd, ld = np.asarray(cells, dtype=np.int16), np.ascontiguousarray(np.asarray(length, dtype=np.int32))
            if width == 2:
                pl = np.zeros(P, np.int16) if planes is None else np.asarray(planes, dtype=np.int16).reshape(P)
                cd = np.concatenate([np.broadcast_to(pl[:, None, None], (P, L, 1)), cd], 2)
            cd = np.ascontiguousarray(cd)
        else:                                                       # paths that are tensors are prepared by torch: the host does not read them
            torch = _torch()
            as_t = lambda a, dt: (a if hasattr(a, "is_cuda") else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))).to(device=side.dev, dtype=dt)
            cd, ld = as_t(cells, torch.int16), as_t(length, torch.int32).contiguous()
            if width == 2:
                pl = torch.zeros(P, dtype=torch.int16, device=side.dev) if planes is None else as_t(planes, torch.int16).reshape(P)
                cd = torch.cat([pl[:, None, None].expand(P, L, 1), cd], 2)
            cd = cd.contiguous()
        Qc = max(Q, 0)
        boxes, seed, link = side.out((P, Qc, 6), "i2"), side.out((P, Qc), "i4"), side.out((P, Qc), "u1")
        count, status = side.out(P, "i4"), side.out(P, "u1")
        side.call(self.L.tsl_tsdf_nav_corridor, self.L.tsl_tsdf_nav_corridor_dev, self.h, C.byref(cfg), side.ptr(cost), side.ptr(cd) if P else None,
                  side.ptr(ld) if P else None, P, L, side.ptr(boxes), side.ptr(seed), side.ptr(link), side.ptr(count), side.ptr(status))
        return {"boxes": boxes, "seed": seed, "link": link, "count": count, "status": status, "free_below": int(free_below),
                "extent": (int(cfg.ext_k), int(cfg.ext_i), int(cfg.ext_j))}

    def flight_volume(self, stride=4, z_range=None, lut=None, cost_unknown=255, cost_outside=255, refresh=True, device=False):
        """The cost volume of nav_field3d from the ESDF: a lattice of one sample per cell of `stride`^3 voxels, through query_esdf(interpolate=False)
        and utils.nav.distance_cost -- no kernel of its own.  Cell (k, i, j) is sampled at the centre of the voxel origin + (k, i, j) * stride +
        stride // 2 in unsigned voxel coordinates (layer, x, y; unsigned = index + half).  The volume covers the whole map in x and y (N // stride
        cells) and the layers of z_range = (z0, z1) in metres (default: all), whole cells only.  lut: the u8 [256] table of utils.nav.flight_lut
        (default: 254 below a quarter voxel, 0 beyond); its `inscribed` must include half a cell diagonal.  Needs an earlier update_esdf; refresh as
        in query_esdf.  Returns {"cost": u8 [D, H, W], "origin": (k0, i0, j0), "stride", "voxel", "half": (Nz // 2, N // 2, N // 2)}; with
        device=True the lattice, the query and the cost stay on the map's device and `cost` is a torch tensor, ordered with torch.cuda.current_stream."""
        from ..utils.nav import distance_cost
        s = int(stride)
        if s < 1:
            raise ValueError("flight_volume: stride must be at least 1")
        vs = float(self.voxel_scale)
        uk0, uk1 = 0, self.Nz - 1
        if z_range is not None:
            z0, z1 = float(z_range[0]), float(z_range[1])
            if not (math.isfinite(z0) and math.isfinite(z1)):
                raise ValueError("flight_volume: z_range is not finite")
            uk0 = max(uk0, math.ceil(z0 / vs) + self.Nz // 2)
            uk1 = min(uk1, math.floor(z1 / vs) + self.Nz // 2)
        D, H, W = (uk1 - uk0 + 1) // s, self.N // s, self.N // s
        if D < 1 or H < 1:
            raise ValueError("flight_volume: the range holds no whole cell")
        if max(D, H, W) > 1024 or D * H * W > (1 << 27):
            raise ValueError("flight_volume: more than 1024 cells along an axis or 2^27 cells; use a larger stride")
        if lut is None:
            lut = np.zeros(256, np.uint8)
            lut[0] = 254
        lut = np.ascontiguousarray(np.asarray(lut.cpu().numpy() if hasattr(lut, "cpu") else lut, dtype=np.uint8)).reshape(-1)
        if lut.shape[0] != 256:
            raise ValueError("flight_volume: lut must have 256 entries")
        origin, half = (uk0, 0, 0), (self.Nz // 2, self.N // 2, self.N // 2)
        # signed voxel index of every sample along each axis, then the lattice in the order [k][i][j] with xyz = (i, j, k) * voxel in float32
        ax = [np.arange(n, dtype=np.int64) * s + s // 2 + o - h for n, o, h in zip((D, H, W), origin, half)]
        if device:
            torch = _torch()
            dev = torch.device(f"cuda:{self.device}")
            tk, ti, tj = (torch.from_numpy(a.astype(np.float32)).to(dev) * np.float32(vs).item() for a in ax)
            xyz = torch.stack([ti[None, :, None].expand(D, H, W), tj[None, None, :].expand(D, H, W), tk[:, None, None].expand(D, H, W)], 3).reshape(-1, 3)
            dist, _, status = self.query_esdf(xyz, interpolate=False, refresh=refresh)
            cost = distance_cost(dist, status, vs, lut, cost_unknown, cost_outside).reshape(D, H, W).contiguous()
        else:
            fk, fi, fj = (a.astype(np.float32) * np.float32(vs) for a in ax)
            xyz = np.empty((D, H, W, 3), np.float32)
            xyz[..., 0], xyz[..., 1], xyz[..., 2] = fi[None, :, None], fj[None, None, :], fk[:, None, None]
            dist, _, status = self.query_esdf(xyz.reshape(-1, 3), interpolate=False, refresh=refresh)
            cost = np.ascontiguousarray(distance_cost(dist, status, vs, lut, cost_unknown, cost_outside).reshape(D, H, W))
        return {"cost": cost, "origin": origin, "stride": s, "voxel": vs, "half": half}

    # ---- terrain layers for ground robots (tsl_nav_terrain.hip) ------------------------------------------
    def nav_terrain(self, bands=None, z_range=None, clearance=1.0, free_run=1, pick="lowest", window=0.2, slope_base=None, max_step=0.1, max_slope_deg=None,
                    min_support=1, radius=1.0, unknown_is_obstacle=False, wall_is_obstacle=False, lut=None, cost_unknown=255, free_thres=None, device=False):
        """The layer between the 3-D map and a ground robot's 2-D planner: per band (bands / z_range as in nav_grid: the range in which the surface is looked
        for) and (x, y) column the height of the surface the robot can stand on, over its footprint the step and the slope of that surface, and a class,
        a distance and a cost in nav_grid's vocabulary -- nav_field, nav_paths, frontier_reach and ros_adapters.occupancy_grid_fields take the result as
        they take nav_grid's.  A layer k is standable when its voxel is occupied, none of the layers up to `clearance` (metres, rounded to layers) above
        it is occupied and the `free_run` layers (a count) directly above it are free; the support is the lowest (pick="lowest") or the highest
        ("highest") standable layer of the band.  `col`: 0 = the column has a support, 1 = obstructed (occupied voxels but nowhere to stand: a wall, a
        top without headroom), 2 = empty.  `height` int16 = 16 * k + q, q in 0 .. 15 the sub-voxel place of the surface level (free_thres as in
        nav_grid) between layers k and k + 1; TERRAIN_NO_HEIGHT = 32767 without a support; in metres height * height_unit.  Over the cells within
        `window` (metres, rounded to cells, at most 16; Chebyshev) `nsup` counts the supported ones and `step` is the largest minus the smallest
        height (65535 = TERRAIN_NO_STAT on a cell without a support).  `slope2` is a Sobel gradient at stride `slope_base` (metres, rounded to 1 .. 16
        cells; None = the window, at least one cell): tan(slope) = sqrt(slope2) / (128 * stride), TERRAIN_NO_SLOPE = 2^32 - 1 where a cell of the stencil
        is outside the grid or has no support.  `cls`: obstructed -> NAV_OCCUPIED, empty -> NAV_UNKNOWN, step > max_step (metres; None = no limit) ->
        occupied, slope above max_slope_deg (None = no limit) -> occupied, fewer than min_support supported cells in the window -> unknown, else
        NAV_FREE.  radius, unknown_is_obstacle, wall_is_obstacle, lut and cost_unknown are nav_grid's and give `d2` and, with lut, `cost` over these
        classes.  Returns a dict of the planes height, col, step, nsup, slope2, cls, d2[, cost], each [B, N, N] indexed [b][i + N / 2][j + N / 2], and
        `voxel`, `origin_xy`, `bands`, `radius_vox`, `height_unit` = voxel / 16 and the integer limits that were passed: `clearance_vox`, `free_run`,
        `pick`, `window_vox`, `slope_base_vox`, `max_step_units`, `max_slope2`, `min_support`.  device=True returns the planes as torch tensors on the
        map's device, asynchronously, ordered with torch.cuda.current_stream (tsl_tsdf_nav_terrain_dev); otherwise numpy arrays."""
        bl = self._nav_bands(bands, z_range)
        vs = float(self.voxel_scale)

        def cells_of(name, x):
            x = float(x)
            if not math.isfinite(x) or x < 0.0:
                raise ValueError(f"nav_terrain: {name} must be finite and not negative")
            return int(round(x / vs))
        R, cl, w = cells_of("radius", radius), cells_of("clearance", clearance), cells_of("window", window)
        s = max(1, min(16, w)) if slope_base is None else max(1, cells_of("slope_base", slope_base))
        if pick not in ("lowest", "highest"):
            raise ValueError("nav_terrain: pick must be 'lowest' or 'highest'")
        if max_step is None:
            ms = 65534
        else:
            max_step = float(max_step)
            if not math.isfinite(max_step) or max_step < 0.0:
                raise ValueError("nav_terrain: max_step must be finite and not negative")
            ms = min(65534, int(round(max_step / vs * 16.0)))
        from ..utils.nav import terrain_slope2
        ms2 = terrain_slope2(max_slope_deg, min(s, 16))
        cfg = _lib.NavTerrainCfg()
        lut = self._nav_head("nav_terrain", cfg, bl, free_thres, R, unknown_is_obstacle, wall_is_obstacle, cost_unknown, lut)
        cfg.clearance, cfg.free_run, cfg.pick, cfg.window, cfg.slope_base = cl, int(free_run), 0 if pick == "lowest" else 1, w, s
        cfg.max_step, cfg.min_support, cfg.max_slope2 = ms, int(min_support), ms2
        B, N = len(bl), self.N
        out = {"voxel": vs, "origin_xy": (-(N // 2) - 0.5) * vs, "bands": bl, "radius_vox": R, "height_unit": vs / 16.0, "clearance_vox": cl,
               "free_run": int(free_run), "pick": pick, "window_vox": w, "slope_base_vox": s, "max_step_units": ms, "max_slope2": ms2, "min_support": int(min_support)}
        kinds = {"height": "i2", "col": "u1", "step": "u2", "nsup": "u2", "slope2": "u4", "cls": "u1", "d2": "u2", "cost": "u1"}
        side = device_side(self.device) if device else HOST
        pl = {k: side.out((B, N, N), kind) for k, kind in kinds.items() if k != "cost" or lut is not None}
        lut = None if lut is None else side.put(lut)
        side.call(self.L.tsl_tsdf_nav_terrain, self.L.tsl_tsdf_nav_terrain_dev, self.h, C.byref(cfg), side.ptr(lut), *(side.ptr(pl.get(k)) for k in kinds))
        out.update(pl)
        return out

    # ---- frame-to-model alignment (tsl_align.hip) ---------------------------------------------------
    def align_linearize(self, depth, R, T, K=None, stride=1, d_min=None, d_max=None, r_max=None, g_max=None, huber=0.0, device=False, counts_only=False):
        """The normal equations of aligning a depth image (uint16 millimetres [h, w]) to the TSDF at the camera-to-map pose (R, T) -- in the frame of
        render_view: Gauss-Newton on s(R p + T), s the trilinear interpolant of the TSDF, over every stride-th pixel of every stride-th row.  Returns a
        dict: H (6 x 6 int64, symmetric), b (6), e -- the sums of J J^T, J s and s^2 in 2^-20 fixed point, J = (grad s, p x grad s) -- the same as
        float64 (H_f, b_f, e_f), the 33 integers as the library orders them (sums) and the counts n_used, n_gate (no depth or outside d_min .. d_max),
        n_unknown (the point touches unobserved voxels), n_far (|s| > r_max), n_grad (gradient 0 or longer than g_max).  The integers do not depend on the
        schedule.  None = the map's default: its depth intrinsics, min / max_ray_length, r_max = internal_voxels * voxel, g_max = 4; huber = 0 is off.
        device=True takes a torch CUDA tensor and returns an int64 tensor of 40 on the device (the 33 integers, then zeros), asynchronously, ordered
        with torch.cuda.current_stream (tsl_tsdf_align_linearize_dev).  counts_only=True leaves H, b and e at 0 and only sorts the pixels into the buckets
        (the A/B switch of tools/bench_track.py: what the gathers cost without the sums)."""
        ptr, shape, keep, on_dev = _depth_image(depth)
        cfg = align_config(K, shape, stride, d_min, d_max, r_max, g_max, huber, counts_only)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        if device:
            if not on_dev:
                raise ValueError("align_linearize: device=True takes a torch CUDA tensor")
            torch = _torch()
            dev = torch.device(f"cuda:{self.device}")
            out = torch.empty(40, dtype=torch.int64, device=dev)
            _lib.check(self.L.tsl_tsdf_align_linearize_dev(self.h, r, t, C.byref(cfg), ptr, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            return out
        if on_dev:
            keep = keep.cpu().numpy().view(np.uint16)
            ptr = _vp(keep)
        sums = _lib.AlignSums()
        _lib.check(self.L.tsl_tsdf_align_linearize(self.h, r, t, C.byref(cfg), ptr, C.byref(sums)))
        return align_sums_dict(np.frombuffer(sums, dtype=np.int64))

    def track_depth(self, depth, R, T, K=None, levels=((8, 4), (4, 4), (2, 6)), min_step=1e-4, damping=0.0, min_used=None, **gates):
        """Refine the camera-to-map pose (R, T) of a depth image against the TSDF: up to 4 levels (stride, iterations) of Gauss-Newton steps on the normal
        equations of align_linearize, solved on the host in float64 (Cholesky) and applied through the Cayley map.  A level ends early when the step
        sqrt(|v|^2 + |omega|^2) falls below min_step.  Returns (R 3 x 3, T 3, info); info["status"]: 0 the last level ended by the threshold, 1 its
        iterations were exhausted, 2 lost (a linearisation used fewer than min_used pixels; default 6), 3 singular -- for 2 and 3 the pose returned is
        the last one that gave a step, or the guess.  info["iterations"] counts the linearisations, info["records"] holds for each the pose it was made
        at (R, T), the step xi = (v, omega) and the dict of align_linearize.  depth: a numpy array or a torch CUDA tensor (ordered with
        torch.cuda.current_stream); gates: the d_min / d_max / r_max / g_max / huber of align_linearize."""
        ptr, shape, keep, on_dev = _depth_image(depth)
        cfg = align_config(K, shape, 1, **gates)
        tc = _track_config(levels, min_step, damping, min_used)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        Ro, To, ro, to = _pose_out()
        rep = _lib.TrackReport()
        side = device_side(keep.device) if on_dev else HOST
        side.call(self.L.tsl_tsdf_track_depth, self.L.tsl_tsdf_track_depth_dev, self.h, r, t, C.byref(cfg), C.byref(tc), ptr, ro, to, C.byref(rep))
        return Ro.reshape(3, 3), To, _track_info(rep)

    # ---- depth-and-colour alignment (tsl_align_rgbd.hip) ------------------------------------------
    def align_rgbd_linearize(self, depth, rgb, R, T, K=None, stride=1, d_min=None, d_max=None, r_max=None, g_max=None, huber=0.0, rc_max=None, gc_max=None,
                             huber_c=0.0, device=False, counts_only=False):
        """The normal equations of aligning a depth image (uint16 millimetres [h, w]) and the colour image registered to it (uint8 [h, w, 3]) to the textured
        TSDF at the camera-to-map pose (R, T): the geometric term of align_linearize and a colour term, the luminance the map stores at the warped pixel
        minus the luminance of the image.  Returns {"geo": ..., "col": ...}, each the dict of align_linearize; geo is exactly what align_linearize returns,
        col has J = (grad Y, p x grad Y) and the residual Y - yi, n_far counting the pixels off the surface (|s| > r_max) or with |Y - yi| > rc_max, n_grad
        those whose luminance gradient is 0 or longer than gc_max.  None = the default: rc_max 1, gc_max 1 / voxel; huber_c = 0 is off.  Both images are
        numpy arrays or both torch CUDA tensors; device=True takes tensors and returns an int64 tensor of 80 on the device (geo in [0, 33), col in
        [40, 73), the rest zeros), asynchronously, ordered with torch.cuda.current_stream (tsl_tsdf_align_rgbd_linearize_dev).  counts_only=True leaves
        H, b and e of both halves at 0 (the A/B switch of tools/bench_track_rgbd.py)."""
        ptr, cptr, shape, keep, side = _rgbd_images("align_rgbd_linearize", depth, rgb, host=not device)
        cfg = align_rgbd_config(K, shape, stride, d_min, d_max, r_max, g_max, huber, rc_max, gc_max, huber_c, counts_only)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        if device:
            if side is HOST:
                raise ValueError("align_rgbd_linearize: device=True takes torch CUDA tensors")
            out = side.out(80, "i8")
            side.call(None, self.L.tsl_tsdf_align_rgbd_linearize_dev, self.h, r, t, C.byref(cfg), ptr, cptr, side.ptr(out))
            return out
        sums = _lib.AlignRgbdSums()
        _lib.check(self.L.tsl_tsdf_align_rgbd_linearize(self.h, r, t, C.byref(cfg), ptr, cptr, C.byref(sums)))
        return align_rgbd_sums_dict(sums)

    def track_rgbd(self, depth, rgb, R, T, K=None, levels=((8, 4), (4, 4), (2, 6)), colour_weight=None, balance=1.0, min_step=1e-4, damping=0.0, min_used=None,
                   **gates):
        """track_depth with the colour term of align_rgbd_linearize: every step solves Hg + lambda Hc, so the pose is also held in the directions in which
        the geometry does not change (along a flat wall, down a corridor) as long as the surface has texture.  colour_weight: lambda >= 0, or None =
        automatic: balance * trace of the translation block of Hg / that of Hc at the first linearisation, held for the whole call (0 when the view has
        no texture: pure geometry).  Returns (R 3 x 3, T 3, info) shaped as track_depth's with info["lambda"] the weight that was used and every record
        holding geo and col, the dicts of align_linearize; the track is lost when the geometric n_used falls below min_used.  depth, rgb: numpy arrays or
        torch CUDA tensors (ordered with torch.cuda.current_stream); gates: the d_min / d_max / r_max / g_max / huber / rc_max / gc_max / huber_c of
        align_rgbd_linearize."""
        ptr, cptr, shape, keep, side = _rgbd_images("track_rgbd", depth, rgb)
        cfg = align_rgbd_config(K, shape, 1, **gates)
        tc = _track_config(levels, min_step, damping, min_used)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        Ro, To, ro, to = _pose_out()
        rep = _lib.TrackRgbdReport()
        lam = -1.0 if colour_weight is None else float(colour_weight)
        if lam < 0.0 and colour_weight is not None:
            raise ValueError("track_rgbd: colour_weight must not be negative (None = automatic)")
        side.call(self.L.tsl_tsdf_track_rgbd, self.L.tsl_tsdf_track_rgbd_dev, self.h, r, t, C.byref(cfg), C.byref(tc), lam, float(balance), ptr, cptr, ro, to,
                  C.byref(rep))
        records = []
        for i in range(rep.iterations):
            it = rep.it[i]
            rec = align_rgbd_sums_dict(it.sums)
            rec.update(R=np.array(it.R[:], np.float64).reshape(3, 3), T=np.array(it.T[:], np.float64), xi=np.array(it.xi[:], np.float64))
            records.append(rec)
        return Ro.reshape(3, 3), To, {"status": int(rep.status), "iterations": int(rep.iterations), "lambda": float(rep.lam), "records": records}

    # ---- scan-to-model alignment (tsl_align_points.hip) -------------------------------------------
    def align_points_linearize(self, xyz, R, T, stride=1, d_min=None, d_max=None, r_max=None, g_max=None, huber=0.0, per_point=False, device=False,
                               counts_only=False):
        """The normal equations of aligning a point cloud (f32 [n, 3], sensor frame) to the TSDF at the sensor-to-map pose (R, T) -- in the frame of
        query_points: Gauss-Newton on s(R p + T) over every stride-th point.  Returns the dict of align_linearize; n_gate counts the points that are
        not finite or whose range lies outside d_min .. d_max (None = the map's min / max_ray_length).  per_point=True adds `bucket` (uint8 per
        visited point: 0 used, 1 gate, 2 unknown, 3 far, 4 grad) and `s` (float32: the signed distance at the pose for used, far and grad, 0 for
        gate and unknown) -- what tells the points of a moving object from the map's.  device=True takes a torch CUDA tensor and returns an int64
        tensor of 40 on the device (with per_point=True a tuple (sums, bucket, s) of device tensors), asynchronously, ordered with
        torch.cuda.current_stream (tsl_tsdf_align_points_linearize_dev).  counts_only as in align_linearize."""
        ptr, n, keep, on_dev = _point_cloud(xyz)
        cfg = align_points_config(stride, d_min, d_max, r_max, g_max, huber, counts_only)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        visited = -(-n // cfg.stride) if cfg.stride >= 1 else 0
        if device:
            if not on_dev:
                raise ValueError("align_points_linearize: device=True takes a torch CUDA tensor")
            torch = _torch()
            dev = torch.device(f"cuda:{self.device}")
            out = torch.empty(40, dtype=torch.int64, device=dev)
            bucket = torch.empty(visited, dtype=torch.uint8, device=dev) if per_point else None
            sd = torch.empty(visited, dtype=torch.float32, device=dev) if per_point else None
            _lib.check(self.L.tsl_tsdf_align_points_linearize_dev(self.h, r, t, C.byref(cfg), ptr, n, out.data_ptr(), bucket.data_ptr() if per_point else None,
                                                                  sd.data_ptr() if per_point else None, torch.cuda.current_stream(dev).cuda_stream))
            return (out, bucket, sd) if per_point else out
        if on_dev:
            keep = keep.cpu().numpy()
            ptr = _vp(keep)
        sums = _lib.AlignSums()
        bucket = np.zeros(visited, np.uint8) if per_point else None
        sd = np.zeros(visited, np.float32) if per_point else None
        _lib.check(self.L.tsl_tsdf_align_points_linearize(self.h, r, t, C.byref(cfg), ptr, n, C.byref(sums), _vp(bucket), _vp(sd)))
        out = align_sums_dict(np.frombuffer(sums, dtype=np.int64))
        if per_point:
            out["bucket"], out["s"] = bucket, sd
        return out

    def track_points(self, xyz, R, T, levels=((8, 4), (4, 4), (1, 6)), min_step=1e-4, damping=0.0, min_used=None, **gates):
        """Refine the sensor-to-map pose (R, T) of a point cloud against the TSDF: track_depth for a cloud.  levels: up to 4 (point stride, iterations).
        Returns (R 3 x 3, T 3, info) shaped as track_depth's.  xyz: a numpy array or a torch CUDA tensor (ordered with torch.cuda.current_stream);
        gates: the d_min / d_max / r_max / g_max / huber of align_points_linearize."""
        ptr, n, keep, on_dev = _point_cloud(xyz)
        cfg = align_points_config(1, **gates)
        tc = _track_config(levels, min_step, damping, min_used)
        r, t = _dptr(R, 9)[1], _dptr(T, 3)[1]
        Ro, To, ro, to = _pose_out()
        rep = _lib.TrackReport()
        side = device_side(keep.device) if on_dev else HOST
        side.call(self.L.tsl_tsdf_track_points, self.L.tsl_tsdf_track_points_dev, self.h, r, t, C.byref(cfg), C.byref(tc), ptr, n, ro, to, C.byref(rep))
        return Ro.reshape(3, 3), To, _track_info(rep)

    # ---- map-to-map registration (tsl_register.hip) -------------------------------------------------
    def register_linearize(self, src, R, T, *, src_sid=None, dst_sid=None, stride=1, w_min=0, band=0, r_max=0, g_max=0, huber=0, counts_only=False):
        """The normal equations of registering a submap of the map `src` against this map at the pose (R, T) that takes source-submap coordinates to
        this map's: Gauss-Newton on s(R q + T) - t over the observed voxels q of the source whose indices are divisible by `stride` (1, 2, 4, 8, 16),
        whose weight is at least w_min and whose stored value t lies within `band` of the surface; s is the trilinear interpolant of this map.  Returns
        the dict of align_linearize: H, b, e (2^-20 fixed point), their float64 forms, the 33 integers (sums) and the counts n_used, n_gate (weight or
        band), n_unknown (the voxel lands on unobserved voxels of this map), n_far (|s| > r_max), n_grad.  src_sid / dst_sid: submap ids, None = the
        active submap (submap 0 on a global map).  0 = the default: band = 2 voxels, r_max = internal_voxels * voxel, g_max = 4; huber = 0 is off.
        `src` may be this map.  Queued frames of both maps are integrated first; neither map is written.  counts_only=True leaves H, b and e at 0 (the
        A/B switch of tools/bench_register.py)."""
        cfg = register_config(stride, w_min, band, r_max, g_max, huber, counts_only)
        sums = _lib.AlignSums()
        _lib.check(self.L.tsl_tsdf_register_linearize(self.h, _sid(dst_sid), src.h, _sid(src_sid),
                                                      _dptr(R, 9)[1], _dptr(T, 3)[1], C.byref(cfg), C.byref(sums)))
        return align_sums_dict(np.frombuffer(sums, dtype=np.int64))

    def register_submap(self, src, R0, T0, *, levels=None, min_step=1e-4, damping=0.0, min_used=None, src_sid=None, dst_sid=None,
                        w_min=0, band=0, r_max=0, g_max=0, huber=0):
        """Refine the pose (R0, T0) that takes a submap of `src` into this map: up to 4 levels (stride, iterations) -- default (4, 4), (2, 4), (1, 6) -- of
        Gauss-Newton steps on the normal equations of register_linearize, solved and retracted as track_depth does.  Returns (R 3 x 3, T 3, info) shaped
        like track_depth's: info["status"] 0 the last level ended by min_step, 1 its iterations were exhausted, 2 lost (fewer than min_used voxels
        used; default 6), 3 singular -- for 2 and 3 the pose returned is the last one that gave a step, or the guess; info["records"] holds for each
        linearisation its pose, its step xi = (v, omega) and the dict of register_linearize.  The last record's H_f is the information matrix of the
        constraint.  w_min / band / r_max / g_max / huber: the gates of register_linearize."""
        cfg = register_config(1, w_min, band, r_max, g_max, huber)
        tc = _track_config(REGISTER_LEVELS if levels is None else levels, min_step, damping, min_used)
        Ro, To, ro, to = _pose_out()
        rep = _lib.TrackReport()
        _lib.check(self.L.tsl_tsdf_register_submap(self.h, _sid(dst_sid), src.h, _sid(src_sid), _dptr(R0, 9)[1], _dptr(T0, 3)[1], C.byref(cfg), C.byref(tc), ro, to,
                                                   C.byref(rep)))
        return Ro.reshape(3, 3), To, _track_info(rep)

    # ---- pose search for the registration (tsl_register_search.hip) -------------------------------
    def register_score(self, src, R, T, *, src_sid=None, dst_sid=None, stride=1, w_min=0, band=0, r_max=0, g_max=0, huber=0, counts_only=False):
        """Score many poses in one call: for every pose (R[k] 3 x 3, T[k] 3) the e, n_used, n_unknown, n_far and n_grad register_linearize returns for it
        with the same arguments, without forming H and b.  Returns a dict of int64 arrays [n] under those names, e_f (e * 2^-20, float64) and gate:
        the pose-independent n_gate, n_pass (the visited voxels that pass the weight and band tests) and sum_i / sum_j / sum_k, the integer sums of
        their voxel indices -- (sum / n_pass) * voxel is the centroid of what is being registered.  At most 65536 poses.  counts_only=True leaves e
        at 0.  Queued frames of both maps are integrated first; neither map is written."""
        R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 9))
        T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1, 3))
        if R.shape[0] != T.shape[0]:
            raise ValueError("register_score: R and T hold different numbers of poses")
        n = R.shape[0]
        cfg = register_config(stride, w_min, band, r_max, g_max, huber, counts_only)
        out = np.zeros(max(n, 1), _SCORE_DTYPE)
        gate = _lib.RegisterGate()
        _lib.check(self.L.tsl_tsdf_register_score(self.h, _sid(dst_sid), src.h, _sid(src_sid),
                                                  R.ctypes.data_as(_lib.dp), T.ctypes.data_as(_lib.dp), n, C.byref(cfg),
                                                  out.ctypes.data_as(C.POINTER(_lib.RegisterScore)), C.byref(gate)))
        return dict(_scores_dict(out[:n]), gate=gate.as_dict())

    def register_score_tile(self, entries, n):
        """The entries of the list of gated source voxels that one workgroup of the scoring kernel stages when register_score scores n poses
        against a list of `entries` (= gate["n_pass"]) on this map's device: 256, 128 or 64.  It changes no result; tests and tools ask it which
        tile a case takes."""
        return int(self.L.tsl_tsdf_register_score_tile(self.h, int(entries), int(n)))

    def register_search(self, src, R0, T0, *, window_t=(0.8, 0.8, 0.4), step_t=0.2, window_r=(0.0, 0.0, np.pi / 3), step_r=np.pi / 18, pivot=None, stride=4,
                        miss=0, min_used=None, levels=None, min_step=1e-4, damping=0.0, refine_min_used=None, src_sid=None, dst_sid=None,
                        w_min=0, band=0, r_max=0, g_max=0, huber=0, return_scores=False):
        """register_submap with a search in front of it, for a guess that may lie outside the basin of the true pose (a loop closure from a drifted
        pose table).  A lattice of candidate poses around (R0, T0) -- per axis round(window / step) steps either way; translations in metres along
        this map's axes, rotations in radians as the vector omega of the Cayley map (an angle of 2 atan(|omega| / 2)) about `pivot`, default: the
        centroid of the source voxels in the band, carried by the guess -- is scored in one call at `stride`; the cost of a candidate is the integer
        J = e + F n_far + U (n_unknown + n_grad), F = r_max^2, U = miss^2 in 2^-20 fixed point (miss 0 = r_max): a source voxel that lands on unknown
        space costs as much as the worst residual admitted.  The candidate of the least J among those with n_used >= min_used (default 6; ties to the
        first) is refined by register_submap with levels / min_step / damping / refine_min_used.  The default lattice is 9 x 9 x 5 translations
        x 13 yaw angles = 5265 candidates (at most 65536).  Returns (R, T, info): register_submap's info plus info["search"] = the report (status,
        n_candidates, n_valid, best, J_best, score_best, pivot, R_best, T_best, gate; scores with return_scores=True).  Status 2 with no records: no
        candidate was valid, or nothing passed the gate; the pose returned is the guess."""
        (nt, st), (nr, sr) = _half_counts(window_t, step_t), _half_counts(window_r, step_r)
        sc = _lib.SearchCfg()
        for a in range(3):
            sc.n_t[a], sc.n_r[a], sc.step_t[a], sc.step_r[a] = nt[a], nr[a], st[a], sr[a]
        if pivot is not None:
            sc.flags = 1
            sc.pivot[:] = [float(v) for v in np.asarray(pivot, np.float64).reshape(3)]
        sc.stride, sc.miss, sc.min_used = int(stride), float(miss), (0 if min_used is None else int(min_used))
        cfg = register_config(1, w_min, band, r_max, g_max, huber)
        tc = _track_config(REGISTER_LEVELS if levels is None else levels, min_step, damping, refine_min_used)
        total = 1
        for v in nr + nt:
            total *= 2 * max(v, 0) + 1
        scores = np.zeros(total, _SCORE_DTYPE) if return_scores and total <= 65536 else None
        Ro, To, ro, to = _pose_out()
        rep, trk = _lib.SearchReport(), _lib.TrackReport()
        _lib.check(self.L.tsl_tsdf_register_search(self.h, _sid(dst_sid), src.h, _sid(src_sid), _dptr(R0, 9)[1], _dptr(T0, 3)[1], C.byref(cfg), C.byref(sc), C.byref(tc),
                                                   ro, to, C.byref(rep), C.byref(trk),
                                                   None if scores is None else scores.ctypes.data_as(C.POINTER(_lib.RegisterScore))))
        info = _track_info(trk)
        sb = rep.score_best
        info["search"] = {"status": int(rep.status), "n_candidates": int(rep.n_candidates), "n_valid": int(rep.n_valid), "best": int(rep.best),
                          "J_best": int(rep.J_best), "score_best": {n: int(getattr(sb, n)) for n in ("e", "n_used", "n_unknown", "n_far", "n_grad")},
                          "pivot": np.array(rep.pivot[:], np.float64), "R_best": np.array(rep.R_best[:], np.float64).reshape(3, 3),
                          "T_best": np.array(rep.T_best[:], np.float64), "gate": rep.gate.as_dict()}
        if scores is not None:
            info["search"]["scores"] = _scores_dict(scores)
        return Ro.reshape(3, 3), To, info

    # ---- ESDF (definition from the legacy dense_esdf.py:228-333) -----------------------------------
    def update_esdf(self, gamma=None, max_dist=None, wait=True):
        """Bring the ESDF of the active submap up to date with its TSDF -- incrementally: only the bricks integrated into since
        the previous call (dilated by max_dist) are recomputed, with the result of a full recompute.  Returns the number of brick
        relaxations; `esdf_stats()` has the breakdown.  The reference's hook ran after every frame (dense_esdf.py:400-402); for that use
        pass wait=False: the update is only enqueued behind the frame (returns None) and `export_esdf` / `esdf_stats` / `esdf_totals`
        wait for whatever is still in flight."""
        g = self.voxel_scale if gamma is None else gamma                 # dense_esdf.py:40 gamma = voxel_scale
        md = self.max_ray_length if max_dist is None else max_dist       # dense_esdf.py:265 sign * max_ray_length
        self._esdf_ever = True
        self._esdf_gamma, self._esdf_max_dist = g, md
        if not wait:
            _lib.check(self.L.tsl_esdf_update(self.h, float(g), float(md), None))
            return None
        it = C.c_int32()
        _lib.check(self.L.tsl_esdf_update(self.h, float(g), float(md), C.byref(it)))
        return it.value

    def esdf_totals(self):
        """Sums over the completed ESDF updates of this map (waits for the ones in flight)."""
        st = _lib.EsdfTotals()
        _lib.check(self.L.tsl_esdf_totals(self.h, C.byref(st)))
        return st.as_dict()

    def esdf_stats(self):
        st = _lib.EsdfStats()
        _lib.check(self.L.tsl_esdf_last_stats(self.h, C.byref(st)))
        return st.as_dict()

    def cvt_ESDF_to_voxels_slice(self, z):
        """dense_esdf.py:498-509: ESDF values of the voxel layer at height z -> export_ESDF / export_ESDF_xyz (device-resident;
        `.to_numpy()` / `.to_torch()`), count in num_export_ESDF_particles[None].  The ESDF is brought up to date first -- the reference updates it
        inside every recast (dense_esdf.py:400-402), so its slice is always current: an incremental update is queued here (it finds nothing to do when
        no frame was integrated since the last one; tsl_esdf_slice waits for it), with the parameters of the last update."""
        self.update_esdf(gamma=getattr(self, "_esdf_gamma", None), max_dist=getattr(self, "_esdf_max_dist", None), wait=False)
        n = C.c_int32()
        _lib.check(self.L.tsl_esdf_slice(self.h, float(z), C.byref(n)))
        self._esdf_slice_n = n.value

    def get_voxels_ESDF_slice(self, z):
        self.cvt_ESDF_to_voxels_slice(z)
        return self._read_esdf_slice(self._esdf_slice_n)

    def query_esdf(self, xyz, interpolate=True, gradient=None, unknown_value=float("nan"), refresh=True):
        """Batched ESDF queries at arbitrary points for planners (trajectory samples, collision checks, node expansions): returns
        (dist f32[n], grad f32[n,3] or None, status u8[n]).  xyz [n,3] is in the frame of the submap the ESDF was last updated for (the frame
        of is_pos_occupy / raycast).  interpolate=False reads the nearest voxel; interpolate=True interpolates the 8 corners of the cell
        trilinearly, and gradient (default: the same as interpolate) adds the gradient of that interpolant.  status: 0 ok, 1 a needed voxel
        is unknown (not observed / unallocated), 2 outside the volume; for those dist = unknown_value and grad = 0.  Flag 0x80 (torch input
        only): the values come from an update that stopped before converging.  numpy in -> numpy out; torch CUDA tensors in -> torch tensors
        on the same device, asynchronously, ordered with torch.cuda.current_stream (tsl_esdf_query_points_dev).
        refresh=True first enqueues an incremental update with the parameters of the last update_esdf call (as cvt_ESDF_to_voxels_slice
        does), so the answer reflects every frame so far; refresh=False reads the last update as it is.  Either needs an earlier update_esdf."""
        mode = 1 if interpolate else 0
        gradient = bool(interpolate) if gradient is None else bool(gradient)
        if gradient and not mode:
            raise ValueError("query_esdf: the gradient needs interpolate=True")
        if refresh:
            self._esdf_refresh("query_esdf")
        x, side = _points_f32(xyz)
        n = x.shape[0]
        dist = side.out(n, "f4")
        grad = side.out((n, 3), "f4") if gradient else None
        status = side.out(n, "u1")
        side.call(self.L.tsl_esdf_query_points, self.L.tsl_esdf_query_points_dev, self.h, mode, float(unknown_value), side.ptr(x), n, side.ptr(dist),
                  side.ptr(grad), side.ptr(status))
        return dist, grad, status

    def _esdf_refresh(self, who):
        """refresh=True of the ESDF's readers: an ESDF must exist, and an incremental update with the parameters of the last update_esdf is queued"""
        if not getattr(self, "_esdf_ever", False):
            raise _lib.TslError(f"{who}: call update_esdf first (refresh repeats the last update's parameters)")
        self.update_esdf(gamma=self._esdf_gamma, max_dist=self._esdf_max_dist, wait=False)

    def score_paths(self, waypoints, radius, margin=0.0, sub=1, lengths=None, interpolate=True, stop=False, unknown_blocks=True, outside_blocks=True,
                    samples=False, unknown_value=float("nan"), refresh=True):
        """Scores candidate paths against the ESDF in one launch (tsl_path_score.hip): which of these motions is free, how close
        does each come to a surface, what does each cost.  waypoints f32 [n, K, 3] (a [K, 3] input is one path) in the frame of query_esdf; lengths
        (integers [n], optional) gives the waypoints each path uses, 1 .. K -- the rest is never read.  Every segment is sampled at `sub` points (its
        start and sub - 1 points between; the last waypoint closes the path), and every sample has the value and status of query_esdf there
        (`interpolate` as there; a NaN value counts as unknown).  A sample is a hit when its distance is below `radius`; it blocks when it is a hit,
        unknown (with unknown_blocks) or outside the volume (with outside_blocks).  Returns a dict of arrays per path: first_stop (the first blocking
        sample, -1 for a free path), n_samples, n_hit, n_unknown, n_outside, argmin / min_dist (the closest known sample; -1 / +inf without one), cost
        (int64: the sum of min(radius + margin - d, 1024) over the known samples closer than radius + margin, in units of 2^-20 m) and short_update
        (0x80 when the ESDF update had stopped before converging; torch input only).  stop=True counts the samples up to first_stop only, and the GPU
        does not evaluate the path much further.  samples=True adds sample_dist f32 [n, S_max] and sample_status u8 [n, S_max], S_max =
        (K - 1) * sub + 1: the query's answer per counted sample, unknown_value / 0xff elsewhere.  Every field is exact and independent of the schedule.
        numpy in -> numpy out; torch CUDA tensors in (lengths then a torch.int32 tensor) -> torch tensors, asynchronously, ordered with
        torch.cuda.current_stream.  refresh as in query_esdf."""
        mode = 1 if interpolate else 0
        flags = (1 if stop else 0) | (2 if unknown_blocks else 0) | (4 if outside_blocks else 0)
        if int(sub) < 1:
            raise ValueError("score_paths: sub must be at least 1")
        if refresh:
            self._esdf_refresh("score_paths")
        w, ln, side, _ = _polylines("score_paths", waypoints, lengths, 1, "path", "waypoints")
        n, K = int(w.shape[0]), int(w.shape[1])
        smax = (K - 1) * int(sub) + 1
        rec = side.out((n, PATH_SCORE_DTYPE.itemsize // 4), "i4")
        sd = side.out((n, smax), "f4") if samples else None
        ss = side.out((n, smax), "u1") if samples else None
        side.call(self.L.tsl_esdf_score_paths, self.L.tsl_esdf_score_paths_dev, self.h, mode, float(unknown_value), side.ptr(w), side.ptr(ln), n, K, int(sub),
                  float(radius), float(margin), flags, side.ptr(rec), side.ptr(sd), side.ptr(ss))
        out = record_columns(rec, PATH_SCORE_DTYPE)
        if samples:
            out["sample_dist"], out["sample_status"] = sd, ss
        return out

    def _traj_inputs(self, who, ctrl, lengths, refresh):
        """(ctrl [n, K, 3] f32 contiguous, lengths int32 [n] or None, the side, one trajectory?) of traj_linearize / traj_optimize"""
        if refresh:
            self._esdf_refresh(who)
        return _polylines(who, ctrl, lengths, 4, "trajectory", "ctrl")

    def traj_linearize(self, ctrl, clearance, sub=4, lengths=None, gradients=True, unknown_value=float("nan"), refresh=True):
        """The collision and smoothness costs of uniform cubic B-spline trajectories against the ESDF, with their gradients over the control points, in
        one launch (tsl_traj_opt.hip).  ctrl f32 [n, K, 3] control points (a [K, 3] input is one trajectory), K in 4 .. 256, in
        the frame of query_esdf; lengths (integers [n], 4 .. K, optional) gives the control points each trajectory uses.  Every span is sampled at `sub`
        points (utils.nav.bspline_points gives the positions); a sample has query_esdf's trilinear value d and gradient, and is penalised by
        (clearance - d)^2 where d < clearance.  Returns a dict of arrays per trajectory: n_samples, n_pen (penalised samples), n_unknown, n_outside
        (samples the map does not know / outside the volume: counted, never penalised), argmin / min_dist (the closest known sample; -1 / +inf without
        one), cost_collision and cost_smooth (int64, units of 2^-20 m^2), short_update, iters_done (0); with gradients=True also grad_collision and
        grad_smooth, int64 [n, K, 3] in units of 2^-20 m.  Every field is exact and independent of the schedule.  numpy in -> numpy out; torch CUDA
        tensors in (lengths then a torch.int32 tensor) -> torch tensors, asynchronously, ordered with torch.cuda.current_stream.  refresh as in
        query_esdf."""
        c, ln, side, _ = self._traj_inputs("traj_linearize", ctrl, lengths, refresh)
        n, K = int(c.shape[0]), int(c.shape[1])
        rec = side.out((n, TRAJ_SCORE_DTYPE.itemsize // 4), "i4")
        gc = side.out((n, K, 3), "i8") if gradients else None
        gs = side.out((n, K, 3), "i8") if gradients else None
        side.call(self.L.tsl_esdf_traj_linearize, self.L.tsl_esdf_traj_linearize_dev, self.h, float(unknown_value), side.ptr(c), side.ptr(ln), n, K, int(sub),
                  float(clearance), side.ptr(rec), side.ptr(gc), side.ptr(gs))
        out = record_columns(rec, TRAJ_SCORE_DTYPE)
        if gradients:
            out["grad_collision"], out["grad_smooth"] = gc, gs
        return out

    def traj_optimize(self, ctrl, clearance, sub=4, iters=50, w_collision=1.0, w_smooth=1.0, step=0.05, momentum=0.8, max_move=None, fix_ends=3,
                      stop_when_free=False, history=False, lengths=None, unknown_value=float("nan"), refresh=True):
        """Pushes uniform cubic B-spline trajectories out of collision and smooths them: `iters` steps of a momentum descent on w_collision *
        cost_collision + w_smooth * cost_smooth of traj_linearize, all inside one launch (tsl_traj_opt.hip).  Per step and
        control point: v = momentum * v - step * gradient, clamped to +-max_move metres per axis (None: half a voxel), c += v.  The first and the last
        fix_ends control points of every trajectory stay where they are (3 pins the end positions and tangents of a spline whose ends are tripled, as
        utils.nav.bspline_from_path makes them).  stop_when_free ends a trajectory at its first linearisation without a penalised sample.  Returns
        the dict of traj_linearize without the gradients, for the control points as they end (iters_done = the steps taken), and ctrl f32 [n, K, 3]
        ([K, 3] for one trajectory); history=True adds history int64 [n, iters + 1, 2], (cost_collision, cost_smooth) of every linearisation and -1
        behind a stop.  Samples that are unknown or outside pull nowhere: check n_unknown and n_outside, or re-check the result with
        score_paths(bspline_points(ctrl, sub), clearance).  Arrays in and out as in traj_linearize."""
        c, ln, side, one = self._traj_inputs("traj_optimize", ctrl, lengths, refresh)
        n, K = int(c.shape[0]), int(c.shape[1])
        o = _lib.TrajOpt(clearance=float(clearance), w_collision=float(w_collision), w_smooth=float(w_smooth), step=float(step), momentum=float(momentum),
                         max_move=0.5 * float(self.voxel_scale) if max_move is None else float(max_move), sub=int(sub), iters=int(iters),
                         fix_head=int(fix_ends), fix_tail=int(fix_ends), flags=1 if stop_when_free else 0)
        rec = side.out((n, TRAJ_SCORE_DTYPE.itemsize // 4), "i4")
        co = side.out((n, K, 3), "f4")
        hist = side.out((n, max(o.iters, 0) + 1, 2), "i8") if history else None
        side.call(self.L.tsl_esdf_traj_optimize, self.L.tsl_esdf_traj_optimize_dev, self.h, float(unknown_value), side.ptr(c), side.ptr(ln), n, K, C.byref(o),
                  side.ptr(co), side.ptr(rec), side.ptr(hist))
        out = record_columns(rec, TRAJ_SCORE_DTYPE)
        out["ctrl"] = co[0] if one else co
        if history:
            out["history"] = hist
        return out

    def export_esdf_torch(self):
        """(indices int16[n,3], esdf f32[n]) as torch tensors on the device: zero-copy views of the map's staging buffer, valid until the
        next exporting call on this map (clone them to keep them)."""
        from .fields import device_view
        n = self.count_active()
        pi, pv, cnt = C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(self.L.tsl_esdf_export_dev(self.h, n, C.byref(pi), C.byref(pv), C.byref(cnt)))
        k = min(n, cnt.value)
        return device_view(pi.value, (k, 3), "<i2", self, self.device), device_view(pv.value, (k,), "<f4", self, self.device)

    def export_esdf(self):
        """(indices int16[n,3], esdf f32[n]) for every observed voxel of the active submap."""
        n = self.count_active()
        idx = np.zeros((n, 3), np.int16)
        val = np.zeros(n, np.float32)
        cnt = C.c_int64()
        _lib.check(self.L.tsl_esdf_export(self.h, _vp(idx), _vp(val), n, C.byref(cnt)))
        return idx[:cnt.value], val[:cnt.value]

    def init_sphere(self, voxels=30, radius=None):
        """dense_tsdf.py:136-146 as intended by tests/marching_cube_test.py: an analytic sphere SDF of
        `voxels`^3 cells centred on the map origin, every cell observed (the reference body is broken at HEAD:
        3-index access on 4-d fields)."""
        radius = self.voxel_scale * 3 if radius is None else radius
        r = np.arange(-(voxels // 2), voxels - voxels // 2, dtype=np.int16)
        ii, jj, kk = np.meshgrid(r, r, r, indexing="ij")
        idx = np.stack([ii, jj, kk], -1).reshape(-1, 3)
        p = idx.astype(np.float32) * np.float32(self.voxel_scale)
        tsdf = (np.sqrt((p * p).sum(1)) - np.float32(radius)).astype(np.float16)
        n = idx.shape[0]
        col = np.zeros((n, 3), np.float16) if self.enable_texture else np.array([])
        self.load_numpy(self.get_active_submap_id(), idx, tsdf, np.ones(n, np.float16), np.zeros(n, np.int8), col)

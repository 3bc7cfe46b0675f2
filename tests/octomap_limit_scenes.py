"""Scenes of tests/test_octomap_limits_gpu.py and tests/test_query_edges_gpu.py, and the runner that plays one list of operations into the HIP Octomap and into
the CPU oracle.  Everything here is numpy and the oracle: tests/test_limit_scenes_cpu.py asserts, without a GPU, that each scene reaches the path it was made for.

An operation is a tuple: ("base", sid, R, T) | ("active", sid) | ("next",) | ("depth", R, T, depth, texture or None, device) | ("points", R, T, xyz, rgb or
None, device); `device` = hand the arrays over as torch tensors on the GPU (the oracle ignores it)."""
import numpy as np

from taichislam_amd.utils import synthetic as syn
from util import small_stream, sorted_rows

I3, Z3 = np.eye(3), np.zeros(3)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
# coordinates that lie outside every map: not finite, or with a cell index that does not fit an int (include/taichislam_hip.h)
BAD_POINTS = np.array([[NAN, 0.5, 0.5], [0.5, NAN, 0.5], [0.5, 0.5, NAN], [NAN, NAN, NAN], [INF, 0.0, 0.0], [0.0, -INF, 0.0], [0.5, 0.5, INF], [-INF, INF, 0.0],
                       [1e12, 0.0, 0.0], [0.0, -1e12, 0.5], [0.5, 0.0, 1e12], [3e38, 1.0, 1.0], [1.0, 1.0, -3e38]], np.float32)
# ... and coordinates that only look odd: -0.0 is cell 0
ZERO_POINTS = np.array([[-0.0, -0.0, -0.0], [0.01, -0.0, 0.0], [-0.02, 0.02, -0.0]], np.float32)


def stats3(s):
    return (s["p_used"], s["p_valid"], s["p_oob"])


def cell_of(x, vs):
    """rnd_i(x / vs) of finite float32 coordinates, in float32 as the kernels and the oracle compute it (round half away from zero)"""
    q = np.asarray(x, np.float32) / np.float32(vs)
    r = np.trunc(q)
    return (r + np.where(np.abs(q - r) >= np.float32(0.5), np.copysign(np.float32(1.0), q), np.float32(0.0))).astype(np.int64)


def mix_bad(valid, bad=BAD_POINTS, seed=0):
    """`valid` with the rows of `bad` put in at random places and one of them at the very end (the largest index colours a leaf: a bad point must not);
    returns (cloud, mask of the bad rows)"""
    rng = np.random.default_rng(seed)
    n = valid.shape[0] + bad.shape[0]
    at = np.sort(rng.choice(n - 1, size=bad.shape[0] - 1, replace=False)).tolist() + [n - 1]
    is_bad = np.zeros(n, bool); is_bad[at] = True
    out = np.empty((n, 3), np.float32)
    out[is_bad] = bad; out[~is_bad] = valid
    return out, is_bad


def leaves(m, color=False):
    """sorted rows (i, j, k, count[, r, g, b]) of the active submap of either side"""
    e = m.export_leaves(with_color=True)
    cols = [e[0].astype(np.float64), e[1][:, None].astype(np.float64)] + ([e[2].astype(np.float64)] if color else [])
    return sorted_rows(np.concatenate(cols, 1))


def run_oracle(o, ops):
    """plays `ops` into an OracleOctomap; returns the statistics of every operation (None where it is no insert)"""
    out, active = [], 0
    for op in ops:
        st = None
        if op[0] == "base":
            o.set_base_pose_submap(op[1], op[2], op[3])
        elif op[0] == "active":
            active = op[1]; o.set_active_submap(active)
        elif op[0] == "next":
            active += 1; o.set_active_submap(active)
        elif op[0] == "depth":
            st = o.integrate_depth(op[1], op[2], op[3], op[4])
        elif op[0] == "points":
            st = o.integrate_points(op[1], op[2], op[3], op[4])
        else:
            raise ValueError(op[0])
        out.append(st)
    return out


def run_gpu(g, ops, read=None):
    """plays `ops` into an Octomap; returns {operation index: last_frame_stats()} for the inserts in `read` (default: every insert)"""
    import torch
    out = {}
    for n, op in enumerate(ops):
        if op[0] == "base":
            g.set_base_pose_submap(op[1], op[2], op[3])
        elif op[0] == "active":
            g.active_submap_id[None] = op[1]
        elif op[0] == "next":
            g.switch_to_next_submap()
        elif op[0] == "depth":
            d, tex = np.ascontiguousarray(op[3]), op[4]
            if op[5]:
                d = torch.from_numpy(d.view(np.int16)).cuda()
                tex = torch.from_numpy(np.ascontiguousarray(tex)).cuda() if tex is not None else None
            g.recast_depth_to_map(op[1], op[2], d, tex)
        elif op[0] == "points":
            x, rgb = np.ascontiguousarray(op[3]), op[4]
            if op[5]:
                x = torch.from_numpy(x).cuda()
                rgb = torch.from_numpy(np.ascontiguousarray(rgb)).cuda() if rgb is not None else None
            g.recast_pcl_to_map(op[1], op[2], x, rgb)
        else:
            raise ValueError(op[0])
        if op[0] in ("depth", "points") and (read is None or n in read):
            out[n] = g.last_frame_stats()
    return out


def bricks_of(idx, hN, hNz):
    """the 16^3 bricks (rows of 3) that the leaves `idx` lie in"""
    u = np.asarray(idx, np.int64) + np.array([hN, hN, hNz])
    return np.unique(u >> 4, axis=0)


# ---- 1. arity ------------------------------------------------------------------------------------------------------------------
ARITY_CASES = [(3, [12.8, 12.8], (729, 729, 6, 6)), (4, [12.8, 12.8], (256, 256, 4, 4)), (3, [12.8, 1.6], (729, 81, 6, 4)), (4, [12.8, 1.6], (256, 64, 4, 3))]


def arity_cfg(K, map_scale):
    return dict(map_scale=map_scale, voxel_scale=0.05, min_occupy_thres=0, min_ray_length=0.3, max_ray_length=5.0, K=K, max_submap_num=4)


def arity_ops():
    """two submaps: depth frames from host and device images and a point cloud each; returns (K, [ops of submap 0, ops of submap 1], base poses)"""
    K, fr = small_stream(4)
    rng = np.random.default_rng(11)
    p0 = rng.uniform(-4, 4, size=(3000, 3)).astype(np.float32)
    p1 = rng.uniform(-4, 4, size=(3001, 3)).astype(np.float32)
    s0 = [("base", 0, fr[0][0], fr[0][1]), ("depth", *fr[0], None, False), ("depth", *fr[1], None, True), ("points", fr[0][0], fr[0][1], p0, None, False)]
    s1 = [("base", 1, fr[2][0], fr[2][1]), ("depth", *fr[2], None, True), ("depth", *fr[3], None, False), ("points", fr[2][0], fr[2][1], p1, None, True)]
    return K, [s0, s1], [(fr[0][0], fr[0][1]), (fr[2][0], fr[2][1])]


# ---- 2. tree edges -------------------------------------------------------------------------------------------------------------
EDGE_CFG = dict(map_scale=[3.2, 1.6], voxel_scale=0.05, min_occupy_thres=0, min_ray_length=0.3, max_ray_length=5.0, K=2, max_submap_num=2)
EDGE_DIMS = dict(N=64, Nz=32, Rxy=6, Rz=5, hN=32, hNz=16, ext_xy=128, ext_z=64)      # cells [-32, 96) x [-32, 96) x [-16, 48)


def edge_cloud():
    """for every axis a point in the cells -hN - 1, -hN, ext - hN - 1 and ext - hN (the other two coordinates inside the tree), a quarter cell off the centre;
    returns (xyz, the cell of every point, whether it is inside the tree)"""
    d, vs = EDGE_DIMS, np.float32(0.05)
    lo = np.array([-d["hN"], -d["hN"], -d["hNz"]]); hi = np.array([d["ext_xy"] - d["hN"], d["ext_xy"] - d["hN"], d["ext_z"] - d["hNz"]])
    cells = []
    for a in range(3):
        for c in (lo[a] - 1, lo[a], hi[a] - 1, hi[a]):
            for other in ((3, 5, 7), (lo[(a + 1) % 3], hi[(a + 2) % 3] - 1, 0)):      # an inner cell, and the tree's corner cells of the other two axes
                row = [0, 0, 0]
                row[a] = c; row[(a + 1) % 3] = other[0]; row[(a + 2) % 3] = other[1]
                cells.append(row)
    cells = np.array(cells, np.int64)
    xyz = ((cells.astype(np.float32) + np.float32(0.25)) * vs).astype(np.float32)
    assert np.array_equal(cell_of(xyz, vs), cells), "an offset rounds across a cell"
    inside = np.all((cells >= lo) & (cells < hi), axis=1)
    return xyz, cells, inside


# ---- 4. a pool that fills ------------------------------------------------------------------------------------------------------
POOL_CFG = dict(map_scale=[12.8, 12.8], voxel_scale=0.05, min_occupy_thres=0, min_ray_length=0.3, max_ray_length=5.0, K=2, max_submap_num=2)
POOL_HN = 128
FOUR_BRICK_K = np.array([50.0, 0, 0, 0, 50.0, 0, 0, 0, 1.0])


def wide_cloud():
    return np.random.default_rng(3).uniform(-3, 3, size=(5000, 3)).astype(np.float32)


def four_brick_cloud():
    """3000 points in the cells [0, 32) x [0, 32) x [0, 16): exactly four bricks of a tree whose hN is a multiple of 16"""
    rng = np.random.default_rng(4)
    xyz = np.stack([rng.uniform(0, 1.55, 3000), rng.uniform(0, 1.55, 3000), rng.uniform(0, 0.77, 3000)], 1).astype(np.float32)
    xyz[:8] = [[0, 0, 0], [1.55, 0, 0], [0, 1.55, 0], [1.55, 1.55, 0], [0, 0, 0.77], [1.55, 0, 0.77], [0, 1.55, 0.77], [1.55, 1.55, 0.77]]
    assert bricks_of(cell_of(xyz, 0.05), POOL_HN, POOL_HN).shape[0] == 4
    return xyz


def four_brick_frame():
    """a 64 x 64 depth image of a wall 1 m in front of a camera with FOUR_BRICK_K at the identity pose: cells [0, 25] x [0, 25] x {20}"""
    return I3, Z3, np.full((64, 64), 1000, np.uint16)


# ---- 5. statistics ring --------------------------------------------------------------------------------------------------------
RING_CFG = dict(EDGE_CFG, texture_enabled=True)
RING_FRAMES = 140
RING_READS_2 = sorted(set(range(7, RING_FRAMES, 8)) | {31, 32, 33, 63, 64, 65, RING_FRAMES - 1})


def ring_ops():
    """140 frames of 50 x 70 (25 x 35 sampled pixels: ragged 16 x 16 tiles on both axes) of a sphere room larger than the tree.  Operation n uses slot (n + 1) % 64 of
    the ring, so 31 and 127 enter a half of it through octo_next_stats (a point cloud, a textured frame) and 63 and 95 through the queued path (device frames);
    host images, a cloud and textured frames surround them."""
    h, w = 50, 70
    K = syn.scaled_intrinsics(h, w)
    rng = np.random.default_rng(21)
    ops = []
    for f in range(RING_FRAMES):
        R, T = syn.camera_pose(f, deg_per_frame=0.6)          # 0 .. 84 degrees: the camera keeps looking into the quadrant the tree extends into
        if f in (31, 65):
            pts = rng.uniform(-2.5, 2.5, size=(500 + f, 3)).astype(np.float32)
            ops.append(("points", R, T, pts, rng.integers(0, 256, size=(pts.shape[0], 3)).astype(np.uint8), f == 65))
            continue
        d = syn.sphere_room_depth(R, T, h, w, radius=2.2 + 0.012 * f, K=K)      # (the room is round and the camera turns about its axis: only the radius tells the frames apart)
        if f in (32, 62, 127):
            ops.append(("depth", R, T, d, rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8), False))
        else:
            ops.append(("depth", R, T, d, None, f not in (30, 64, 96)))
    return K, ops


# ---- 6. group sizes ------------------------------------------------------------------------------------------------------------
COARSE_CFG = dict(map_scale=[12.8, 12.8], voxel_scale=0.5, recast_step=1, min_occupy_thres=0, min_ray_length=0.3, max_ray_length=5.0, K=2, max_submap_num=2)
FINE_CFG = dict(map_scale=[5.12, 5.12], voxel_scale=0.005, min_occupy_thres=0, min_ray_length=0.3, max_ray_length=5.0, K=2, max_submap_num=2)



def wall_frame(h=120, w=160, mm=1000):
    """a flat wall `mm` in front of a camera at the identity pose"""
    return syn.scaled_intrinsics(h, w), I3, Z3, np.full((h, w), mm, np.uint16)


def wave_tiles(K, d, step, vs):
    """the leaf of every sampled pixel of a frame at the identity pose, as the insert computes it in float32, cut into the 4 x 16 tiles of sampled pixels that
    one wave of k_octo_depth_batch handles: returns a list of [<= 64, 3] cell arrays"""
    f = np.float32
    hh, ww = int(f(d.shape[0]) / f(step)), int(f(d.shape[1]) / f(step))
    jj, ii = np.meshgrid(np.arange(hh), np.arange(ww), indexing="ij")
    dep = d[jj * step, ii * step].astype(f) / f(1000.0)
    px = (ii * step).astype(f) - f(K[2]); py = (jj * step).astype(f) - f(K[5])
    cells = np.stack([cell_of(px * dep / f(K[0]), vs), cell_of(py * dep / f(K[4]), vs), cell_of(dep, vs)], -1)
    return [cells[r:r + 4, c:c + 16].reshape(-1, 3) for r in range(0, hh, 4) for c in range(0, ww, 16)]


# ---- 7. depth gate -------------------------------------------------------------------------------------------------------------
GATE_CFG = dict(map_scale=[12.8, 12.8], voxel_scale=0.05, min_occupy_thres=0, min_ray_length=0.3, max_ray_length=3.3333, K=2, max_submap_num=2)
GATE_VALUES = np.array([0, 299, 300, 3333, 3334, 65535], np.uint16)      # 0, thr_min - 1, thr_min, the last and the first integer around thr_max = 3333.3, the largest
GATE_PASS = (300, 3333)


def gate_frame():
    """40 x 60, recast_step 2: the sampled pixel (ii, jj) holds GATE_VALUES[(ii + jj) % 6], its unsampled neighbours 1000 (they must not be read)"""
    h, w = 40, 60
    d = np.full((h, w), 1000, np.uint16)
    jj, ii = np.meshgrid(np.arange(h // 2), np.arange(w // 2), indexing="ij")
    d[::2, ::2] = GATE_VALUES[(ii + jj) % 6]
    return syn.scaled_intrinsics(h, w), I3, Z3, d


# ---- 3. / 9. / 12. clouds with bad points ------------------------------------------------------------------------------------------
def bad_cloud(n_valid=4000, span=3.0, seed=7):
    """valid points in +-span m (some of them, and ZERO_POINTS, in cell (0, 0, 0)) with BAD_POINTS mixed in; returns (cloud, mask of the bad rows)"""
    rng = np.random.default_rng(seed)
    valid = rng.uniform(-span, span, size=(n_valid, 3)).astype(np.float32)
    valid[:ZERO_POINTS.shape[0]] = ZERO_POINTS
    valid[ZERO_POINTS.shape[0]:ZERO_POINTS.shape[0] + 5] = rng.uniform(-0.02, 0.02, size=(5, 3)).astype(np.float32)
    return mix_bad(valid, seed=seed)


# ---- 9. - 11. queries on a TSDF ------------------------------------------------------------------------------------------------------
QUERY_RADIUS = 2.0


def query_scene(cfg):
    """(K, frames, blocks): three frames of a camera at distance 1 from the origin that looks through it at a sphere room (voxel (0, 0, 0) ends observed and
    free), and observed voxels to load at the walls -- a 5 x 5 x 5 block against each of the six faces and one in two opposite corners, free (TSDF 0.2)
    except for every seventh, which is occupied (TSDF -0.1) -- so that the last cell inside a wall reads differently from the first one outside"""
    from oracle import OracleTSDF
    K, frames = small_stream(3, orbit=-1.0, radius=QUERY_RADIUS)
    o = OracleTSDF(**cfg)
    lo = np.array([-(o.N // 2), -(o.N // 2), -(o.Nz // 2)]); hi = lo + np.array([o.N, o.N, o.Nz])
    idx = []
    r5 = np.arange(5)
    for a in range(3):
        for side in (0, 1):
            base = np.array([7, -9, 3])
            base[a] = lo[a] if side == 0 else hi[a] - 5
            idx.append(base + np.stack(np.meshgrid(r5, r5, r5, indexing="ij"), -1).reshape(-1, 3))
    for corner in (lo, hi - 5):
        idx.append(corner + np.stack(np.meshgrid(r5, r5, r5, indexing="ij"), -1).reshape(-1, 3))
    idx = np.unique(np.concatenate(idx), axis=0).astype(np.int16)
    tsdf = np.where(np.arange(idx.shape[0]) % 7 == 3, -0.1, 0.2).astype(np.float16)
    blocks = dict(indices=idx, TSDF=tsdf, W_TSDF=np.ones(idx.shape[0], np.float16), occupy=np.zeros(idx.shape[0], np.int8))
    return K, frames, blocks, lo, hi


def query_bad_points():
    """BAD_POINTS, ZERO_POINTS and the origin, points 10 m out on every axis, and valid points around them"""
    far = np.concatenate([np.eye(3) * 10.0, np.eye(3) * -10.0, [[10.0, 10.0, 10.0], [-10.0, 0.3, 0.2]]]).astype(np.float32)
    valid = np.random.default_rng(31).uniform(-2.5, 2.5, size=(3000, 3)).astype(np.float32)
    special = np.concatenate([BAD_POINTS, ZERO_POINTS, np.zeros((1, 3), np.float32), far])
    pts, is_special = mix_bad(valid, special, seed=31)
    return pts, is_special, special.shape[0]


def wall_points(lo, hi, vs):
    """the last cell inside and the first outside each of the six faces (beside the loaded blocks, and in the corners), a quarter cell off the centre;
    returns (xyz, cells)"""
    cells = []
    for a in range(3):
        for c in (lo[a] - 1, lo[a], lo[a] + 4, hi[a] - 5, hi[a] - 1, hi[a]):
            for other in (np.array([8, -8, 4]), lo + 1, hi - 2):
                row = other.copy(); row[a] = c
                cells.append(row)
    cells = np.array(cells, np.int64)
    xyz = ((cells.astype(np.float32) + np.float32(0.25)) * np.float32(vs)).astype(np.float32)
    assert np.array_equal(cell_of(xyz, vs), cells)
    return xyz, cells


def half_points(vs, kmax=70):
    """points at (k + 0.5) * vs whose float32 quotient by vs is exactly k + 0.5 (round half away from zero decides the cell), on every axis"""
    k = np.arange(-kmax, kmax).astype(np.float32) + np.float32(0.5)
    x = (k * np.float32(vs)).astype(np.float32)
    exact = (x / np.float32(vs)) == k
    x, k = x[exact], k[exact]
    assert (k > 0).sum() >= 10 and (k < 0).sum() >= 10, "too few exact halves"
    assert np.array_equal(cell_of(x, vs), np.where(k > 0, np.ceil(k), np.floor(k)).astype(np.int64))
    rows = []
    for a in range(3):
        p = np.tile(np.array([0.01, -0.01, 0.02], np.float32), (x.shape[0], 1)); p[:, a] = x
        rows.append(p)
    rows.append(np.stack([x, x, x[::-1]], 1))
    return np.concatenate(rows).astype(np.float32)


def ray_set(frames, lo, hi, vs, n=2000, seed=17):
    """(pos, dir) of `n` rays: origins in observed free space (on the cameras' viewing rays), in the unobserved region, on the surface, outside the volume and
    with a NaN, an inf or 1e12; directions of length 1, 0.3, 3 and 0, along the axes, and with a NaN, an inf or a 3e38 component"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, len(frames), n)
    R = np.stack([frames[i][0] for i in f]); T = np.stack([frames[i][1] for i in f])
    view = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.3, 0.3, n), np.ones(n)], 1)
    view = np.einsum("nij,nj->ni", R, view); view /= np.linalg.norm(view, axis=1, keepdims=True)
    pos = T + view * rng.uniform(0.4, 1.6, n)[:, None]                                        # free space between the camera and the wall
    kind = rng.integers(0, 10, n)
    hit_t = -np.einsum("ni,ni->n", T, view) + np.sqrt(np.einsum("ni,ni->n", T, view) ** 2 - (np.einsum("ni,ni->n", T, T) - QUERY_RADIUS ** 2))
    pos[kind == 6] = (T + view * hit_t[:, None])[kind == 6]                                   # on the surface
    pos[kind == 7] = (T - view * rng.uniform(0.2, 1.0, n)[:, None])[kind == 7]                # behind the cameras: unobserved
    out = rng.uniform(-1, 1, size=(n, 3)) * (hi - lo) * vs * 0.5 + np.sign(rng.normal(size=(n, 3))) * (hi - lo) * vs * 0.75 * (rng.integers(0, 3, size=(n, 3)) == 0)
    pos[kind == 8] = out[kind == 8]                                                           # mostly outside the volume
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[1::2] = view[1::2]                                                                      # half of them look where the cameras looked
    dk = rng.integers(0, 12, n)
    d[dk == 7] *= 0.3; d[dk == 8] *= 3.0; d[dk == 9] = 0.0
    ax = np.eye(3)[rng.integers(0, 3, n)] * np.sign(rng.normal(size=(n, 1)))
    d[dk == 10] = ax[dk == 10]
    pos, d = pos.astype(np.float32), d.astype(np.float32)
    bad = np.nonzero(dk == 11)[0]
    for q, i in enumerate(bad):
        d[i, q % 3] = (NAN, INF, -INF, np.float32(3e38))[(q // 3) % 4]                     # (3e38: finite, but a step of it overflows)
    nanpos = np.nonzero(kind == 9)[0]
    for q, i in enumerate(nanpos):
        pos[i, q % 3] = (NAN, INF, np.float32(1e12))[(q // 3) % 3]                          # (1e12: finite, but no int cell)
    finite = np.all(np.isfinite(pos), axis=1) & np.all(np.isfinite(d), axis=1)
    return pos, d, finite

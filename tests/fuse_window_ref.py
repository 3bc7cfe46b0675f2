"""The LDS-window arithmetic of k_fuse_splat_lds (taichislam_amd/csrc/tsl_fuse.hip), restated in numpy float32.

The kernel gives a workgroup one 8^3 block of a source brick, places a window of FW^3 = 15^3 global voxels at `org` = the least floor over the block's
eight corner voxels, one below, and sums the block's corner splats in LDS.  A splat whose corner lies outside the window -- a MISS -- goes straight to
global memory through a branch of its own and is counted (option "fuse_window_misses").  Which splats miss is a pure function of the source's index list,
the f32 pose and the two geometries: this file computes it, so that the GPU tests can require the counter to EQUAL the prediction and can name the
global voxels (and bricks) that only the miss branch reaches.

Every expression is evaluated in the kernel's written order with float32 array arithmetic: one rounding per operation, nothing fused (the library is
built with -ffp-contract=off).  No number here comes from the HIP path."""
import numpy as np

FW = 15
F32 = np.float32


def pose_f32(R, T):
    """the float64 pose rounded to f32 once, as upload_poses does"""
    return np.asarray(R, np.float64).astype(F32).reshape(3, 3), np.asarray(T, np.float64).astype(F32).reshape(3)


def _transform(idx, R, T, vs):
    """x / vs per axis for integer voxel indices idx [n, 3]: ((R[a,0]*p0 + R[a,1]*p1) + R[a,2]*p2) + T[a], p = (float)i * vs"""
    p = idx.astype(F32) * vs
    f = np.empty(p.shape, F32)
    for a in range(3):
        x = ((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + T[a]
        f[:, a] = x / vs
    assert f.dtype == F32
    return f


def splat_table(indices, R, T, vs, src_dims, dst_dims, fw=FW):
    """Every corner splat (corners 1..7) of every source voxel that lands inside the global volume.

    indices   int [n, 3] observed source voxels (signed, centred); src_dims = (N, Nz) of the submap collection, dst_dims = (N, Nz) of the global map
    R, T      the pose, rounded to f32 here
    Returns a dict of arrays over the splats: "dst" int32 [m, 3] global voxel, "miss" bool [m] (outside the block's fw^3 window), "block" int64 [m] a key
    of the source 8^3 block the splat came from."""
    R, T = pose_f32(R, T)
    vs = F32(vs)
    idx = np.asarray(indices, np.int32).reshape(-1, 3)
    half_s = np.array([src_dims[0] // 2, src_dims[0] // 2, src_dims[1] // 2], np.int32)
    half_d = np.array([dst_dims[0] // 2, dst_dims[0] // 2, dst_dims[1] // 2], np.int32)
    ext_d = np.array([dst_dims[0], dst_dims[0], dst_dims[1]], np.int32)
    # the 8^3 blocks are aligned in the UNSIGNED brick coordinates ui = i + N / 2
    blk0 = (((idx + half_s) >> 3) << 3) - half_s                         # first voxel of the voxel's block
    bkey = ((blk0[:, 0].astype(np.int64) + 32768) << 32) | ((blk0[:, 1].astype(np.int64) + 32768) << 16) | (blk0[:, 2].astype(np.int64) + 32768)
    ukey, first, inv = np.unique(bkey, return_index=True, return_inverse=True)
    ub0 = blk0[first]
    org = np.full(ub0.shape, 1 << 30, np.int32)
    for c8 in range(8):
        corner = ub0 + 7 * np.array([(c8 >> 2) & 1, (c8 >> 1) & 1, c8 & 1], np.int32)
        org = np.minimum(org, np.floor(_transform(corner, R, T, vs)).astype(np.int32) - 1)
    org = org[inv.reshape(-1)]
    f = _transform(idx, R, T, vs)
    lo = np.floor(f).astype(np.int32)
    dst, miss, blk = [], [], []
    for c in range(1, 8):
        ci = lo + np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1], np.int32)
        inside = ((ci >= -half_d) & (ci < ext_d - half_d)).all(1)       # in_volume of the global map
        w = ci - org
        out = ((w < 0) | (w >= fw)).any(1)
        dst.append(ci[inside]); miss.append(out[inside]); blk.append(bkey[inside])
    return {"dst": np.concatenate(dst), "miss": np.concatenate(miss), "block": np.concatenate(blk)}


def window_misses(indices, R, T, vs, src_dims, dst_dims, fw=FW):
    """(number of missed corner splats, int32 [k, 3] the distinct global voxels they land on)"""
    t = splat_table(indices, R, T, vs, src_dims, dst_dims, fw)
    hit = t["dst"][t["miss"]]
    return int(t["miss"].sum()), np.unique(hit, axis=0) if hit.size else np.zeros((0, 3), np.int32)


def brick_ids(dst, dst_dims):
    """brick_of: the id of the 16^3 brick of each global voxel (the index of the merge's touched-brick mask)"""
    N, Nz = dst_dims
    u = np.asarray(dst, np.int64) + np.array([N // 2, N // 2, Nz // 2], np.int64)
    return ((u[:, 0] >> 4) * (N // 16) + (u[:, 1] >> 4)) * (Nz // 16) + (u[:, 2] >> 4)


def bricks_reached_only_with_misses(tables, dst_dims):
    """Global bricks ALL of whose splats (over the given splat tables, one per submap) come from source blocks that have a miss, i.e. bricks that enter
    the map -- and the merge's mask -- only through the miss branch or through the flush of such a block.  Also returns those reached by misses alone."""
    b, blk_has_miss, miss = [], [], []
    for t in tables:
        bad_blocks = np.unique(t["block"][t["miss"]])
        b.append(brick_ids(t["dst"], dst_dims)); blk_has_miss.append(np.isin(t["block"], bad_blocks)); miss.append(t["miss"])
    b, blk_has_miss, miss = np.concatenate(b), np.concatenate(blk_has_miss), np.concatenate(miss)
    clean = np.unique(b[~blk_has_miss])
    hit = np.unique(b[~miss])
    allb = np.unique(b)
    return np.setdiff1d(allb, clean), np.setdiff1d(allb, hit)

"""A numpy restatement of brick eviction (tests/test_evict_cpu.py, tests/test_evict_gpu.py): the selection rules over a key list, the hole-filling plan that
keeps the pool dense, and the brick ranges of a voxel box.  Nothing here reads the product.

A brick key is s * nb3 + (bi * nbx + bj) * nbz + bk; brick (bi, bj, bk) holds the voxels 16 * bi - N / 2 .. 16 * bi + 15 - N / 2 of the map-centred index
(k with Nz / 2).  `owner` is the key of every pool brick in pool order."""
import numpy as np

BRK = 16


def geometry(N, Nz):
    """(nbx, nbz, nb3, hN, hNz) of a volume of N x N x Nz voxels"""
    nbx, nbz = -(-N // BRK), -(-Nz // BRK)
    return nbx, nbz, nbx * nbx * nbz, N // 2, Nz // 2


def make_key(sid, bi, bj, bk, N, Nz):
    nbx, nbz, nb3, _, _ = geometry(N, Nz)
    return np.asarray(sid, np.int64) * nb3 + (np.asarray(bi, np.int64) * nbx + bj) * nbz + bk


def key_of_voxel(idx, sid, N, Nz):
    """the key of the brick that holds voxel (i, j, k) in slot sid"""
    _, _, _, hN, hNz = geometry(N, Nz)
    i = np.asarray(idx, np.int64).reshape(-1, 3)
    return make_key(sid, (i[:, 0] + hN) >> 4, (i[:, 1] + hN) >> 4, (i[:, 2] + hNz) >> 4, N, Nz)


def local_index(idx, N, Nz):
    """the element of a plane row that holds voxel (i, j, k)"""
    _, _, _, hN, hNz = geometry(N, Nz)
    i = np.asarray(idx, np.int64).reshape(-1, 3)
    return (((i[:, 0] + hN) & 15) << 8) | (((i[:, 1] + hN) & 15) << 4) | ((i[:, 2] + hNz) & 15)


def brick_range(keys, N, Nz):
    """(sid [n], lo [n, 3], hi [n, 3]): the slot and the inclusive voxel range of every brick"""
    nbx, nbz, nb3, hN, hNz = geometry(N, Nz)
    k = np.asarray(keys, np.int64).reshape(-1)
    b = k % nb3
    lo = np.stack([BRK * (b // (nbz * nbx)) - hN, BRK * ((b // nbz) % nbx) - hN, BRK * (b % nbz) - hNz], -1)
    return k // nb3, lo, lo + (BRK - 1)


def bricks_of_box(lo, hi, N, Nz):
    """(first [3], last [3]): the brick coordinates the inclusive voxel box lo .. hi reaches on every axis (not clamped to the volume)"""
    _, _, _, hN, hNz = geometry(N, Nz)
    h = np.array([hN, hN, hNz])
    return (np.asarray(lo, np.int64) + h) >> 4, (np.asarray(hi, np.int64) + h) >> 4


def select_box(owner, rule, lo, hi, sid, N, Nz):
    """bool [n]: rule "keep_box" selects the bricks (of slot sid; -1 = all) that do not intersect the box, "clear_box" those wholly inside it"""
    s, b0, b1 = brick_range(owner, N, Nz)
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    meets = ((b0 <= hi) & (b1 >= lo)).all(1)
    inside = ((b0 >= lo) & (b1 <= hi)).all(1)
    mine = np.ones(s.shape, bool) if sid < 0 else s == sid
    return mine & (~meets if rule == "keep_box" else inside)


def select_keys(owner, keys):
    """(bool [n], missing): the pool bricks a key list names; duplicates count once, `missing` = the distinct keys without a brick"""
    owner = np.asarray(owner, np.int64)
    u = np.unique(np.asarray(keys, np.int64))
    return np.isin(owner, u), int((~np.isin(u, owner)).sum())


def plan(owner, sel):
    """The release: (new_owner [new_top], moves [(dst, src)], payload_keys ascending).  Holes = selected pool indices below new_top, movers = kept
    ones at or above it, both ascending; mover k goes to hole k."""
    owner, sel = np.asarray(owner, np.int64), np.asarray(sel, bool)
    top = owner.shape[0]
    new_top = top - int(sel.sum())
    p = np.arange(top)
    holes, movers = p[sel & (p < new_top)], p[~sel & (p >= new_top)]
    assert holes.shape == movers.shape
    new_owner = owner[:new_top].copy()
    new_owner[holes] = owner[movers]
    return new_owner, list(zip(holes.tolist(), movers.tolist())), np.sort(owner[sel])

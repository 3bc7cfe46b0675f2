"""numpy restatement of the frontier extraction (include/taichislam_hip.h "exploration frontiers") over an export_sparse
dictionary: dense class array, neighbour tests, union-find labelling, the records and rows in exactly the order of the ABI.  No scipy."""
import numpy as np

OUT, UNKNOWN, FREE, OCC = 0, 1, 2, 3
CLUSTER_DTYPE = np.dtype({"names": ["key", "count", "sum", "nsum", "lo", "hi"],
                          "formats": [np.int32, np.int32, (np.int64, 3), (np.int32, 3), (np.int16, 3), (np.int16, 3)],
                          "offsets": [0, 4, 8, 32, 44, 50], "itemsize": 64})
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))          # mask bits 0 .. 5
# the 13 lexicographically positive neighbour offsets: every unordered pair of neighbours once
HALF = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0)]


def surf_thres(voxel_scale):
    """the map's surface threshold as the library holds it: (float)(voxel_scale * 1.8)"""
    return np.float32(float(voxel_scale) * 1.8)


def class_array(e, N, Nz, thres):
    """u8 [N + 2, N + 2, Nz + 2]: the class of every voxel of the volume, with a rim of OUT (no class) around it; a voxel the export does not hold is UNKNOWN"""
    c = np.zeros((N + 2, N + 2, Nz + 2), np.uint8)
    c[1:-1, 1:-1, 1:-1] = UNKNOWN
    idx = np.asarray(e["indices"]).astype(np.int64).reshape(-1, 3)
    t = np.asarray(e["TSDF"]).view(np.float16).astype(np.float32).reshape(-1)
    u = idx + np.array([N // 2 + 1, N // 2 + 1, Nz // 2 + 1])
    c[u[:, 0], u[:, 1], u[:, 2]] = np.where(t < np.float32(thres), OCC, FREE).astype(np.uint8)
    return c


def _shift(a, d):
    """a[x + d] over the interior of the padded array"""
    n0, n1, n2 = a.shape
    return a[1 + d[0]:n0 - 1 + d[0], 1 + d[1]:n1 - 1 + d[1], 1 + d[2]:n2 - 1 + d[2]]


def frontier_mask(c, Nz, min_unknown=1, clear_of_occupied=False, k_range=None):
    """(frontier bool [N, N, Nz], mask u8 [N, N, Nz]) from the padded class array"""
    free = _shift(c, (0, 0, 0)) == FREE
    mask = np.zeros(free.shape, np.uint8)
    for b, d in enumerate(FACES):
        mask |= ((_shift(c, d) == UNKNOWN).astype(np.uint8) << b).astype(np.uint8)
    cnt = np.zeros(free.shape, np.uint8)
    for b in range(6):
        cnt += (mask >> b) & 1
    fr = free & (cnt >= max(1, int(min_unknown)))
    if clear_of_occupied:
        occ = np.zeros(free.shape, bool)
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                for d in (-1, 0, 1):
                    occ |= _shift(c, (a, b, d)) == OCC
        fr &= ~occ
    if k_range is not None and k_range[0] <= k_range[1]:
        k = np.arange(Nz) - Nz // 2
        fr &= ((k >= k_range[0]) & (k <= k_range[1]))[None, None, :]
    return fr, np.where(fr, mask, 0).astype(np.uint8)


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def label(u, N, Nz, connectivity=26):
    """root index per voxel of u (int64 [n, 3] unsigned coordinates, sorted by key): union-find, roots are the smaller index -- the least key of the component"""
    n = u.shape[0]
    key = (u[:, 0] * N + u[:, 1]) * Nz + u[:, 2]
    par = list(range(n))
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    for d in HALF:
        if abs(d[0]) + abs(d[1]) + abs(d[2]) > limit:
            continue
        v = u + np.array(d)
        ok = (v >= 0).all(1) & (v[:, 0] < N) & (v[:, 1] < N) & (v[:, 2] < Nz)
        kv = (v[:, 0] * N + v[:, 1]) * Nz + v[:, 2]
        pos = np.searchsorted(key, kv)
        pos[pos >= n] = n - 1
        hit = np.nonzero(ok & (key[pos] == kv))[0]
        for a, b in zip(hit.tolist(), pos[hit].tolist()):
            ra, rb = _find(par, a), _find(par, b)
            if ra != rb:
                par[max(ra, rb)] = min(ra, rb)
    return np.array([_find(par, x) for x in range(n)], np.int64)


def extract(e, N, Nz, voxel_scale, free_thres=None, k_range=None, min_unknown=1, connectivity=26, min_cluster=1, clear_of_occupied=False):
    """The result of tsl_tsdf_frontier_extract for the map whose export_sparse dictionary is `e`: {indices int16 [n, 3], mask u8 [n], cluster int32 [n],
    keys int64 [n], clusters CLUSTER_DTYPE [m]}, voxels and clusters sorted by key.  k_range: (k_min, k_max) voxel layers or None."""
    assert N * N * Nz < 2 ** 31
    thres = surf_thres(voxel_scale) if free_thres is None else np.float32(free_thres)
    c = class_array(e, N, Nz, thres)
    fr, mask = frontier_mask(c, Nz, min_unknown, clear_of_occupied, k_range)
    u = np.argwhere(fr).astype(np.int64)                      # C order = ascending key
    key = (u[:, 0] * N + u[:, 1]) * Nz + u[:, 2]
    m6 = mask[u[:, 0], u[:, 1], u[:, 2]]
    root = label(u, N, Nz, connectivity or 26)
    idx = u - np.array([N // 2, N // 2, Nz // 2])
    roots, inv, counts = np.unique(root, return_inverse=True, return_counts=True)      # ascending root index = ascending least key
    keep = counts >= max(1, int(min_cluster))
    row = np.cumsum(keep) - 1
    vk = keep[inv]
    clusters = np.zeros(int(keep.sum()), CLUSTER_DTYPE)
    cl = row[inv][vk].astype(np.int32)
    idx_k, m_k = idx[vk], m6[vk]
    clusters["key"] = key[roots[keep]]
    clusters["count"] = counts[keep]
    for a in range(3):
        np.add.at(clusters["sum"][:, a], cl, idx_k[:, a])
        np.add.at(clusters["nsum"][:, a], cl, ((m_k >> (2 * a + 1)) & 1).astype(np.int32) - ((m_k >> (2 * a)) & 1).astype(np.int32))
        lo = np.full(clusters.shape[0], 32767, np.int64); hi = np.full(clusters.shape[0], -32768, np.int64)
        np.minimum.at(lo, cl, idx_k[:, a]); np.maximum.at(hi, cl, idx_k[:, a])
        clusters["lo"][:, a] = lo; clusters["hi"][:, a] = hi
    return {"indices": idx_k.astype(np.int16), "mask": m_k.astype(np.uint8), "cluster": cl, "keys": key[vk], "clusters": clusters}


def room_quantities(r, N, Nz):
    """(frontier voxels, clusters, bricks the largest cluster's voxels lie in)"""
    big = int(np.argmax(r["clusters"]["count"]))
    u = r["indices"][r["cluster"] == big].astype(np.int64) + np.array([N // 2, N // 2, Nz // 2])
    return r["indices"].shape[0], r["clusters"].shape[0], np.unique(u >> 4, axis=0).shape[0]


def assert_equal(got, want, what=""):
    """every array of the ABI's result, exactly"""
    assert got["indices"].shape == want["indices"].shape, f"{what}: {got['indices'].shape[0]} voxels, expected {want['indices'].shape[0]}"
    assert got["clusters"].shape == want["clusters"].shape, f"{what}: {got['clusters'].shape[0]} clusters, expected {want['clusters'].shape[0]}"
    for k in ("indices", "mask", "cluster"):
        assert np.array_equal(np.asarray(got[k]), want[k]), f"{what}: {k} differs"
    for k in CLUSTER_DTYPE.names:
        assert np.array_equal(got["clusters"][k], want["clusters"][k]), f"{what}: cluster field {k} differs"

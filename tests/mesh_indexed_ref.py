"""The indexed marching-cubes mesh restated in numpy over an export_sparse dictionary (include/taichislam_hip.h, "indexed mesh"): the oracle for
tests/test_mesh_indexed_cpu.py and tests/test_mesh_indexed_gpu.py.  Cells, validity, case table, sign and eps snap are those of generate_mesh(1); a vertex is
a grid edge (lower-corner voxel, axis), rows ascend in edge key, triangles in cell key.  Every f16 step takes np.float16 operands: numpy evaluates add,
subtract, multiply and square root of halves in f32 and rounds once, which is what the kernels do."""
import os
import re

import numpy as np

EPS = np.float32(1e-6)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNER = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])          # grid_xyz :196-206
EDGE = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 7], [7, 4], [0, 4], [1, 5], [2, 6], [3, 7]])      # edges_grid_id :208-221
# table edge -> (offset of its lower corner, axis): the grid edge it is, whichever way the table walks it
EDGE_LOW = np.minimum(CORNER[EDGE[:, 0]], CORNER[EDGE[:, 1]])
EDGE_AXIS = np.argmax(CORNER[EDGE[:, 0]] != CORNER[EDGE[:, 1]], axis=1)


def load_table():
    """(TRI int [256, 5, 3] edge ids, -1 where the case has no such triangle; NTRI int [256]) from the packed table of oracle/mc_tables_data.h"""
    txt = open(os.path.join(ROOT, "oracle", "mc_tables_data.h")).read()
    words = [int(w, 16) for w in re.findall(r"0x([0-9A-Fa-f]{16})ull", txt)]
    assert len(words) == 256
    tri = -np.ones((256, 5, 3), np.int64)
    for c, w in enumerate(words):
        n = 0
        for t in range(5):
            if (w >> (12 * t)) & 0xf != 0xf:
                tri[c, n] = [(w >> (4 * (3 * t + q))) & 0xf for q in range(3)]
                n += 1
    return tri, (tri[:, :, 0] >= 0).sum(1)


TRI, NTRI = load_table()


def cell_key(ijk, N, Nz):
    """int64 cell key of signed voxel indices [n, 3]: brick-major, then the voxel's place in its brick"""
    u = np.asarray(ijk, np.int64) + np.array([N // 2, N // 2, Nz // 2])
    nbx, nbz = N // 16, Nz // 16
    b = ((u[:, 0] >> 4) * nbx + (u[:, 1] >> 4)) * nbz + (u[:, 2] >> 4)
    return b * 4096 + ((u[:, 0] & 15) << 8 | (u[:, 1] & 15) << 4 | (u[:, 2] & 15))


def _rnd(x):
    """ti.round: half away from zero"""
    r = np.trunc(x)
    return np.where(np.abs(x - r) >= np.float32(0.5), r + np.copysign(np.float32(1), x), r)


def extract(e, N, Nz, voxel_scale, thres, texture=False):
    """The canonical indexed mesh of the map `e` (export_sparse / export_submap): {"vertices", "normals", "colors" | None, "edges", "triangles", "keys"}"""
    idx = np.asarray(e["indices"], np.int64).reshape(-1, 3)
    out = {"vertices": np.zeros((0, 3), np.float32), "normals": np.zeros((0, 3), np.float32), "colors": np.zeros((0, 3), np.float32) if texture else None,
           "edges": np.zeros((0, 4), np.int16), "triangles": np.zeros((0, 3), np.int32), "keys": np.zeros(0, np.int64), "cell_keys": np.zeros(0, np.int64)}
    if idx.shape[0] == 0:
        return out
    # dense padded value / observed arrays over the bounding box: what lies outside it, or outside the volume, reads 0 and is unobserved
    lo = idx.min(0) - 2
    dim = idx.max(0) + 3 - lo
    val = np.zeros(dim, np.float16)
    obs = np.zeros(dim, bool)
    loc = idx - lo
    val[loc[:, 0], loc[:, 1], loc[:, 2]] = np.asarray(e["TSDF"]).view(np.float16)
    obs[loc[:, 0], loc[:, 1], loc[:, 2]] = True
    col = None
    if texture:
        col = np.zeros(tuple(dim) + (3,), np.float16)
        col[loc[:, 0], loc[:, 1], loc[:, 2]] = np.asarray(e["color"]).view(np.float16).reshape(-1, 3)
    v32 = val.astype(np.float32)
    sx, sy, sz = dim - 1

    def sh(a, d):
        return a[d[0]:d[0] + sx, d[1]:d[1] + sy, d[2]:d[2] + sz]
    valid = sh(obs, (0, 0, 0)) & (sh(v32, (0, 0, 0)) < np.float32(thres))
    cube = np.zeros((sx, sy, sz), np.int64)
    for q in range(8):
        valid &= sh(obs, CORNER[q])
        cube |= (sh(v32, CORNER[q]) < 0).astype(np.int64) << q
    cells = np.argwhere(valid & (NTRI[cube] > 0))
    if cells.shape[0] == 0:
        return out
    ck = cell_key(cells + lo, N, Nz)
    o = np.argsort(ck, kind="stable")
    cells, ck = cells[o], ck[o]
    cc = cube[cells[:, 0], cells[:, 1], cells[:, 2]]
    rep = np.repeat(np.arange(cells.shape[0]), NTRI[cc])                      # a row per triangle, in cell-key order, then in the order of the table row
    slot = np.concatenate([np.arange(n) for n in NTRI[cc]])
    te = TRI[cc[rep], slot]                                                    # [T, 3] table edges
    owner = cells[rep][:, None, :] + EDGE_LOW[te]                              # [T, 3, 3] the voxel that owns each corner's edge (box coordinates)
    axis = EDGE_AXIS[te]
    ek = cell_key((owner + lo).reshape(-1, 3), N, Nz) * 3 + axis.reshape(-1)
    keys, first = np.unique(ek, return_index=True)
    tris = np.searchsorted(keys, ek).reshape(-1, 3).astype(np.int32)
    p0i = owner.reshape(-1, 3)[first]
    ax = axis.reshape(-1)[first]
    p1i = p0i + np.eye(3, dtype=np.int64)[ax]
    with np.errstate(all="ignore"):
        h0, h1 = val[p0i[:, 0], p0i[:, 1], p0i[:, 2]], val[p1i[:, 0], p1i[:, 1], p1i[:, 2]]
        v0, v1 = h0.astype(np.float32), h1.astype(np.float32)
        p0, p1 = (p0i + lo).astype(np.float32), (p1i + lo).astype(np.float32)
        mu = (np.float32(0) - v0) / (h1 - h0).astype(np.float32)               # (valp2 - valp1 of two f16 values is an f16 operation)
        snap0 = np.abs(np.float32(0) - v0) < EPS
        snap1 = ~snap0 & (np.abs(np.float32(0) - v1) < EPS)
        mu = np.where(snap0 | snap1, np.float32(0), mu).astype(np.float32)
        pv = (p0 + mu[:, None] * (p1 - p0)).astype(np.float32)
        pv = np.where(snap0[:, None], p0, np.where(snap1[:, None], p1, pv)).astype(np.float32)
        verts = (pv * np.float32(voxel_scale)).astype(np.float32)
        # generate_normal :84-93 around the voxel nearest to the vertex
        q = _rnd(pv).astype(np.int64) - lo
        q = np.clip(q, 1, dim - 2)                                               # (a NaN vertex: anything inside the box)
        n = []
        for a in range(3):
            d = np.eye(3, dtype=np.int64)[a]
            n.append(val[q[:, 0] + d[0], q[:, 1] + d[1], q[:, 2] + d[2]] - val[q[:, 0] - d[0], q[:, 1] - d[1], q[:, 2] - d[2]])
        nrm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        inv = (np.float32(1) / nrm.astype(np.float32)).astype(np.float16)
        normals = np.stack([(inv * c).astype(np.float32) for c in n], 1)
        colors = None
        if texture:
            c0, c1 = col[p0i[:, 0], p0i[:, 1], p0i[:, 2]], col[p1i[:, 0], p1i[:, 1], p1i[:, 2]]
            mix = (c0.astype(np.float32) + mu[:, None] * (c1 - c0).astype(np.float32)).astype(np.float16).astype(np.float32)
            z0, z1 = c0[:, :1].astype(np.float32) == 0, c1[:, :1].astype(np.float32) == 0
            colors = np.where(z0, c1.astype(np.float32), np.where(z1, c0.astype(np.float32), mix)).astype(np.float32)
    edges = np.concatenate([p0i + lo, ax[:, None]], 1).astype(np.int16)
    return {"vertices": verts, "normals": normals, "colors": colors, "edges": edges, "triangles": tris, "keys": keys, "cell_keys": ck[rep]}


def _same(a, b):
    """equal bit for bit, a NaN matching a NaN of any payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.uint32), np.where(nb, 0, b).view(np.uint32))


def assert_equal(got, want, what):
    """got: get_indexed_mesh() (or extract()); want: extract().  Counts and all five arrays, row for row, nothing sorted."""
    nv, nt = want["vertices"].shape[0], want["triangles"].shape[0]
    if "num_vertices" in got:
        assert (got["num_vertices"], got["num_triangles"]) == (nv, nt), f"{what}: counts {got['num_vertices']}, {got['num_triangles']} != {nv}, {nt}"
    for k in ("edges", "triangles", "vertices", "normals"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, f"{what}: {k} is {got[k].dtype} {got[k].shape}, want {want[k].dtype} {want[k].shape}"
        if not _same(got[k], want[k]):
            bad = np.nonzero((got[k] != want[k]).any(1) & ~(np.isnan(got[k].astype(np.float64)).any(1) & np.isnan(want[k].astype(np.float64)).any(1)))[0]
            r = bad[0] if bad.size else 0
            raise AssertionError(f"{what}: {k} differs in {bad.size} of {want[k].shape[0]} rows, first row {r}: {got[k][r]} != {want[k][r]}")
    if want["colors"] is not None:
        assert got["colors"] is not None and _same(got["colors"], want["colors"]), f"{what}: colors differ"


def check_invariants(m, what):
    """what every canonical mesh satisfies: keys strictly ascending, indices in range, every vertex used, cells ascending"""
    k, t = m["keys"], m["triangles"]
    assert (np.diff(k) > 0).all(), f"{what}: edge keys do not ascend strictly"
    assert (np.diff(m["cell_keys"]) >= 0).all(), f"{what}: cell keys do not ascend"
    if t.size:
        assert t.min() >= 0 and t.max() < k.shape[0], f"{what}: an index out of range"
        assert np.unique(t).shape[0] == k.shape[0], f"{what}: a vertex no triangle names"
    e = m["edges"].astype(np.int64)
    assert ((e[:, 3] >= 0) & (e[:, 3] <= 2)).all()


def edge_of_soup_vertex(xyz, voxel_scale):
    """(lower corner int64 [n, 3], axis int64 [n], ambiguous bool [n]) of soup vertices: coordinates within 1e-3 of an integer are integers, the one
    fractional coordinate gives the axis and its floor the lower corner; rows with three integer coordinates are ambiguous (corner and axis meaningless)"""
    q = np.asarray(xyz, np.float64) / float(voxel_scale)
    r = np.rint(q)
    whole = np.abs(q - r) < 1e-3
    nfrac = (~whole).sum(1)
    assert (nfrac <= 1).all(), "a soup vertex off the grid's edges"
    amb = nfrac == 0
    axis = np.argmax(~whole, axis=1)
    low = np.where(whole, r, np.floor(q)).astype(np.int64)
    return low, axis, amb


def soup_relation(soup_xyz, mesh, N, Nz, voxel_scale, what):
    """The soup of the same map against the indexed mesh: every soup vertex with a recoverable edge lies within 2^-10 voxel of the mesh's vertex on that
    edge; the two name the same edges; the ambiguous share is <= 1 %.  Returns (ambiguous rows, largest distance in voxels)."""
    low, axis, amb = edge_of_soup_vertex(soup_xyz, voxel_scale)
    n = soup_xyz.shape[0]
    share = amb.sum() / max(n, 1)
    print(f"{what}: {n} soup vertices, {int(amb.sum())} ambiguous ({100 * share:.2f} %)")
    assert share <= 0.01, f"{what}: {100 * share:.2f} % of the soup rows are ambiguous"
    ok = ~amb
    ek = cell_key(low[ok], N, Nz) * 3 + axis[ok]
    row = np.searchsorted(mesh["keys"], ek)
    found = (row < mesh["keys"].shape[0])
    found[found] = mesh["keys"][row[found]] == ek[found]
    assert found.all(), f"{what}: {int((~found).sum())} soup vertices on edges the mesh does not hold"
    d = np.abs(np.asarray(soup_xyz, np.float64)[ok] - mesh["vertices"][row].astype(np.float64)).max(1) / float(voxel_scale)
    worst = float(d.max()) if d.size else 0.0
    print(f"{what}: largest distance soup vertex - mesh vertex {worst:.4e} voxel (bound 2^-10 = {2.0 ** -10:.4e})")
    assert worst <= 2.0 ** -10, f"{what}: a soup vertex {worst} voxel from its edge's vertex"
    # every vertex is named by some soup vertex: the ambiguous rows stand for an edge the others do not cover only at a snapped corner
    named = np.zeros(mesh["keys"].shape[0], bool)
    named[row] = True
    if amb.any() and not named.all():
        c = np.rint(np.asarray(soup_xyz, np.float64)[amb] / float(voxel_scale)).astype(np.int64)
        corner = {tuple(x) for x in c}
        e = mesh["edges"].astype(np.int64)
        for r in np.nonzero(~named)[0]:
            up = e[r, :3] + np.eye(3, dtype=np.int64)[e[r, 3]]
            if tuple(e[r, :3]) in corner or tuple(up) in corner:
                named[r] = True
    assert named.all(), f"{what}: {int((~named).sum())} mesh vertices no soup vertex names"
    return int(amb.sum()), worst


def manifold(tris, nv, what):
    """closed 2-manifold: every undirected index pair in exactly two triangles, once in each direction, and V - E + F = 2"""
    t = np.asarray(tris, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    assert (d[:, 0] != d[:, 1]).all(), f"{what}: a degenerate triangle"
    dk = d[:, 0] * nv + d[:, 1]
    assert np.unique(dk).shape[0] == dk.shape[0], f"{what}: a directed edge occurs twice"
    uk = np.minimum(d[:, 0], d[:, 1]) * nv + np.maximum(d[:, 0], d[:, 1])
    u, c = np.unique(uk, return_counts=True)
    assert (c == 2).all(), f"{what}: {int((c != 2).sum())} of {u.shape[0]} undirected edges are not in exactly two triangles"
    chi = nv - u.shape[0] + t.shape[0]
    assert chi == 2, f"{what}: V - E + F = {chi}"

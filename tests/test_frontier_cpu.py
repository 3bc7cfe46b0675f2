"""The numpy restatement of the frontier extraction (tests/frontier_ref.py) against analytic answers, against an independent flood fill, and over the
oracle's map of the room scene.  No GPU: tests/test_frontier_gpu.py holds the kernels to this restatement."""
from collections import deque

import numpy as np
import pytest

import frontier_ref as ref
import frontier_scenes as fs
from util import SMALL

VS = SMALL["voxel_scale"]


def _through_oracle(sc, geo="SMALL", sid=0):
    """the scene imported into the oracle and exported again: what the GPU tests feed the restatement"""
    from oracle import OracleTSDF
    g = fs.GEOMETRIES[geo]
    o = OracleTSDF(**g["cfg"])
    assert (o.N, o.Nz) == (g["N"], g["Nz"])
    o.import_sparse(sid, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    o.set_active_submap(sid)
    return o.export_sparse(), o.N, o.Nz


def _extract(sc, geo="SMALL", **kw):
    g = fs.GEOMETRIES[geo]
    return ref.extract(fs.place(sc, geo), g["N"], g["Nz"], VS, **kw)


def test_shell_across_a_brick_corner_is_analytic():
    e, N, Nz = _through_oracle(fs.shell())
    r = ref.extract(e, N, Nz, VS)
    assert r["indices"].shape[0] == fs.SHELL_VOXELS and r["clusters"].shape[0] == 1
    idx = r["indices"].astype(int)
    on = ((idx == -10) | (idx == 9))
    assert (on.sum(1) >= 1).all()                                            # every frontier voxel lies on the cube's surface
    assert np.array_equal(np.array([bin(m).count("1") for m in r["mask"]]), on.sum(1))      # faces one bit, edges two, corners three
    want = (idx[:, 0] == -10) * 1 + (idx[:, 0] == 9) * 2 + (idx[:, 1] == -10) * 4 + (idx[:, 1] == 9) * 8 + (idx[:, 2] == -10) * 16 + (idx[:, 2] == 9) * 32
    assert np.array_equal(r["mask"], want.astype(np.uint8))
    c = r["clusters"][0]
    assert c["count"] == fs.SHELL_VOXELS and c["key"] == ((118 * 256) + 118) * 256 + 118
    assert c["sum"].tolist() == [-fs.SHELL_VOXELS // 2] * 3 and c["nsum"].tolist() == [0, 0, 0]      # symmetric about -0.5
    assert c["lo"].tolist() == [-10] * 3 and c["hi"].tolist() == [9] * 3
    assert np.all(np.diff(r["keys"]) > 0) and (r["cluster"] == 0).all()
    r2, r3 = ref.extract(e, N, Nz, VS, min_unknown=2), ref.extract(e, N, Nz, VS, min_unknown=3)
    assert r2["indices"].shape[0] == fs.SHELL_EDGES_CORNERS and r2["clusters"].shape[0] == 1
    assert r3["indices"].shape[0] == fs.SHELL_CORNERS and r3["clusters"].shape[0] == 8 and (r3["clusters"]["count"] == 1).all()
    assert ref.extract(e, N, Nz, VS, min_unknown=4)["indices"].shape[0] == 0


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
def test_diagonal_contact_depends_on_the_connectivity(geo):
    for conn, n in fs.DIAGONAL_CLUSTERS.items():
        r = _extract(fs.diagonal(), geo, connectivity=conn)
        assert r["indices"].shape[0] == 32 and r["clusters"].shape[0] == n, (geo, conn)
        assert sorted(r["clusters"]["count"].tolist()) == sorted([16] * (4 - n) + [8] * (2 * n - 4))
    assert _extract(fs.diagonal(), geo, connectivity=6, min_cluster=9)["indices"].shape[0] == 0
    assert _extract(fs.diagonal(), geo, connectivity=26, min_cluster=9)["clusters"].shape[0] == 2


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
def test_the_volume_wall_is_no_frontier(geo):
    g = fs.GEOMETRIES[geo]
    r = _extract(fs.wall(geo), geo)
    assert r["indices"].shape[0] == fs.WALL_VOXELS and r["clusters"].shape[0] == 1
    axis, top = (2, g["Nz"] // 2 - 1) if g["swap"] else (0, g["N"] // 2 - 1)
    at_wall = r["indices"][:, axis] == top
    assert at_wall.any() and not (r["mask"][at_wall] & (2 << (2 * axis))).any()      # voxels on the wall: their outward bit is never set
    assert r["clusters"][0]["hi"][axis] == top


def test_both_kinds_of_unknown_count():
    r = _extract(fs.two_unknowns())
    assert r["indices"].shape[0] == fs.TWO_UNKNOWNS_VOXELS and r["clusters"].shape[0] == 2
    idx = r["indices"].astype(int)
    lo_face = r["mask"][(idx[:, 0] == 0) & (idx[:, 1] == 8) & (idx[:, 2] == 8)]
    hi_face = r["mask"][(idx[:, 0] == 15) & (idx[:, 1] == 8) & (idx[:, 2] == 8)]
    assert lo_face.tolist() == [1] and hi_face.tolist() == [2]             # the absent brick at -x, the unobserved voxels of the allocated brick at +x


def test_spiral_is_one_long_simple_path():
    p = fs.spiral_path()
    assert p.shape[0] > 500 and p.min() >= 0 and p.max() <= 15
    assert np.unique(p, axis=0).shape[0] == p.shape[0]
    assert (np.abs(np.diff(p, axis=0)).sum(1) == 1).all()                   # consecutive voxels share a face
    s = {tuple(v) for v in p.tolist()}
    nb = [sum((v[0] + d[0], v[1] + d[1], v[2] + d[2]) in s for d in ref.FACES) for v in p.tolist()]
    assert nb[0] == 1 and nb[-1] == 1 and all(n == 2 for n in nb[1:-1])     # no shortcut under 6-connectivity: the chain is the path
    for conn in (6, 26):
        r = _extract(fs.spiral(), connectivity=conn)
        assert r["indices"].shape[0] == p.shape[0] and r["clusters"].shape[0] == 1


def test_tube_is_one_cluster_labelled_by_a_key_inside_the_chain():
    sc = fs.tube()
    for geo in ("SMALL", "SLAB", "TALL"):
        g = fs.GEOMETRIES[geo]
        placed = fs.place(sc, geo)
        u = placed["indices"].astype(np.int64) + np.array([g["N"] // 2, g["N"] // 2, g["Nz"] // 2])
        bricks = np.unique(u >> 4, axis=0).shape[0]
        assert bricks >= 6
        key = (u[:, 0] * g["N"] + u[:, 1]) * g["Nz"] + u[:, 2]
        at = int(np.argmin(key))
        assert 10 < at < key.shape[0] - 10                                   # the least key is neither end of the chain
        for conn in (6, 26):
            r = ref.extract(placed, g["N"], g["Nz"], VS, connectivity=conn)
            assert r["clusters"].shape[0] == 1 and r["clusters"][0]["count"] == key.shape[0] and r["clusters"][0]["key"] == key.min()


def test_options():
    full = _extract(fs.shell())
    z = _extract(fs.shell(), k_range=(0, 3))
    assert 0 < z["indices"].shape[0] < full["indices"].shape[0] and z["indices"][:, 2].min() == 0 and z["indices"][:, 2].max() == 3
    p0, p1 = _extract(fs.plate()), _extract(fs.plate(), clear_of_occupied=True)
    gone = {tuple(v) for v in p0["indices"].tolist()} - {tuple(v) for v in p1["indices"].tolist()}
    assert gone and (9, 0, 0) in gone and (9, 1, 0) not in gone              # (9, 0, k) sees the plate's edge (10, -1, k) diagonally
    assert all(v[0] == 9 for v in gone)                                      # only the cube's face beside the plate is touched
    t0, t1 = _extract(fs.two_values()), _extract(fs.two_values(), free_thres=0.2)
    assert t0["indices"].shape[0] == fs.SHELL_VOXELS and t1["indices"][:, 2].min() == 0 and t1["indices"].shape[0] < t0["indices"].shape[0]


def _flood_fill(fr, conn):
    """independent labelling of a dense boolean array: breadth-first fill, components numbered in the order of their first voxel in C order"""
    lim = {6: 1, 18: 2, 26: 3}[conn]
    dirs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < abs(a) + abs(b) + abs(c) <= lim]
    lab = np.full(fr.shape, -1, np.int64)
    n = 0
    for v in map(tuple, np.argwhere(fr)):
        if lab[v] >= 0:
            continue
        lab[v] = n
        q = deque([v])
        while q:
            x = q.popleft()
            for d in dirs:
                y = (x[0] + d[0], x[1] + d[1], x[2] + d[2])
                if min(y) >= 0 and y[0] < fr.shape[0] and y[1] < fr.shape[1] and y[2] < fr.shape[2] and fr[y] and lab[y] < 0:
                    lab[y] = n
                    q.append(y)
        n += 1
    return lab, n


def _check_against_flood_fill(e, N, Nz, conn, **kw):
    r = ref.extract(e, N, Nz, VS, connectivity=conn, **kw)
    c = ref.class_array(e, N, Nz, ref.surf_thres(VS))
    fr, _ = ref.frontier_mask(c, Nz)
    lab, n = _flood_fill(fr, conn)
    u = r["indices"].astype(np.int64) + np.array([N // 2, N // 2, Nz // 2])
    assert u.shape[0] == int(fr.sum()) and r["clusters"].shape[0] == n
    assert np.array_equal(lab[u[:, 0], u[:, 1], u[:, 2]], r["cluster"])      # the first voxel in C order has the least key: the same numbering
    return r


def test_restatement_against_a_flood_fill():
    rng = np.random.default_rng(7)
    idx = fs.box((-12, -12, -12), (11, 11, 11))
    noise = fs.scene([(idx[rng.random(idx.shape[0]) < 0.35], fs.FREE_T)])      # dense random blobs over eight bricks
    for sc, conns in ((fs.shell(), (26,)), (fs.tube(), (6,)), (fs.spiral(), (6,)), (fs.diagonal(), (6, 18, 26)), (noise, (6, 18, 26))):
        for conn in conns:
            _check_against_flood_fill(fs.place(sc, "SMALL"), 256, 256, conn)


def test_room_map_of_the_oracle():
    import render_view_scenes as rv
    K, frames = rv.room_scene()
    o = rv.room_oracle(K, frames, SMALL)
    e = o.export_sparse()
    r = _check_against_flood_fill(e, o.N, o.Nz, 26)
    nv, nc, nb = ref.room_quantities(r, o.N, o.Nz)
    print(f"room on SMALL: {e['indices'].shape[0]} observed voxels, {nv} frontier voxels, {nc} clusters, largest cluster in {nb} bricks")
    assert nv >= 1000 and nc >= 10 and nb >= 8

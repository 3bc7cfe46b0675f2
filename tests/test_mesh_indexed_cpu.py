"""The indexed marching-cubes mesh without a GPU: the numpy restatement (tests/mesh_indexed_ref.py) against the CPU oracle's soup on the hand-built
scenes (tests/mesh_indexed_scenes.py) and on an integrated stream, the closed-manifold property no soup has, and the PLY writer."""
import numpy as np
import pytest

import mesh_indexed_ref as ref
import mesh_indexed_scenes as ms
from frontier_scenes import GEOMETRIES
from util import SMALL, small_stream

VS = SMALL["voxel_scale"]


def _oracle(geo):
    from oracle import OracleTSDF
    return OracleTSDF(**GEOMETRIES[geo]["cfg"])


def _scene_mesh(name, geo):
    o = _oracle(geo)
    sc = ms.build(name, geo)
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    return o, sc, ref.extract(o.export_sparse(), o.N, o.Nz, VS, sc["thres"])


_STREAM = {}


def _stream():
    """(oracle, restatement, soup) of SMALL after small_stream(3), meshed at 5 voxels; built once"""
    from oracle import BATCHED, OracleTSDF
    if not _STREAM:
        K, frames = small_stream(3)
        o = OracleTSDF(**SMALL)
        o.set_intrinsics(K, K)
        for R, T, d in frames:
            o.integrate_depth(R, T, d, mode=BATCHED)
        _STREAM["v"] = (o, ref.extract(o.export_sparse(), o.N, o.Nz, VS, 5 * VS), o.generate_mesh(1, 5 * VS))
    return _STREAM["v"]


def test_a_case_names_exactly_the_edges_whose_corners_differ_in_sign():
    """what lets the kernel mark an edge used from its two corner signs and the validity of the four cells around it"""
    for c in range(256):
        named = set(int(e) for e in ref.TRI[c].reshape(-1) if e >= 0)
        cross = {e for e in range(12) if ((c >> ref.EDGE[e, 0]) & 1) != ((c >> ref.EDGE[e, 1]) & 1)}
        assert named == cross, c


@pytest.mark.parametrize("geo", ["SMALL", "SLAB", "TALL"])
@pytest.mark.parametrize("name", ms.SCENE_NAMES)
def test_scenes_keep_the_invariants_and_the_soup_count(name, geo):
    o, sc, m = _scene_mesh(name, geo)
    ref.check_invariants(m, f"{name} on {geo}")
    v, _, _, n = o.generate_mesh(1, sc["thres"])
    assert m["triangles"].shape[0] == n > 0, f"{name} on {geo}: {m['triangles'].shape[0]} triangles, the soup has {n}"
    if name == "cases":
        assert n == ms.CASES_TRIANGLES
    if name == "orphan":
        assert np.unique(m["cell_keys"]).shape[0] == ms.ORPHAN_CELLS


def test_stream_keeps_the_invariants_and_the_soup_count():
    o, m, (v, nr, _, n) = _stream()
    ref.check_invariants(m, "stream")
    assert m["triangles"].shape[0] == n and n > 5000
    print(f"stream: {n} triangles, {3 * n} soup rows, {m['keys'].shape[0]} vertices ({3 * n / m['keys'].shape[0]:.2f} copies each)")


def test_soup_vertices_lie_within_2_pow_minus_10_voxel_of_their_edge_vertex():
    o, m, (v, nr, _, n) = _stream()
    ref.soup_relation(v, m, o.N, o.Nz, VS, "stream")
    # a soup vertex that equals the mesh vertex bit for bit has its normal bit for bit
    low, axis, amb = ref.edge_of_soup_vertex(v, VS)
    row = np.searchsorted(m["keys"], ref.cell_key(low, o.N, o.Nz) * 3 + axis)
    row = np.minimum(row, m["keys"].shape[0] - 1)
    same = ~amb & (v.view(np.uint32) == m["vertices"][row].view(np.uint32)).all(1)
    assert same.sum() > 0.4 * v.shape[0], f"only {int(same.sum())} of {v.shape[0]} soup vertices equal their edge's vertex bit for bit"
    assert ref._same(nr[same], m["normals"][row[same]])


@pytest.mark.parametrize("name", ["ball", "cases", "orphan"])
def test_soup_relation_on_scenes(name):
    o, sc, m = _scene_mesh(name, "SLAB")
    v, _, _, n = o.generate_mesh(1, sc["thres"])
    ref.soup_relation(v, m, o.N, o.Nz, VS, name)


def test_ball_is_a_closed_manifold_and_its_soup_is_not():
    o, sc, m = _scene_mesh("ball", "SMALL")
    ref.manifold(m["triangles"], m["keys"].shape[0], "ball")
    v, _, _, n = o.generate_mesh(1, sc["thres"])
    # the soup welded by position: copies of one vertex differ, so pairs of triangles that share an edge do not share its two end points
    _, inv = np.unique(v.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    with pytest.raises(AssertionError):
        ref.manifold(inv.reshape(-1, 3), int(inv.max()) + 1, "ball soup welded by position")


def test_snap_keeps_coincident_vertices_apart_and_takes_the_lower_corner():
    o, sc, m = _scene_mesh("snap", "SMALL")
    e = m["edges"].astype(np.int64)
    r = np.nonzero((e == np.array(ms.SNAP_SUB_EDGE)).all(1))[0]
    assert r.shape[0] == 1
    assert np.array_equal(m["vertices"][r[0]], (np.array(ms.SNAP_SUB_EDGE[:3], np.float32) * np.float32(VS)))
    # the zero plane: several edges end in one corner, each is a row of its own with that corner's position
    pos, cnt = np.unique(m["vertices"].view(np.uint32).reshape(-1, 3), axis=0, return_counts=True)
    assert cnt.max() >= 3 and pos.shape[0] < m["keys"].shape[0]


def _read_ply(path):
    """minimal reader of what write_ply writes: (header lines, vertex rows, faces)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[2])
    nf = int([h for h in head if h.startswith("element face")][0].split()[2])
    props = [h.split() for h in head if h.startswith("property") and "list" not in h]
    vt = np.dtype([(p[2], "<f4" if p[1] == "float" else "u1") for p in props])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    if "binary_little_endian" in head[1]:
        assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize
        return head, np.frombuffer(raw, vt, nv, end), np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    lines = raw[end:].decode("ascii").splitlines()
    assert len(lines) == nv + nf
    rows = np.zeros(nv, vt)
    for r, ln in enumerate(lines[:nv]):
        rows[r] = tuple(float(x) for x in ln.split())
    faces = np.zeros(nf, ft)
    for r, ln in enumerate(lines[nv:]):
        x = [int(y) for y in ln.split()]
        faces[r] = (x[0], x[1:])
    return head, rows, faces


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("textured", [False, True])
def test_save_ply_round_trip(tmp_path, binary, textured):
    from taichislam_amd.mapping.marching_cube_mesher import write_ply
    o, sc, m = _scene_mesh("ball", "SMALL")
    nv = m["vertices"].shape[0]
    colors = (np.arange(nv * 3).reshape(nv, 3) % 256 / 255.0).astype(np.float32) if textured else None
    mesh = dict(m, colors=colors, normals=np.nan_to_num(m["normals"]))
    p = str(tmp_path / "ball.ply")
    write_ply(p, mesh, binary=binary)
    head, rows, faces = _read_ply(p)
    assert head[0] == "ply" and f"element vertex {nv}" in head and f"element face {m['triangles'].shape[0]}" in head
    assert ("property uchar red" in head) == textured
    for a, name in enumerate("xyz"):
        assert np.array_equal(rows[name].view(np.uint32), mesh["vertices"][:, a].view(np.uint32))
        assert np.array_equal(rows["n" + name].view(np.uint32), mesh["normals"][:, a].view(np.uint32))
    if textured:
        assert np.array_equal(np.stack([rows["red"], rows["green"], rows["blue"]], 1), np.arange(nv * 3).reshape(nv, 3) % 256)
    assert (faces["n"] == 3).all() and np.array_equal(faces["v"], m["triangles"])
    with pytest.raises(ValueError):
        write_ply(p, dict(mesh, vertices=mesh["vertices"][:-1], normals=mesh["normals"][:-1], colors=None if colors is None else colors[:-1]), binary=binary)

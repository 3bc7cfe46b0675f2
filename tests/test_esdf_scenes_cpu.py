"""The hand-built ESDF volumes of tests/esdf_scenes.py, with the oracle alone: each scene has the property it is there to exercise on the GPU
(tests/test_esdf_scenes_gpu.py), and the oracle's Dijkstra gives the values worked out by hand for it."""
import numpy as np
import pytest

import esdf_scenes as es
from util import SMALL, lin

F32 = np.float32
VS = F32(es.VS)
C2 = F32(np.sqrt(F32(2.0))) * VS          # the edge costs as the package forms them: sqrt(f32 sum of squares) * vs
C3 = F32(np.sqrt(F32(3.0))) * VS


def _oracle(geo="EXACT"):
    from oracle import OracleTSDF
    return OracleTSDF(**es.GEOMETRIES[geo]["cfg"])


def _esdf(sc, gamma=None, max_dist=5.0, geo="EXACT"):
    o = _oracle(geo)
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    return o.esdf(gamma=gamma, max_dist=max_dist)


def _scene_esdf(name):
    return _esdf(es.SCENES[name](), *es.params(name))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def _chain(start, step, n):
    """start + step + step + ... in f32, as a path accumulates it"""
    v = F32(start)
    for _ in range(n):
        v = F32(v + step)
    return v


@pytest.mark.parametrize("name", sorted(es.SCENES))
def test_no_voxel_twice_and_every_scene_fits_its_geometries(name):
    sc = es.SCENES[name]()
    assert np.unique(sc["indices"], axis=0).shape[0] == sc["indices"].shape[0] == sc["TSDF"].shape[0] > 0
    es.place(sc, "EXACT")                                          # (asserts the fit)
    if name in es.PLACED:
        for geo in ("SLAB", "TALL"):
            p = es.placed(name, geo)
            assert np.unique(p["indices"], axis=0).shape[0] == sc["indices"].shape[0]
    gamma, md = es.params(name)
    assert md > 0 and (gamma is None or gamma > 0)


def test_a_value_enters_the_second_brick_through_one_corner_or_one_edge():
    i, e = _scene_esdf("corner_only")
    t = F32(np.float16(0.03))
    got = es.values_at(i, e, [(-1, -1, -1), (0, 0, 0), (15, 15, 15)])
    assert np.array_equal(_bits(got), _bits([_chain(t, C3, 15), _chain(t, C3, 16), _chain(t, C3, 31)]))
    assert [round(float(v), 4) for v in got] == [1.6538, 1.7620, 3.3858]
    # the two bricks touch in that voxel pair alone: no voxel of one is a neighbour of a voxel of the other otherwise
    idx = es.corner_only()["indices"].astype(np.int64)
    a, b = idx[idx[:, 0] < 0], idx[idx[:, 0] >= 0]
    near = [(tuple(p), tuple(q)) for p in a[(a >= -1).all(1)] for q in b[(b <= 0).all(1)] if np.abs(p - q).max() <= 1]
    assert near == [((-1, -1, -1), (0, 0, 0))] and (a.max(0) == -1).all() and (b.min(0) == 0).all()
    assert np.unique(idx // 16, axis=0).tolist() == [[-1, -1, -1], [0, 0, 0]]
    i, e = _scene_esdf("edge_only")
    idx = es.edge_only()["indices"].astype(np.int64)
    assert np.unique(idx // 16, axis=0).tolist() == [[-1, -1, 0], [0, 0, 0]]
    # across the edge: 15 steps in the plane z = 0 to (-1, -1, 0), one more to (0, 0, 0), then along the diagonal of the second brick
    got = es.values_at(i, e, [(-1, -1, 0), (0, 0, 0), (15, 15, 15)])
    assert np.array_equal(_bits(got), _bits([_chain(t, C2, 15), _chain(t, C2, 16), _chain(_chain(t, C2, 16), C3, 15)]))


@pytest.mark.parametrize("kind", ["corner", "edge"])
def test_late_scenes_feed_one_brick_through_a_face_first_and_through_a_diagonal_neighbour_later(kind):
    sc = es.late(kind)
    idx = sc["indices"].astype(np.int64)
    z = -1 if kind == "corner" else 0
    assert np.unique(idx // 16, axis=0).tolist() == [[-2, -1, z], [-1, -1, z], [0, 0, 0], [1, 0, 0]]
    band = idx[sc["TSDF"] == 0]
    assert sorted((band // 16)[:, 0].tolist()) == [-2, 1]          # no band voxel in P or Q: each is listed by a neighbour, P one round after Q
    i, e = _scene_esdf("late_" + kind)
    # through the diagonal contact: 16 axis steps to P's voxel next to Q, one diagonal step into Q
    near = (0, 0, 0) if kind == "corner" else (0, 0, 8)
    assert es.values_at(i, e, [near])[0] == _chain(_chain(F32(0), VS, 16), C3 if kind == "corner" else C2, 1)
    assert es.values_at(i, e, [(15, 8, 8)])[0] == 1.0              # through the face: 16 axis steps from the far band voxel
    # both reach a good part of Q: against the field of the far band voxel alone, Q's voxels near the contact are lower and the others are the same
    fi, fe = _esdf(es.late(kind, near=False))
    q = es.box((0, 0, 0), (15, 15, 15))
    both, far = es.values_at(i, e, q), es.values_at(fi, fe, q)
    assert (both <= far).all() and 100 < (both < far).sum() < 4096 - 100


@pytest.mark.parametrize("name", ["cube27", "cube27_corner"])
def test_cube27_is_exact_along_the_axes_through_its_band_voxel(name):
    sc = es.SCENES[name]()
    idx = sc["indices"].astype(np.int64)
    assert idx.shape[0] == 48 ** 3 and np.unique(idx // 16, axis=0).shape[0] == 27
    band = idx[sc["TSDF"] == 0]
    assert band.shape == (1, 3)
    band = band[0]
    if name == "cube27_corner":                                    # the band voxel's brick is the lowest of the volume on every axis
        assert (band // 16 == -8).all() and (idx.min(0) == -128).all()
    else:
        assert tuple(band) == es.CUBE27_BAND
    i, e = _scene_esdf(name)
    assert i.shape[0] == 48 ** 3
    for a in range(3):
        n = np.arange(int(idx[:, a].min() - band[a]), int(idx[:, a].max() - band[a]) + 1)
        v = np.repeat(band[None], n.size, 0); v[:, a] += n
        assert n.size == 48 and (es.values_at(i, e, v) == np.abs(n) * 0.0625).all()          # n * vs, exactly
    assert np.abs(e).max() < 5.0                                   # every voxel is reached


def test_zigzag_crosses_a_brick_face_more_often_than_the_blind_batch_has_rounds():
    cells = es.zigzag_cells()
    assert cells.shape == (64, 3) and es.zigzag_crossings(cells) == 31
    assert np.abs(np.diff(cells, axis=0)).max() == 1               # consecutive cells are neighbours,
    far = np.abs(cells[:, None] - cells[None]).max(-1) <= 1
    assert (far.sum(1) <= 3).all()                                 # and no cell has another neighbour than the one before and the one after: one path
    reach = int(np.ceil(5.0 / (es.VS * 16)))
    assert 2 * reach + 8 == 18 < es.zigzag_crossings(cells)
    i, e = _scene_esdf("zigzag")
    assert i.shape[0] == 64
    got = es.values_at(i, e, cells)
    want, v = [F32(0)], F32(0)
    for d in np.abs(np.diff(cells, axis=0)).sum(1):
        v = F32(v + (VS if d == 1 else C2)); want.append(v)
    assert np.array_equal(_bits(got), _bits(want))
    assert round(float(got[-1]), 4) == 4.74 and got[-1] < 5.0      # the far end is reached below max_dist
    for geo in ("SLAB", "TALL"):                                   # at 4 cm the far end is nearer still, and the batch (24 rounds) is still shorter than the path
        vs = es.GEOMETRIES[geo]["cfg"]["voxel_scale"]
        assert 2 * int(np.ceil(5.0 / (vs * 16))) + 8 < 31
        pi, pe = _esdf(es.placed("zigzag", geo), None, 5.0, geo)
        assert 0 < np.abs(pe).max() < 5.0


def test_pocket_keeps_max_dist_and_the_field_bends_around_it():
    sc = es.pocket()
    t = sc["TSDF"].astype(F32)
    assert (t < 0).sum() == 64 and (np.abs(t) < es.VS).sum() == 1          # a negative pocket, and the only band voxel is a positive one elsewhere
    i, e = _scene_esdf("pocket")
    assert np.array_equal(_bits(es.values_at(i, e, es.POCKET)), _bits(np.full(64, -2.0)))
    v = es.values_at(i, e, [(2, 2, 2)])[0]
    assert round(float(v), 4) == 1.2631
    assert v > _chain(F32(np.float16(0.01)), C3, 10)               # more than the straight diagonal through the pocket would give
    # planes through the pocket hold both signs, the pocket's own rows seen from inside only the negative one
    idx = sc["indices"].astype(np.int64)
    assert {-0.5, 0.5} <= set(t[idx[:, 2] == 0].tolist())


def test_checker_signs_propagate_along_edge_diagonals_only():
    sc = es.checker_signs()
    idx, t = sc["indices"].astype(np.int64), sc["TSDF"].astype(F32)
    assert ((t > 0) == (idx.sum(1) % 2 == 0)).all() and idx.shape[0] == 18 ** 3
    assert sum(es.CHECKER_POS_BAND) % 2 == 0 and sum(es.CHECKER_NEG_BAND) % 2 == 1
    for a in range(3):                                             # every plane of every sweep is mixed
        for c in range(-1, 17):
            s = t[idx[:, a] == c]
            assert (s > 0).any() and (s < 0).any()
    i, e = _scene_esdf("checker_signs")
    e = e[np.argsort(lin(i))]
    tt = t[np.argsort(lin(sc["indices"]))]
    pos = {float(_chain(F32(np.float16(0.02)), C2, n)) for n in range(1, 64)}
    neg = {-v for v in pos}
    free = np.abs(tt) >= es.VS
    assert free.sum() == 18 ** 3 - 2
    assert set(e[free & (tt > 0)].tolist()) <= pos and set(e[free & (tt < 0)].tolist()) <= neg          # sqrt(2) steps only, and every voxel is reached
    assert np.abs(e).max() < 5.0


@pytest.mark.parametrize("name", sorted(es.BAND_ROWS))
def test_band_rows(name):
    r = es.BAND_ROWS[name]
    i, e = _scene_esdf(name)
    got = es.values_at(i, e, es.row_voxels(len(r["values"])))
    assert np.array_equal(_bits(got), _bits(r["want"])), (got, r["want"])
    if name == "neg_zero":
        assert _bits(got)[1] == 0x80000000
    if name == "band_strict":
        assert np.float16(es.BELOW_VS) == es.BELOW_VS < es.VS and np.nextafter(np.float16(es.BELOW_VS), np.float16(1)) == es.VS
        assert [round(float(v), 8) for v in got] == [0.12496948, 0.06246948, 0.12496948, 0.18746948]


def test_far_bricks_stay_at_max_dist():
    i, e = _scene_esdf("far_brick")
    assert np.array_equal(_bits(es.values_at(i, e, es.FAR_POS)), _bits(np.full(4096, 1.0)))
    assert np.array_equal(_bits(es.values_at(i, e, es.FAR_NEG)), _bits(np.full(4096, -1.0)))
    assert np.abs(es.values_at(i, e, [(-15, -15, -15)])[0]) < 1.0          # while the scene next to them has values below it
    idx = es.far_brick()["indices"].astype(np.int64)
    b = np.unique(idx // 16, axis=0)
    assert b.shape[0] == 4 and all(np.abs(p - q).max() > 1 for p in b[[0, 3]] for q in b[[1, 2]])          # more than one brick = max_dist away


def test_the_other_submap_does_not_show_through():
    wall, sc = es.other_submap_wall(), es.corner_only()
    a, b = wall["indices"].astype(np.int64), sc["indices"].astype(np.int64)
    assert set(map(tuple, np.unique(b // 16, axis=0).tolist())) <= set(map(tuple, np.unique(a // 16, axis=0).tolist()))          # the same bricks
    assert (np.abs(wall["TSDF"].astype(F32)) < es.VS).sum() == 4 * 32 * 32
    o = _oracle()
    o.import_sparse(0, wall["indices"], wall["TSDF"], wall["W_TSDF"], wall["occupy"])
    o.set_active_submap(1)
    o.import_sparse(1, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    i1, e1 = o.esdf(max_dist=5.0)
    i0, e0 = _scene_esdf("corner_only")
    p, q = np.argsort(lin(i1)), np.argsort(lin(i0))
    assert np.array_equal(i1[p], i0[q]) and np.array_equal(_bits(e1[p]), _bits(e0[q]))
    o.set_active_submap(0)                                         # and the wall alone gives another field
    iw, ew = o.esdf(max_dist=5.0)
    assert iw.shape[0] == 32 ** 3 and np.abs(ew).max() < 1.0


def test_the_edit_after_the_import_moves_distances():
    """case B: the point cloud puts a surface where the imported block had free space at max_dist"""
    from oracle import OracleTSDF
    o = OracleTSDF(**SMALL)
    sc = es.edit_block()
    assert sc["indices"].shape[0] == 80 ** 3 and np.unique(sc["indices"].astype(np.int64) // 16, axis=0).shape[0] == 125
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    i0, e0 = o.esdf(max_dist=es.EDIT_MAX_DIST)
    R, T, xyz = es.edit_points()
    o.integrate_points(R, T, xyz)
    i1, e1 = o.esdf(max_dist=es.EDIT_MAX_DIST)
    t1 = o.export_sparse()
    before = dict(zip(lin(i0).tolist(), e0.tolist()))
    tsdf = dict(zip(lin(t1["indices"]).tolist(), t1["TSDF"].astype(F32).tolist()))
    vs = SMALL["voxel_scale"]
    moved = [k for k, v in zip(lin(i1).tolist(), e1.tolist()) if k in before and abs(tsdf[k]) >= vs and abs(v - before[k]) > vs]
    assert len(moved) > 100
    # the changed bricks lie next to the face opposite the band plane, whose distances stay as they were
    assert all(((k >> 32) - 32768) > 0 for k in moved)
    assert np.unique(i1.astype(np.int64) // 16, axis=0).shape[0] == 125          # the edit allocates no brick: total_bricks stays 125


def test_the_ball_makes_distances_fall_and_rise_again():
    """case A: band voxels appear in free space in front of the wall and vanish again"""
    from oracle import BATCHED, OracleTSDF
    K, R, T, frames = es.vanishing_ball()
    assert len(frames) == 12 and not np.array_equal(frames[3], frames[0]) and np.array_equal(frames[-1], frames[0])
    o = OracleTSDF(**SMALL)
    o.set_intrinsics(K, K)
    fields = {}
    for f, d in enumerate(frames):
        o.integrate_depth(R, T, d, mode=BATCHED)
        if f in (es.BALL_WARM - 1,) + es.BALL_ORACLE_FRAMES:
            i, e = o.esdf(max_dist=es.BALL_MAX_DIST)
            fields[f] = dict(zip(lin(i).tolist(), e.tolist()))
    vs = SMALL["voxel_scale"]
    room, ball, after = (fields[f] for f in (es.BALL_WARM - 1,) + es.BALL_ORACLE_FRAMES)
    fell = [k for k in room if room[k] > 0 and ball[k] > 0 and room[k] - ball[k] > vs]
    rose = [k for k in ball if ball[k] > 0 and after[k] > 0 and after[k] - ball[k] > vs]
    assert len(fell) > 100 and len(rose) > 100

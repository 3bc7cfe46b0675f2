"""The ESDF update (csrc/tsl_esdf.hip) on the hand-built volumes of tests/esdf_scenes.py and on surfaces that vanish: the exported field equals the oracle's
Dijkstra bit for bit (the fixed point is unique: there is no tolerance in this file), no lowered voxel lost its support, and the point queries at the voxel
centres return the exported values.  Every test runs for both forms of the update.  One handle per (geometry, form) serves all scenes with reset() in
between, the pocket scene first, so that later scenes are computed in pool bricks that still hold the magnitudes, flags, parent codes and state bytes of
earlier ones.  tests/test_esdf_scenes_cpu.py shows with the oracle alone that each scene has the property it is here for."""
import gc

import numpy as np
import pytest

import esdf_scenes as es
from util import SMALL, lin

pytestmark = pytest.mark.gpu

_MAPS = {}
POOL = dict(max_submap_num=2, max_bricks=1024)          # the scenes use at most 64 bricks and two submaps: a pool of 1024 bricks instead of the default 131072 (7 GB with an ESDF)


@pytest.fixture(scope="module", autouse=True)
def _release_the_maps():
    yield
    _MAPS.clear()
    gc.collect()


@pytest.fixture(autouse=True, params=[1, 0], ids=["wavefront", "regional"])
def esdf_mode(request, monkeypatch):
    """as in tests/test_esdf_gpu.py: esdf_mode 1, the raise / lower wavefront with parent directions, and esdf_mode 0, the regional recompute (the default)"""
    monkeypatch.setenv("TSL_ESDF_MODE", str(request.param))
    return request.param


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _map(geo, mode, hip_lib):
    """the handle of (geometry, form) for the whole module, reset before every use"""
    from taichislam_amd.mapping import DenseTSDF
    if (geo, mode) not in _MAPS:
        _MAPS[geo, mode] = DenseTSDF(**es.GEOMETRIES[geo]["cfg"], **POOL)
        assert _MAPS[geo, mode].get_option("esdf_mode") == mode
    g = _MAPS[geo, mode]
    g.reset()
    g.active_submap_id[None] = 0
    return g


def _oracle(geo):
    from oracle import OracleTSDF
    return OracleTSDF(**es.GEOMETRIES[geo]["cfg"])


def _sorted(i, e):
    o = np.argsort(lin(i))
    return i[o], e[o]


def _assert_fields_equal(gi, ge, wi, we, what):
    assert gi.shape == wi.shape and np.array_equal(gi, wi), f"{what}: voxel index sets differ ({gi.shape[0]} vs {wi.shape[0]})"
    bad = np.nonzero(_bits(ge) != _bits(we))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {ge.size} voxels differ, largest error {np.abs(ge[bad] - we[bad]).max()}, first {gi[bad[0]].tolist()}: "
                           f"{ge[bad[0]]!r} vs {we[bad[0]]!r}")


def _check(g, o, what, gamma=None, max_dist=5.0, update=True):
    """update, export and point queries against the oracle; returns the sorted export"""
    if update:
        g.update_esdf(gamma=gamma, max_dist=max_dist)
    gi, ge = _sorted(*g.export_esdf())
    wi, we = _sorted(*o.esdf(gamma=gamma, max_dist=max_dist))
    _assert_fields_equal(gi, ge, wi, we, what)
    assert g.get_option("esdf_orphans") == 0, what
    centres = gi.astype(np.float32) * np.float32(g.voxel_scale)          # the position convention of tests/esdf_query_ref.py: voxel i is the one nearest to i * vs
    d, _, st = g.query_esdf(centres, interpolate=False, refresh=False)
    assert (st == 0).all(), f"{what}: {np.count_nonzero(st)} voxel centres without a value"
    bad = np.nonzero(_bits(d) != _bits(ge))[0]
    assert bad.size == 0, f"{what}: the query differs from the export at {bad.size} voxels, first {gi[bad[0]].tolist()}: {d[bad[0]]!r} vs {ge[bad[0]]!r}"
    return gi, ge


def _run(name, geo, mode, hip_lib, sc=None):
    g, o = _map(geo, mode, hip_lib), _oracle(geo)
    sc = es.place(es.SCENES[name](), geo) if sc is None else sc
    es.load_pair(g, o, sc)
    gamma, md = es.params(name)
    before = g.esdf_totals()["updates"]
    out = _check(g, o, f"{name} on {geo}, esdf_mode {mode}", gamma, md)
    st = g.esdf_stats()
    bricks = np.unique((sc["indices"].astype(np.int64) + np.array([g.N // 2, g.N // 2, g.Nz // 2])) // 16, axis=0).shape[0]
    assert st["incremental"] == 0 and st["total_bricks"] == bricks, st
    return g, out, g.esdf_totals()["updates"] - before


@pytest.mark.parametrize("name", es.ORDER)
def test_scenes_equal_the_oracle(hip_lib, esdf_mode, name):
    """Every scene on EXACT (N = 256, a voxel of 2^-4 m).  zigzag: the corridor crosses a brick face 31 times and only interior voxels are written, so a value
    advances one crossing per round, and the blind batch has 2 * 5 + 8 = 18 rounds: the update stops short and the first reader gets the repair.  MEASURED on
    an MI355X (2026-10-20): 2 updates until the first read in either form -- the blind batch of 18 rounds, then one full recompute with 34, of which 32 had work."""
    g, (gi, ge), updates = _run(name, "EXACT", esdf_mode, hip_lib)
    if name in es.BAND_ROWS:                                     # the values worked out by hand, from the GPU's own export
        r = es.BAND_ROWS[name]
        assert np.array_equal(_bits(es.values_at(gi, ge, es.row_voxels(len(r["values"])))), _bits(r["want"]))
    if name == "far_brick":
        assert np.array_equal(_bits(es.values_at(gi, ge, es.FAR_POS)), _bits(np.full(4096, 1.0)))
        assert np.array_equal(_bits(es.values_at(gi, ge, es.FAR_NEG)), _bits(np.full(4096, -1.0)))
    if name.startswith("late_"):                                 # round 0: the two bricks with a band voxel; round 1: P and Q; round 2: Q again, told by P alone
        st = g.esdf_stats()
        print(f"{name}, esdf_mode {esdf_mode}: {st}")
        assert st["rounds"] >= 3 and st["brick_relaxations"] >= 5, st
    if name == "pocket":
        assert np.array_equal(_bits(es.values_at(gi, ge, es.POCKET)), _bits(np.full(64, -2.0)))
    if name == "zigzag":
        print(f"zigzag, esdf_mode {esdf_mode}: {updates} updates until the first read, last {g.esdf_stats()}")
        assert updates >= ZIGZAG_UPDATES[esdf_mode]
    else:
        assert updates >= 1


ZIGZAG_UPDATES = {0: 2, 1: 2}          # the repair ran: the blind batch and at least one full recompute with a longer one (measured: exactly 2 in either form)


@pytest.mark.parametrize("geo", ["SLAB", "TALL"])
@pytest.mark.parametrize("name", es.PLACED)
def test_placed_scenes_equal_the_oracle(hip_lib, esdf_mode, geo, name):
    """scenes 1, 2 and 4 where the brick faces lie at 8 mod 16 (SLAB) and with x and z swapped in a volume with more bricks along z than along x (TALL)"""
    g, _, updates = _run(name, geo, esdf_mode, hip_lib, sc=es.placed(name, geo))
    if name == "zigzag":
        assert updates >= 2                                      # 24 rounds in the blind batch at 4 cm, 31 crossings


def test_another_submap_in_the_same_bricks(hip_lib, esdf_mode):
    """submap 0 holds a band wall in the bricks of corner_only and has an ESDF of its own; the field of submap 1 must be that of a map that never saw it"""
    g = _map("EXACT", esdf_mode, hip_lib)
    wall, sc = es.other_submap_wall(), es.corner_only()
    ow = _oracle("EXACT")
    es.load_pair(g, ow, wall, 0)
    _check(g, ow, "the wall in submap 0")
    g.active_submap_id[None] = 1
    o = _oracle("EXACT")
    g.load_numpy(1, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], None)
    o.import_sparse(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"])
    gi, ge = _check(g, o, "corner_only in submap 1 over the wall of submap 0")
    assert gi.shape[0] == 2 * 4096 and g.esdf_stats()["incremental"] == 0
    g.active_submap_id[None] = 0                                 # and back: submap 0 is recomputed as well
    _check(g, ow, "the wall again")


def test_bricks_handed_out_again_carry_nothing_over(hip_lib, esdf_mode):
    """E.mag, E.fl, E.par and E.ok survive reset() in the pool's bricks.  A handle that has computed other scenes with other parameters, then scenes 1 and 6: the
    same bytes as a handle that never held anything else"""
    from taichislam_amd.mapping import DenseTSDF
    for name in ("pocket", "checker_signs", "cube27"):           # whatever ran before, this handle is used now
        _run(name, "EXACT", esdf_mode, hip_lib)
    for name in ("corner_only", "far_brick"):
        _, (ui, ue), _ = _run(name, "EXACT", esdf_mode, hip_lib)
        fresh, o = DenseTSDF(**es.EXACT, **POOL), _oracle("EXACT")
        es.load_pair(fresh, o, es.SCENES[name]())
        gamma, md = es.params(name)
        fi, fe = _check(fresh, o, f"{name} on a fresh handle", gamma, md)
        assert ui.tobytes() == fi.tobytes() and ue.tobytes() == fe.tobytes()


def _full(K=None):
    from taichislam_amd.mapping import DenseTSDF
    full = DenseTSDF(**SMALL, max_bricks=4096)
    if K is not None:
        full.set_dep_camera_intrinsic(K)
    full.set_option("esdf_full", 1); full.set_option("esdf_mode", 0)
    return full


def test_a_ball_that_crosses_the_view_and_vanishes(hip_lib, esdf_mode):
    """tools/esdf_sparse_probe.py at small size: a static camera, three frames of the room, six with a ball that moves 0.12 m per frame 1.5 m ahead, three
    without it.  Band voxels appear in free space and go again, so values fall and then rise by many voxels (tests/test_esdf_scenes_cpu.py).  After every
    frame the incremental update equals the full recompute, on two frames the oracle.  How many updates ended in the repair is printed, not asserted."""
    from oracle import BATCHED
    from util import make_pair
    K, R, T, frames = es.vanishing_ball()
    inc, o = make_pair(SMALL, K, max_bricks=4096)
    full = _full(K)
    md, repaired = es.BALL_MAX_DIST, 0
    for f, d in enumerate(frames):
        for m in (inc, full):
            m.recast_depth_to_map(R, T, d, None)
        before = inc.esdf_totals()["updates"]
        inc.update_esdf(max_dist=md); full.update_esdf(max_dist=md)
        repaired += inc.esdf_totals()["updates"] - before - 1
        o.integrate_depth(R, T, d, mode=BATCHED)
        (ii, ie), (fi, fe) = _sorted(*inc.export_esdf()), _sorted(*full.export_esdf())
        _assert_fields_equal(ii, ie, fi, fe, f"frame {f}: incremental against full")
        if f in es.BALL_ORACLE_FRAMES:
            _check(inc, o, f"frame {f} against the oracle", None, md, update=False)
    t = inc.esdf_totals()
    print(f"vanishing_ball, esdf_mode {esdf_mode}: {repaired} repairs in {len(frames)} frames, totals {t}")
    assert t["incremental"] == len(frames) - 1 and t["updates"] == len(frames) + repaired
    assert inc.get_option("esdf_orphans") == 0 and inc.get_option("esdf_mode") == esdf_mode


def test_an_edit_on_top_of_an_imported_map(hip_lib, esdf_mode):
    """import_sparse invalidates the ESDF: the next update is a full one, and the one after it, behind an integrated point cloud, runs from the touch marks"""
    from util import make_pair
    from taichislam_amd.utils import synthetic as syn
    inc, o = make_pair(SMALL, syn.K_DEPTH, max_bricks=4096)
    full = _full(syn.K_DEPTH)
    sc, md = es.edit_block(), es.EDIT_MAX_DIST
    es.load_pair(inc, o, sc)
    full.load_numpy(0, sc["indices"], sc["TSDF"], sc["W_TSDF"], sc["occupy"], None)
    _check(inc, o, "the imported block", None, md)
    assert inc.esdf_stats()["incremental"] == 0
    R, T, xyz = es.edit_points()
    for m in (inc, full):
        m.recast_pcl_to_map(R, T, xyz, None)
    o.integrate_points(R, T, xyz)
    inc.update_esdf(max_dist=md); full.update_esdf(max_dist=md)
    st = inc.esdf_stats()
    assert st["incremental"] == 1 and 0 < st["changed_bricks"] and full.esdf_stats()["incremental"] == 0, st
    if esdf_mode == 0:
        assert st["region_bricks"] < st["total_bricks"], st
    (ii, ie), (fi, fe) = _sorted(*inc.export_esdf()), _sorted(*full.export_esdf())
    _assert_fields_equal(ii, ie, fi, fe, "the edit: incremental against full")
    _check(inc, o, "the edit against the oracle", None, md, update=False)
    assert inc.esdf_stats()["incremental"] == 1

"""Every map kernel on volumes whose height differs from their width (tests/util.py: SLAB 144 x 144 x 48, TALL 64 x 64 x 128, GSLAB 256 x 256 x 64).

The reference's own node maps a flat slab (scripts/taichislam_node.py:150-161: map_size_xy = 100, map_size_z = 10).  In a cube nbx == nbz, N == Nz and
hN == hNz: a brick id decoded with the wrong stride, a bound taken from the wrong axis, a swapped pair of brick counts all give the right answer.  Here
they do not: the HIP result is compared with the CPU oracle and the numpy restatements through the comparators of the cubic tests, with the same equality
or the same bound as the cubic case of the same call.  In SLAB N / 2 = 72 and Nz / 2 = 24 are both 8 (mod 16): the faces of the 16^3 storage bricks lie at
voxel indices 8 (mod 16) on every axis, not at the origin.  In TALL there are more bricks along z than along x.

Every test asserts from the ORACLE's result that its input reaches what it is there for: SLAB -- rays leave the volume (steps_oob > 10000) and the data
touches both z faces (k = -24 and 23); TALL -- data beyond k = N / 2 = 32, where a z index tested against N / 2 would be cut off."""
import functools

import numpy as np
import pytest

from util import GSLAB, SLAB, TALL, assert_export_equal, lin, make_pair, small_stream, sort_export, sorted_rows, tall_stream, tilt

pytestmark = pytest.mark.gpu

STAT_KEYS = ("p_used", "p_valid", "p_oob", "v_pcl", "v_skipped", "steps", "steps_oob", "unique", "bricks")
GEOM = {"slab": (SLAB, small_stream), "tall": (TALL, tall_stream)}
BOTH = pytest.mark.parametrize("geom", ["slab", "tall"])
THRES = 5 * SLAB["voxel_scale"]                               # scripts/taichislam_node.py:209


@functools.lru_cache(maxsize=None)
def _oracle(geom, n=3, mode=None):
    """The oracle's map of the geometry's stream (BATCHED unless told otherwise), computed once and never changed: (K, frames, oracle, stats per frame)."""
    from oracle import BATCHED, OracleTSDF
    cfg, stream = GEOM[geom]
    K, frames = stream(n)
    o = OracleTSDF(**cfg)
    o.set_intrinsics(K, K)
    stats = [o.integrate_depth(R, T, d, mode=BATCHED if mode is None else mode) for R, T, d in frames]
    _covers(geom, o.export_sparse()["indices"], stats)
    return K, frames, o, stats


def _covers(geom, idx, stats):
    """the coverage condition of the geometry, from the oracle's output"""
    k = idx[:, 2]
    if geom == "slab":
        assert stats[-1]["steps_oob"] > 10000 and k.min() == -24 and k.max() == 23, (stats[-1], k.min(), k.max())
    else:
        assert k.max() > 32, k.max()


def _hip(geom, n=3, **options):
    from taichislam_amd.mapping import DenseTSDF
    K, frames, o, stats = _oracle(geom, n)
    g = DenseTSDF(**GEOM[geom][0])
    g.set_dep_camera_intrinsic(K)
    g.set_color_camera_intrinsic(K)
    for k, v in options.items():
        g.set_option(k, v)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    return g, o, frames


# ------------------------------------------------------------------------------------------------------------------ 1. integration
@BOTH
@pytest.mark.parametrize("variant", [None, 0, 1])
def test_integration_equals_the_oracle_frame_by_frame(hip_lib, geom, variant):
    """dense_tsdf.py:157-270.  The default path and the kernel variants 0 / 1: every frame counter after every frame (steps_oob and bricks included), then the map."""
    from taichislam_amd.mapping import DenseTSDF
    K, frames, o, stats = _oracle(geom)
    g = DenseTSDF(**GEOM[geom][0])
    g.set_dep_camera_intrinsic(K)
    if variant is not None:
        g.set_option("variant", variant)
    for (R, T, d), so in zip(frames, stats):
        g.recast_depth_to_map(R, T, d, np.array([], dtype=int))
        sg = g.last_frame_stats()
        assert {k: sg[k] for k in STAT_KEYS} == {k: so[k] for k in STAT_KEYS}
    assert g.count_active() == o.count_active()
    assert_export_equal(g.export_submap(), o.export_sparse(), f"{geom}, variant {variant}")


@BOTH
def test_sequential_semantics_equal_faithful(hip_lib, geom):
    """semantics = 1 (csrc/tsl_sequential.hip) against the oracle's reference-literal replay, frame counters included"""
    from oracle import FAITHFUL
    from taichislam_amd.mapping import DenseTSDF
    K, frames, o, stats = _oracle(geom, 3, FAITHFUL)
    g = DenseTSDF(**GEOM[geom][0])
    g.set_dep_camera_intrinsic(K)
    g.set_option("semantics", 1)
    for (R, T, d), so in zip(frames, stats):
        g.recast_depth_to_map(R, T, d, None)
        sg = g.last_frame_stats()
        assert {k: sg[k] for k in STAT_KEYS} == {k: so[k] for k in STAT_KEYS}
    assert_export_equal(g.export_submap(), o.export_sparse(), f"{geom}, sequential vs FAITHFUL")


@BOTH
def test_point_cloud_frame(hip_lib, geom):
    """recast_pcl_to_map (dense_tsdf.py:167-186): points in every direction from the last sensor position, so that rays leave through every face"""
    from oracle import BATCHED
    K, frames, ref, _ = _oracle(geom)
    g, o = make_pair(GEOM[geom][0], K)
    R, T, _ = frames[-1]
    rng = np.random.default_rng(7)
    d = rng.normal(size=(6000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (d * rng.uniform(0.2, 6.0, size=(6000, 1))).astype(np.float32)
    g.recast_pcl_to_map(R, T, pts, np.array([]))
    so = o.integrate_points(R, T, pts, None, mode=BATCHED)
    k = o.export_sparse()["indices"][:, 2]
    assert so["steps_oob"] > 10000 and (k.min() == -24 and k.max() == 23 if geom == "slab" else k.max() > 32)
    sg = g.last_frame_stats()
    assert {k_: sg[k_] for k_ in STAT_KEYS} == {k_: so[k_] for k_ in STAT_KEYS}
    assert_export_equal(g.export_submap(), o.export_sparse(), f"{geom}, points")


def test_nine_device_frames_back_to_back(hip_lib):
    """Nine device tensors handed over without a read in between: a full batch of eight forms and is walked by the batched brick kernel"""
    import torch
    from taichislam_amd.mapping import DenseTSDF
    K, frames, o, stats = _oracle("slab", 9)
    g = DenseTSDF(**SLAB)
    g.set_dep_camera_intrinsic(K)
    dev = [torch.from_numpy(d.view(np.int16)).cuda() for _, _, d in frames]
    for (R, T, _), t in zip(frames, dev):
        g.recast_depth_to_map(R, T, t, None)
    g.sync()
    assert g.get_option("overlapped_launches") + g.get_option("dry_launches") > 0
    sg = g.last_frame_stats()
    assert {k: sg[k] for k in STAT_KEYS} == {k: stats[-1][k] for k in STAT_KEYS}
    assert_export_equal(g.export_submap(), o.export_sparse(), "slab, nine frames back to back")


# ------------------------------------------------------------------------------------------------------------------ 2. exports
@BOTH
def test_exports(hip_lib, geom):
    """export_occupied, count_active, the particle exports (dense_tsdf.py:339-389) as sorted rows, and load_numpy of the oracle's export (:412-454)"""
    from taichislam_amd.mapping import DenseTSDF
    g, o, _ = _hip(geom)
    assert g.count_active() == o.count_active() > 10000
    gi, go = g.export_occupied()
    oi, oo = o.export_occupied()
    assert gi.shape[0] > 100 and np.array_equal(sorted_rows(np.concatenate([gi, go[:, None]], 1)), sorted_rows(np.concatenate([oi, oo[:, None]], 1)))
    g.cvt_TSDF_surface_to_voxels()
    n = g.num_TSDF_particles[None]
    oxyz, orgb, on = o.surface_voxels()
    assert n == on > 100
    a = sorted_rows(np.concatenate([g.export_TSDF_xyz.to_numpy()[:n], g.export_color.to_numpy()[:n]], 1))
    b = sorted_rows(np.concatenate([oxyz, orgb], 1))
    assert np.array_equal(a[:, :3], b[:, :3])
    assert np.allclose(a[:, 3:], b[:, 3:], atol=1e-6)
    for z in ((0.37, -0.52) if geom == "slab" else (1.9,)):
        g.cvt_TSDF_to_voxels_slice(z, dz=0.5)
        n = g.num_TSDF_particles[None]
        sxyz, sval, _, sn = o.slice_voxels(z, 0.5)
        assert n == sn > 100, (z, n, sn)
        a = sorted_rows(np.concatenate([g.export_TSDF_xyz.to_numpy()[:n], g.export_TSDF.to_numpy()[:n, None]], 1))
        assert np.array_equal(a, sorted_rows(np.concatenate([sxyz, sval[:, None]], 1))), z
    e = o.export_sparse()
    m = DenseTSDF(**GEOM[geom][0])
    m.load_numpy(0, e["indices"], e["TSDF"], e["W_TSDF"], e["occupy"], e["color"])
    assert_export_equal(m.export_submap(), e, f"{geom}: oracle export -> load_numpy -> export")


# ------------------------------------------------------------------------------------------------------------------ 3. queries
@BOTH
def test_point_queries_and_ray_casts(hip_lib, geom):
    """mapping_common.py:159-201: is_pos_occupy / is_pos_unobserved / is_near_pos_occupy for points in and around the volume, BaseMap.raycast for rays from
    the last sensor position and steep rays that leave through the top and bottom faces; host and device-tensor forms.  A ray "hits" where the TSDF is below
    the surface threshold, and an unobserved voxel or one outside the volume reads 0: a ray only misses when it stays in observed free space to its end.  So
    the steep rays start at observed free voxels (from the sensor position, outside the frustum, they would stop at once), and the rays are cast twice:
    over 4 m (they all end somewhere, in SLAB some beyond a z face) and over 1 m (some end in free space)."""
    import torch
    g, o, frames = _hip(geom)
    vs = SLAB["voxel_scale"]
    rng = np.random.default_rng(5)
    half = np.array([g.N, g.N, g.Nz]) * vs / 2 + 0.3
    pts = rng.uniform(-half, half, size=(4096, 3)).astype(np.float32)
    for mode in (0, 1, 2):
        want = o.query_points(mode, pts, 2).astype(bool)
        host = g._query_points(mode, pts, 2)
        dev = g._query_points(mode, torch.from_numpy(pts).cuda(), 2)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
        assert 0 < want.sum() < want.size and np.array_equal(host, want), f"mode {mode}"
    dirs = rng.normal(size=(128, 3))
    ang, phi = np.radians(rng.uniform(0, 20, 64)), rng.uniform(0, 2 * np.pi, 64)
    up = np.stack([np.sin(ang) * np.cos(phi), np.sin(ang) * np.sin(phi), np.cos(ang) * np.where(np.arange(64) % 2, -1.0, 1.0)], 1)
    dirs = np.concatenate([dirs / np.linalg.norm(dirs, axis=1, keepdims=True), up]).astype(np.float32)
    pos = np.tile(frames[-1][1].astype(np.float32), (192, 1))
    e = o.export_sparse()
    free = e["indices"][e["TSDF"].astype(np.float32) > 0.3]
    pos[128:] = free[rng.integers(0, len(free), 64)].astype(np.float32) * np.float32(vs)
    for max_dist in (4.0, 1.0):
        oh, oe, ol = o.raycast(pos, dirs, max_dist)
        if max_dist == 1.0:
            assert 0 < oh.sum() < 192 and 0 < oh[128:].sum() < 64
        elif geom == "slab":
            assert (np.abs(oe[128:, 2]) > g.Nz * vs / 2).sum() >= 8     # steep rays that end beyond the top or the bottom face
        h0, e0, l0 = g.raycast(pos, dirs, max_dist)
        h1, e1, l1 = g.raycast(torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda(), max_dist)
        assert np.array_equal(h1.cpu().numpy(), h0) and np.array_equal(e1.cpu().numpy(), e0) and np.array_equal(l1.cpu().numpy(), l0)
        assert np.array_equal(h0, oh.astype(bool)) and np.array_equal(e0, oe) and np.array_equal(l0, ol), max_dist


# ------------------------------------------------------------------------------------------------------------------ 4. marching cubes
def _tri_keys(v, n):
    return sorted_rows(np.concatenate([v.reshape(-1, 9), n.reshape(-1, 9)], axis=1))


@BOTH
@pytest.mark.parametrize("step,gather", [(1, 0), (1, 1), (2, 0)])
def test_marching_cubes(hip_lib, geom, step, gather):
    """marching_cube_mesher.py:44-187: the LDS tile kernel (step 1), the gather kernel at step 1 (mesh_gather) and at step 2, as sorted triangle rows"""
    from taichislam_amd.mapping import MarchingCubeMesher
    g, o, _ = _hip(geom)
    g.set_option("mesh_gather", gather)
    mesher = MarchingCubeMesher(g, 400000, tsdf_surface_thres=THRES)
    mesher.generate_mesh(step)
    ov, on, _, ontri = o.generate_mesh(step, THRES, 400000)
    assert mesher.num_facelets[None] == ontri > 1000
    gv, gn, _ = mesher.get_mesh()
    a, b = _tri_keys(gv, gn), _tri_keys(ov, on)
    assert np.array_equal(a[:, :9], b[:, :9]), "mesh vertices differ"
    assert np.array_equal(np.isnan(a[:, 9:]), np.isnan(b[:, 9:]))
    assert np.array_equal(np.nan_to_num(a[:, 9:]), np.nan_to_num(b[:, 9:])), "mesh normals differ"


# ------------------------------------------------------------------------------------------------------------------ 5. ESDF
@pytest.fixture(params=[1, 0], ids=["wavefront", "regional"])
def esdf_mode(request, monkeypatch):
    """both forms of the incremental update, as tests/test_esdf_gpu.py runs them"""
    monkeypatch.setenv("TSL_ESDF_MODE", str(request.param))
    return request.param


@functools.lru_cache(maxsize=None)
def _oracle_esdf(geom, max_dist=1.0):
    oi, oe = _oracle(geom)[2].esdf(max_dist=max_dist)
    oo = np.argsort(lin(oi))
    return oi[oo], oe[oo]


def _esdf_sorted(m):
    i, e = m.export_esdf()
    o = np.argsort(lin(i))
    return i[o], e[o]


@BOTH
def test_esdf_equals_the_oracle(hip_lib, esdf_mode, geom):
    g, o, _ = _hip(geom)
    g.update_esdf(max_dist=1.0)
    assert g.get_option("esdf_mode") == esdf_mode and g.get_option("esdf_orphans") == 0
    gi, ge = _esdf_sorted(g)
    oi, oe = _oracle_esdf(geom)
    assert gi.shape[0] == oi.shape[0] > 50000 and np.array_equal(gi, oi)
    assert np.array_equal(ge, oe), f"{(ge != oe).sum()} voxels differ, first {gi[ge != oe][:4]}, max diff {np.abs(ge - oe).max()}"


def test_esdf_incremental_equals_full_equals_oracle_after_every_frame(hip_lib, esdf_mode):
    from oracle import BATCHED, OracleTSDF
    from taichislam_amd.mapping import DenseTSDF
    K, frames, ref, stats = _oracle("slab", 6)
    inc, full = DenseTSDF(**SLAB), DenseTSDF(**SLAB)
    for m in (inc, full):
        m.set_dep_camera_intrinsic(K)
    full.set_option("esdf_full", 1); full.set_option("esdf_mode", 0)
    o = OracleTSDF(**SLAB)
    o.set_intrinsics(K, K)
    for f, (R, T, d) in enumerate(frames):
        for m in (inc, full):
            m.recast_depth_to_map(R, T, d, None)
            m.update_esdf(max_dist=1.0)
        o.integrate_depth(R, T, d, mode=BATCHED)
        assert inc.esdf_stats()["incremental"] == (1 if f else 0) and full.esdf_stats()["incremental"] == 0
        (ii, ie), (fi, fe) = _esdf_sorted(inc), _esdf_sorted(full)
        assert np.array_equal(ii, fi) and np.array_equal(ie, fe), f"frame {f}: incremental != full at {(ie != fe).sum()} voxels, first {ii[ie != fe][:4]}"
        oi, oe = o.esdf(max_dist=1.0)
        oo = np.argsort(lin(oi))
        assert np.array_equal(ii, oi[oo]) and np.array_equal(ie, oe[oo]), f"frame {f}: != oracle at {(ie != oe[oo]).sum()} voxels"
    assert inc.get_option("esdf_orphans") == 0


def test_esdf_slice_matches_the_oracle_layer(hip_lib, esdf_mode):
    """cvt_ESDF_to_voxels_slice(z) (dense_esdf.py:498-509): the layer index counts from the bottom of the volume, Nz / 2 below the origin -- built as
    tests/test_boundary_gpu.py builds it"""
    g, o, _ = _hip("slab")
    vs = SLAB["voxel_scale"]
    g.update_esdf(max_dist=1.0)
    oi, oe = _oracle_esdf("slab")
    assert g.Nz == 48 != g.N
    for z in (0.0, 0.37, -0.52):
        g.cvt_ESDF_to_voxels_slice(z)
        n = g.num_export_ESDF_particles[None]
        xyz, val = g.export_ESDF_xyz.to_numpy(n), g.export_ESDF.to_numpy(n)
        index_f = np.float32((z + g.Nz * vs / 2.0) / vs)
        ku = (oi[:, 2].astype(np.int32) + g.Nz // 2).astype(np.float32)
        sel = (index_f - np.float32(0.5) < ku) & (ku < index_f + np.float32(0.5))
        want_xyz = oi[sel].astype(np.float32) * np.float32(vs)
        assert n == int(sel.sum()) > 500, (z, n, int(sel.sum()))
        a = sorted_rows(np.concatenate([xyz, val[:, None]], 1)); b = sorted_rows(np.concatenate([want_xyz, oe[sel][:, None]], 1))
        assert np.array_equal(a, b), f"slice z={z}"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@BOTH
def test_esdf_queries_equal_the_restatement_over_the_oracle(hip_lib, esdf_mode, geom):
    """query_esdf, nearest and interpolated (csrc/tsl_esdf_query.hip), against tests/esdf_query_ref.py on an N x N x Nz grid: status bytes, distances and
    gradients bit for bit, as tests/test_esdf_query_gpu.py compares them.  A quarter of the points lie within one voxel of a z face."""
    import esdf_query_ref as ref
    g, o, _ = _hip(geom)
    g.update_esdf(max_dist=1.0)
    oi, oe = _oracle_esdf(geom)
    val, known, lo = ref.grid_from_export(oi, oe, g.N, g.Nz)
    assert val.shape[2] != val.shape[0]
    vs = np.float32(g.voxel_scale)
    unk = np.float32(-3.5)
    rng = np.random.default_rng(7)
    half = np.array([g.N, g.N, g.Nz]) * float(vs) / 2
    kidx = oi[rng.integers(0, len(oi), 1024)]
    pts = np.concatenate([rng.uniform(-half - 0.2, half + 0.2, (1024, 3)),
                          (kidx + rng.uniform(-1, 1, kidx.shape)) * float(vs),
                          (oi[rng.integers(0, len(oi), 1024)] + rng.uniform(0, 1, (1024, 3))) * float(vs)])
    face = rng.uniform(-half, half, (1024, 3))
    col = oi[np.abs(oi[:, 2] + 0.5) > g.Nz // 2 - 3][:, :2] if geom == "slab" else oi[:, :2]       # above and below observed columns
    face[:, :2] = (col[rng.integers(0, len(col), 1024)] + rng.uniform(0, 1, (1024, 2))) * float(vs)
    face[:, 2] = np.where(np.arange(1024) % 2, -1.0, 1.0) * half[2] + rng.uniform(-1, 1, 1024) * float(vs)
    pts = np.concatenate([pts, face]).astype(np.float32)
    assert pts.shape == (4096, 3)
    for mode in (0, 1):
        d, gr, s = g.query_esdf(pts, interpolate=bool(mode), unknown_value=unk, refresh=False)
        wd, wg, ws = ref.query(pts, mode, vs, val, known, lo, unknown=unk)
        counts = np.bincount(ws, minlength=3)
        assert counts[0] > 500 and counts[1] > 100 and counts[2] > 100, counts
        if geom == "slab":                                            # known cells next to the z faces, and refusals beyond them
            assert (ws[3072:] == 0).sum() > 20 and (ws[3072:] == 2).sum() > 100, np.bincount(ws[3072:], minlength=3)
        bad = np.nonzero((_bits(d) != _bits(wd)) | (s != ws))[0]
        assert bad.size == 0, f"mode {mode}: {bad.size} queries differ, first {pts[bad[:4]]}: {d[bad[:4]]} / {wd[bad[:4]]}, status {s[bad[:4]]} / {ws[bad[:4]]}"
        if mode:
            assert np.array_equal(_bits(gr), _bits(wg)), f"gradient differs at {(_bits(gr) != _bits(wg)).any(1).sum()} queries"
        else:
            assert gr is None


# ------------------------------------------------------------------------------------------------------------------ 6. fusion and merge
BASES = ((tilt(np.eye(3), 0.17, 0.05), np.array([0.013, 0.021, -0.037])), (tilt(np.eye(3), -0.11, 0.08), np.array([-0.027, 0.009, 0.031])))
SUBCFG = dict(SLAB, max_submap_num=8)
GCFG = dict(GSLAB, max_submap_num=8)


@functools.lru_cache(maxsize=None)
def _oracle_fusion():
    """two level SLAB submaps of two frames each, fused by the oracle (BATCHED) into GSLAB; (K, frames, sorted export of the global map)"""
    from oracle import BATCHED, OracleTSDF
    K, frames = small_stream(4)
    o = OracleTSDF(**SUBCFG)
    o.set_intrinsics(K, K)
    stats = []
    for sid, (Rb, Tb) in enumerate(BASES):
        o.set_active_submap(sid)
        o.set_base_pose_submap(sid, Rb, Tb)
        stats += [o.integrate_depth(R, T, d, mode=BATCHED) for R, T, d in frames[2 * sid:2 * sid + 2]]
        _covers("slab", o.export_sparse()["indices"], stats)
    o.set_active_submap(2)
    og = OracleTSDF(**GCFG)
    for sid, (Rb, Tb) in enumerate(BASES):
        og.set_base_pose_submap(sid, Rb, Tb)
    og.fuse_submaps(o, mode=BATCHED)
    e = sort_export(og.export_sparse())
    k = e["indices"][:, 2]
    assert e["indices"].shape[0] > 50000 and -32 < k.min() < -24 and 23 < k.max() < 31 and not np.isnan(e["TSDF"].view(np.float16)).any()
    return K, frames, e


def _hip_submaps():
    from taichislam_amd.mapping import DenseTSDF
    K, frames, _ = _oracle_fusion()
    g = DenseTSDF(**SUBCFG)
    g.set_dep_camera_intrinsic(K)
    for sid, (Rb, Tb) in enumerate(BASES):
        g.active_submap_id[None] = sid
        g.set_base_pose_submap(sid, Rb, Tb)
        for R, T, d in frames[2 * sid:2 * sid + 2]:
            g.recast_depth_to_map(R, T, d, None)
    g.active_submap_id[None] = 2                                       # closed, as create_new_submap would
    return g


def _hip_global():
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**GCFG)
    for sid, (Rb, Tb) in enumerate(BASES):
        g.set_base_pose_submap(sid, Rb, Tb)
    return g


def _assert_fused(got, want, what):
    assert got["indices"].shape == want["indices"].shape and np.array_equal(got["indices"], want["indices"]), f"{what}: voxel sets differ"
    tg, to = got["TSDF"].view(np.float16), want["TSDF"].view(np.float16)
    assert np.array_equal(np.isnan(tg), np.isnan(to)), what
    ok = ~np.isnan(tg)
    for k in ("TSDF", "W_TSDF", "occupy"):
        bad = np.nonzero((got[k] != want[k]) & (ok if k == "TSDF" else True))[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} voxels, first {got['indices'][bad[:4]]}"


@pytest.mark.parametrize("direct", [0, 1])
def test_fuse_submaps_into_a_slab(hip_lib, direct):
    """dense_tsdf.py:272-318, default and with fuse_direct = 1, with the NaN handling of tests/test_fusion_mesh_gpu.py::test_fuse_submaps_bit_exact"""
    _, _, want = _oracle_fusion()
    sub, g = _hip_submaps(), _hip_global()
    g.set_option("fuse_direct", direct)
    g.fuse_submaps(sub)
    # true for these yaw-like base poses, not for every pose: tests/test_fuse_poses_gpu.py has the rotations at which corner splats leave the window
    assert g.get_option("fuse_window_misses") == 0
    _assert_fused(sort_export(g.export_submap()), want, f"fuse_direct {direct}")
    g.fuse_submaps(sub)                                                # the global map is rebuilt from scratch (dense_tsdf.py:313)
    _assert_fused(sort_export(g.export_submap()), want, f"fuse_direct {direct}, fused again")


def test_one_rank_merge_into_a_slab(hip_lib):
    """csrc/tsl_merge.hip: the one-call merge, its records form (merge_exchange = 1) and the step protocol give the TSDF / W of the fusion, as
    tests/test_merge_gpu.py checks on cubes"""
    from taichislam_amd import distributed as D
    _, _, want = _oracle_fusion()
    sub = _hip_submaps()

    def same(g, what):
        got = sort_export(g.export_submap())
        assert got["indices"].shape == want["indices"].shape and np.array_equal(got["indices"], want["indices"]), f"{what}: voxel sets differ"
        ok = ~np.isnan(got["TSDF"].view(np.float16))
        assert np.array_equal(got["TSDF"][ok], want["TSDF"][ok]) and np.array_equal(got["W_TSDF"], want["W_TSDF"]) and np.array_equal(got["occupy"], want["occupy"]), what
    g = _hip_global()
    assert g.allreduce_merge(sub, None) == 0
    same(g, "native, one rank")
    g1 = _hip_global()
    g1.set_option("merge_exchange", 1)
    assert g1.allreduce_merge(sub, None) == 0
    same(g1, "native, one rank, records")
    g2 = _hip_global()
    assert D.allreduce_merge(g2, sub) == 0
    same(g2, "steps, one rank")
    g3 = _hip_global()
    assert D.allreduce_merge(g3, sub, exchange="scatter_gather") == 0
    same(g3, "steps, one rank, records")


# ------------------------------------------------------------------------------------------------------------------ 7. render, track, register
def _slab_grid():
    import render_view_ref as rv
    o = _oracle("slab")[2]
    e = o.export_sparse()
    grid = rv.grid_from_export(e["indices"], e["TSDF"], o.N, o.Nz)
    assert grid[0].shape[2] != grid[0].shape[0]
    return grid


@functools.lru_cache(maxsize=None)
def _slab_source():
    """A second SLAB submap for the registration, built as tests/register_scenes.py builds its source: frames 1 .. 3 of the stream integrated at D^-1 P, D a
    fixed displacement of a few voxels on every axis, z included, and 2 degrees about a skew axis; (D, the oracle's export)"""
    import track_scenes as ts
    from oracle import BATCHED, OracleTSDF
    Rd, Td = ts.rotation((1.0, -2.0, 0.5), 2.0), np.array([0.11, -0.07, 0.09])
    K, frames = small_stream(4)
    o = OracleTSDF(**SLAB)
    o.set_intrinsics(K, K)
    src_frames = [(Rd.T @ R, Rd.T @ (T - Td), d) for R, T, d in frames[1:]]
    stats = [o.integrate_depth(R, T, d, mode=BATCHED) for R, T, d in src_frames]
    e = o.export_sparse()
    _covers("slab", e["indices"], stats)
    return (Rd, Td), K, src_frames, e


def _hip_source():
    from taichislam_amd.mapping import DenseTSDF
    _, K, src_frames, e = _slab_source()
    s = DenseTSDF(**SLAB)
    s.set_dep_camera_intrinsic(K)
    for R, T, d in src_frames:
        s.recast_depth_to_map(R, T, d, None)
    assert_export_equal(s.export_submap(), e, "the source submap against the oracle's")
    return s


def test_render_view_of_a_slab(hip_lib):
    """csrc/tsl_render.hip against tests/render_view_ref.py over the oracle's map, as tests/test_render_view_gpu.py compares its room views: from the pose of
    frame 1, inside the map, and from above the slab, looking down through its top face at the wall"""
    import render_view_ref as rv
    import render_view_scenes as sc
    from taichislam_amd.utils import synthetic as syn
    from test_render_view_gpu import _check_equal
    g, o, frames = _hip("slab")
    val, known, lo = _slab_grid()
    h, w = 120, 160
    K = syn.scaled_intrinsics(h, w)
    vs = np.float32(SLAB["voxel_scale"])
    top = SLAB["map_scale"][1] / 2
    Ta = np.array([1.2, 0.1, top + 0.45])
    fwd = np.array([2.9, 0.0, 0.0]) - Ta
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
    Ra = np.stack([right, np.cross(fwd, right), fwd], 1)
    for name, R, T in (("frame1", frames[1][0], frames[1][1]), ("above", Ra, Ta)):
        for step in (None, float(np.float32(0.4) * vs)):
            dt = sc.default_step(vs) if step is None else np.float32(step)
            want = rv.render(R, T, K, h, w, 0.3, 5.0, dt, vs, val, known, lo, None)
            hits = ((want[3] & ~np.uint8(0x40)) == 0).mean()
            assert hits >= 0.2 and (want[3] == 1).any(), (name, hits)        # (the slab holds the wall only within 0.96 m of the camera's height)
            _check_equal(g.render_view(R, T, K=K, shape=(h, w), step=step), want, f"slab, {name}, step {step}")
            _check_equal(g.render_view(R, T, K=K, shape=(h, w), step=step, skip=False), want, f"slab, {name}, step {step}, no skipping")
    assert Ta[2] > top


def test_align_linearize_on_a_slab(hip_lib):
    """csrc/tsl_align.hip: the 33 integers against tests/track_ref.py over the oracle's map: frame 1 at its own pose and at a pose 3 cm / 1.5 degrees off"""
    import track_ref as tr
    import track_scenes as ts
    g, o, frames = _hip("slab")
    grid = _slab_grid()
    K = _oracle("slab")[0]
    R, T, depth = frames[1]
    gates = dict(d_min=SLAB["min_ray_length"], d_max=SLAB["max_ray_length"], r_max=float(np.float32(SLAB["internal_voxels"] * SLAB["voxel_scale"])), g_max=4.0)
    vs = np.float32(SLAB["voxel_scale"])
    for name, Rp, Tp in (("true", R, T), ("perturbed", ts.rotation((0.3, -1.0, 0.6), 1.5) @ R, T + np.array([0.012, -0.017, 0.021]))):
        for stride, huber in ((1, 0.0), (2, 0.02)):
            want = tr.linearize(depth, Rp, Tp, K, stride, vs, grid, huber=huber, **gates)
            assert want[tr.I_USED] > 1000 and want[tr.I_UNKNOWN] > 1000, (name, want[tr.I_USED:])
            got = g.align_linearize(depth, Rp, Tp, K=K, stride=stride, huber=huber)
            bad = np.nonzero(got["sums"] != want)[0]
            assert bad.size == 0, f"{name}, stride {stride}, huber {huber}: sums {bad.tolist()} differ: {got['sums'][bad]} / {want[bad]}"


def test_register_linearize_score_and_search_on_a_slab(hip_lib):
    """csrc/tsl_register.hip, tsl_register_search.hip against tests/register_ref.py / register_search_ref.py over the oracle's maps: the linearisation at D and
    at a pose off D, the scores of a batch of eight poses, one search window of 27 translations x 3 yaw angles"""
    import register_ref as rr
    import register_search_ref as sr
    import track_ref as tr
    import track_scenes as ts
    from test_register_search_gpu import _same_scores, _same_search
    dst, o, _ = _hip("slab")
    src = _hip_source()
    (Rd, Td), _, _, e = _slab_source()
    grid = _slab_grid()
    sv = rr.source(e)
    vs = np.float32(SLAB["voxel_scale"])
    gates = rr.defaults(vs, SLAB["internal_voxels"], SLAB["voxel_scale"])
    R0, T0 = ts.rotation((0.2, 0.5, -1.0), 1.5) @ Rd, Td + np.array([0.02, -0.015, 0.025])
    for name, R, T, stride in (("D", Rd, Td, 1), ("off D", R0, T0, 2)):
        want = rr.linearize(sv, R, T, stride, vs, grid, **gates)
        assert want[tr.I_USED] > 500 and want[tr.I_UNKNOWN] > 500, want[tr.I_E:]
        got = dst.register_linearize(src, R, T, stride=stride)["sums"]
        assert np.array_equal(got, want), f"{name}: sums differ at {np.nonzero(got != want)[0].tolist()}"
    rng = np.random.default_rng(29)
    poses = [(Rd, Td), (R0, T0)] + [(ts.rotation(rng.standard_normal(3), rng.uniform(-4, 4)) @ Rd, Td + rng.uniform(-0.15, 0.15, 3)) for _ in range(6)]
    Rs, Ts = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    want = sr.score(sv, Rs, Ts, 2, vs, grid, **gates)
    assert (np.asarray(want["n_used"]) > 300).all()
    _same_scores(dst.register_score(src, Rs, Ts, stride=2), want, "slab, eight poses")
    kw = dict(window_t=(0.1, 0.1, 0.1), step_t=0.1, window_r=(0, 0, 0.05), step_r=0.05)
    n_t, steps_t = sr.half_counts(kw["window_t"], kw["step_t"])
    n_r, steps_r = sr.half_counts(kw["window_r"], kw["step_r"])
    Rw, Tw, winfo = sr.search(sv, R0, T0, vs, grid, SLAB["voxel_scale"], n_t, steps_t, n_r, steps_r, **gates)
    assert winfo["search"]["n_candidates"] == 81 and winfo["search"]["n_valid"] > 0
    Rg, Tg, info = dst.register_search(src, R0, T0, return_scores=True, **kw)
    _same_search(info, winfo, "slab, 81 candidates")
    b = lambda a: np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)
    assert np.array_equal(b(Rg), b(Rw)) and np.array_equal(b(Tg), b(Tw))


# ------------------------------------------------------------------------------------------------------------------ 8. Octomap
OCFG = dict(map_scale=[12.8, 1.6], voxel_scale=0.05, min_occupy_thres=2, min_ray_length=0.3, max_ray_length=5.0, K=2, max_submap_num=8)


def _octo_pair(**kw):
    from oracle import OracleOctomap
    from taichislam_amd.mapping import Octomap
    cfg = dict(OCFG, **kw)
    g, o = Octomap(**cfg), OracleOctomap(**{k: v for k, v in cfg.items() if k != "max_disp_particles"})
    assert (g.N, g.Nz, g.Rxy, g.Rz) == (o.N, o.Nz, o.Rxy, o.Rz) == (256, 32, 8, 5)
    return g, o


def _leaves_equal(g, o, colour=False):
    """as tests/test_octomap_gpu.py compares them; returns the oracle's leaf indices"""
    gl, ol = g.export_leaves(with_color=colour), o.export_leaves(with_color=colour)
    a = sorted_rows(np.concatenate([gl[0].astype(np.float64), gl[1][:, None]] + ([gl[2]] if colour else []), 1))
    b = sorted_rows(np.concatenate([ol[0].astype(np.float64), ol[1][:, None]] + ([ol[2]] if colour else []), 1))
    assert a.shape == b.shape and a.shape[0] > 100 and np.array_equal(a, b)
    return ol[0]


def test_octomap_slab_depth_points_and_levels(hip_lib):
    """taichi_octomap.py:116-169 with Rxy = 8, Rz = 5: the last three levels of the tree have cells of K x K x 1.  Leaves, frame counters and the exports of
    levels 0 .. 3 against the oracle.
    The leaves reach k = 27 although Nz / 2 = 16, and that is the reference: the root of its tree has K cells per axis ON TOP of the Rxy levels
    (taichi_octomap.py:65-70), so the tree spans K^(Rxy + 1) = 2 N cells in x and y and K^(1 + min(Rxy, Rz)) = 2 Nz cells in z, from -N / 2 and -Nz / 2
    (:72): k = -16 .. 47 here.  The oracle and the HIP tree (ext_z) keep exactly those leaves; points below -Nz / 2 or above are dropped and counted (p_oob)."""
    K, frames = small_stream(3)
    g, o = _octo_pair()
    g.set_dep_camera_intrinsic(K); o.set_intrinsics(K)
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, np.array([], dtype=int))
        so = o.integrate_depth(R, T, d)
        sg = g.last_frame_stats()
        assert so["p_oob"] > 0 and so["p_valid"] > so["p_oob"]
        assert (sg["p_used"], sg["p_valid"], sg["p_oob"]) == (so["p_used"], so["p_valid"], so["p_oob"])
    k = _leaves_equal(g, o)[:, 2]
    assert k.min() == -16 and 16 < k.max() < 48
    for level in (0, 1, 2, 3):
        gx, _ = g.get_occupy_voxels(level)
        ox, on = o.occupied_voxels(level)
        assert gx.shape[0] == on > 100 and np.array_equal(sorted_rows(gx), sorted_rows(ox)), f"level {level}"
    rng = np.random.default_rng(3)
    pts = np.tile((rng.uniform(-1, 1, size=(5000, 3)) * [4.0, 4.0, 3.0]).astype(np.float32), (3, 1))      # three hits per leaf: above min_occupy_thres
    g.recast_pcl_to_map(frames[0][0], frames[0][1], pts, None, 15000)
    so = o.integrate_points(frames[0][0], frames[0][1], pts)
    sg = g.last_frame_stats()
    assert so["p_oob"] > 500 and (sg["p_used"], sg["p_valid"], sg["p_oob"]) == (so["p_used"], so["p_valid"], so["p_oob"])
    k = _leaves_equal(g, o)[:, 2]
    assert k.min() == -16 and k.max() == 47
    for level in (0, 1, 2, 3):
        gx, _ = g.get_occupy_voxels(level)
        ox, on = o.occupied_voxels(level)
        assert gx.shape[0] == on > 100 and np.array_equal(sorted_rows(gx), sorted_rows(ox)), f"level {level}, after the point cloud"


def test_octomap_slab_colour(hip_lib):
    """leaf colours (taichi_octomap.py:120-124) of depth frames with textures and of a coloured point cloud, and the coloured export"""
    K, frames = small_stream(3)
    g, o = _octo_pair(texture_enabled=True, max_disp_particles=200000)
    g.set_dep_camera_intrinsic(K); g.set_color_camera_intrinsic(K); o.set_intrinsics(K, K)
    rng = np.random.default_rng(5)
    for R, T, d in frames:
        tex = rng.integers(0, 256, size=(d.shape[0], d.shape[1], 3)).astype(np.uint8)
        g.recast_depth_to_map(R, T, d, tex)
        assert o.integrate_depth(R, T, d, tex)["p_oob"] > 0
    _leaves_equal(g, o, colour=True)
    pts = (rng.uniform(-1, 1, size=(20000, 3)) * [3.0, 3.0, 2.6]).astype(np.float32)
    pts[:4000] = pts[4000:8000]                                               # several points per leaf: the last one wins
    rgb = rng.integers(0, 256, size=(20000, 3)).astype(np.uint8)
    g.recast_pcl_to_map(frames[0][0], frames[0][1], pts, rgb)
    assert o.integrate_points(frames[0][0], frames[0][1], pts, rgb)["p_oob"] > 0
    _leaves_equal(g, o, colour=True)
    gx, gcol = g.get_occupy_voxels(0)
    ox, ocol, on = o.occupied_voxels(0, with_color=True)
    assert gx.shape[0] == on > 0 and np.any(gcol > 0)
    assert np.array_equal(sorted_rows(np.concatenate([gx, gcol], 1)), sorted_rows(np.concatenate([ox, ocol], 1)))


def test_octomap_slab_fusion(hip_lib):
    """fuse_submaps (taichi_octomap.py:171-189) of two level submaps into a slab global tree"""
    from oracle import OracleOctomap
    from taichislam_amd.mapping import Octomap
    K, frames = small_stream(4)
    g, o = _octo_pair(min_occupy_thres=0)
    g.set_dep_camera_intrinsic(K); o.set_intrinsics(K)
    for sid, (Rb, Tb) in enumerate(BASES):
        g.set_base_pose_submap(sid, Rb, Tb); o.set_base_pose_submap(sid, Rb, Tb)
        for R, T, d in frames[2 * sid:2 * sid + 2]:
            g.recast_depth_to_map(R, T, d, None)
            assert o.integrate_depth(R, T, d)["p_oob"] > 0
        _leaves_equal(g, o)
        g.switch_to_next_submap(); o.set_active_submap(sid + 1)
    gcfg = dict(OCFG, is_global_map=True, min_occupy_thres=0)
    gg, og = Octomap(**gcfg), OracleOctomap(**gcfg)
    for sid, (Rb, Tb) in enumerate(BASES):
        gg.set_base_pose_submap(sid, Rb, Tb); og.set_base_pose_submap(sid, Rb, Tb)
    gg.fuse_submaps(g); og.fuse_submaps(o)
    k = _leaves_equal(gg, og)[:, 2]
    assert k.min() < -8 and k.max() > 16

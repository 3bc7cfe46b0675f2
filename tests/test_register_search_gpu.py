"""The pose search for the registration on the GPU (tsl_register_search.hip): the scores of many poses against tsl_tsdf_register_linearize on the GPU and
against the numpy restatement (tests/register_search_ref.py), bit for bit, at the edges of a pose chunk and of the 64-, 128- and 256-entry tiles of
the voxel list, each one asked for by enough poses that the library takes it; small sources, many bricks and two submaps in one handle; the search (candidates, ranking, refinement) against the restatement from the two guesses the
plain registration loses; handles, refusals and SubmapMapping.search_submaps."""
import ctypes as C

import numpy as np
import pytest

import register_ref as rr
import register_scenes as rs
import register_search_ref as sr
import register_search_scenes as ss
import render_view_ref as rv
import track_ref as tr
import track_scenes as ts
from util import SMALL, assert_export_equal, sort_export

pytestmark = pytest.mark.gpu

F32 = np.float32
OTHER_GATES = dict(w_min=2.0, band=0.05, r_max=0.06, g_max=1.2)
LIGHT = dict(SMALL, max_bricks=4096)                              # a whole 256^3 volume of bricks
COUNTS = ("n_used", "n_unknown", "n_far", "n_grad")
_SLOT = dict(e=tr.I_E, n_used=tr.I_USED, n_unknown=tr.I_UNKNOWN, n_far=tr.I_FAR, n_grad=tr.I_GRAD)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _gates(**kw):
    return rr.defaults(rs.VS, SMALL["internal_voxels"], SMALL["voxel_scale"], **kw)


def _tsdf(frames=(), **kw):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**dict(LIGHT, **kw))
    g.set_dep_camera_intrinsic(ts.intrinsics())
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    return g


@pytest.fixture(scope="module")
def maps(hip_lib):
    """(destination, source): HIP maps of frames 0..5 and of the six source frames, compared once with the oracle's maps the restatement reads; no
    test writes them"""
    dst, src = _tsdf(rs.dst_frames()), _tsdf(rs.src_frames())
    assert_export_equal(dst.export_submap(), rs.dst_oracle().export_sparse(), "the destination against the oracle's")
    assert_export_equal(src.export_submap(), rs.src_export(), "the source against the oracle's")
    return dst, src


def _load(g, sid, e):
    if len(e["TSDF"]):
        g.load_numpy(sid, e["indices"], np.asarray(e["TSDF"]).view(np.float16), np.asarray(e["W_TSDF"]).view(np.float16), e["occupy"], None)


def _loaded(export, sid=0, **kw):
    """a map holding a sparse export in submap `sid`"""
    g = _tsdf(**kw)
    _load(g, sid, export)
    return g


def _export(idx, t, w=None):
    idx = np.asarray(idx, np.int16).reshape(-1, 3)
    n = idx.shape[0]
    return dict(indices=idx, TSDF=np.asarray(t, np.float16).reshape(n), W_TSDF=np.ones(n, np.float16) if w is None else np.asarray(w, np.float16).reshape(n),
                occupy=np.zeros(n, np.int8))


def busy_brick():
    """base index of the source brick with the most voxels in the band"""
    idx, t, w = rs.src_voxels()
    band = (np.abs(t) <= rs.GATES["band"])
    b = (idx[band] + 128) // 16
    key, cnt = np.unique(b[:, 0] * 65536 + b[:, 1] * 256 + b[:, 2], return_counts=True)
    k = int(key[np.argmax(cnt)])
    return np.array([k // 65536, (k // 256) % 256, k % 256]) * 16 - 128


def brick_export(n_band):
    """a source of one whole brick (all 4096 voxels observed): n_band of them within the band (values from default_rng(3), weight 1), the rest 0.5 m off"""
    base = busy_brick()
    loc = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    t = np.full(4096, 0.5, np.float16)
    pick = rng.permutation(4096)[:n_band]
    t[pick] = rng.uniform(-0.07, 0.07, n_band).astype(np.float16)
    return _export(base + loc, t)


def corner_cell():
    """index c of a destination voxel that is the last of its brick on all three axes and whose cell is KNOWN, the one nearest the surface: cells with
    base c + d, d in {-1, 0, 1}^3, read 1, 2, 4 and 8 bricks"""
    val, known, lo = rs.dst_grid()
    k8 = known[:-1, :-1, :-1].copy()
    for c in rv.CORNERS[1:]:
        k8 &= known[c[0]:known.shape[0] - 1 + c[0], c[1]:known.shape[1] - 1 + c[1], c[2]:known.shape[2] - 1 + c[2]]
    sel = np.zeros_like(k8)
    sel[15::16, 15::16, 15::16] = True
    cand = np.argwhere(k8 & sel)
    assert cand.shape[0] > 0
    best = cand[np.argmin(np.abs(val[cand[:, 0], cand[:, 1], cand[:, 2]]))]
    return best + lo


def corner_export():
    c = corner_cell()
    d = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
    return _export(c + d, np.full(27, 0.01, np.float16))


def slab_export():
    """a wide destination: the 16 voxel layers k = -8 .. 7 over the whole 256 x 256 plane (512 bricks), a tilted plane's distance, every voxel observed"""
    r = np.arange(-128, 128, dtype=np.int16)
    idx = np.stack(np.meshgrid(r, r, np.arange(-8, 8, dtype=np.int16), indexing="ij"), -1).reshape(-1, 3)
    t = (idx.astype(F32) * F32(rs.VS)) @ np.array([0.02, 0.01, 1.0], F32)
    return _export(idx, t.astype(np.float16))


def many_brick_sources():
    """(source, other): `source` spreads over 3005 of the 4096 bricks of the volume -- three bricks wholly in the band, two with 65 voxels in it, four
    voxels in each of the rest -- and `other`, for another submap of the same handle, one voxel in each of 1000 bricks; values from default_rng(17)"""
    rng = np.random.default_rng(17)
    bricks = rng.permutation(4096)
    loc = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    base = lambda b: np.array([b // 256, (b // 16) % 16, b % 16]) * 16 - 128
    heavy = [b for b in bricks[:3005] if b % 16 in (7, 8)][:5]      # the five heavy bricks lie in the slab's two brick layers
    idx, t = [], []
    for b in bricks[:3005]:
        if b in heavy[:3]:
            sel, tv = np.arange(4096), rng.uniform(-0.07, 0.07, 4096)
        elif b in heavy[3:]:
            sel, tv = np.arange(4096), np.full(4096, 0.5)
            tv[rng.permutation(4096)[:65]] = rng.uniform(-0.07, 0.07, 65)
        else:
            sel, tv = rng.choice(4096, 4, replace=False), rng.uniform(-0.07, 0.07, 4)
        idx.append(base(b) + loc[sel])
        t.append(tv)
    other = bricks[rng.permutation(4096)[:1000]]
    oidx = np.stack([base(b) + loc[rng.integers(4096)] for b in other])
    return _export(np.concatenate(idx), np.concatenate(t).astype(np.float16)), _export(oidx, rng.uniform(-0.07, 0.07, 1000).astype(np.float16))


def five_poses():
    """D, the three perturbed poses, the outside pose"""
    return [rs.displacement()] + rs.perturbed_poses() + [rs.outside_pose()]


def seventy_poses(centre=None, shift=0.3, deg=8.0):
    """the five poses, the centre pose (default D), then the centre moved by up to `shift` m and `deg` degrees (default_rng(29)), 70 in all"""
    Rc, Tc = rs.displacement() if centre is None else centre
    out = five_poses() + [(np.asarray(Rc, np.float64), np.asarray(Tc, np.float64))]
    rng = np.random.default_rng(29)
    while len(out) < 70:
        out.append((ts.rotation(rng.standard_normal(3), rng.uniform(-deg, deg)) @ Rc, Tc + rng.uniform(-shift, shift, 3)))
    return np.stack([p[0] for p in out]), np.stack([p[1] for p in out])


def _same_scores(got, want, what):
    for f in sr.FIELDS:
        bad = np.nonzero(np.asarray(got[f]) != np.asarray(want[f]))[0]
        assert bad.size == 0, f"{what}: {f} differs at poses {bad[:8].tolist()}: {np.asarray(got[f])[bad[:8]]} / {np.asarray(want[f])[bad[:8]]}"


def _check(dst, src, e, R, T, what, dst_grid=None, counts_only=False, **kw):
    """one score call against the restatement over the export `e` of the source (scores and gate); returns the dict"""
    gates = {k: kw.pop(k) for k in ("w_min", "band", "r_max", "g_max", "huber") if k in kw}
    stride = kw.get("stride", 1)
    full = _gates(**gates)
    sv = rr.source(e)
    want = sr.score(sv, R, T, stride, rs.VS, rs.dst_grid() if dst_grid is None else dst_grid, counts_only=counts_only, **full)
    got = dst.register_score(src, R, T, counts_only=counts_only, **gates, **kw)
    _same_scores(got, want, what)
    assert got["gate"] == sr.gate(sv, stride, **full), f"{what}: gate {got['gate']}"
    assert np.array_equal(got["e_f"], got["e"] * 2.0 ** -20) and all(got[f].dtype == np.int64 and got[f].shape == (len(np.asarray(T).reshape(-1, 3)),) for f in sr.FIELDS)
    return got


def _same_records(got, want, what):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"] == len(got["records"]), \
        f"{what}: status {got['status']} / {want['status']}, iterations {got['iterations']} / {want['iterations']}"
    for k, (a, b) in enumerate(zip(got["records"], want["records"])):
        assert np.array_equal(a["sums"], b["sums"]), f"{what}, record {k}: sums differ at {np.nonzero(a['sums'] != b['sums'])[0].tolist()}"
        for f in ("R", "T", "xi"):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), f"{what}, record {k}: {f} differs: {a[f]} / {b[f]}"


def _same_search(got, want, what, scores=True):
    """the report of a search against the restatement's, bit for bit"""
    g, w = got["search"], want["search"]
    for f in ("status", "n_candidates", "n_valid", "best", "J_best", "gate"):
        assert g[f] == w[f], f"{what}: {f} {g[f]} / {w[f]}"
    if w["best"] >= 0:
        assert g["score_best"] == w["score_best"], f"{what}: {g['score_best']} / {w['score_best']}"
    if scores and w["scores"] is not None:
        _same_scores(g["scores"], w["scores"], what)
    if w["pivot"] is not None:
        assert np.array_equal(_bits(g["pivot"]), _bits(w["pivot"])), f"{what}: pivot {g['pivot']} / {w['pivot']}"
    assert np.array_equal(_bits(g["R_best"]), _bits(w["R_best"])) and np.array_equal(_bits(g["T_best"]), _bits(w["T_best"])), f"{what}: the best candidate differs"
    _same_records(got, want, what)


def test_score_equals_linearize_and_the_restatement(maps):
    """The five scores of D, the three perturbed poses and the outside pose, repeated and shuffled to n = 1, 63, 64, 65, 256, 257 and 300 poses: against
    tsl_tsdf_register_linearize on the GPU and register_ref.linearize, strides 1, 4 and 16, huber 0 and 0.02; other gates; counts only; the gate."""
    dst, src = maps
    sv, grid = rs.src_voxels(), rs.dst_grid()
    P = five_poses()
    rng = np.random.default_rng(41)
    seen = np.zeros(5, np.int64)
    cases = [(st, dict(huber=h), False) for st in (1, 4, 16) for h in (0.0, 0.02)] + [(1, OTHER_GATES, False), (2, OTHER_GATES, False), (1, {}, True), (4, {}, True)]
    for stride, gates, counts_only in cases:
        full = _gates(**gates)
        lin_gpu = [dst.register_linearize(src, R, T, stride=stride, counts_only=counts_only, **gates)["sums"] for R, T in P]
        lin_ref = [rr.linearize(sv, R, T, stride, rs.VS, grid, **full) for R, T in P]
        for a, b in zip(lin_gpu, lin_ref):
            assert np.array_equal(a[tr.I_USED:], b[tr.I_USED:]) and (counts_only or np.array_equal(a, b))
        want_gate = sr.gate(sv, stride, **full)
        assert want_gate["n_gate"] == int(lin_gpu[0][tr.I_GATE])
        for n in (1, 63, 64, 65, 256, 257, 300):
            pick = rng.permutation(np.arange(n) % 5) if n > 1 else np.array([int(rng.integers(5))])
            R, T = np.stack([P[i][0] for i in pick]), np.stack([P[i][1] for i in pick])
            got = dst.register_score(src, R, T, stride=stride, counts_only=counts_only, **gates)
            what = f"stride {stride}, {gates}, counts only {counts_only}, {n} poses"
            for f in sr.FIELDS:
                want = np.array([int(lin_gpu[i][_SLOT[f]]) for i in pick], np.int64)
                assert np.array_equal(got[f], want), f"{what}: {f} differs at {np.nonzero(got[f] != want)[0][:8].tolist()}"
            assert got["gate"] == want_gate, f"{what}: gate {got['gate']} / {want_gate}"
            if counts_only:
                assert not got["e"].any()
        seen += [int(lin_ref[0][tr.I_USED]) > 0, want_gate["n_gate"] > 0] + [any(int(s[_SLOT[f]]) > 0 for s in lin_ref) for f in COUNTS[1:]]
    assert (seen > 0).all(), f"buckets used / gate / unknown / far / grad occurred in {seen.tolist()} cases"
    # the restatement's fast path on poses of its own: 70 at once
    R, T = seventy_poses()
    got = _check(dst, src, rs.src_export(), R, T, "70 poses, stride 4", stride=4)
    assert (got["n_used"][:4] > 150).all() and got["n_used"][4] == 0 and got["n_unknown"][4] == got["gate"]["n_pass"]


def test_small_sources(maps):
    """Sources built with load_numpy, 70 poses each: one voxel; an empty submap; one whole brick with 64, 65, 128, 129, 257, 1024, 1025 and 4096
    voxels in the band (70 poses are two chunks, so every list here is scored in tiles of 64 entries: these are that tile's edges, and a brick whole
    in the band fills the 4096 entries of the fill pass's queue; test_score_tiles has the larger tiles); the 27 cells around a destination brick
    corner."""
    dst, _ = maps
    Rd, Td = rs.displacement()
    idx, t, w = rs.src_voxels()
    R, T = seventy_poses()
    base = busy_brick()
    inb = np.nonzero(((idx >= base) & (idx < base + 16)).all(1) & (np.abs(t) <= rs.GATES["band"]))[0]
    one = inb[np.argmin(np.abs(t[inb]))]
    e = _export(idx[one], np.float16(t[one]), np.float16(w[one]))
    got = _check(dst, _loaded(e), e, R, T, "one voxel")
    assert got["gate"]["n_pass"] == 1 and got["n_used"][0] == 1 and ((got["n_used"] + got["n_unknown"] + got["n_far"] + got["n_grad"]) == 1).all()
    # an empty source submap: every score is zero, and so is the gate
    got = dst.register_score(_tsdf(), R, T)
    assert not any(got[f].any() for f in sr.FIELDS) and not any(got["gate"].values())
    # whole bricks
    for n_band in (64, 65, 128, 129, 257, 1024, 1025, 4096):
        e = brick_export(n_band)
        s = _loaded(e)
        for stride, huber in ((1, 0.0), (2, 0.02)):
            got = _check(dst, s, e, R, T, f"{n_band} of a brick in the band, stride {stride}", stride=stride, huber=huber)
            if stride == 1:
                assert got["gate"] == dict(got["gate"], n_pass=n_band, n_gate=4096 - n_band) and got["n_used"][0] > n_band // 4
    # 27 cells around a destination brick corner: 1, 2, 4 and 8 bricks per cell; poses within a voxel of the shift that puts voxel i into cell i
    e = corner_export()
    Rc, Tc = seventy_poses(centre=(np.eye(3), np.array([0.3, 0.4, 0.6]) * float(rs.VS)), shift=0.5 * float(rs.VS), deg=1.0)
    got = _check(dst, _loaded(e), e, Rc, Tc, "brick faces, edges and corners")
    assert got["n_used"][5] + got["n_far"][5] + got["n_grad"][5] >= 8 and got["n_used"][5] >= 1      # pose 5 is the shift itself


def _poses_for_tile(dst, entries, tile):
    """the least number of chunks of 64 poses at which a list of `entries` is scored in tiles of `tile`, less one pose: the last chunk is not full"""
    for chunks in range(1, 1025):
        if dst.register_score_tile(entries, chunks * 64) == tile:
            assert dst.register_score_tile(entries, chunks * 64 - 1) == tile
            return chunks * 64 - 1
    pytest.fail(f"no number of poses scores {entries} entries in tiles of {tile}")


def test_score_tiles(maps):
    """The tile of the list is 256 entries, halved down to 64 while tiles x chunks of poses would leave compute units idle: every case above ends at
    64.  Here the number of poses is chosen, by asking the library, so that it takes 128 and 256: the room's list at stride 1 (22387 entries, a
    multiple of neither: a tail of 115) against tsl_tsdf_register_linearize on the GPU and the restatement, and one brick with 129, 257, 1024, 1025
    and 4096 voxels in the band (a tail of one entry, whole tiles only) against the restatement.  The poses are few, repeated and shuffled."""
    dst, src = maps
    sv, grid = rs.src_voxels(), rs.dst_grid()
    rng = np.random.default_rng(43)
    assert dst.register_score_tile(0, 64) == dst.register_score_tile(100, 0) == dst.register_score_tile(100, 65537) == 0
    taken = set()

    def spread(want, m, n):
        pick = rng.permutation(np.arange(n) % m)
        return pick, {f: np.asarray(want[f])[pick] for f in sr.FIELDS}

    # the room
    P = five_poses()
    R5, T5 = np.stack([p[0] for p in P]), np.stack([p[1] for p in P])
    want5 = sr.score(sv, R5, T5, 1, rs.VS, grid, **_gates(huber=0.02))
    lin = [dst.register_linearize(src, R, T, huber=0.02)["sums"] for R, T in P]
    for f in sr.FIELDS:
        assert np.array_equal(want5[f], [int(s[_SLOT[f]]) for s in lin]), f
    entries = sr.gate(sv, 1, **rs.GATES)["n_pass"]
    assert entries % 128 and dst.register_score_tile(entries, 300) == 64
    for tile in (128, 256):
        n = _poses_for_tile(dst, entries, tile)
        pick, want = spread(want5, 5, n)
        got = dst.register_score(src, R5[pick], T5[pick], huber=0.02)
        _same_scores(got, want, f"the room, {n} poses, tiles of {tile}")
        assert got["gate"]["n_pass"] == entries
        taken.add((tile, entries % tile != 0))
    # one brick
    R70, T70 = seventy_poses()
    for n_band, tiles in ((129, (128,)), (257, (128, 256)), (1024, (128, 256)), (1025, (128, 256)), (4096, (128, 256))):
        e = brick_export(n_band)
        s = _loaded(e)
        want70 = sr.score(rr.source(e), R70, T70, 1, rs.VS, grid, **rs.GATES)
        for tile in tiles:
            n = _poses_for_tile(dst, n_band, tile)
            pick, want = spread(want70, 70, n)
            got = dst.register_score(s, R70[pick], T70[pick])
            _same_scores(got, want, f"{n_band} of a brick in the band, {n} poses, tiles of {tile}")
            assert got["gate"]["n_pass"] == n_band and want["n_used"].max() > n_band // 4
            taken.add((tile, n_band % tile != 0))
    assert taken == {(128, False), (128, True), (256, False), (256, True)}


def test_many_bricks(maps):
    """The 3005-brick source interleaved in the pool with another submap's 1000 bricks, against the 512-brick slab: src_sid 2 and 1, 70 poses, strides 1
    and 2.  The list holds 24 000 entries from thousands of bricks; the other submap's bricks are skipped."""
    from taichislam_amd.mapping import DenseTSDF
    se, oe = many_brick_sources()
    de = slab_export()
    dst = _loaded(de)
    grid = rv.grid_from_export(de["indices"], de["TSDF"], dst.N, dst.Nz)
    src = DenseTSDF(**dict(SMALL, max_submap_num=4, max_bricks=8192))
    n, m = se["TSDF"].shape[0], oe["TSDF"].shape[0]
    part = lambda e, a, b: {k: e[k][a:b] for k in ("indices", "TSDF", "W_TSDF", "occupy")}
    for c in range(8):                                        # alternate the two submaps so that their bricks interleave in the pool
        _load(src, 2, part(se, c * n // 8, (c + 1) * n // 8))
        _load(src, 1, part(oe, c * m // 8, (c + 1) * m // 8))
    src.active_submap_id[None] = 2
    assert src.bricks_in_use() >= 3005 + 900
    R, T = seventy_poses(centre=(ts.rotation(rs.D_AXIS, 1.0), rs.D_T), shift=0.1, deg=2.0)
    for stride in (1, 2):
        got = _check(dst, src, se, R, T, f"3005 bricks, stride {stride}", dst_grid=grid, src_sid=2, stride=stride, huber=0.02 if stride == 2 else 0.0)
        if stride == 1:
            assert got["gate"]["n_gate"] == 2 * (4096 - 65) and got["gate"]["n_pass"] == 3 * 4096 + 2 * 65 + 3000 * 4 and got["n_used"][5] > 5000
        got = _check(dst, src, oe, R, T, f"the other submap, stride {stride}", dst_grid=grid, src_sid=1, stride=stride)
        assert got["gate"]["n_pass"] + got["gate"]["n_gate"] == rr.visited(rr.source(oe), stride)
    assert src.get_active_submap_id() == 2


@pytest.mark.parametrize("name", ["B", "C"])
def test_search_equals_the_restatement(maps, name):
    """From the two guesses register_submap loses, with the defaults of register_search: the counts, the best candidate, its cost, all 5265 scores,
    the pivot and the best pose as bits, every refinement record and the pose out equal the restatement's; the result lies within
    register_scenes.REGISTER_BOUND_M / REGISTER_BOUND_DEG of D.  register_submap from the same guess does not."""
    dst, src = maps
    Rd, Td = rs.displacement()
    R0, T0 = ss.guess(name)
    Rw, Tw, want = ss.reference_search(name)
    R, T, info = dst.register_search(src, R0, T0, return_scores=True)
    _same_search(info, want, f"guess {name}")
    assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
    s = info["search"]
    em, ed = ts.pose_error(R, T, Rd, Td)
    print(f"guess {name}: best {s['best']} of {s['n_candidates']} ({s['n_valid']} valid), J {s['J_best']}, final error {em:.6f} m {ed:.6f} deg, status {info['status']}")
    assert s["n_candidates"] == 5265 and (s["best"], s["J_best"], s["n_valid"]) == ss.MEASURED_BEST[name]
    assert info["status"] == s["status"] == 0 and em <= rs.REGISTER_BOUND_M and ed <= rs.REGISTER_BOUND_DEG
    Rp, Tp, direct = dst.register_submap(src, R0, T0)
    dm, dd = ts.pose_error(Rp, Tp, Rd, Td)
    assert (dm > 1.0 or dd > 45.0) and direct["status"] == ss.MEASURED_DIRECT[name][2]
    # without the scores
    R2, T2, info2 = dst.register_search(src, R0, T0)
    assert "scores" not in info2["search"] and np.array_equal(_bits(R2), _bits(R)) and np.array_equal(_bits(T2), _bits(T)) and info2["search"]["best"] == s["best"]


def test_search_lattices(maps):
    """A given pivot with rotation offsets about all three axes on a 3^6 lattice; a lattice of one candidate (the registration from the guess); a
    huge min_used and an empty source: status 2 and the guess."""
    dst, src = maps
    sv, grid = rs.src_voxels(), rs.dst_grid()
    R0, T0 = rs.perturbed_poses()[2]
    pivot = np.array([1.4, 2.1, 0.2])
    kw = dict(window_t=(0.1, 0.1, 0.1), step_t=0.1, window_r=(0.05, 0.05, 0.05), step_r=0.05)
    for piv, stride, miss in ((pivot, 4, 0.0), (None, 2, 0.1)):
        R, T, info = dst.register_search(src, R0, T0, pivot=piv, stride=stride, miss=miss, return_scores=True, huber=0.02, **kw)
        Rw, Tw, want = sr.search(sv, R0, T0, rs.VS, grid, ss.VOXEL, (1, 1, 1), (0.1,) * 3, (1, 1, 1), (0.05,) * 3, pivot=piv, stride=stride, miss=miss, **_gates(huber=0.02))
        _same_search(info, want, f"3^6 lattice, pivot {piv}")
        assert info["search"]["n_candidates"] == 729 and np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
        assert len({int(v) for v in info["search"]["scores"]["e"]}) > 700            # the rotation offsets move the score on every axis
    assert np.array_equal(_bits(info["search"]["pivot"]), _bits(sr.auto_pivot(sv, R0, T0, 2, ss.VOXEL, **_gates(huber=0.02))[0]))
    # one candidate: the guess itself
    R, T, info = dst.register_search(src, R0, T0, window_t=(0, 0, 0), window_r=(0, 0, 0), return_scores=True)
    Rw, Tw, want = rs.reference_runs()[2]
    _same_records(info, want, "one candidate")
    s = info["search"]
    assert s["n_candidates"] == 1 and s["best"] == 0 and np.array_equal(_bits(s["R_best"]), _bits(R0)) and np.array_equal(_bits(s["T_best"]), _bits(T0))
    assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw)) and s["scores"]["n_used"][0] == s["score_best"]["n_used"] > 100
    # no valid candidate; nothing passes the gate
    R, T, info = dst.register_search(src, R0, T0, min_used=10 ** 9, **kw)
    s = info["search"]
    assert info["status"] == s["status"] == 2 and info["iterations"] == 0 and s["best"] == -1 and s["n_valid"] == 0 and s["n_candidates"] == 729
    assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(T), _bits(T0)) and s["gate"]["n_pass"] > 300
    for piv in (None, pivot):
        R, T, info = dst.register_search(_tsdf(), R0, T0, pivot=piv, **kw)
        assert info["status"] == info["search"]["status"] == 2 and info["iterations"] == 0 and info["search"]["gate"]["n_pass"] == 0
        assert np.array_equal(_bits(R), _bits(R0)) and np.array_equal(_bits(T), _bits(T0))


def test_handles(maps):
    """Two submaps of one handle without switching the active one; a global map as the destination; no map is written."""
    from taichislam_amd.mapping import DenseTSDF
    dst, src = maps
    sv, grid = rs.src_voxels(), rs.dst_grid()
    R, T = seventy_poses()
    want = sr.score(sv, R, T, 2, rs.VS, grid, **rs.GATES)
    both = _tsdf(max_submap_num=4, max_bricks=8192)
    _load(both, 0, rs.dst_oracle().export_sparse())
    _load(both, 2, rs.src_export())
    both.active_submap_id[None] = 1
    _same_scores(both.register_score(both, R, T, src_sid=2, dst_sid=0, stride=2), want, "one handle")
    swapped = both.register_score(both, R, T, src_sid=0, dst_sid=2, stride=2)          # the other direction reads the other table
    assert not np.array_equal(swapped["n_used"], want["n_used"]) and swapped["n_used"][0] > 1000
    assert not both.register_score(both, R, T, dst_sid=0)["n_used"].any() and both.get_active_submap_id() == 1      # src_sid None: the active submap, which is empty
    kw = dict(window_t=(0.1, 0, 0), step_t=0.1, window_r=(0, 0, 0.05), step_r=0.05)
    R0, T0 = rs.perturbed_poses()[0]
    Rw, Tw, winfo = sr.search(sv, R0, T0, rs.VS, grid, ss.VOXEL, (1, 0, 0), (0.1,) * 3, (0, 0, 1), (0.05,) * 3, **rs.GATES)
    Rg, Tg, info = both.register_search(both, R0, T0, src_sid=2, dst_sid=0, return_scores=True, **kw)
    _same_search(info, winfo, "one handle")
    assert np.array_equal(_bits(Rg), _bits(Rw)) and both.get_active_submap_id() == 1
    # a global map as the destination
    G = DenseTSDF(**dict(LIGHT, is_global_map=True))
    _load(G, 0, rs.dst_oracle().export_sparse())
    for sid in (None, 0):
        _same_scores(G.register_score(src, R, T, stride=2, dst_sid=sid), want, f"a global map, sid {sid}")
    Rg, Tg, info = G.register_search(src, R0, T0, return_scores=True, **kw)
    _same_search(info, winfo, "a global map")
    # neither map's export changes across the calls
    assert_export_equal(dst.export_submap(), rs.dst_oracle().export_sparse(), "the destination after the calls")
    assert_export_equal(src.export_submap(), rs.src_export(), "the source after the calls")
    ed, es = sort_export(dst.export_submap()), sort_export(src.export_submap())
    dst.register_score(src, R, T)
    dst.register_search(src, R0, T0, **kw)
    for a, b in ((ed, sort_export(dst.export_submap())), (es, sort_export(src.export_submap()))):
        assert all(np.array_equal(a[k], b[k]) for k in ("indices", "TSDF", "W_TSDF", "occupy"))


def test_refusals(hip_lib):
    """Every refusal of the two entry points, with the entry point named in the text.  The refusal of maps on different devices needs a second GPU."""
    from taichislam_amd import _lib
    from taichislam_amd.mapping import DenseTSDF
    dst, src = _loaded(rs.dst_oracle().export_sparse(), max_submap_num=4), _loaded(rs.src_export(), max_submap_num=4)
    G = DenseTSDF(**dict(LIGHT, is_global_map=True))
    other_vs = DenseTSDF(map_scale=[3.2, 3.2], voxel_scale=0.05, max_bricks=64)
    Rd, Td = rs.displacement()
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    NULL = object()
    L = dst.L
    SENTINEL = -12345

    def cfgs(stride=1, w_min=0.0, band=0.0, r_max=0.0, g_max=0.0, huber=0.0, levels=((2, 1),), min_step=1e-4, damping=0.0):
        c = _lib.RegisterCfg()
        c.stride, c.w_min, c.band, c.r_max, c.g_max, c.huber = stride, w_min, band, r_max, g_max, huber
        t = _lib.TrackCfg()
        t.n_levels = len(levels)
        for i, (st, it) in enumerate(levels[:4]):
            t.stride[i], t.iters[i] = st, it
        t.min_step, t.damping = min_step, damping
        return c, t

    def score(R=None, T=None, n=2, out=True, cfg=True, d=dst, s=src, dst_sid=-1, src_sid=-1, gate=True, **kw):
        c, _ = cfgs(**kw)
        Rn = np.tile(np.asarray(Rd).reshape(1, 9), (max(n, 1), 1)) if R is None else R
        Tn = np.tile(np.asarray(Td).reshape(1, 3), (max(n, 1), 1)) if T is None else T
        buf = (_lib.RegisterScore * max(n, 1))()
        for k in range(max(n, 1)):
            buf[k].e = SENTINEL
        g = _lib.RegisterGate()
        rc = L.tsl_tsdf_register_score(None if d is NULL else d.h, dst_sid, None if s is NULL else s.h, src_sid, None if R is NULL else dp(Rn), None if T is NULL else dp(Tn),
                                       n, C.byref(c) if cfg else None, buf if out else None, C.byref(g) if gate else None)
        score.untouched = all(buf[k].e == SENTINEL for k in range(max(n, 1)))
        return rc

    def search(R=Rd, T=Td, n_t=(1, 0, 0), step_t=(0.1, 0.1, 0.1), n_r=(0, 0, 1), step_r=(0.05, 0.05, 0.05), pivot=None, stride=4, miss=0.0, min_used=0, cfg=True, scfg=True,
               tcfg=True, out=True, rep=True, d=dst, s=src, dst_sid=-1, src_sid=-1, levels=((4, 1),), **kw):
        c, t = cfgs(levels=levels, **kw)
        sc = _lib.SearchCfg()
        for a in range(3):
            sc.n_t[a], sc.n_r[a], sc.step_t[a], sc.step_r[a] = n_t[a], n_r[a], step_t[a], step_r[a]
        if pivot is not None:
            sc.flags = 1
            sc.pivot[:] = list(pivot)
        sc.stride, sc.miss, sc.min_used = stride, miss, min_used
        Ro, To = np.zeros(9), np.zeros(3)
        r = _lib.SearchReport()
        return L.tsl_tsdf_register_search(None if d is NULL else d.h, dst_sid, None if s is NULL else s.h, src_sid, None if R is NULL else dp(R), None if T is NULL else dp(T),
                                          C.byref(c) if cfg else None, C.byref(sc) if scfg else None, C.byref(t) if tcfg else None, dp(Ro) if out else None, dp(To),
                                          C.byref(r) if rep else None, None, None)

    Rn = np.array(Rd, np.float64); Rn[1, 1] = np.nan
    for entry, call in (("register_score", score), ("register_search", search)):
        def refused(**kw):
            rc = call(**kw)
            return rc == -1 and entry.encode() in L.tsl_last_error()
        assert call() == 0, L.tsl_last_error()
        assert call(dst_sid=0, src_sid=0) == 0 and call(dst_sid=3, src_sid=3) == 0 and call(d=G, dst_sid=0) == 0 and call(d=dst, s=dst) == 0
        # a null argument
        assert refused(d=NULL) and refused(s=NULL) and refused(R=NULL) and refused(T=NULL) and refused(cfg=False) and refused(out=False)
        # a non-finite or negative parameter
        assert refused(w_min=float("nan")) and refused(band=float("inf")) and refused(r_max=float("nan")) and refused(g_max=float("inf")) and refused(huber=float("nan"))
        assert refused(w_min=-1.0) and refused(band=-0.1) and refused(r_max=-0.1) and refused(g_max=-1.0) and refused(huber=-0.02)
        # a submap id outside the handle's range; a non-zero id on a global map; different voxel sizes; the overflow bound
        assert refused(dst_sid=4) and refused(src_sid=4) and refused(dst_sid=-2) and refused(src_sid=-2) and refused(d=G, dst_sid=1) and refused(s=G, src_sid=1)
        assert refused(s=other_vs) and refused(d=other_vs)
        assert refused(g_max=1e6) and refused(r_max=1e7) and refused(band=1e7)
        for st in (0, -2, 3, 5, 6, 12, 32, 64):
            assert refused(stride=st), st
        for st in (1, 2, 4, 8, 16):
            assert call(stride=st) == 0
    # the score: n outside 1 .. 65536, a non-finite pose anywhere -- nothing is written
    entry = "register_score"
    named = lambda rc: rc == -1 and b"register_score" in L.tsl_last_error()
    assert named(score(n=0)) and named(score(n=-1)) and named(score(n=65537)) and score.untouched
    assert score(n=65536, stride=16) == 0 and not score.untouched
    assert score(gate=False) == 0
    for n in (1, 2, 300):
        Rs, Ts = np.tile(np.asarray(Rd).reshape(1, 9), (n, 1)), np.tile(np.asarray(Td).reshape(1, 3), (n, 1))
        Rbad, Tbad = Rs.copy(), Ts.copy()
        Rbad[n - 1, 4], Tbad[n - 1, 1] = np.nan, np.inf
        assert named(score(R=Rbad, n=n)) and score.untouched and named(score(T=Tbad, n=n)) and score.untouched and score(R=Rs, T=Ts, n=n) == 0
    # V = 4096 bricks * (16 / stride)^3: g_max = 100 gives M^2 2^20 V = 1.8e19 at stride 1 (refused) and 2.3e18 at stride 2
    assert named(score(g_max=100.0, stride=1)) and score(g_max=100.0, stride=2) == 0
    # the search: the guess, the lattice, the pivot, miss, min_used, the levels of the refinement
    named = lambda rc: rc == -1 and b"register_search" in L.tsl_last_error()
    assert named(search(R=Rn)) and named(search(T=[0.0, np.inf, 0.0])) and named(search(scfg=False)) and named(search(tcfg=False)) and named(search(rep=False))
    assert named(search(n_t=(-1, 0, 0))) and named(search(n_r=(0, -1, 0)))
    assert named(search(n_t=(8, 8, 8), n_r=(8, 8, 0))) and named(search(n_t=(32768, 0, 0), n_r=(0, 0, 0))) and named(search(n_t=(2 ** 30, 2 ** 30, 2 ** 30)))      # 17^5, 65537
    assert search(n_t=(7, 7, 7), n_r=(0, 0, 9), stride=16, step_t=(0.01,) * 3, step_r=(0.01,) * 3) == 0                        # 15^3 * 19 = 64125
    assert named(search(step_t=(float("nan"), 0.1, 0.1))) and named(search(step_r=(0.1, float("inf"), 0.1)))
    assert named(search(step_t=(0.0, 0.1, 0.1))) and named(search(step_r=(0.1, 0.1, -0.05))) and search(step_t=(0.1, 0.0, -1.0)) == 0      # only where n > 0
    assert named(search(pivot=(0.0, float("nan"), 0.0))) and search(pivot=(1.0, 2.0, 0.0)) == 0
    assert named(search(miss=float("nan"))) and named(search(miss=-0.1)) and named(search(min_used=-1)) and search(miss=0.1, min_used=50) == 0
    assert named(search(miss=1e7))                                                            # M >= miss: the overflow bound
    assert named(search(levels=((0, 1),))) and named(search(levels=((3, 1),))) and named(search(levels=((2, 1),) * 5)) and named(search(levels=())) and named(search(levels=((2, 65),)))
    assert named(search(min_step=float("nan"))) and named(search(damping=-1.0))
    assert named(search(g_max=100.0, stride=4, levels=((2, 1), (1, 1)))) and search(g_max=100.0, stride=4, levels=((2, 1),)) == 0      # every level is checked first
    if _lib.device_count() > 1:
        far = DenseTSDF(**dict(LIGHT, device=1))
        assert score(s=far) == -1 and b"different devices" in L.tsl_last_error()
    with pytest.raises(_lib.TslError, match="register_score"):
        dst.register_score(src, Rn, Td)
    with pytest.raises(_lib.TslError, match="register_search"):
        dst.register_search(src, Rd, Td, stride=3)
    with pytest.raises(_lib.TslError, match="register_search"):
        dst.register_search(src, Rd, Td, window_t=(100.0, 100.0, 100.0))


def test_submap_mapping_search_submaps(hip_lib):
    """The scenario of test_register_gpu.py::test_submap_mapping_register_submaps with the pose table off by guess B instead of 3 cm / 1.5 deg:
    register_submaps from that guess ends far from D, search_submaps returns D within the recorded bound -- the constraint register_submaps returns
    from a good guess -- with the restatement's search from the same guess; nothing moves."""
    from taichislam_amd.mapping import DenseTSDF, SubmapMapping
    opts = dict(LIGHT, max_submap_num=4, max_bricks=8192)
    sm = SubmapMapping(DenseTSDF, keyframe_step=6, sub_opts=opts, global_opts=opts)
    sm.set_dep_camera_intrinsic(ts.intrinsics())
    body = (np.eye(3), np.zeros(3))
    for f, (R, T, d) in enumerate(rs.dst_frames() + rs.src_frames()):
        sm.recast_depth_to_map_by_frame(f, True, body, (R, T), d, np.array([], dtype=int))
    assert sm.submaps == {0: 0, 6: 1} and sm.submap_collection.get_active_submap_id() == 1
    Rd, Td = rs.displacement()
    Ra, Ta = ts.rotation((0.2, -0.4, 1.0), 25.0), np.array([0.7, -1.3, 0.4])
    Rg, Tg = ss.guess("B")
    sm.set_frame_poses({0: (Ra, Ta), 6: (Ra @ Rg, Ra @ Tg + Ta)}, from_remote=True)
    poses = (sm.global_map.submaps_base_R_np.copy(), sm.global_map.submaps_base_T_np.copy())
    Rp, Tp, direct = sm.register_submaps(6, 0)
    dm, dd = ts.pose_error(Rp, Tp, Rd, Td)
    assert dm > 1.0 or dd > 45.0
    R, T, info = sm.search_submaps(6, 0, return_scores=True)
    assert info["submaps"] == (1, 0) and np.allclose(info["guess"][0], Rg, rtol=0, atol=1e-12) and np.allclose(info["guess"][1], Tg, rtol=0, atol=1e-12)
    em, ed = ts.pose_error(R, T, Rd, Td)
    print(f"search_submaps: best {info['search']['best']}, status {info['status']}, {info['iterations']} linearisations, final error {em:.6f} m {ed:.6f} deg")
    assert info["status"] == 0 and em <= rs.REGISTER_BOUND_M and ed <= rs.REGISTER_BOUND_DEG
    Rw, Tw, want = sr.search(rs.src_voxels(), info["guess"][0], info["guess"][1], rs.VS, rs.dst_grid(), ss.VOXEL, ss.N_T, ss.STEPS_T, ss.N_R, ss.STEPS_R, stride=ss.STRIDE, **rs.GATES)
    _same_search(info, want, "search_submaps")
    assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
    assert info["information"].shape == (6, 6) and np.array_equal(info["information"], info["records"][-1]["H_f"]) and np.linalg.eigvalsh(info["information"]).min() > 0
    assert sm.submap_collection.get_active_submap_id() == 1
    assert np.array_equal(poses[0], sm.global_map.submaps_base_R_np) and np.array_equal(poses[1], sm.global_map.submaps_base_T_np)

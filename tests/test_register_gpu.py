"""Map-to-map registration on the GPU (tsl_register.hip): the 33 integers of a linearisation and every record of a registration against the numpy
restatement (tests/register_ref.py) over the oracle's maps of the box room (tests/register_scenes.py); small sources built with import_sparse where the
kernel's queue, its tail and its multi-entry accumulation can go wrong; one handle with two submaps, a global map, frames in flight; the refusals;
SubmapMapping.register_submaps."""
import ctypes as C

import numpy as np
import pytest

import register_ref as rr
import register_scenes as rs
import render_view_ref as rv
import track_ref as tr
import track_scenes as ts
from util import SMALL, assert_export_equal, sort_export

pytestmark = pytest.mark.gpu

F32 = np.float32
OTHER_GATES = dict(w_min=2.0, band=0.05, r_max=0.06, g_max=1.2)
LIGHT = dict(SMALL, max_bricks=4096)                              # a whole 256^3 volume of bricks: what a small source or a second map needs at the most
_CHECKED = []


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _tsdf(frames=(), **kw):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**dict(LIGHT, **kw))
    g.set_dep_camera_intrinsic(ts.intrinsics())
    for R, T, d in frames:
        g.recast_depth_to_map(R, T, d, None)
    return g


def _maps():
    """(destination, source): HIP maps of frames 0..5 and of the six source frames; once per session they are compared with the oracle's maps the
    restatement reads"""
    dst, src = _tsdf(rs.dst_frames()), _tsdf(rs.src_frames())
    if not _CHECKED:
        assert_export_equal(dst.export_submap(), rs.dst_oracle().export_sparse(), "the destination against the oracle's")
        assert_export_equal(src.export_submap(), rs.src_export(), "the source against the oracle's")
        _CHECKED.append(True)
    return dst, src


def _loaded(export, sid=0, **kw):
    """a map holding a sparse export in submap `sid`"""
    g = _tsdf(**kw)
    _load(g, sid, export)
    return g


def _load(g, sid, e):
    if len(e["TSDF"]):
        g.load_numpy(sid, e["indices"], np.asarray(e["TSDF"]).view(np.float16), np.asarray(e["W_TSDF"]).view(np.float16), e["occupy"], None)


def _export(idx, t, w=None):
    idx = np.asarray(idx, np.int16).reshape(-1, 3)
    n = idx.shape[0]
    return dict(indices=idx, TSDF=np.asarray(t, np.float16).reshape(n), W_TSDF=np.ones(n, np.float16) if w is None else np.asarray(w, np.float16).reshape(n),
                occupy=np.zeros(n, np.int8))


def busy_brick():
    """base index of the source brick with the most voxels used at D"""
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


def corner_pose():
    """no rotation, a shift of (0.3, 0.4, 0.6) voxels: source voxel i lands in the destination cell with base i"""
    return np.eye(3), np.array([0.3, 0.4, 0.6]) * float(rs.VS)


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
    # the five heavy bricks lie in the slab's two brick layers (brick z index 7 and 8)
    heavy = [b for b in bricks[:3005] if b % 16 in (7, 8)][:5]
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


def _check(dst, src, e, R, T, what, dst_grid=None, **kw):
    """one linearisation against the restatement over the export `e` of the source; returns the dict"""
    gates = {k: kw.pop(k) for k in ("w_min", "band", "r_max", "g_max", "huber") if k in kw}
    stride = kw.get("stride", 1)
    want = rr.linearize(rr.source(e), R, T, stride, rs.VS, rs.dst_grid() if dst_grid is None else dst_grid, **rr.defaults(rs.VS, SMALL["internal_voxels"], SMALL["voxel_scale"], **gates))
    got = dst.register_linearize(src, R, T, **gates, **kw)
    bad = np.nonzero(got["sums"] != want)[0]
    assert bad.size == 0, f"{what}: sums {bad.tolist()} differ: {got['sums'][bad]} / {want[bad]}"
    return got


def _same_records(got, want, what):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"] == len(got["records"]), \
        f"{what}: status {got['status']} / {want['status']}, iterations {got['iterations']} / {want['iterations']}"
    for k, (a, b) in enumerate(zip(got["records"], want["records"])):
        assert np.array_equal(a["sums"], b["sums"]), f"{what}, record {k}: sums differ at {np.nonzero(a['sums'] != b['sums'])[0].tolist()}"
        for f in ("R", "T", "xi"):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), f"{what}, record {k}: {f} differs: {a[f]} / {b[f]}"


def test_linearize_equals_the_restatement(hip_lib):
    """All 33 integers at D, the three perturbed poses and a pose that carries the source outside the destination's volume; strides 1, 2, 4 and 16; huber
    off and 0.02; then other gates, counts only and the dict."""
    dst, src = _maps()
    e = rs.src_export()
    sv = rs.src_voxels()
    poses = [("true",) + rs.displacement()] + [(f"perturbed {n}", R, T) for n, (R, T) in enumerate(rs.perturbed_poses())] + [("outside",) + rs.outside_pose()]
    seen = np.zeros(5, np.int64)
    for name, R, T in poses:
        for stride in (1, 2, 4, 16):
            for huber in (0.0, 0.02):
                got = _check(dst, src, e, R, T, f"{name}, stride {stride}, huber {huber}", stride=stride, huber=huber)
                assert got["sums"][tr.I_USED:].sum() == rr.visited(sv, stride)
                seen += got["sums"][tr.I_USED:] > 0
                if name == "outside":
                    assert got["n_unknown"] + got["n_gate"] == rr.visited(sv, stride) and got["n_unknown"] > 0 and not got["sums"][:tr.I_USED].any()
    # a non-default w_min, band, r_max and g_max move voxels between the buckets as the restatement says
    for stride in (1, 2):
        got = _check(dst, src, e, *rs.perturbed_poses()[2], f"other gates, stride {stride}", stride=stride, **OTHER_GATES)
        seen += got["sums"][tr.I_USED:] > 0
    assert got["n_far"] > 0 and got["n_grad"] > 0
    assert (seen > 0).all(), f"buckets used / gate / unknown / far / grad occurred in {seen.tolist()} cases"
    # the dict: H symmetric with the upper triangle in row-major order, the float forms scaled by 2^-20, the counts by name
    Rd, Td = rs.displacement()
    got = dst.register_linearize(src, Rd, Td)
    want = rr.linearize(sv, Rd, Td, 1, rs.VS, rs.dst_grid(), **rs.GATES)
    assert np.array_equal(got["sums"], want) and got["H"].dtype == np.int64 and np.array_equal(got["H"], got["H"].T)
    assert np.array_equal(got["H"][np.triu_indices(6)], want[:21]) and np.array_equal(got["b"], want[21:27]) and got["e"] == want[27]
    assert np.array_equal(got["H_f"], got["H"] * 2.0 ** -20) and np.array_equal(got["b_f"], got["b"] * 2.0 ** -20) and got["e_f"] == got["e"] * 2.0 ** -20
    assert [got[n] for n in ("n_used", "n_gate", "n_unknown", "n_far", "n_grad")] == want[tr.I_USED:].tolist() and got["n_used"] > 15000
    # counts only (the A/B switch of tools/bench_register.py): the same buckets, no sums
    for stride in (1, 4):
        co = dst.register_linearize(src, Rd, Td, stride=stride, counts_only=True)
        want = rr.linearize(sv, Rd, Td, stride, rs.VS, rs.dst_grid(), **rs.GATES)
        assert np.array_equal(co["sums"][tr.I_USED:], want[tr.I_USED:]) and not co["sums"][:tr.I_USED].any()


def test_register_submap_equals_the_restatement(hip_lib):
    """From 3 cm / 1.5 deg, 6 cm / 3 deg and 10 cm / 5 deg with the default levels: every record (pose, sums, step), the status and the count equal the
    restatement's bit for bit; the final pose lies within register_scenes.REGISTER_BOUND_M / REGISTER_BOUND_DEG of D."""
    dst, src = _maps()
    Rd, Td = rs.displacement()
    for n, ((Rp, Tp), (Rw, Tw, want)) in enumerate(zip(rs.perturbed_poses(), rs.reference_runs())):
        R, T, info = dst.register_submap(src, Rp, Tp)
        _same_records(info, want, f"perturbation {n}")
        assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
        em, ed = ts.pose_error(R, T, Rd, Td)
        print(f"perturbation {n}: status {info['status']}, {info['iterations']} linearisations, final error {em:.6f} m {ed:.6f} deg")
        assert info["status"] == rs.MEASURED_STATUS[n] == 0 and em <= rs.REGISTER_BOUND_M and ed <= rs.REGISTER_BOUND_DEG
    # other levels, damping, a robust weight and other gates, exhausted iterations: status 1
    Rp, Tp = rs.perturbed_poses()[0]
    kw = dict(levels=((16, 1), (8, 1), (2, 2)), min_step=1e-9, damping=1e-3)
    R, T, info = dst.register_submap(src, Rp, Tp, huber=0.02, band=0.1, **kw)
    Rw, Tw, want = rr.register(rs.src_voxels(), Rp, Tp, rs.VS, rs.dst_grid(), **kw, **rr.defaults(rs.VS, SMALL["internal_voxels"], SMALL["voxel_scale"], huber=0.02, band=0.1))
    _same_records(info, want, "three levels, damped")
    assert info["status"] == 1 and info["iterations"] == 4 and np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))


def test_small_sources(hip_lib):
    """Sources built with import_sparse: one voxel; a brick with all 4096 voxels in the band (the queue's capacity, 16 entries per lane); a brick with 65
    (one full wave and one lane); an empty submap; cells across destination brick faces, edges and corners."""
    dst, _ = _maps()
    Rd, Td = rs.displacement()
    idx, t, w = rs.src_voxels()
    # one voxel: the in-band source voxel with the smallest |t| of the busiest brick
    base = busy_brick()
    inb = np.nonzero(((idx >= base) & (idx < base + 16)).all(1) & (np.abs(t) <= rs.GATES["band"]))[0]
    one = inb[np.argmin(np.abs(t[inb]))]
    e = _export(idx[one], np.float16(t[one]), np.float16(w[one]))
    got = _check(dst, _loaded(e), e, Rd, Td, "one voxel")
    assert got["sums"][tr.I_USED:].sum() == 1 and got["n_used"] == 1
    R, T, info = dst.register_submap(_loaded(e), Rd, Td, levels=((1, 3),), min_used=1)         # one row of J cannot fix six unknowns: singular, as in the restatement
    Rw, Tw, want = rr.register(rr.source(e), Rd, Td, rs.VS, rs.dst_grid(), levels=((1, 3),), min_used=1, **rs.GATES)
    _same_records(info, want, "one voxel")
    assert info["status"] == want["status"] == 3 and np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
    # whole bricks
    for n_band in (4096, 65, 64, 257):
        e = brick_export(n_band)
        s = _loaded(e)
        for stride in (1, 2):
            for name, (R, T) in (("D", (Rd, Td)), ("perturbed", rs.perturbed_poses()[1])):
                got = _check(dst, s, e, R, T, f"{n_band} of a brick in the band, stride {stride}, {name}", stride=stride, huber=0.02 if stride == 2 else 0.0)
                assert got["sums"][tr.I_USED:].sum() == 4096 // stride ** 3
                if stride == 1:
                    assert got["n_gate"] == 4096 - n_band and got["n_used"] > n_band // 4
    # an empty source submap
    empty = _tsdf()
    got = dst.register_linearize(empty, Rd, Td)
    assert not got["sums"].any()
    R, T, info = dst.register_submap(empty, Rd, Td)
    assert info["status"] == 2 and info["iterations"] == 1 and not info["records"][0]["sums"].any() and not info["records"][0]["xi"].any()
    assert np.array_equal(_bits(R), _bits(Rd)) and np.array_equal(_bits(T), _bits(Td))
    # 27 cells around a destination brick corner: 1, 2, 4 and 8 bricks per cell
    e = corner_export()
    got = _check(dst, _loaded(e), e, *corner_pose(), "brick faces, edges and corners")
    assert got["n_used"] + got["n_far"] + got["n_grad"] >= 8 and got["n_used"] >= 1          # the 8 cells c + {-1, 0}^3 lie inside the known cell block or next to it
    centre = _export(corner_cell(), np.float16(0.01))
    got = _check(dst, _loaded(centre), centre, *corner_pose(), "the corner cell")
    assert got["n_unknown"] == 0 and got["n_gate"] == 0


def test_many_bricks_per_workgroup(hip_lib):
    """A source of 3005 bricks, more than the launch has workgroups (4 per CU), interleaved in the pool with 1000 bricks of another submap of the same
    handle: every workgroup takes several bricks, so the queue's running counter, its reuse, the accumulators carried from brick to brick and the skip of
    the other submap's bricks all run.  The destination is a slab of 512 bricks, so that hundreds of source bricks hold used voxels.  All 33 integers
    against the restatement."""
    import torch
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
    assert_export_equal(src.export_submap(), se, "the imported source")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert src.bricks_in_use() >= 3005 + 900 and 3005 >= 2 * 4 * cus, (src.bricks_in_use(), cus)
    R, T = ts.rotation(rs.D_AXIS, 1.0), rs.D_T
    for stride, huber in ((1, 0.0), (1, 0.02), (2, 0.0), (16, 0.0)):
        got = _check(dst, src, se, R, T, f"3005 bricks, stride {stride}, huber {huber}", dst_grid=grid, src_sid=2, stride=stride, huber=huber)
        assert got["sums"][tr.I_USED:].sum() == rr.visited(rr.source(se), stride)
        if stride == 1:
            assert got["n_used"] > 5000 and got["n_gate"] == 2 * (4096 - 65) and got["n_unknown"] > 5000
    # the other submap alone, and the registration loop over the many bricks
    got = _check(dst, src, oe, R, T, "the other submap", dst_grid=grid, src_sid=1)
    assert got["sums"][tr.I_USED:].sum() == 1000
    Rp, Tp = ts.rotation((0.3, 1.0, -0.2), 0.5) @ R, T + np.array([0.0, 0.0, 0.02])
    Rg, Tg, info = dst.register_submap(src, Rp, Tp, src_sid=2, levels=((2, 2), (1, 2)), min_step=0.0)
    Rw, Tw, want = rr.register(rr.source(se), Rp, Tp, rs.VS, grid, levels=((2, 2), (1, 2)), min_step=0.0, **rs.GATES)
    _same_records(info, want, "3005 bricks")                  # the scattered values are no surface: the run ends lost, as the restatement's does
    assert info["iterations"] == want["iterations"] >= 3 and np.array_equal(_bits(Rg), _bits(Rw)) and np.array_equal(_bits(Tg), _bits(Tw))


def test_handles(hip_lib):
    """Two submaps of one handle without switching the active one; a global map as the destination; frames queued on both handles; no map is written."""
    from taichislam_amd.mapping import DenseTSDF
    Rd, Td = rs.displacement()
    Rp, Tp = rs.perturbed_poses()[0]
    sv = rs.src_voxels()
    want = rr.linearize(sv, Rp, Tp, 2, rs.VS, rs.dst_grid(), **rs.GATES)
    # one handle: the destination in submap 0, the source in submap 2, submap 1 active
    both = _tsdf(max_submap_num=4, max_bricks=8192)
    _load(both, 0, rs.dst_oracle().export_sparse())
    _load(both, 2, rs.src_export())
    both.active_submap_id[None] = 1
    got = both.register_linearize(both, Rp, Tp, src_sid=2, dst_sid=0, stride=2)
    assert np.array_equal(got["sums"], want) and both.get_active_submap_id() == 1
    swapped = both.register_linearize(both, Rp, Tp, src_sid=0, dst_sid=2, stride=2)          # the other direction reads the other table
    assert not np.array_equal(swapped["sums"], want) and swapped["n_used"] > 1000
    assert not both.register_linearize(both, Rp, Tp, dst_sid=0)["sums"].any()                 # src_sid None: the active submap, which is empty
    R, T, info = both.register_submap(both, Rp, Tp, src_sid=2, dst_sid=0)
    _same_records(info, rs.reference_runs()[0][2], "one handle")
    assert np.array_equal(_bits(R), _bits(rs.reference_runs()[0][0])) and both.get_active_submap_id() == 1
    # a global map as the destination
    G = DenseTSDF(**dict(LIGHT, is_global_map=True))
    _load(G, 0, rs.dst_oracle().export_sparse())
    src = _loaded(rs.src_export())
    for sid in (None, 0):
        assert np.array_equal(G.register_linearize(src, Rp, Tp, stride=2, dst_sid=sid)["sums"], want)
    # frames still queued on both handles: the call integrates them first
    dst, src = _tsdf(rs.dst_frames()[:4]), _tsdf(rs.src_frames()[:4])
    dst.sync(); src.sync()
    before = dst.register_linearize(src, Rp, Tp, stride=2)
    for (R, T, d), (R2, T2, d2) in zip(rs.dst_frames()[4:], rs.src_frames()[4:]):
        dst.recast_depth_to_map(R, T, d, None)
        src.recast_depth_to_map(R2, T2, d2, None)
    got = dst.register_linearize(src, Rp, Tp, stride=2)                                      # no sync in between
    dst.sync(); src.sync()
    again = dst.register_linearize(src, Rp, Tp, stride=2)
    assert np.array_equal(got["sums"], again["sums"]) and np.array_equal(got["sums"], want) and (before["sums"] != want).sum() > 20
    # neither map's export changes across the calls
    ed, es = sort_export(dst.export_submap()), sort_export(src.export_submap())
    dst.register_linearize(src, Rd, Td)
    dst.register_submap(src, Rp, Tp)
    assert_export_equal(dst.export_submap(), rs.dst_oracle().export_sparse(), "the destination after the calls")
    assert_export_equal(src.export_submap(), rs.src_export(), "the source after the calls")
    for a, b in ((ed, sort_export(dst.export_submap())), (es, sort_export(src.export_submap()))):
        assert all(np.array_equal(a[k], b[k]) for k in ("indices", "TSDF", "W_TSDF", "occupy"))


def test_refusals(hip_lib):
    """Every refusal of the C ABI.  The refusal of maps on different devices needs a second GPU: on a one-GPU machine that branch does not run and
    the refusal stays unverified."""
    from taichislam_amd import _lib
    from taichislam_amd.mapping import DenseTSDF
    dst, src = _loaded(rs.dst_oracle().export_sparse(), max_submap_num=4), _loaded(rs.src_export(), max_submap_num=4)
    G = DenseTSDF(**dict(LIGHT, is_global_map=True))
    other_vs = DenseTSDF(map_scale=[3.2, 3.2], voxel_scale=0.05, max_bricks=64)
    Rd, Td = rs.displacement()
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    Ro, To = np.zeros(9), np.zeros(3)
    NULL = object()
    L = dst.L

    def call(entry, R=Rd, T=Td, stride=1, w_min=0.0, band=0.0, r_max=0.0, g_max=0.0, huber=0.0, out=None, cfg=True, levels=((2, 1),), min_step=1e-4, damping=0.0,
             d=dst, s=src, dst_sid=-1, src_sid=-1, tcfg=True):
        c = _lib.RegisterCfg()
        c.stride, c.w_min, c.band, c.r_max, c.g_max, c.huber = stride, w_min, band, r_max, g_max, huber
        t = _lib.TrackCfg()
        t.n_levels = len(levels)
        for i, (st, it) in enumerate(levels[:4]):
            t.stride[i], t.iters[i] = st, it
        t.min_step, t.damping = min_step, damping
        dh, sh = (None if d is NULL else d.h), (None if s is NULL else s.h)
        cp = C.byref(c) if cfg else None
        Rp, Tp = (None if R is NULL else dp(R)), (None if T is NULL else dp(T))
        sums = _lib.AlignSums()
        if entry == "register_linearize":
            return L.tsl_tsdf_register_linearize(dh, dst_sid, sh, src_sid, Rp, Tp, cp, None if out is NULL else C.byref(sums))
        return L.tsl_tsdf_register_submap(dh, dst_sid, sh, src_sid, Rp, Tp, cp, C.byref(t) if tcfg else None, None if out is NULL else dp(Ro), dp(To), None)

    Rn = np.array(Rd, np.float64); Rn[1, 1] = np.nan
    for entry in ("register_linearize", "register_submap"):
        lin = entry == "register_linearize"

        def refused(**kw):
            rc = call(entry, **kw)
            return rc == -1 and entry.encode() in L.tsl_last_error()
        assert call(entry) == 0, L.tsl_last_error()
        assert call(entry, dst_sid=0, src_sid=0) == 0 and call(entry, dst_sid=3, src_sid=3) == 0 and call(entry, d=G, dst_sid=0) == 0 and call(entry, d=dst, s=dst) == 0
        # a null argument
        assert refused(d=NULL) and refused(s=NULL) and refused(R=NULL) and refused(T=NULL) and refused(cfg=False) and refused(out=NULL)
        # a non-finite pose or parameter
        assert refused(R=Rn) and refused(T=[0.0, np.inf, 0.0])
        assert refused(w_min=float("nan")) and refused(band=float("inf")) and refused(r_max=float("nan")) and refused(g_max=float("inf")) and refused(huber=float("nan"))
        # a negative parameter
        assert refused(w_min=-1.0) and refused(band=-0.1) and refused(r_max=-0.1) and refused(g_max=-1.0) and refused(huber=-0.02)
        # a submap id outside the handle's range; a non-zero id on a global map
        assert refused(dst_sid=4) and refused(src_sid=4) and refused(dst_sid=-2) and refused(src_sid=-2) and refused(d=G, dst_sid=1) and refused(s=G, src_sid=1)
        # different voxel sizes
        assert refused(s=other_vs) and refused(d=other_vs)
        # the overflow bound: L = 5.12 m; with g_max = 1e6 M^2 2^20 = 1.1e20 > 2^62 = 4.6e18 for any count
        assert refused(g_max=1e6) and refused(r_max=1e7) and refused(band=1e7)
        if lin:
            # a stride that is not a power of two in 1 .. 16
            for st in (0, -2, 3, 5, 6, 12, 32, 64):
                assert refused(stride=st), st
            for st in (1, 2, 4, 8, 16):
                assert call(entry, stride=st) == 0
            # V = 4096 bricks * (16 / stride)^3: g_max = 100 gives M^2 2^20 V = 1.8e19 at stride 1 (refused) and 2.3e18 at stride 2
            assert refused(g_max=100.0, stride=1) and call(entry, g_max=100.0, stride=2) == 0
        else:
            assert refused(tcfg=False)
            assert refused(levels=((0, 1),)) and refused(levels=((3, 1),)) and refused(levels=((32, 1),)) and refused(levels=((2, 1), (6, 1)))
            assert refused(levels=((2, 1),) * 5) and refused(levels=()) and refused(levels=((2, 33), (1, 32))) and refused(levels=((2, 65),))
            assert refused(min_step=float("nan")) and refused(damping=-1.0) and refused(min_step=-1.0)
            assert call(entry, levels=((16, 16), (8, 16), (4, 16), (2, 16))) == 0             # 4 levels, 64 iterations
            assert refused(g_max=100.0, levels=((2, 1), (1, 1))) and call(entry, g_max=100.0, levels=((2, 1),)) == 0      # the bound is checked for every level first
    # different devices: only where a second device exists
    if _lib.device_count() > 1:
        far = DenseTSDF(**dict(LIGHT, device=1))
        assert call("register_linearize", s=far) == -1 and b"different devices" in L.tsl_last_error()
    with pytest.raises(_lib.TslError, match="register_linearize"):
        dst.register_linearize(src, Rn, Td)
    with pytest.raises(_lib.TslError, match="register_submap"):
        dst.register_submap(src, Rd, Td, levels=((3, 1),))
    with pytest.raises(_lib.TslError, match="register_linearize"):
        dst.register_linearize(src, Rd, Td, stride=3)


def test_submap_mapping_register_submaps(hip_lib):
    """A two-submap run of the room: submap 0 holds frames 0..5, submap 1 the six source frames, whose camera poses carry the displacement D^-1 (both
    submaps are integrated at the identity).  The pose table is then given non-identity poses for both, whose relative pose is D 3 cm / 1.5 deg off;
    register_submaps(frame 6, frame 0) starts from that guess and returns D within the recorded bound, with the records of the restatement; nothing moves."""
    from taichislam_amd.mapping import DenseTSDF, SubmapMapping
    opts = dict(LIGHT, max_submap_num=4, max_bricks=8192)
    sm = SubmapMapping(DenseTSDF, keyframe_step=6, sub_opts=opts, global_opts=opts)
    sm.set_dep_camera_intrinsic(ts.intrinsics())
    body = (np.eye(3), np.zeros(3))
    for f, (R, T, d) in enumerate(rs.dst_frames() + rs.src_frames()):
        sm.recast_depth_to_map_by_frame(f, True, body, (R, T), d, np.array([], dtype=int))
    assert sm.submaps == {0: 0, 6: 1} and sm.submap_collection.get_active_submap_id() == 1
    # the pose graph anchors both submaps away from the identity: submap 0 at A, submap 1 at A o Dp, Dp the first perturbed pose.  The guess P_b^-1 P_a
    # is then Dp (up to float64 rounding), which a swapped or transposed composition would not give
    Rd, Td = rs.displacement()
    Ra, Ta = ts.rotation((0.2, -0.4, 1.0), 25.0), np.array([0.7, -1.3, 0.4])
    Rp, Tp = rs.perturbed_poses()[0]
    sm.set_frame_poses({0: (Ra, Ta), 6: (Ra @ Rp, Ra @ Tp + Ta)}, from_remote=True)
    poses = (sm.global_map.submaps_base_R_np.copy(), sm.global_map.submaps_base_T_np.copy())
    R, T, info = sm.register_submaps(6, 0)
    assert info["submaps"] == (1, 0) and np.allclose(info["guess"][0], Rp, rtol=0, atol=1e-12) and np.allclose(info["guess"][1], Tp, rtol=0, atol=1e-12)
    assert ts.pose_error(info["guess"][0], info["guess"][1], Rd, Td)[0] > 0.029
    em, ed = ts.pose_error(R, T, Rd, Td)
    print(f"register_submaps: status {info['status']}, {info['iterations']} linearisations, final error {em:.6f} m {ed:.6f} deg")
    assert info["status"] == 0 and em <= rs.REGISTER_BOUND_M and ed <= rs.REGISTER_BOUND_DEG
    Rw, Tw, want = rr.register(rs.src_voxels(), info["guess"][0], info["guess"][1], rs.VS, rs.dst_grid(), **rs.GATES)
    _same_records(info, want, "register_submaps")
    assert np.array_equal(_bits(R), _bits(Rw)) and np.array_equal(_bits(T), _bits(Tw))
    assert info["information"].shape == (6, 6) and np.array_equal(info["information"], info["records"][-1]["H_f"]) and np.linalg.eigvalsh(info["information"]).min() > 0
    assert sm.submap_collection.get_active_submap_id() == 1
    assert np.array_equal(poses[0], sm.global_map.submaps_base_R_np) and np.array_equal(poses[1], sm.global_map.submaps_base_T_np)

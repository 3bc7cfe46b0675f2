"""Submap fusion (csrc/tsl_fuse.hip) and the merge that shares its splat, at poses that are not yaw-like: rotations near a body diagonal of the voxel
lattice push corner splats out of the 15^3 LDS window of k_fuse_splat_lds into its miss branch (global atomics and a pool_claim of its own, on the merge path
the only way such a brick enters the touched-brick mask); translations put half of the source outside each wall of the global volume.

Yardsticks: map bits come from the oracle (BATCHED, or FAITHFUL for the literal fusion); the number of missed splats and the voxels they land on come from
the numpy restatement tests/fuse_window_ref.py, pinned by tests/test_fuse_window_cpu.py.  The kernel's counter "fuse_window_misses" must EQUAL the prediction:
if it is off by a few, the f32 evaluation order of the kernel and of the restatement differ -- find out which; `> 0` is not the assertion.

Scenes (tests/fuse_scenes.py): 64^3 submaps loaded with load_numpy / import_sparse on both sides, global maps of 128^3 and 128 x 128 x 48 voxels."""
import functools

import numpy as np
import pytest

import fuse_scenes as S
import fuse_window_ref as W
from util import lin, sort_export

pytestmark = pytest.mark.gpu

CASES = [(c, p, g) for c in S.CONTENTS for p in S.ALL_POSES for g in S.GLOBALS]
# the cases with a miss: every pose but the controls (submap 1 of "both" turns by another pose than submap 0: its tilt case has the misses of SHELL at diag_x_t0)
MISS_CASES = [(c, p, g) for c in ("dense", "both") for p in S.ALL_POSES if p not in ("yaw30", "outside") and (c, p) != ("dense", "tilt") for g in S.GLOBALS]


@functools.lru_cache(maxsize=None)
def _collection(content, textured=False):
    """(HIP collection, oracle collection) holding the scenes of `content`, closed as create_new_submap would: the poses of all its submaps get refreshed"""
    from oracle import OracleTSDF
    from taichislam_amd.mapping import DenseTSDF
    cfg = S.SUB_TEX if textured else S.SUB
    g, o = DenseTSDF(**cfg), OracleTSDF(**cfg)
    for sid, scene in S.CONTENTS[content]:
        idx, t, w, occ, col = scene(textured)
        g.load_numpy(sid, idx, t, w, occ, col)
        o.import_sparse(sid, idx, t, w, occ, col)
    n = len(S.CONTENTS[content])
    g.active_submap_id[None] = n
    o.set_active_submap(n)
    return g, o


def _hip_global(gmap, poses, textured=False, **kw):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**dict(S.GLOBALS[gmap], texture_enabled=textured), **kw)
    for sid, (R, T) in enumerate(poses):
        g.set_base_pose_submap(sid, R, T)
    return g


def _oracle_global(gmap, poses, textured=False):
    from oracle import OracleTSDF
    o = OracleTSDF(**dict(S.GLOBALS[gmap], texture_enabled=textured))
    for sid, (R, T) in enumerate(poses):
        o.set_base_pose_submap(sid, R, T)
    return o


@functools.lru_cache(maxsize=None)
def _want(content, pose, gmap, textured=False, literal=False):
    """the oracle's fused map, sorted; computed once per case and left unchanged"""
    from oracle import BATCHED, FAITHFUL
    og = _oracle_global(gmap, S.poses_of(content, pose), textured)
    og.fuse_submaps(_collection(content, textured)[1], mode=FAITHFUL if literal else BATCHED)
    return sort_export(og.export_sparse())


@functools.lru_cache(maxsize=None)
def _tables(content, pose, gmap):
    return [W.splat_table(scene()[0], R, T, S.VS, S.SUB_DIMS, S.GLOBAL_DIMS[gmap]) for (_, scene), (R, T) in zip(S.CONTENTS[content], S.poses_of(content, pose))]


def _predicted(content, pose, gmap):
    """(missed splats, distinct global voxels they land on) of the whole collection"""
    tabs = _tables(content, pose, gmap)
    hit = np.concatenate([t["dst"][t["miss"]] for t in tabs])
    return sum(int(t["miss"].sum()) for t in tabs), np.unique(hit, axis=0) if hit.size else np.zeros((0, 3), np.int32)


def _assert_fused(got, want, what):
    """bit for bit, with the NaN handling of tests/test_fusion_mesh_gpu.py::test_fuse_submaps_bit_exact: a voxel whose weights all quantise to 0 holds 0 / 0 on
    both sides, the NaN's payload is not compared"""
    assert got["indices"].shape == want["indices"].shape and np.array_equal(got["indices"], want["indices"]), \
        f"{what}: voxel sets differ ({got['indices'].shape[0]} vs {want['indices'].shape[0]})"
    tg, to = got["TSDF"].view(np.float16), want["TSDF"].view(np.float16)
    assert np.array_equal(np.isnan(tg), np.isnan(to)), what
    ok = ~np.isnan(tg)
    for k in ("TSDF", "W_TSDF", "occupy"):
        bad = np.nonzero((got[k] != want[k]) & (ok if k == "TSDF" else True))[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} voxels, first {got['indices'][bad[:4]]}"
    assert ("color" in got) == ("color" in want), what
    if "color" in want:
        cg, co = got["color"].view(np.float16), want["color"].view(np.float16)
        assert np.array_equal(np.isnan(cg), np.isnan(co)), f"{what}: colour NaNs"
        bad = np.nonzero(((got["color"] != want["color"]) & ~np.isnan(cg)).any(1))[0]
        assert bad.size == 0, f"{what}: colour differs at {bad.size} voxels, first {got['indices'][bad[:4]]}"


def _assert_bits(got, want, what):
    """every bit, NaN payloads included (the rule of tests/test_sequential_gpu.py and tests/test_ref_golden.py for the literal semantics)"""
    assert got["indices"].shape == want["indices"].shape and np.array_equal(got["indices"], want["indices"]), f"{what}: voxel sets differ"
    for k in ("TSDF", "W_TSDF", "occupy") + (("color",) if "color" in want else ()):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} places, first voxel {got['indices'][bad[0]]}"


def _misses(g):
    return g.get_option("fuse_window_misses")


@pytest.mark.parametrize("content,pose,gmap", CASES)
def test_lds_fusion_equals_the_oracle_and_counts_its_misses(hip_lib, content, pose, gmap):
    """the default form (k_fuse_splat_lds) against the oracle's BATCHED fusion; the miss counter rises by exactly the predicted number, on every fusion (it is
    cumulative over the life of the handle: reset clears only the first word of pool_top)"""
    sub, _ = _collection(content)
    want = _want(content, pose, gmap)
    n_pred, _ = _predicted(content, pose, gmap)
    g = _hip_global(gmap, S.poses_of(content, pose))
    assert _misses(g) == 0
    g.fuse_submaps(sub)
    got = sort_export(g.export_submap())
    print(f"{content} {pose} {gmap}: {want['indices'].shape[0]} voxels, misses {_misses(g)} (predicted {n_pred})")
    assert _misses(g) == n_pred
    _assert_fused(got, want, f"{content}, {pose}, {gmap}")
    if pose == "outside" and content != "both":                        # wholly outside: an empty map and no error
        assert got["indices"].shape[0] == 0 and g.bricks_in_use() == 0
    else:
        assert got["indices"].shape[0] > 3000
    g.fuse_submaps(sub)                                                # rebuilt from scratch (dense_tsdf.py:313): the same map, the same misses again
    assert _misses(g) == 2 * n_pred
    _assert_fused(sort_export(g.export_submap()), want, f"{content}, {pose}, {gmap}, fused again")


@pytest.mark.parametrize("content,pose,gmap", CASES)
def test_direct_fusion_gives_the_bits_of_the_default(hip_lib, content, pose, gmap):
    """fuse_direct = 1 (k_fuse_splat, one set of global atomics per corner) has no window: its counter does not move, its map is the default's, bit for bit"""
    from util import assert_export_equal
    sub, _ = _collection(content)
    poses = S.poses_of(content, pose)
    d, g = _hip_global(gmap, poses), _hip_global(gmap, poses)
    d.set_option("fuse_direct", 1)
    d.fuse_submaps(sub); g.fuse_submaps(sub)
    assert _misses(d) == 0
    ed = d.export_submap()
    assert_export_equal(ed, g.export_submap(), f"fuse_direct vs default: {content}, {pose}, {gmap}")
    _assert_fused(sort_export(ed), _want(content, pose, gmap), f"fuse_direct vs oracle: {content}, {pose}, {gmap}")


@pytest.mark.parametrize("content,pose,gmap", MISS_CASES)
def test_voxels_the_misses_land_on_carry_the_oracles_bits(hip_lib, content, pose, gmap):
    """THE MISS BRANCH (tsl_fuse.hip, the `else` of the in-window test): every global voxel that a missed splat lands on is in the map, with the oracle's bits.
    A dropped or misplaced term of that branch fails here, and the failure names it"""
    n_pred, vox = _predicted(content, pose, gmap)
    assert n_pred > 0 and vox.shape[0] > 0, f"{content}, {pose}, {gmap}: the case was chosen to have misses"
    sub, _ = _collection(content)
    want = _want(content, pose, gmap)
    g = _hip_global(gmap, S.poses_of(content, pose))
    g.fuse_submaps(sub)
    got = sort_export(g.export_submap())
    keys = lin(vox)
    kg, kw = lin(got["indices"]), lin(want["indices"])
    pw = np.searchsorted(kw, keys)
    assert (pw < kw.size).all() and np.array_equal(kw[pw], keys), "the restatement names a voxel the oracle's map does not have"
    pg = np.minimum(np.searchsorted(kg, keys), max(kg.size - 1, 0))
    absent = kg.size == 0 or kg[pg] != keys
    assert not np.any(absent), f"miss branch: {int(np.sum(absent))} of {keys.size} voxels that missed splats land on are absent, first {vox[np.nonzero(absent)[0][:4]]}"
    nan = np.isnan(want["TSDF"].view(np.float16)[pw])
    for k in ("TSDF", "W_TSDF", "occupy"):
        bad = np.nonzero((got[k][pg] != want[k][pw]) & (~nan if k == "TSDF" else True))[0]
        assert bad.size == 0, f"miss branch: {k} differs at {bad.size} of {keys.size} voxels that missed splats land on, first {vox[bad[:4]]}"
    assert np.array_equal(np.isnan(got["TSDF"].view(np.float16)[pg]), nan)


@pytest.mark.parametrize("pose,gmap", [("general", "cube"), ("general", "flat"), ("wall_z_hi", "flat"), ("wall_x_lo", "flat")])
def test_textured_fusion_equals_the_oracle(hip_lib, pose, gmap):
    """textured maps always take the direct kernel, with three more sums per corner: TSDF, weights, occupancy and colours against the oracle"""
    sub, _ = _collection("dense", True)
    want = _want("dense", pose, gmap, True)
    assert "color" in want and want["indices"].shape[0] > 5000
    g = _hip_global(gmap, S.poses_of("dense", pose), True)
    for again in range(2):
        g.fuse_submaps(sub)
        _assert_fused(sort_export(g.export_submap()), want, f"textured, {pose}, {gmap}, fusion {again}")
    assert _misses(g) == 0


@pytest.mark.parametrize("pose,gmap", [("diag_x", "cube"), ("wall_z_lo", "flat")])
def test_literal_fusion_equals_faithful(hip_lib, pose, gmap):
    """semantics = 1 on the global map (csrc/tsl_sequential.hip) against the oracle's FAITHFUL fusion of the same submap bits: every bit, NaN payloads included"""
    sub, _ = _collection("both")
    want = _want("both", pose, gmap, literal=True)
    assert want["indices"].shape[0] > 5000
    g = _hip_global(gmap, S.poses_of("both", pose))
    g.set_option("semantics", 1)
    for again in range(2):
        g.fuse_submaps(sub)
        _assert_bits(sort_export(g.export_submap()), want, f"literal fusion, {pose}, {gmap}, fusion {again}")


def _rank_collection(sid):
    """what one rank of two holds: submap `sid` of content "both", closed"""
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**S.SUB)
    idx, t, w, occ, col = S.CONTENTS["both"][sid][1]()
    g.load_numpy(sid, idx, t, w, occ, col)
    g.active_submap_id[None] = sid + 1
    return g


@pytest.mark.parametrize("pose", ["diag_x", "scaled"])
def test_merge_step_protocol_at_a_miss_pose(hip_lib, pose):
    """The merge shares the splat: one rank, two simulated ranks (reductions by hand, as test_merge_gpu.py::test_two_ranks_simulated_in_one_process) and the
    record form all equal fuse_submaps of the whole collection, which equals the oracle.  A brick enters the exchange only through the touched-brick mask, and
    the mask only through pool_claim: at diag_x one brick of the union is claimed only by the flush of blocks that also have misses, at the scaled pose one
    brick is claimed by the miss branch ALONE (tests/test_fuse_window_cpu.py pins both) -- those bricks must be in the mask."""
    import torch
    gmap, dims = "cube", S.GLOBAL_DIMS["cube"]
    poses = S.poses_of("both", pose)
    sub, _ = _collection("both")
    want = _want("both", pose, gmap)
    whole = _hip_global(gmap, poses)
    whole.fuse_submaps(sub)
    ref = sort_export(whole.export_submap())
    _assert_fused(ref, want, f"fuse_submaps, {pose}")
    via_blocks, alone = W.bricks_reached_only_with_misses(_tables("both", pose, gmap), dims)
    assert len(via_blocks) >= 1 and (pose != "scaled" or len(alone) >= 1)
    occupied = np.unique(W.brick_ids(want["indices"], dims))

    def covers(mask, what):
        m = mask.cpu().numpy()
        assert m[occupied].all(), f"{what}: the mask lacks {int((m[occupied] == 0).sum())} of the {occupied.size} bricks the fused map occupies"
        assert m[via_blocks].all() and m[alone].all(), f"{what}: a brick that only the miss branch (or the flush of a block with misses) claims is not in the mask"

    # one rank
    g1 = _hip_global(gmap, poses)
    mask = g1.merge_begin(sub)
    covers(mask, "one rank")
    acc, cnt = g1.merge_pack(mask)
    assert acc.shape[0] == int(mask.sum())
    g1.merge_finish(acc, cnt)
    _assert_fused(sort_export(g1.export_submap()), ref, f"one rank, {pose}")
    # the record form on the same sums
    g2 = _hip_global(gmap, poses)
    m2 = g2.merge_begin(sub)
    assert torch.equal(m2, mask)
    a2, c2 = g2.merge_pack(m2)
    g2.merge_finish_records(g2.merge_finalize_slice(a2, c2))
    _assert_fused(sort_export(g2.export_submap()), ref, f"one rank, records, {pose}")
    # two simulated ranks: submap 0 on one, submap 1 on the other
    subs = [_rank_collection(0), _rank_collection(1)]
    gs = [_hip_global(gmap, poses) for _ in range(2)]
    masks = [g.merge_begin(s) for g, s in zip(gs, subs)]
    union = torch.maximum(masks[0], masks[1])
    covers(union, "two ranks")
    assert torch.equal(union, mask)
    packs = [g.merge_pack(union) for g in gs]
    acc, cnt = packs[0][0] + packs[1][0], packs[0][1] + packs[1][1]
    torch.cuda.synchronize()
    n = acc.shape[0]; nper = (n + 1) // 2
    pa = torch.cat([acc, torch.zeros((2 * nper - n, 4096, 2), dtype=acc.dtype, device=acc.device)])
    pc = torch.cat([cnt, torch.zeros((2 * nper - n, 4096), dtype=cnt.dtype, device=cnt.device)])
    recs = torch.cat([gs[r].merge_finalize_slice(pa[r * nper:(r + 1) * nper].contiguous(), pc[r * nper:(r + 1) * nper].contiguous()) for r in range(2)])
    gs[1].merge_finish_records(recs)
    _assert_fused(sort_export(gs[1].export_submap()), ref, f"two simulated ranks, records, {pose}")
    gs[0].merge_finish(acc, cnt)
    _assert_fused(sort_export(gs[0].export_submap()), ref, f"two simulated ranks, {pose}")
    n_pred, _ = _predicted("both", pose, gmap)
    assert _misses(g1) == _misses(g2) == n_pred and _misses(gs[0]) + _misses(gs[1]) == n_pred


@pytest.mark.parametrize("pose,direct", [("general", 0), ("scaled", 0), ("general", 1)])
def test_pool_exhaustion_during_a_fusion(hip_lib, pose, direct):
    """A global brick pool that fills up DURING a fusion (gp < 0 in the flush, in the miss branch -- the scaled pose sends 14 163 splats through it -- and in the
    direct kernel), as tests/test_tsdf_parity_gpu.py::test_capacity_errors_are_reported_and_do_not_stick has it for integration: reported once, the handle
    keeps working.  A surviving brick has ALL of its terms: pool_claim hands out a brick at the first claim or, once the counter has reached the capacity,
    never again within the fusion (claim_index_1 puts the entry back to EMPTY and the counter only grows until the next reset), so no brick is claimed part
    way through its terms -- every exported voxel carries the oracle's bits, and a brick present holds every voxel the oracle has in it.  Afterwards a
    fusion of a one-brick source on the same handle equals the oracle: no accumulator was left dirty."""
    from oracle import BATCHED, OracleTSDF
    from taichislam_amd import _lib
    from taichislam_amd.mapping import DenseTSDF
    gmap, dims = "cube", S.GLOBAL_DIMS["cube"]
    poses = S.poses_of("dense", pose)
    sub, _ = _collection("dense")
    want = _want("dense", pose, gmap)
    roomy = _hip_global(gmap, poses)
    roomy.fuse_submaps(sub)
    need = roomy.bricks_in_use()
    assert need == np.unique(W.brick_ids(want["indices"], dims)).size and need > 8
    cap = need - 3
    g = _hip_global(gmap, poses, max_bricks=cap)
    g.set_option("fuse_direct", direct)
    with pytest.raises(_lib.TslError, match="brick pool"):
        g.fuse_submaps(sub)
    g.sync()                                                             # reported once
    assert g.bricks_in_use() == cap
    got = sort_export(g.export_submap())
    kg, kw = lin(got["indices"]), lin(want["indices"])
    assert 0 < kg.size < kw.size
    pw = np.searchsorted(kw, kg)
    assert (pw < kw.size).all() and np.array_equal(kw[np.minimum(pw, kw.size - 1)], kg), "a voxel the oracle's map does not have"
    nan = np.isnan(want["TSDF"].view(np.float16)[pw])
    for k in ("TSDF", "W_TSDF", "occupy"):
        bad = np.nonzero((got[k] != want[k][pw]) & (~nan if k == "TSDF" else True))[0]
        assert bad.size == 0, f"{k} of a surviving brick differs at {bad.size} voxels (a brick with some of its terms?), first {got['indices'][bad[:4]]}"
    bg, ng = np.unique(W.brick_ids(got["indices"], dims), return_counts=True)
    bw, nw = np.unique(W.brick_ids(want["indices"], dims), return_counts=True)
    assert bg.size == cap and np.array_equal(ng, nw[np.searchsorted(bw, bg)]), "a surviving brick lacks voxels"
    # the same handle, a source that fits
    one = DenseTSDF(**S.SUB)
    oone = OracleTSDF(**S.SUB)
    idx, t, w, occ, _ = S.one_brick()
    one.load_numpy(0, idx, t, w, occ, None); oone.import_sparse(0, idx, t, w, occ)
    one.active_submap_id[None] = 1; oone.set_active_submap(1)
    og = _oracle_global(gmap, poses)
    og.fuse_submaps(oone, mode=BATCHED)
    g.fuse_submaps(one)
    want_one = sort_export(og.export_sparse())
    assert g.bricks_in_use() == np.unique(W.brick_ids(want_one["indices"], dims)).size < cap      # (a turned brick reaches into up to 27 global bricks)
    _assert_fused(sort_export(g.export_submap()), want_one, f"one brick after the exhausted fusion, {pose}")

"""GPU tests of the multi-GPU global-map merge (csrc/tsl_merge.hip, taichislam_amd.distributed) on real DenseTSDF handles.

Reference role: taichi_slam/mapping/submap_mapping.py:157-160,226-253 + dense_tsdf.py:272-318 (every agent fuses every agent's
submaps).  Claim under test: the merged map is bit-identical to ONE process fusing all submaps -- for one rank, for two ranks
simulated inside one process, for the library's own RCCL communicator, and for two real processes sharing this GPU over gloo
(RCCL refuses two ranks on one device; the driver's 8-GPU run exercises the nccl path through bench.py --gpus N)."""
import os
import socket
import sys

import numpy as np
import pytest

from taichislam_amd.utils import synthetic as syn
from util import SMALL, sort_export

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(SMALL, map_scale=[5.12, 5.12], max_submap_num=8)
H, W, FRAMES_PER_RANK = 120, 160, 2


def _rank_stream(rank):
    from taichislam_amd import distributed as D
    K = syn.scaled_intrinsics(H, W)
    out = []
    for f in range(FRAMES_PER_RANK):
        R, T = syn.camera_pose(f, start_deg=D.stream_start_deg(rank) * 0.5)      # 22.5 degrees apart: heavily overlapping submaps
        out.append((R, T, syn.sphere_room_depth(R, T, H, W, K=K)))
    return K, out


def _rank_submaps(rank, device=0):
    """Rank r integrates its stream into submap id r of its own collection (base pose = its first camera pose)."""
    from taichislam_amd.mapping import DenseTSDF
    K, fr = _rank_stream(rank)
    sub = DenseTSDF(**CFG, device=device)
    sub.set_dep_camera_intrinsic(K)
    sub.active_submap_id[None] = rank
    sub.set_base_pose_submap(rank, fr[0][0], fr[0][1])
    for R, T, d in fr:
        sub.recast_depth_to_map(R, T, d, None)
    sub.active_submap_id[None] = rank + 1                 # closed, as create_new_submap would
    return sub


def _global(world, device=0):
    from taichislam_amd.mapping import DenseTSDF
    g = DenseTSDF(**dict(CFG, is_global_map=True), device=device)
    for r in range(world):
        _, fr = _rank_stream(r)
        g.set_base_pose_submap(r, fr[0][0], fr[0][1])
    return g


def _single_process_reference(world):
    """One collection holding every rank's submap, fused directly (dense_tsdf.py:312-318)."""
    from taichislam_amd.mapping import DenseTSDF
    both = DenseTSDF(**CFG)
    for r in range(world):
        K, fr = _rank_stream(r)
        both.set_dep_camera_intrinsic(K)
        both.active_submap_id[None] = r
        both.set_base_pose_submap(r, fr[0][0], fr[0][1])
        for R, T, d in fr:
            both.recast_depth_to_map(R, T, d, None)
    both.active_submap_id[None] = world
    g = _global(world)
    g.fuse_submaps(both)
    # true for these yaw-like poses, not for every pose: tests/test_fuse_poses_gpu.py has the rotations at which corner splats leave the window
    assert g.get_option("fuse_window_misses") == 0
    return sort_export(g.export_submap())


def _assert_same(a, b, what):
    assert a["indices"].shape == b["indices"].shape and np.array_equal(a["indices"], b["indices"]), f"{what}: voxel sets differ"
    ok = ~np.isnan(a["TSDF"].view(np.float16))
    assert np.array_equal(a["TSDF"][ok], b["TSDF"][ok]) and np.array_equal(a["W_TSDF"], b["W_TSDF"]) and np.array_equal(a["occupy"], b["occupy"]), what


def test_one_rank_merge_equals_fuse_submaps(hip_lib):
    from taichislam_amd import distributed as D
    ref = _single_process_reference(1)
    assert ref["indices"].shape[0] > 50000
    sub = _rank_submaps(0)
    g = _global(1)
    assert g.allreduce_merge(sub, None) == 0                       # native one-call form, no communicator: nothing travels
    _assert_same(sort_export(g.export_submap()), ref, "native, one rank")
    g2 = _global(1)
    assert D.allreduce_merge(g2, sub) == 0                          # step protocol, no process group
    _assert_same(sort_export(g2.export_submap()), ref, "steps, one rank")
    g2.allreduce_merge(sub, None)                                   # merging again rebuilds the same map (accumulators were left at zero)
    _assert_same(sort_export(g2.export_submap()), ref, "second merge")
    # the reduce-scatter + all-gather form of the exchange: one rank finalises every union brick into records and writes the map from them
    g3 = _global(1)
    g3.set_option("merge_exchange", 1)
    assert g3.allreduce_merge(sub, None) == 0
    _assert_same(sort_export(g3.export_submap()), ref, "native, one rank, records")
    g4 = _global(1)
    assert D.allreduce_merge(g4, sub, exchange="scatter_gather") == 0
    _assert_same(sort_export(g4.export_submap()), ref, "steps, one rank, records")


def test_two_ranks_simulated_in_one_process(hip_lib):
    """The step protocol with the two reductions done by hand (torch.maximum / add): exactly what the all-reduces compute."""
    import torch
    ref = _single_process_reference(2)
    subs = [_rank_submaps(r) for r in range(2)]
    gs = [_global(2) for _ in range(2)]
    masks = [g.merge_begin(s) for g, s in zip(gs, subs)]
    assert not torch.equal(masks[0], masks[1])                      # the ranks touch different brick sets
    m = torch.maximum(masks[0], masks[1])
    packs = [g.merge_pack(m) for g in gs]
    assert packs[0][0].shape == packs[1][0].shape and packs[0][0].shape[0] == int(m.sum())
    acc, cnt = packs[0][0] + packs[1][0], packs[0][1] + packs[1][1]
    torch.cuda.synchronize()
    # second form: rank r gets the reduced sums of ITS half of the (padded) union, finalises it, the records are gathered
    n = acc.shape[0]; nper = (n + 1) // 2
    pa = torch.cat([acc, torch.zeros((2 * nper - n, 4096, 2), dtype=acc.dtype, device=acc.device)])
    pc = torch.cat([cnt, torch.zeros((2 * nper - n, 4096), dtype=cnt.dtype, device=cnt.device)])
    recs = torch.cat([gs[r].merge_finalize_slice(pa[r * nper:(r + 1) * nper].contiguous(), pc[r * nper:(r + 1) * nper].contiguous()) for r in range(2)])
    assert recs.shape == (2 * nper, 4096 * 4 + 4096 + 512)
    gs[1].merge_finish_records(recs)
    _assert_same(sort_export(gs[1].export_submap()), ref, "two simulated ranks, reduce-scatter + all-gather")
    gs[0].merge_finish(acc, cnt)
    _assert_same(sort_export(gs[0].export_submap()), ref, "two simulated ranks")


def test_three_simulated_ranks_with_a_padded_last_slice(hip_lib):
    """The reduce-scatter form cuts the union into nranks slices of WHOLE bricks: with three ranks the union (not a multiple of three here, or made so by dropping
    nothing: the pad is asserted) ends in zero bricks that every rank finalises into empty records and nobody writes.  Also: records finalised by DIFFERENT handles
    are interchangeable (finalising is a pure function of the sums)."""
    import torch
    world = 3
    ref = _single_process_reference(world)
    subs = [_rank_submaps(r) for r in range(world)]
    gs = [_global(world) for _ in range(world)]
    masks = [g.merge_begin(s) for g, s in zip(gs, subs)]
    m = masks[0]
    for x in masks[1:]:
        m = torch.maximum(m, x)
    packs = [g.merge_pack(m) for g in gs]
    acc, cnt = sum(p[0] for p in packs), sum(p[1] for p in packs)
    n = acc.shape[0]
    if n % world == 0:                                             # force a pad: pretend the communicator had one rank more than divides the union
        world_x = next(w for w in (4, 5, 7) if n % w)
    else:
        world_x = world
    nper = (n + world_x - 1) // world_x
    assert nper * world_x > n
    pa = torch.cat([acc, torch.zeros((nper * world_x - n, 4096, 2), dtype=acc.dtype, device=acc.device)])
    pc = torch.cat([cnt, torch.zeros((nper * world_x - n, 4096), dtype=cnt.dtype, device=cnt.device)])
    recs = torch.cat([gs[r % world].merge_finalize_slice(pa[r * nper:(r + 1) * nper].contiguous(), pc[r * nper:(r + 1) * nper].contiguous()) for r in range(world_x)])
    assert recs.shape[0] == nper * world_x and not recs[n:].any()          # the pad's records are empty
    for g in gs:
        g.merge_finish_records(recs)
        _assert_same(sort_export(g.export_submap()), ref, "three simulated ranks, padded reduce-scatter + all-gather")


def test_native_rccl_communicator_world_1(hip_lib):
    """tsl_comm_* + tsl_tsdf_allreduce_merge on a one-rank RCCL communicator created by the library itself."""
    from taichislam_amd import distributed as D
    ref = _single_process_reference(1)
    comm = D.Communicator(D.Communicator.unique_id(), 1, 0, device=0)
    sub, g = _rank_submaps(0), _global(1)
    nbytes = D.allreduce_merge(g, sub, comm=comm)
    assert nbytes > 32 * 32 * 32 // 64 and nbytes % 20 in (0, ((g.N // 16) ** 2 * (g.Nz // 16) + 1) % 20)      # brick mask + status byte, 20 bytes per union voxel
    _assert_same(sort_export(g.export_submap()), ref, "RCCL world 1")
    g2 = _global(1)
    D.allreduce_merge(g2, sub, comm=comm, exchange="scatter_gather")      # ncclReduceScatter / ncclAllGather on the one-rank communicator
    _assert_same(sort_export(g2.export_submap()), ref, "RCCL world 1, reduce-scatter + all-gather")
    comm.close()


def _worker(rank, world, port, out, exchange="allreduce"):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from taichislam_amd import distributed as D
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    sub, g = _rank_submaps(rank), _global(world)
    nbytes = D.allreduce_merge(g, sub, exchange=exchange)           # CUDA tensors through gloo: real HIP handles, real 2-rank reductions
    e = sort_export(g.export_submap())
    np.savez(os.path.join(out, f"rank{rank}.npz"), indices=e["indices"], TSDF=e["TSDF"], W_TSDF=e["W_TSDF"], occupy=e["occupy"], nbytes=nbytes)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["allreduce", "scatter_gather"])
def test_two_processes_on_one_gpu_over_gloo(hip_lib, tmp_path, exchange):
    import torch.multiprocessing as mp
    ref = _single_process_reference(2)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path), exchange), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    _assert_same(dict(r0), ref, "rank 0 vs single process")
    _assert_same(dict(r1), ref, "rank 1 vs single process")
    nvox_dense = (512 // 4) ** 3 * 20
    assert int(r0["nbytes"]) == int(r1["nbytes"]) and 0 < int(r0["nbytes"]) < nvox_dense // 2


def test_config5_eight_submaps_at_512_cubed_against_the_oracle(hip_lib):
    """BASELINE configs[4] at its full geometry, asserted: eight ranks, each with ONE submap of the 640 x 480 stream that
    starts 45 degrees after the previous rank's (taichislam_amd.distributed.stream_start_deg), merged into a 512^3 / 2 cm global map through the
    step protocol -- merge_begin -> MAX of the masks -> merge_pack -> SUM -> merge_finish -- with the eight ranks simulated in this process
    (the reductions done with torch: exactly what the all-reduces compute).  The yardstick is NOT the HIP fusion: the ORACLE integrates the same
    eight streams (BATCHED, the order-free semantics the merge is defined on) and fuses the eight submaps (dense_tsdf.py:272-318 over every
    agent's submaps); the merged map must equal it bit for bit on every rank.  The bytes a rank puts on the links are asserted as well."""
    import torch
    from oracle import BATCHED, OracleTSDF
    from taichislam_amd import distributed as D
    from taichislam_amd.mapping import DenseTSDF
    from util import C2
    world, frames_per_rank = 8, 2
    cfg = dict(C2, max_submap_num=16)                      # ids 0..7 hold the submaps, a rank closes its submap by moving on to id r + 1

    def stream(r):
        return list(syn.sphere_room_stream(frames_per_rank, start_deg=D.stream_start_deg(r)))

    # the oracle: one collection with the eight submaps, fused into one global map
    osub = OracleTSDF(**cfg); osub.set_intrinsics(syn.K_DEPTH)
    oglob = OracleTSDF(**dict(cfg, is_global_map=True))
    for r in range(world):
        fr = stream(r)
        osub.set_active_submap(r); osub.set_base_pose_submap(r, fr[0][0], fr[0][1]); oglob.set_base_pose_submap(r, fr[0][0], fr[0][1])
        for R, T, d in fr:
            osub.integrate_depth(R, T, d, mode=BATCHED)
    osub.set_active_submap(world)
    oglob.fuse_submaps(osub, mode=BATCHED)
    want = sort_export(oglob.export_sparse())
    assert want["indices"].shape[0] > 5_000_000

    subs, globs, masks = [], [], []
    for r in range(world):
        fr = stream(r)
        s = DenseTSDF(**cfg, max_bricks=4096); s.set_dep_camera_intrinsic(syn.K_DEPTH)
        s.active_submap_id[None] = r
        s.set_base_pose_submap(r, fr[0][0], fr[0][1])
        for R, T, d in fr:
            s.recast_depth_to_map(R, T, torch.from_numpy(d.view(np.int16)).cuda(), None)
        s.active_submap_id[None] = r + 1
        g = DenseTSDF(**dict(cfg, is_global_map=True))
        for q in range(world):
            g.set_base_pose_submap(q, *stream(q)[0][:2])
        subs.append(s); globs.append(g)
        masks.append(g.merge_begin(s))
    union = masks[0]
    for m in masks[1:]:
        union = torch.maximum(union, m)
    n_union = int(union.sum())
    acc = cnt = None
    for g in globs:                                        # SUM: one rank's packed planes at a time (8 x 220 MB would fit, this is the ring's order anyway)
        a, c = g.merge_pack(union)
        assert a.shape[0] == n_union
        acc, cnt = (a, c) if acc is None else (acc + a, cnt + c)
        del a, c
    torch.cuda.synchronize()
    nbytes = union.numel() + 1 + n_union * 4096 * 20       # what tsl_tsdf_allreduce_merge / distributed.allreduce_merge put through the all-reduces per rank
    print(f"config 5: union {n_union} bricks, {nbytes / 1e6:.0f} MB all-reduced per rank, {want['indices'].shape[0]} global voxels")
    assert 150e6 < nbytes < 350e6, nbytes                  # ~2 700 bricks x 4096 voxels x 20 B = ~220 MB
    # the second form of the exchange: reduce-scatter of the same planes, rank r finalises its eighth of the union bricks, all-gather of
    # the records -- emulated like the sums above -- and what a rank then puts on its links
    nper = (n_union + world - 1) // world
    pa = torch.cat([acc, torch.zeros((nper * world - n_union, 4096, 2), dtype=acc.dtype, device=acc.device)])
    pc = torch.cat([cnt, torch.zeros((nper * world - n_union, 4096), dtype=cnt.dtype, device=cnt.device)])
    recs = torch.cat([globs[r].merge_finalize_slice(pa[r * nper:(r + 1) * nper].contiguous(), pc[r * nper:(r + 1) * nper].contiguous()) for r in range(world)])
    del pa, pc
    ring_allreduce = 2 * (world - 1) / world * n_union * 4096 * 20
    ring_scatter_gather = (world - 1) / world * (nper * world * 4096 * 20 + recs.numel())
    print(f"config 5: a rank sends {ring_allreduce / 1e6:.0f} MB round a ring with the all-reduce, {ring_scatter_gather / 1e6:.0f} MB with reduce-scatter + all-gather")
    assert ring_scatter_gather < 0.65 * ring_allreduce and ring_scatter_gather / 2 < 140e6      # (VERDICT r5's mark, in its units: half the ring traffic <= 140 MB)
    for r in (2, 7):
        globs[r].merge_finish_records(recs)
        got = sort_export(globs[r].export_submap())
        assert got["indices"].shape == want["indices"].shape and np.array_equal(got["indices"], want["indices"]), f"rank {r} (records): voxel sets differ"
        ok = ~np.isnan(want["TSDF"].view(np.float16))
        assert np.array_equal(got["TSDF"][ok], want["TSDF"][ok]) and np.array_equal(got["W_TSDF"], want["W_TSDF"]) and np.array_equal(got["occupy"], want["occupy"]), f"rank {r} (records)"
    del recs
    # (true for yaw-like poses only; tests/test_fuse_poses_gpu.py fuses at the rotations where the counter is not 0)
    assert all(g.get_option("fuse_window_misses") == 0 for g in globs)      # eight poses 45 degrees apart: every corner splat landed inside its block's 15^3 LDS window
    for r in (0, 5):                                       # every rank ends with the same map (tested for all ranks at small size above): two of them here
        globs[r].merge_finish(acc, cnt)
        got = sort_export(globs[r].export_submap())
        assert got["indices"].shape == want["indices"].shape and np.array_equal(got["indices"], want["indices"]), f"rank {r}: voxel sets differ"
        ok = ~np.isnan(want["TSDF"].view(np.float16))
        assert np.array_equal(np.isnan(got["TSDF"].view(np.float16)), ~ok)
        assert np.array_equal(got["TSDF"][ok], want["TSDF"][ok]) and np.array_equal(got["W_TSDF"], want["W_TSDF"]) and np.array_equal(got["occupy"], want["occupy"]), f"rank {r}"

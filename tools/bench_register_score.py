"""Time of scoring many poses in one call (tsl_register_search.hip, tsl_tsdf_register_score) against the only way to score poses without it: one
tsl_tsdf_register_linearize(counts only) per pose -- one launch, one copy and one stream synchronisation each.  Two scenes: the box room of
tests/register_scenes.py (256^3 / 4 cm, frames 0..5 against the displaced frames 3..8) and the config-4 scene of taichislam_amd/utils/bench_configs.py
(512^3 / 2 cm, the sphere-room stream: frames 0..9 in submap 0 against frames 10..19 in submap 1 of one handle).  K = 256 and 5265 poses from the
default lattice of DenseTSDF.register_search around the true pose (a seeded shuffle of its 9 x 9 x 5 x 13 candidates), strides 4 and 1.

Per case: the kernel time of the one k_register_score launch (HIP events around it: tsl_tsdf_prof_query, TSL_K_REGISTER_SCORE), the wall time of the
whole call (two gather passes, upload, launch, copy back, synchronise) -- medians of REPEATS after WARMUP -- and the wall time of the K-call loop,
measured in the same process on the same device, median of LOOP_REPEATS.  The counts of both ways are compared before anything is timed.  Lastly one
whole default register_search on the room from guess B (0.7, -0.6, 0.3) m / 55 deg.  Writes the table to --out (default
profiles/register_score.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from taichislam_amd import _lib
from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, LOOP_REPEATS = 2, 7, 3
WINDOW_T, STEP_T, YAW, STEP_YAW = (0.8, 0.8, 0.4), 0.2, np.pi / 3, np.pi / 18


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def lattice_poses(R0, T0, pivot, k):
    """k poses of the 5265-candidate lattice around (R0, T0) in a seeded shuffle: a yaw about `pivot`, then a shift"""
    ax = [np.arange(-round(w / STEP_T), round(w / STEP_T) + 1) * STEP_T for w in WINDOW_T]
    yaw = np.arange(-round(YAW / STEP_YAW), round(YAW / STEP_YAW) + 1) * STEP_YAW
    grid = np.stack(np.meshgrid(yaw, ax[0], ax[1], ax[2], indexing="ij"), -1).reshape(-1, 4)
    assert grid.shape[0] == 5265
    pick = np.random.default_rng(7).permutation(grid.shape[0])[:k]
    R = np.stack([rot_z(g[0]) @ R0 for g in grid[pick]])
    T = np.stack([rot_z(g[0]) @ (T0 - pivot) + pivot + g[1:] for g in grid[pick]])
    return R, T


def median_ms(fn, warmup, repeats, sync):
    ms = []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def kernel_ms(m, fn):
    ms = []
    for i in range(WARMUP + REPEATS):
        m.kernel_time(_lib.K_REGISTER_SCORE)
        fn()
        t, n = m.kernel_time(_lib.K_REGISTER_SCORE)
        assert n == 1, n
        if i >= WARMUP:
            ms.append(t)
    return statistics.median(ms), min(ms)


def case(lines, name, dst, src, R0, T0, kw):
    g = dst.register_score(src, R0[None], T0[None], stride=1, **kw)["gate"]
    pivot = R0 @ (np.array([g["sum_i"], g["sum_j"], g["sum_k"]], np.float64) / max(g["n_pass"], 1) * dst.voxel_scale) + T0
    for stride in (4, 1):
        for k in (256, 5265):
            R, T = lattice_poses(R0, T0, pivot, k)
            one = dst.register_score(src, R, T, stride=stride, counts_only=True, **kw)
            loop = [dst.register_linearize(src, R[i], T[i], stride=stride, counts_only=True, **kw) for i in range(k)]
            for f in ("n_used", "n_unknown", "n_far", "n_grad"):
                assert np.array_equal(one[f], np.array([s[f] for s in loop], np.int64)), (name, stride, k, f)
            dst.enable_profiling(True, only=[_lib.K_REGISTER_SCORE])
            kern, kern_min = kernel_ms(dst, lambda: dst.register_score(src, R, T, stride=stride, **kw))
            dst.enable_profiling(False)
            wall, wall_min = median_ms(lambda: dst.register_score(src, R, T, stride=stride, **kw), WARMUP, REPEATS, dst.sync)

            def loop_fn():
                for i in range(k):
                    dst.register_linearize(src, R[i], T[i], stride=stride, counts_only=True, **kw)
            lp, lp_min = median_ms(loop_fn, 1, LOOP_REPEATS, dst.sync)
            lines.append(f"{name:<8} stride {stride}  K {k:>5}  list {one['gate']['n_pass']:>7}  tile {dst.register_score_tile(one['gate']['n_pass'], k):>3}  score kernel {kern:9.3f} ms (min {kern_min:9.3f})  "
                         f"score call {wall:9.3f} ms (min {wall_min:9.3f})  loop of K linearize(counts only) {lp:10.3f} ms (min {lp_min:10.3f})  loop / call {lp / wall:7.1f}x")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_score.txt"))
    args = ap.parse_args()
    import register_scenes as rs
    import track_scenes as ts
    from util import SMALL
    lines = [f"tools/bench_register_score.py: medians of {REPEATS} after {WARMUP} warm-up calls (loop: median of {LOOP_REPEATS} after 1); one MI355X, one process",
             "score kernel = the k_register_score launch alone (HIP events); score call = tsl_tsdf_register_score in wall time; loop = K x tsl_tsdf_register_linearize(counts only) in wall time",
             "lane mapping: lanes = poses (one wave per tile x 64 poses); the other mapping (lanes = entries, a wave reduction per pose) was not built"]
    # the box room
    opts = dict(SMALL, max_bricks=4096)
    dst, src = DenseTSDF(**opts), DenseTSDF(**opts)
    for m, frames in ((dst, rs.dst_frames()), (src, rs.src_frames())):
        m.set_dep_camera_intrinsic(ts.intrinsics())
        for R, T, d in frames:
            m.recast_depth_to_map(R, T, d, None)
        m.sync()
    Rd, Td = rs.displacement()
    case(lines, "room", dst, src, Rd, Td, {})
    # one whole search from guess B
    g = dst.register_score(src, Rd[None], Td[None])["gate"]
    c = Rd @ (np.array([g["sum_i"], g["sum_j"], g["sum_k"]], np.float64) / g["n_pass"] * dst.voxel_scale) + Td
    Cg = ts.rotation((0.0, 0.0, 1.0), 55.0)
    R0, T0 = Cg @ Rd, Cg @ (Td - c) + c + np.array([0.7, -0.6, 0.3])
    info = {}

    def run():
        info["r"] = dst.register_search(src, R0, T0)
    wall, wall_min = median_ms(run, WARMUP, REPEATS, dst.sync)
    Rf, Tf, inf = info["r"]
    em, ed = ts.pose_error(Rf, Tf, Rd, Td)
    lines.append(f"room     register_search from guess B (5265 candidates at stride 4, then {inf['iterations']} linearisations): {wall:.3f} ms (min {wall_min:.3f}), "
                 f"status {inf['status']}, best {inf['search']['best']}, final error {em:.6f} m {ed:.6f} deg")
    print(lines[-1], flush=True)
    del dst, src
    # the config-4 scene: two submaps of one handle, the true relative pose is the identity
    m = DenseTSDF(**C2, max_submap_num=2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for f, (R, T, d) in enumerate(syn.sphere_room_stream(20)):
        if f == 10:
            m.switch_to_next_submap()
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "config-4", m, m, np.eye(3), np.zeros(3), dict(src_sid=1, dst_sid=0))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

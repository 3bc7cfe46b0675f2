"""Time of the cost-to-go field (tsl_nav_field.hip, DenseTSDF.nav_field / nav_paths) on the two maps of tools/bench_nav_grid.py: the room of the tests
(tests/render_view_scenes.py: four 320 x 240 frames, 256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames
(512^3 / 2 cm).

Per map, medians of REPEATS after WARMUP.  Case 1: one goal on the cost plane of nav_grid for one band of 32 layers at R = 25 -- the device call (cost
tensor in, tensors out, the host checking the counter every check_every rounds), the host call (numpy in and out), the device call with rounds_fixed (no
host read), its kernels through the handle's profiler (seed, all rounds, parents), rounds and tile visits -- against what a caller does today: the cost
plane copied to the host plus scipy.sparse.csgraph.dijkstra over a graph built with numpy where scipy imports, else the heap Dijkstra of
tests/nav_field_ref.py (the table says which).  Case 2: the same with 8 planes (8 bands of 32 layers, a goal in each).  Case 3: a 512 x 512 serpentine of
pitch 16, the bad case of the tile scheme.  On the room: check_every = 1, 8 and 32.  And 256 paths of nav_paths.  The field of the GPU is compared with
the baseline's before anything is timed.  No threshold is set.  Writes the table to --out (default profiles/nav_field.txt) and prints it.  One process;
run it under `timeout`."""
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
from taichislam_amd.utils import inflation_lut
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3
STAGES = (("seed", _lib.K_NAV_FIELD_SEED), ("rounds", _lib.K_NAV_FIELD_ROUND), ("parents", _lib.K_NAV_FIELD_PARENT))
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))

try:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra as sp_dijkstra
    BASELINE = "scipy.sparse.csgraph.dijkstra over a numpy-built graph"
except ImportError:
    sp_dijkstra = None
    BASELINE = "the heap Dijkstra of tests/nav_field_ref.py (scipy does not import)"


def median_ms(fn, warmup, repeats, sync):
    ms = []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def stage_ms(m, fn):
    kids = [k for _, k in STAGES]
    rows = {k: [] for k in kids}
    m.enable_profiling(True, only=kids)
    for i in range(WARMUP + REPEATS):
        for k in kids:
            m.kernel_time(k)
        fn()
        m.sync()
        for k in kids:
            t, _ = m.kernel_time(k)
            if i >= WARMUP:
                rows[k].append(t)
    m.enable_profiling(False)
    return {k: statistics.median(v) for k, v in rows.items()}


def host_baseline(cost, goals, neutral=50, lethal=253):
    """the field of one plane [H, W] on the host: (field, ms of the graph build, ms of the search)"""
    import nav_field_ref as ref
    if len(goals) == 0:
        return np.full(cost.shape, ref.UNREACHED, np.uint32), 0.0, 0.0
    goals = [[0] + list(g[1:]) for g in np.asarray(goals).tolist()]
    if sp_dijkstra is None:
        t0 = time.perf_counter()
        f, _ = ref.dijkstra(cost, goals, neutral, lethal, 8)
        return f[0], 0.0, (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    H, W = cost.shape
    ok = ref.move_masks(cost, lethal, 8)
    w = neutral + cost.astype(np.int64)
    ids = np.arange(H * W).reshape(H, W)
    src, dst, wt = [], [], []
    for d, (di, dj) in enumerate(DIRS):
        a = np.nonzero(ok[d][0])
        # an edge n -> x for the move x -> n: the search runs from the goal, the cell that is left pays
        src.append(ids[a[0] + di, a[1] + dj])
        dst.append(ids[a])
        wt.append(ref.STEP[d] * w[a])
    g = csr_matrix((np.concatenate(wt).astype(np.float64), (np.concatenate(src), np.concatenate(dst))), shape=(H * W, H * W))
    t1 = time.perf_counter()
    seeds = [int(ids[r, c]) for _, r, c in np.asarray(goals)[:, :3].tolist()]
    dist = sp_dijkstra(g, directed=True, indices=seeds, min_only=True)
    t2 = time.perf_counter()
    f = np.where(np.isfinite(dist), dist, float(ref.UNREACHED)).astype(np.uint32).reshape(H, W)
    return f, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def first_goal(plane, centre):
    cand = np.argwhere(plane < 253)
    return cand[np.argmin(((cand - centre) ** 2).sum(1))]


def field_case(lines, name, m, cost_dev, goals, baseline=True):
    """one cost tensor [B, H, W] on the device and its goals: everything the table says about a case"""
    import torch
    cost = cost_dev.cpu().numpy()
    B, H, W = cost.shape
    got = m.nav_field(cost, goals)
    trav = int((cost < 253).sum())
    reached = int((got["field"] != _lib.NAV_UNREACHED).sum())
    lines.append(f"{name}: {B} x {H} x {W} cells, {trav} traversable, {reached} reached, {len(goals)} goals; {got['rounds']} rounds, {got['tile_visits']} tile visits, "
                 f"converged {got['converged']} (default max_rounds {4 * ((H + 31) // 32) * ((W + 31) // 32) + 64})")
    if baseline:
        bt, bs = [], []
        for _ in range(HOST_REPEATS):
            t0 = time.perf_counter()
            ch = cost_dev.cpu().numpy()
            tc = (time.perf_counter() - t0) * 1e3
            b_ms, s_ms = 0.0, 0.0
            for p in range(B):
                f, tb, ts = host_baseline(ch[p], [g for g in np.asarray(goals).tolist() if g[0] == p])
                assert np.array_equal(f, got["field"][p]), f"{name}: plane {p} differs from the host baseline"
                b_ms += tb
                s_ms += ts
            bt.append(tc + b_ms + s_ms)
            bs.append((tc, b_ms, s_ms))
        k = int(np.argsort(bt)[len(bt) // 2])
        lines.append(f"{name}: today's route (copy to the host + {BASELINE}) {bt[k]:10.3f} ms = copy {bs[k][0]:8.3f} + graph {bs[k][1]:10.3f} + search {bs[k][2]:10.3f}; equal to the GPU's field")
        base = bt[k]
    st = stage_ms(m, lambda: m.nav_field(cost_dev, goals))
    lines.append(f"{name}: kernels per call  " + "  ".join(f"{s} {st[k] * 1e3:9.1f} us" for s, k in STAGES) + f"  sum {sum(st.values()) * 1e3:9.1f} us "
                 f"(the rounds launched: {-(-max(got['rounds'], 1) // 8) * 8} with check_every 8; {st[_lib.K_NAV_FIELD_ROUND] * 1e3 / max(1, -(-max(got['rounds'], 1) // 8) * 8):7.2f} us per round)")

    def dev_call():
        m.nav_field(cost_dev, goals)
        torch.cuda.synchronize()

    def fixed_call():
        m.nav_field(cost_dev, goals, rounds_fixed=max(1, got["rounds"]))
        torch.cuda.synchronize()
    dev, dev_min = median_ms(dev_call, WARMUP, REPEATS, m.sync)
    fix, fix_min = median_ms(fixed_call, WARMUP, REPEATS, m.sync)
    host, host_min = median_ms(lambda: m.nav_field(cost, goals), WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: device call {dev:9.3f} ms (min {dev_min:9.3f})  with rounds_fixed = {max(1, got['rounds'])} {fix:9.3f} ms (min {fix_min:9.3f})  "
                 f"host call (field and parent copied back) {host:9.3f} ms (min {host_min:9.3f})" + (f"; today's route / device call {base / dev:8.1f}x, / host call {base / host:8.1f}x" if baseline else ""))
    return got


def map_case(lines, name, m):
    import torch
    first = len(lines)
    vs = float(m.voxel_scale)
    R = 25
    lut = inflation_lut(vs, R, 6 * vs, 20 * vs, scale=3.0)
    g1 = m.nav_grid(bands=[(-16, 15)], radius=R * vs, lut=lut, device=True)
    torch.cuda.synchronize()
    c1 = g1["cost"]
    goal = first_goal(c1[0].cpu().numpy(), m.N // 2)
    goals = np.array([[0, goal[0], goal[1]]], np.int32)
    got = field_case(lines, f"{name}, case 1 (one band, one goal)", m, c1, goals)
    # paths
    rng = np.random.default_rng(1)
    cand = np.argwhere(got["field"][0] != _lib.NAV_UNREACHED)
    starts = np.concatenate([np.zeros((256, 1), np.int64), cand[rng.integers(0, len(cand), 256)]], 1)
    m.enable_profiling(True, only=[_lib.K_NAV_FIELD_PATHS])
    ts = []
    for i in range(WARMUP + REPEATS):
        m.kernel_time(_lib.K_NAV_FIELD_PATHS)
        p = m.nav_paths(got, starts, 1024)
        t, _ = m.kernel_time(_lib.K_NAV_FIELD_PATHS)
        ts.append(t)
    m.enable_profiling(False)
    hp, _ = median_ms(lambda: m.nav_paths(got, starts, 1024), WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: nav_paths, 256 starts, max_len 1024: kernel {statistics.median(ts[WARMUP:]) * 1e3:8.1f} us, host call (field and parent copied in, cells out) {hp:8.3f} ms; "
                 f"longest path {int(p['length'].max())} cells, {int((p['status'] == 0).sum())} end on the goal")
    if name == "room":
        for ce in (1, 8, 32):
            def call():
                m.nav_field(c1, goals, check_every=ce)
                torch.cuda.synchronize()
            t, tmin = median_ms(call, WARMUP, REPEATS, m.sync)
            r = m.nav_field(c1, goals, check_every=ce)
            lines.append(f"{name}, case 1: check_every = {ce:2d}: device call {t:9.3f} ms (min {tmin:9.3f}), {r['rounds']} rounds of work, {-(-max(r['rounds'] + 1, 1) // ce) * ce} launched at most")
    bands8 = [(-128 + 32 * b, -128 + 32 * b + 31) for b in range(8)]
    bands8 = [(max(k0, -(m.Nz // 2)), min(k1, m.Nz // 2 - 1)) for k0, k1 in bands8 if k0 < m.Nz // 2 and k1 >= -(m.Nz // 2)]
    g8 = m.nav_grid(bands=bands8, radius=R * vs, lut=lut, device=True)
    torch.cuda.synchronize()
    c8 = g8["cost"]
    ch = c8.cpu().numpy()
    goals8 = [[b, *first_goal(ch[b], m.N // 2)] for b in range(len(bands8)) if (ch[b] < 253).any()]
    field_case(lines, f"{name}, case 2 ({len(bands8)} bands, {len(goals8)} goals)", m, c8, np.array(goals8, np.int32))
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_field.txt"))
    args = ap.parse_args()
    import torch
    import nav_field_scenes as sc
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_nav_field.py: medians of {REPEATS} after {WARMUP} warm-up calls (today's route: median of {HOST_REPEATS}); one MI355X, one process",
             "kernels = HIP events around each launch (tsl_tsdf_prof_query), summed over a call; calls in wall time, the host call with its copies, the device call with the",
             "statistics read back (24 bytes) and, without rounds_fixed, one 4-byte read per check_every rounds"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    map_case(lines, "room", m)
    first = len(lines)
    cost, goals = sc.serpentine(512, 16, 3)
    field_case(lines, "case 3 (512 x 512 serpentine, pitch 16)", m, torch.from_numpy(cost[None]).cuda(), goals)
    for ln in lines[first:]:
        print(ln, flush=True)
    del m
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(20):
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    map_case(lines, "config-2", m)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Time of the 3-D cost-to-go field (tsl_nav_field3.hip, DenseTSDF.nav_field3d / flight_volume) on the two maps of tools/bench_nav_field.py: the room of
the tests (tests/render_view_scenes.py: four 320 x 240 frames, 256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20
frames (512^3 / 2 cm), each as a flight volume at stride 4 and 2 with one goal at the camera; a 128^3 serpentine, the bad case of the tile scheme; and a
volume of one layer against nav_field on the same plane.

The kernels have no profiling id: a call is timed with events on the caller's stream around tsl_tsdf_nav_field3_dev with rounds_fixed = the rounds of an
earlier call (asynchronous: nothing is read in between), once with and once without the parent pass.  Medians of REPEATS after WARMUP.  Against what a
caller does today: the volume copied to the host plus scipy.sparse.csgraph.dijkstra over a 26-neighbour graph built with numpy where scipy imports, else
the heap Dijkstra of tests/nav_field3d_ref.py (the table says which).  The field of the GPU is compared with the baseline's before anything is timed.  No
threshold is set.  Writes the table to --out (default profiles/nav_field3d.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import ctypes as C
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
from taichislam_amd.utils import flight_lut, inflation_lut
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3
TK, TI, TJ = 8, 8, 16

try:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra as sp_dijkstra
    BASELINE = "scipy.sparse.csgraph.dijkstra over a numpy-built 26-neighbour graph"
except ImportError:
    sp_dijkstra = None
    BASELINE = "the heap Dijkstra of tests/nav_field3d_ref.py (scipy does not import)"


def host_baseline(cost, goals, neutral=50, lethal=253):
    """the field of a volume on the host: (field, ms of the graph build, ms of the search)"""
    import nav_field3d_ref as ref
    if sp_dijkstra is None:
        t0 = time.perf_counter()
        f, _ = ref.dijkstra(cost, goals, neutral, lethal, 26)
        return f, 0.0, (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ok = ref.move_masks(cost, lethal, 26)
    w = neutral + cost.astype(np.int64)
    ids = np.arange(cost.size).reshape(cost.shape)
    src, dst, wt = [], [], []
    for d, (dk, di, dj) in enumerate(ref.DIRS):
        a = np.nonzero(ok[d])
        # an edge n -> x for the move x -> n: the search runs from the goal, the cell that is left pays
        src.append(ids[a[0] + dk, a[1] + di, a[2] + dj])
        dst.append(ids[a])
        wt.append(ref.STEP[d] * w[a])
    g = csr_matrix((np.concatenate(wt).astype(np.float64), (np.concatenate(src), np.concatenate(dst))), shape=(cost.size, cost.size))
    t1 = time.perf_counter()
    seeds = [int(ids[k, r, c]) for k, r, c in np.asarray(goals)[:, :3].tolist()]
    dist = sp_dijkstra(g, directed=True, indices=seeds, min_only=True)
    t2 = time.perf_counter()
    f = np.where(np.isfinite(dist), dist, float(ref.UNREACHED)).astype(np.uint32).reshape(cost.shape)
    return f, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def event_ms(fn):
    """median and minimum of the time between two events on the current stream around fn()"""
    import torch
    ms = []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def fixed_call(m, cost_dev, goals, rounds, parent, connectivity=26):
    """tsl_tsdf_nav_field3_dev with rounds_fixed on buffers allocated once: returns the closure that enqueues it and the field it fills"""
    import torch
    dev = cost_dev.device
    cfg = _lib.NavField3Cfg()
    cfg.D, cfg.H, cfg.W = tuple(cost_dev.shape)
    cfg.neutral, cfg.lethal, cfg.connectivity, cfg.rounds_fixed = 50, 253, connectivity, max(1, int(rounds))
    g = np.zeros((len(goals), 4), np.int32)
    g[:, :3] = np.asarray(goals)[:, :3]
    seeds = torch.from_numpy(g).to(dev)
    field = torch.empty(tuple(cost_dev.shape), dtype=torch.int32, device=dev)
    par = torch.empty(tuple(cost_dev.shape), dtype=torch.uint8, device=dev) if parent else None
    stats = torch.zeros(6, dtype=torch.int32, device=dev)

    def call():
        _lib.check(m.L.tsl_tsdf_nav_field3_dev(m.h, C.byref(cfg), cost_dev.data_ptr(), seeds.data_ptr(), len(goals), field.data_ptr(),
                                               None if par is None else par.data_ptr(), stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return call, field, stats


def field_case(lines, name, m, cost_dev, goals, baseline=True):
    import torch
    cost = cost_dev.cpu().numpy()
    D, H, W = cost.shape
    tiles = -(-D // TK) * -(-H // TI) * -(-W // TJ)
    got = m.nav_field3d(cost_dev, goals)
    field = got["field"].cpu().numpy().view(np.uint32)
    trav = int((cost < 253).sum())
    reached = int((field != _lib.NAV_UNREACHED).sum())
    lines.append(f"{name}: {D} x {H} x {W} = {cost.size} cells in {tiles} tiles, {trav} traversable, {reached} reached; {got['rounds']} rounds, {got['tile_visits']} tile visits, "
                 f"converged {got['converged']} (default max_rounds {min(4 * tiles + 64, 65536)})")
    base = None
    if baseline:
        bt, bs = [], []
        for _ in range(HOST_REPEATS):
            t0 = time.perf_counter()
            ch = cost_dev.cpu().numpy()
            tc = (time.perf_counter() - t0) * 1e3
            f, tb, ts = host_baseline(ch, goals)
            assert np.array_equal(f, field), f"{name}: the field differs from the host baseline"
            bt.append(tc + tb + ts)
            bs.append((tc, tb, ts))
        k = int(np.argsort(bt)[len(bt) // 2])
        base = bt[k]
        lines.append(f"{name}: today's route (copy to the host + {BASELINE}) {bt[k]:10.3f} ms = copy {bs[k][0]:8.3f} + graph {bs[k][1]:10.3f} + search {bs[k][2]:10.3f}; equal to the GPU's field")
    rounds = max(1, got["rounds"])
    with_p, f1, s1 = fixed_call(m, cost_dev, goals, rounds, True)
    without, f2, _ = fixed_call(m, cost_dev, goals, rounds, False)
    tp, tp_min = event_ms(with_p)
    tn, tn_min = event_ms(without)
    assert np.array_equal(f1.cpu().numpy().view(np.uint32), field) and np.array_equal(f2.cpu().numpy().view(np.uint32), field) and int(s1.cpu()[0]) == 1
    lines.append(f"{name}: device call, rounds_fixed = {rounds}, events: with parents {tp:9.3f} ms (min {tp_min:9.3f}), without {tn:9.3f} ms (min {tn_min:9.3f}): "
                 f"parent pass {max(tp - tn, 0.0) * 1e3:8.1f} us, {tn * 1e3 / rounds:7.2f} us per round (memsets and the seed launch included)"
                 + (f"; today's route / device call with parents {base / tp:8.1f}x" if base is not None else ""))

    def checked():
        m.nav_field3d(cost_dev, goals)
        torch.cuda.synchronize()
    ms = []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        checked()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"{name}: device call with the host checking every 8 rounds, wall time {statistics.median(ms):9.3f} ms (min {min(ms):9.3f})")
    return got


def map_case(lines, name, m, T):
    import torch
    first = len(lines)
    vs = float(m.voxel_scale)
    m.update_esdf(max_dist=2.0)
    m.sync()
    for stride in (4, 2):
        lut = flight_lut(vs, 0.1 + stride * vs * np.sqrt(3.0) / 2.0, 0.8, scale=3.0)
        tv, tv_min = event_ms(lambda: m.flight_volume(stride=stride, lut=lut, device=True))
        vol = m.flight_volume(stride=stride, lut=lut, device=True)
        torch.cuda.synchronize()
        cost = vol["cost"].cpu().numpy()
        cam = np.array([T[2], T[0], T[1]], np.float64) / vs + np.array(vol["half"])
        cand = np.argwhere(cost < 253)
        lines.append(f"{name}, stride {stride}: flight_volume (lattice, ESDF query and cost on the device, events) {tv:9.3f} ms (min {tv_min:9.3f}) for {cost.size} cells")
        if len(cand) == 0:
            lines.append(f"{name}, stride {stride}: no traversable cell")
            continue
        seed = cand[np.argmin(((cand * stride + stride // 2 - cam) ** 2).sum(1))]
        field_case(lines, f"{name}, stride {stride}", m, vol["cost"], np.array([seed], np.int32))
    for ln in lines[first:]:
        print(ln, flush=True)


def plane_case(lines, m):
    """one layer against nav_field on the same plane: the cost plane of nav_grid for one band of the room"""
    import torch
    first = len(lines)
    vs = float(m.voxel_scale)
    g1 = m.nav_grid(bands=[(-16, 15)], radius=25 * vs, lut=inflation_lut(vs, 25, 6 * vs, 20 * vs, scale=3.0), device=True)
    torch.cuda.synchronize()
    c1 = g1["cost"]
    plane = c1[0].cpu().numpy()
    cand = np.argwhere(plane < 253)
    goal = cand[np.argmin(((cand - m.N // 2) ** 2).sum(1))]
    goals = np.array([[0, goal[0], goal[1]]], np.int32)
    three = field_case(lines, "one layer (room, nav_grid cost plane)", m, c1, goals, baseline=False)
    two = m.nav_field(c1, goals)
    assert np.array_equal(two["field"].cpu().numpy(), three["field"].cpu().numpy())
    cfg = _lib.NavFieldCfg()
    cfg.B, cfg.H, cfg.W = tuple(c1.shape)
    cfg.neutral, cfg.lethal, cfg.connectivity, cfg.rounds_fixed = 50, 253, 8, max(1, two["rounds"])
    seeds = torch.from_numpy(np.array([[0, goal[0], goal[1], 0]], np.int32)).cuda()
    field = torch.empty(tuple(c1.shape), dtype=torch.int32, device="cuda")
    par = torch.empty(tuple(c1.shape), dtype=torch.uint8, device="cuda")

    def call():
        _lib.check(m.L.tsl_tsdf_nav_field_dev(m.h, C.byref(cfg), c1.data_ptr(), seeds.data_ptr(), 1, field.data_ptr(), par.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    t2, t2_min = event_ms(call)
    lines.append(f"one layer: nav_field on the same plane, rounds_fixed = {max(1, two['rounds'])} ({two['tile_visits']} visits of 32 x 32 tiles), events, with parents {t2:9.3f} ms (min {t2_min:9.3f}); "
                 f"equal fields")
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_field3d.txt"))
    ap.add_argument("--skip-config2", action="store_true")
    args = ap.parse_args()
    import torch
    import nav_field3d_scenes as sc
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_nav_field3d.py: medians of {REPEATS} after {WARMUP} warm-up calls (today's route: median of {HOST_REPEATS}); one MI355X, one process",
             "device calls = events on the caller's stream around tsl_tsdf_nav_field3_dev with rounds_fixed (asynchronous; memsets, seed launch, every round, the statistics and,",
             "where said, the parent pass); tiles are 16 x 8 x 8 cells"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    map_case(lines, "room", m, frames[0][1])
    plane_case(lines, m)
    first = len(lines)
    cost, goals = sc.serpentine(128, 8, 8)
    field_case(lines, "128^3 serpentine (slabs of 7 layers, bands of 7 rows)", m, torch.from_numpy(cost).cuda(), goals)
    for ln in lines[first:]:
        print(ln, flush=True)
    del m
    if not args.skip_config2:
        m = DenseTSDF(**C2)
        m.set_dep_camera_intrinsic(syn.K_DEPTH)
        T0 = None
        for R, T, d in syn.sphere_room_stream(20):
            T0 = T if T0 is None else T0
            m.recast_depth_to_map(R, T, d, None)
        m.sync()
        map_case(lines, "config-2", m, T0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

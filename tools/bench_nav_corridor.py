"""Time of the safe corridors (tsl_nav_corridor.hip, DenseTSDF.nav_corridor / nav_boxes) on the maps of tools/bench_nav_field3d.py: the room of the tests
(tests/render_view_scenes.py, 256^3 / 4 cm) as a flight volume at stride 4 and 2, and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20
frames (512^3 / 2 cm) at stride 4; the path to one frontier cluster and the paths to all reached clusters; extent 8 and 32.

The kernels have no profiling id.  A call is timed with events on the caller's stream around the asynchronous _dev entry points, on buffers allocated
once: tsl_tsdf_nav_corridor_dev (pack + inflate every path cell + chain), tsl_tsdf_nav_boxes_dev over the same cells (pack + inflate) and over one cell
(pack + one wave), and the one-cell call over a volume of 64 cells at extent 0, which is what a call costs before any work: the two orderings with the caller's
stream and two launches.  The split is the difference of those medians: pack and one seed's wave (at a large extent a long chain of dependent tries) = one cell - one cell on
64 cells, the other seeds = all cells - one cell, chain = corridor - all cells.
Medians of REPEATS after WARMUP.  Reported beside them: the boxes inflated against the boxes the chain keeps, and the mean share of lanes with work in
the inflation -- counted on the host from the definition over a sample of the seeds: a try over n slab items occupies ceil(n / 64) passes of the wave, the
share is sum n / sum 64 * passes (a try that fails is counted in full, the kernel leaves at the first pass that fails).  Against what a caller does today:
the volume copied to the host plus the slicing restatement of tests/nav_corridor_ref.py, which inflates only the seeds the chain visits.  The GPU's result
is compared with the baseline's before anything is timed.  No threshold is set.  Writes the table to --out (default profiles/nav_corridor.txt) and prints
it.  One process; run it under `timeout`."""
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
from taichislam_amd.utils import flight_lut, frontier_reach3d
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3
MAX_LEN, SAMPLE = 512, 300
KEYS = ("boxes", "seed", "link", "count", "status")


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


def lane_share(free, cells, ext):
    """(items, lane slots) of the inflation of `cells`, from the definition: per try the slab's items -- (k, i) pairs for +-j, (row, word) pairs else"""
    items = slots = 0
    D, H, W = free.shape
    for c in cells:
        ck, ci, cj = (int(v) for v in c)
        if not (0 <= ck < D and 0 <= ci < H and 0 <= cj < W) or not free[ck, ci, cj]:
            continue
        lo, hi, live = [ck, ci, cj], [ck, ci, cj], [(2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1)]
        while live:
            for f in list(live):
                a, sgn = f
                n = lo[a] - 1 if sgn < 0 else hi[a] + 1
                good = abs(n - (ck, ci, cj)[a]) <= ext[a] and 0 <= n < free.shape[a]
                if good:
                    sl = [slice(lo[x], hi[x] + 1) for x in range(3)]
                    sl[a] = n
                    words = (hi[2] >> 6) - (lo[2] >> 6) + 1
                    cnt = (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) if a == 2 else ((hi[0] - lo[0] + 1) if a == 1 else (hi[1] - lo[1] + 1)) * words
                    items += cnt
                    slots += 64 * -(-cnt // 64)
                    good = bool(free[tuple(sl)].all())
                if good:
                    (lo if sgn < 0 else hi)[a] = n
                else:
                    live.remove(f)
    return items, slots


def corridor_case(lines, name, m, cost_dev, cost, paths_dev, ext):
    import torch
    import nav_corridor_ref as ref
    dev = cost_dev.device
    cells, length = paths_dev["cells"].contiguous(), paths_dev["length"].contiguous()
    P, L = int(cells.shape[0]), int(cells.shape[1])
    hc, hl = cells.cpu().numpy(), length.cpu().numpy()
    got = m.nav_corridor(cost_dev, (cells, length), extent=ext, max_boxes=L)
    torch.cuda.synchronize()
    bt = []
    for _ in range(HOST_REPEATS):                                   # today's route
        t0 = time.perf_counter()
        ch = cost_dev.cpu().numpy()
        t1 = time.perf_counter()
        want = ref.corridor(ch, hc, hl, 253, ext, L)
        bt.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
    for k in KEYS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), f"{name}: {k} differs from the host restatement"
    base, base_copy = sorted(bt)[len(bt) // 2]
    kept, inflated = int(want["count"].sum()), int(np.minimum(hl, L).clip(0).sum())
    flat = np.concatenate([hc[p, :max(0, min(int(hl[p]), L))] for p in range(P)]).astype(np.int64)
    rng = np.random.default_rng(1)
    pick = flat if len(flat) <= SAMPLE else flat[rng.choice(len(flat), SAMPLE, replace=False)]
    items, slots = lane_share(cost < 253, pick, ext)

    cfg = _lib.NavCorridorCfg(*cost.shape)
    cfg.free_below, cfg.ext_k, cfg.ext_i, cfg.ext_j, cfg.max_boxes = 253, ext[0], ext[1], ext[2], L
    boxes = torch.empty((P, L, 6), dtype=torch.int16, device=dev)
    seed = torch.empty((P, L), dtype=torch.int32, device=dev)
    link = torch.empty((P, L), dtype=torch.uint8, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.uint8, device=dev)
    all_cells = torch.from_numpy(flat.astype(np.int32)).to(dev)
    cb = torch.empty((len(flat), 6), dtype=torch.int16, device=dev)
    cf = torch.empty(len(flat), dtype=torch.uint8, device=dev)
    st = lambda: torch.cuda.current_stream(dev).cuda_stream

    def call_corridor():
        _lib.check(m.L.tsl_tsdf_nav_corridor_dev(m.h, C.byref(cfg), cost_dev.data_ptr(), cells.data_ptr(), length.data_ptr(), P, L, boxes.data_ptr(), seed.data_ptr(),
                                                 link.data_ptr(), count.data_ptr(), status.data_ptr(), st()))

    def call_boxes(n):
        return lambda: _lib.check(m.L.tsl_tsdf_nav_boxes_dev(m.h, C.byref(cfg), cost_dev.data_ptr(), all_cells.data_ptr(), n, cb.data_ptr(), cf.data_ptr(), st()))
    tiny = torch.zeros((1, 1, 64), dtype=torch.uint8, device=dev)
    tiny_cfg = _lib.NavCorridorCfg(1, 1, 64, 253, 0, 0, 0, 1)              # extent 0: the one wave tries six faces and is done
    zero = torch.zeros((1, 3), dtype=torch.int32, device=dev)

    def call_tiny():
        _lib.check(m.L.tsl_tsdf_nav_boxes_dev(m.h, C.byref(tiny_cfg), tiny.data_ptr(), zero.data_ptr(), 1, cb.data_ptr(), cf.data_ptr(), st()))
    tc, tc_min = event_ms(call_corridor)
    ta, ta_min = event_ms(call_boxes(len(flat)))
    t1, t1_min = event_ms(call_boxes(1))
    t0, t0_min = event_ms(call_tiny)
    assert np.array_equal(boxes.cpu().numpy(), want["boxes"]) and np.array_equal(count.cpu().numpy(), want["count"])
    lines.append(f"{name}, extent {ext[0]}: {P} paths, {inflated} cells inflated, {kept} boxes kept ({inflated / max(kept, 1):5.1f} x); lanes with work {100.0 * items / max(slots, 1):5.1f} % "
                 f"(sample of {len(pick)} seeds)")
    lines.append(f"{name}, extent {ext[0]}: corridor call {tc * 1e3:9.1f} us (min {tc_min * 1e3:9.1f}) = an empty call {t0 * 1e3:8.1f} + pack and one seed {max(t1 - t0, 0.0) * 1e3:8.1f} + the other seeds "
                 f"{max(ta - t1, 0.0) * 1e3:8.1f} + chain {max(tc - ta, 0.0) * 1e3:8.1f} (differences of medians: boxes call over all cells {ta * 1e3:9.1f} us, over one cell "
                 f"{t1 * 1e3:9.1f} us, over one cell of a 64-cell volume {t0 * 1e3:9.1f} us)")
    lines.append(f"{name}, extent {ext[0]}: today's route (copy to the host + slicing restatement, visited seeds only) {base:10.3f} ms, of which the copy {base_copy:8.3f}; "
                 f"equal results; today's route / corridor call {base / tc:8.1f} x")


def map_case(lines, name, m, T, strides):
    import torch
    first = len(lines)
    vs = float(m.voxel_scale)
    m.update_esdf(max_dist=2.0)
    m.sync()
    fr = m.extract_frontiers()
    for stride in strides:
        lut = flight_lut(vs, 0.1 + stride * vs * np.sqrt(3.0) / 2.0, 0.8, scale=3.0)
        vol = m.flight_volume(stride=stride, lut=lut, device=True)
        torch.cuda.synchronize()
        cost = vol["cost"].cpu().numpy()
        cam = np.array([T[2], T[0], T[1]], np.float64) / vs + np.array(vol["half"]) - np.array(vol["origin"])      # the camera in unsigned voxels from the volume's first
        cand = np.argwhere(cost < 253)
        if len(cand) == 0:
            lines.append(f"{name}, stride {stride}: no traversable cell")
            continue
        seed = cand[np.argmin(((cand * stride + stride // 2 - cam) ** 2).sum(1))]
        field = m.nav_field3d(vol, np.array([seed], np.int32))
        reach = frontier_reach3d(fr, field, vol)
        hit = np.nonzero(reach["reached"])[0]
        lines.append(f"{name}, stride {stride}: volume {cost.shape[0]} x {cost.shape[1]} x {cost.shape[2]} = {cost.size} cells, {len(cand)} free; {len(hit)} of {len(fr['clusters'])} "
                     f"frontier clusters reached")
        if len(hit) == 0:
            continue
        u = fr["indices"][reach["voxel"][hit]].astype(int)
        org, half = vol["origin"], vol["half"]
        starts = np.stack([(u[:, 2] + half[0] - org[0]) // stride, (u[:, 0] + half[1] - org[1]) // stride, (u[:, 1] + half[2] - org[2]) // stride], 1).astype(np.int32)
        far = int(np.argmax(reach["value"][hit]))
        for which, rows in (("one path", [far]), ("all paths", list(range(len(hit))))):
            paths = m.nav_paths3d(field, starts[rows], MAX_LEN)
            for e in (8, 32):
                corridor_case(lines, f"{name}, stride {stride}, {which}", m, vol["cost"], cost, paths, (e, e, e))
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_corridor.txt"))
    ap.add_argument("--skip-config2", action="store_true")
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_nav_corridor.py: medians of {REPEATS} after {WARMUP} warm-up calls (today's route: median of {HOST_REPEATS}); one MI355X, one process",
             "device calls = events on the caller's stream around tsl_tsdf_nav_corridor_dev / tsl_tsdf_nav_boxes_dev (asynchronous); free_below 253, max_boxes = L = "
             f"{MAX_LEN}"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    map_case(lines, "room", m, frames[0][1], (4, 2))
    del m
    if not args.skip_config2:
        m = DenseTSDF(**C2)
        m.set_dep_camera_intrinsic(syn.K_DEPTH)
        T0 = None
        for R, T, d in syn.sphere_room_stream(20):
            T0 = T if T0 is None else T0
            m.recast_depth_to_map(R, T, d, None)
        m.sync()
        map_case(lines, "config-2", m, T0, (4,))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Time of the frontier extraction (tsl_frontier.hip, DenseTSDF.extract_frontiers) on two maps: the config-2 scene of taichislam_amd/utils/bench_configs.py
after 20 frames of the sphere-room stream (512^3 / 2 cm) and the room of the tests (tests/render_view_scenes.py: four 320 x 240 frames, 256^3 / 4 cm).

Per map, medians of REPEATS after WARMUP: the time of every stage through the handle's profiler (HIP events around the stage's launches: mark, label,
join + flatten, the sums, the sorts + output), the wall time of the host call and of the device call, for scale generate_mesh(1) on the same map (its
kernel through the profiler and its wall time: similar brick-plus-halo traffic), and the host route the extraction replaces: export_submap() plus the
numpy restatement of tests/frontier_ref.py.  The result of the GPU is compared with that restatement before anything is timed.  No threshold is set.
Writes the table to --out (default profiles/frontier.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from taichislam_amd import _lib
from taichislam_amd.mapping import DenseTSDF, MarchingCubeMesher
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3
STAGES = (("mark", _lib.K_FRONTIER_MARK), ("label", _lib.K_FRONTIER_LABEL), ("join+flatten", _lib.K_FRONTIER_JOIN), ("sums", _lib.K_FRONTIER_SUM),
          ("sorts+output", _lib.K_FRONTIER_EMIT))


def median_ms(fn, warmup, repeats, sync):
    ms = []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def stage_ms(m, kids, fn):
    """median per kernel id of the profiler's time for one call of fn"""
    rows = {k: [] for k in kids}
    m.enable_profiling(True, only=list(kids))
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


def case(lines, name, m):
    import torch
    import frontier_ref as ref
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        e = m.export_submap()
    got = m.extract_frontiers()
    ref.assert_equal(got, ref.extract(e, m.N, m.Nz, m.voxel_scale), name)
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {m.voxel_scale} m, {m.bricks_in_use()} bricks, {e['indices'].shape[0]} observed voxels, "
                 f"{got['indices'].shape[0]} frontier voxels in {got['clusters'].shape[0]} clusters (equal to the numpy restatement)")
    st = stage_ms(m, [k for _, k in STAGES], m.extract_frontiers)
    lines.append(f"{name}: stages  " + "  ".join(f"{n} {st[k] * 1e3:8.1f} us" for n, k in STAGES) + f"  sum {sum(st.values()) * 1e3:8.1f} us")
    host, host_min = median_ms(m.extract_frontiers, WARMUP, REPEATS, m.sync)

    def dev_call():
        m.extract_frontiers(device=True)
        torch.cuda.synchronize()
    dev, dev_min = median_ms(dev_call, WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: host call {host:8.3f} ms (min {host_min:8.3f})  device call {dev:8.3f} ms (min {dev_min:8.3f})")
    mesher = MarchingCubeMesher(m, max_triangles=4_000_000, tsdf_surface_thres=5 * m.voxel_scale)
    with contextlib.redirect_stdout(quiet):
        mk = stage_ms(m, [_lib.K_MESH], lambda: mesher.generate_mesh(1))[_lib.K_MESH]
        mw, mw_min = median_ms(lambda: mesher.generate_mesh(1), WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: for scale generate_mesh(1) kernels {mk * 1e3:8.1f} us, call {mw:8.3f} ms (min {mw_min:8.3f})")

    def host_route():
        with contextlib.redirect_stdout(quiet):
            ex = m.export_submap()
        return ref.extract(ex, m.N, m.Nz, m.voxel_scale)
    hr, hr_min = median_ms(host_route, 0, HOST_REPEATS, m.sync)
    with contextlib.redirect_stdout(quiet):
        ex, ex_min = median_ms(m.export_submap, 1, HOST_REPEATS, m.sync)
    lines.append(f"{name}: the host route export_submap + numpy restatement {hr:10.3f} ms (min {hr_min:10.3f}), of that export_submap {ex:8.3f} ms; host route / host call {hr / host:8.1f}x")
    for ln in lines[-4:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier.txt"))
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_frontier.py: medians of {REPEATS} after {WARMUP} warm-up calls (host route: median of {HOST_REPEATS}); one MI355X, one process",
             "stages = HIP events around each stage's launches (tsl_tsdf_prof_query); calls in wall time, the host call with its copies, the device call without"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "room", m)
    del m
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(20):
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "config-2", m)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Time of the view gain (tsl_view_gain.hip, DenseTSDF.score_views) on two maps: the room of the tests (tests/render_view_scenes.py: four 320 x 240 frames,
256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames of the sphere-room stream (512^3 / 2 cm).

Per map: fans of 80 x 60 rays with the field of view of the sensor, the map's default range and step, 1, 64 and 1024 poses on a circle of 1 m, skipping on and
off, unknown_run 0 and 25.  Medians of REPEATS after WARMUP: the kernel through the handle's profiler (HIP events around the launch), the wall time of the host
call (with its copies) and of the device call.  Baselines: (a) the cheapest equivalent without this kernel, one render_view(device=True) call per pose over the
same fan, range and step -- the same rays with eight gathers per sample, and no counts; (b) the host route, export_submap() plus the numpy restatement of
tests/view_gain_ref.py (1 pose; 64 poses on the room).  The result of the GPU is compared with the restatement before anything is timed.  No threshold is
set.  Writes the table to --out (default profiles/view_gain.txt) and prints it.  One process; run it under `timeout`."""
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
from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS = 2, 7
H, W = 60, 80
POSES = (1, 64, 1024)


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
    """median of the profiler's time of the view-gain kernel for one call of fn"""
    rows = []
    m.enable_profiling(True, only=[_lib.K_VIEW_GAIN])
    for i in range(WARMUP + REPEATS):
        m.kernel_time(_lib.K_VIEW_GAIN)
        fn()
        m.sync()
        t, _ = m.kernel_time(_lib.K_VIEW_GAIN)
        if i >= WARMUP:
            rows.append(t)
    m.enable_profiling(False)
    return statistics.median(rows)


def circle(n):
    Rs, Ts = [], []
    for k in range(n):
        R, T = syn.camera_pose(k, orbit=1.0, deg_per_frame=360.0 / n)
        Rs.append(np.asarray(R, np.float64).reshape(3, 3)); Ts.append(np.asarray(T, np.float64).reshape(3))
    return np.stack(Rs), np.stack(Ts)


def case(lines, name, m, cfg, host_poses):
    import torch
    import view_gain_ref as ref
    quiet = io.StringIO()
    K = syn.scaled_intrinsics(H, W)
    kw = dict(K=K, shape=(H, W))
    tmin, tmax = np.float32(cfg["min_ray_length"]), np.float32(cfg["max_ray_length"])
    first = len(lines)

    def host_route(n, run=0):
        R, T = circle(n)
        with contextlib.redirect_stdout(quiet):
            e = m.export_submap()
        return ref.score_export(e, m.N, m.Nz, m.voxel_scale, R, T, K, H, W, tmin, tmax, unknown_run=run)
    R1, T1 = circle(1)
    for run in (0, 25):
        ref.assert_equal(m.score_views(R1, T1, rays=True, unknown_run=run, **kw), host_route(1, run), f"{name}, unknown_run {run}")
    S = ref.sample_count(tmin, tmax, ref.default_step(m.voxel_scale))
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {m.voxel_scale} m, {m.bricks_in_use()} bricks; fans of {W} x {H} rays, {S} samples per ray "
                 f"(one pose equal to the numpy restatement, unknown_run 0 and 25)")
    per_pose = {}
    for n in POSES:
        R, T = circle(n)
        for run in (0, 25):
            for skip in (True, False):
                call = lambda: m.score_views(R, T, unknown_run=run, skip=skip, **kw)
                kt = kernel_ms(m, call)
                host, host_min = median_ms(call, WARMUP, REPEATS, m.sync)

                def dev_call():
                    m.score_views(R, T, unknown_run=run, skip=skip, device=True, **kw)
                    torch.cuda.synchronize()
                dev, dev_min = median_ms(dev_call, WARMUP, REPEATS, m.sync)
                per_pose[(n, run, skip)] = dev / n
                lines.append(f"{name}: {n:5d} poses  unknown_run {run:2d}  skip {'on ' if skip else 'off'}  kernel {kt * 1e3:10.1f} us ({kt * 1e3 / n:9.2f} us / pose)  "
                             f"host call {host:9.3f} ms (min {host_min:9.3f})  device call {dev:9.3f} ms (min {dev_min:9.3f})")

        # (a) one render_view per pose: the same fan, range and step
        def render_loop():
            for k in range(n):
                m.render_view(R[k], T[k], K=K, shape=(H, W), normals=False, colors=False, device=True)
            torch.cuda.synchronize()
        ra, ra_min = median_ms(render_loop, 1 if n > 64 else WARMUP, 3 if n > 64 else REPEATS, m.sync)
        lines.append(f"{name}: {n:5d} poses  (a) a loop of render_view(device=True) {ra:9.3f} ms (min {ra_min:9.3f}), {ra * 1e3 / n:9.2f} us / pose; "
                     f"(a) / device call: unknown_run 0 {ra / (per_pose[(n, 0, True)] * n):7.2f}x, unknown_run 25 {ra / (per_pose[(n, 25, True)] * n):7.2f}x")
    for n in host_poses:
        hr, _ = median_ms(lambda: host_route(n), 0, 1, m.sync)
        R, T = circle(n)
        hc, _ = median_ms(lambda: m.score_views(R, T, **kw), WARMUP, REPEATS, m.sync)
        lines.append(f"{name}: {n:5d} poses  (b) export_submap + numpy restatement {hr:12.3f} ms; (b) / host call {hr / hc:10.1f}x")
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_gain.txt"))
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_view_gain.py: medians of {REPEATS} after {WARMUP} warm-up calls ((a) at 1024 poses: median of 3 after 1; (b): one run); one MI355X, one process",
             "kernel = HIP events around the launch (tsl_tsdf_prof_query); calls in wall time, the host call with its copies, the device call without"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "room", m, SMALL, (1, 64))
    del m
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(20):
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "config-2", m, C2, (1,))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

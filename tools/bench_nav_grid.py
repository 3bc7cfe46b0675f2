"""Time of the navigation grids (tsl_nav_grid.hip, DenseTSDF.nav_grid) on two maps: the room of the tests (tests/render_view_scenes.py: four 320 x 240 frames,
256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames of the sphere-room stream (512^3 / 2 cm).

Per map, medians of REPEATS after WARMUP: one band of 32 layers at R = 25 as a device call and as a host call, its three stages through the handle's
profiler (HIP events around the stage's launch: projection, distance pass along j, distance pass along i with the cost lookup), against the host route it
replaces, export_submap() plus the numpy restatement of tests/nav_grid_ref.py; 8 bands in one call against 8 one-band calls (the projection reads the map
once however many bands there are); the projection's bytes against its model (5 bytes per voxel of the bricks whose layers meet the band) and the
fraction of the 8 TB/s HBM peak that gives; the two distance passes at R = 25 and R = 254.  The result of the GPU is compared with the restatement before
anything is timed.  No threshold is set.  Writes the table to --out (default profiles/nav_grid.txt) and prints it.  One process; run it under `timeout`."""
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
from taichislam_amd.utils import inflation_lut
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3
STAGES = (("project", _lib.K_NAV_PROJECT), ("rows (along j)", _lib.K_NAV_EDT_ROWS), ("columns (along i) + cost", _lib.K_NAV_EDT))
HBM_PEAK = 8.0e12


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
    """median per kernel id of the profiler's time for one call of fn (a call may launch a stage several times: the sum)"""
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
    import nav_grid_ref as ref
    first = len(lines)
    quiet = io.StringIO()
    vs = float(m.voxel_scale)
    R, band = 25, (-16, 15)
    lut = inflation_lut(vs, R, 6 * vs, 20 * vs, scale=3.0)
    kw = dict(bands=[band], radius=R * vs, lut=lut)
    with contextlib.redirect_stdout(quiet):
        e = m.export_submap()
    got = m.nav_grid(counts=True, span=True, **kw)
    ref.assert_equal(got, ref.nav_grid(e, m.N, m.Nz, vs, [band], R, lut=lut), name, keys=("cls", "counts", "span", "d2", "cost"))
    u = e["indices"].astype(np.int64) + np.array([m.N // 2, m.N // 2, m.Nz // 2])
    bricks = np.unique(u >> 4, axis=0)
    uk0, uk1 = band[0] + m.Nz // 2, band[1] + m.Nz // 2
    met = int(((bricks[:, 2] * 16 + 15 >= uk0) & (bricks[:, 2] * 16 <= uk1)).sum())
    n = [int((got["cls"] == c).sum()) for c in (ref.FREE, ref.OCCUPIED, ref.UNKNOWN)]
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {vs} m, {m.bricks_in_use()} bricks, {bricks.shape[0]} of them hold an observed voxel, {met} of those meet the band "
                 f"{band}; {n[0]} free, {n[1]} occupied, {n[2]} unknown cells (every plane equal to the numpy restatement)")
    kids = [k for _, k in STAGES]
    st = stage_ms(m, kids, lambda: m.nav_grid(device=True, **kw))
    lines.append(f"{name}: one band of 32 layers, R = 25: stages  " + "  ".join(f"{s} {st[k] * 1e3:8.1f} us" for s, k in STAGES) + f"  sum {sum(st.values()) * 1e3:8.1f} us")
    model = met * 4096 * 5
    tp = st[_lib.K_NAV_PROJECT] * 1e-3
    lines.append(f"{name}: projection model {model / 1e6:8.3f} MB (5 bytes per voxel of {met} bricks) in {tp * 1e6:8.1f} us = {model / tp / 1e9:8.1f} GB/s, "
                 f"{100.0 * model / tp / HBM_PEAK:5.2f} % of the 8 TB/s HBM peak (plus {m.N * m.N * 1} cells of u8 classes written)")

    def dev_call():
        m.nav_grid(device=True, **kw)
        torch.cuda.synchronize()
    dev, dev_min = median_ms(dev_call, WARMUP, REPEATS, m.sync)
    host, host_min = median_ms(lambda: m.nav_grid(**kw), WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: device call {dev:8.3f} ms (min {dev_min:8.3f})  host call (cls, d2, cost copied back) {host:8.3f} ms (min {host_min:8.3f})")

    def host_route():
        with contextlib.redirect_stdout(quiet):
            ex = m.export_submap()
        return ref.nav_grid(ex, m.N, m.Nz, vs, [band], R, lut=lut)
    hr, hr_min = median_ms(host_route, 0, HOST_REPEATS, m.sync)
    with contextlib.redirect_stdout(quiet):
        ex, _ = median_ms(m.export_submap, 1, HOST_REPEATS, m.sync)
    lines.append(f"{name}: the host route export_submap + numpy restatement {hr:10.3f} ms (min {hr_min:10.3f}), of that export_submap {ex:8.3f} ms; "
                 f"host route / host call {hr / host:8.1f}x, / device call {hr / dev:8.1f}x")
    # 8 bands of 32 layers in one call against 8 one-band calls
    bands8 = [(-128 + 32 * b, -128 + 32 * b + 31) for b in range(8)]
    k8 = dict(radius=R * vs, lut=lut, device=True)
    s8 = stage_ms(m, kids, lambda: m.nav_grid(bands=bands8, **k8))
    s1 = stage_ms(m, kids, lambda: [m.nav_grid(bands=[b], **k8) for b in bands8])
    met8 = int(((bricks[:, 2] * 16 + 15 >= bands8[0][0] + m.Nz // 2) & (bricks[:, 2] * 16 <= bands8[-1][1] + m.Nz // 2)).sum())
    lines.append(f"{name}: 8 bands of 32 layers ({bands8[0][0]} .. {bands8[-1][1]}, {met8} bricks): one call  " + "  ".join(f"{s} {s8[k] * 1e3:8.1f} us" for s, k in STAGES)
                 + f"  sum {sum(s8.values()) * 1e3:8.1f} us")
    lines.append(f"{name}: 8 bands of 32 layers: 8 one-band calls  " + "  ".join(f"{s} {s1[k] * 1e3:8.1f} us" for s, k in STAGES) + f"  sum {sum(s1.values()) * 1e3:8.1f} us; "
                 f"projection, one call / one band of 32 layers {s8[_lib.K_NAV_PROJECT] / st[_lib.K_NAV_PROJECT]:5.2f}x")

    def both():
        m.nav_grid(bands=bands8, **k8)
        torch.cuda.synchronize()

    def each():
        for b in bands8:
            m.nav_grid(bands=[b], **k8)
        torch.cuda.synchronize()
    w8, _ = median_ms(both, WARMUP, REPEATS, m.sync)
    w1, _ = median_ms(each, WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: 8 bands, wall: one device call {w8:8.3f} ms, 8 device calls {w1:8.3f} ms")
    # the two distance passes at R = 25 and R = 254
    for r in (25, 254):
        sr = stage_ms(m, kids[1:], lambda: m.nav_grid(bands=[band], radius=r * vs, device=True))
        lines.append(f"{name}: distance transform at R = {r:3d}: rows {sr[_lib.K_NAV_EDT_ROWS] * 1e3:8.1f} us  columns {sr[_lib.K_NAV_EDT] * 1e3:8.1f} us "
                     f"({m.N * m.N} cells, {(2 * r + 16) * 64} bytes of LDS per workgroup)")
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_grid.txt"))
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_nav_grid.py: medians of {REPEATS} after {WARMUP} warm-up calls (host route: median of {HOST_REPEATS}); one MI355X, one process",
             "stages = HIP events around each stage's launch (tsl_tsdf_prof_query); calls in wall time, the host call with its copies, the device call without"]
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

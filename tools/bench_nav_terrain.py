"""Time of the terrain layers (tsl_nav_terrain.hip, DenseTSDF.nav_terrain) on two maps: the room of the tests (tests/render_view_scenes.py: four 320 x 240
frames, 256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames of the sphere-room stream (512^3 / 2 cm).

Per map, medians of REPEATS after WARMUP: one band (the lower half of the volume) as a device call and as a host call, its four stages through the handle's
profiler (HIP events around the stage's launch: the column walk, the window pass, the two distance passes), against the host route it replaces,
export_submap() plus the numpy restatement of tests/nav_terrain_ref.py; 8 bands in one call against 8 one-band calls (the column walk reads the map once
however many bands there are); the column walk's bytes against its model (5 bytes per voxel of the bricks at or under the highest layer a band can ask
about) and the fraction of the 8 TB/s HBM peak that gives; the window pass at window / slope_base 1, 4 and 16.  The result of the GPU is compared with the
restatement before anything is timed.  No threshold is set.  Writes the table to --out (default profiles/nav_terrain.txt) and prints it.  One process; run
it under `timeout`."""
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
STAGES = (("columns", _lib.K_NAV_TERRAIN_COLUMNS), ("window", _lib.K_NAV_TERRAIN_WINDOW), ("rows (along j)", _lib.K_NAV_EDT_ROWS), ("columns (along i) + cost", _lib.K_NAV_EDT))
HBM_PEAK = 8.0e12
PLANES = ("height", "col", "step", "nsup", "slope2", "cls", "d2", "cost")


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
    import nav_terrain_ref as ref
    first = len(lines)
    quiet = io.StringIO()
    vs = float(m.voxel_scale)
    R, band, cl, w, s = 25, (-(m.Nz // 2), -1), 25, 2, 2
    lut = inflation_lut(vs, R, 6 * vs, 20 * vs, scale=3.0)
    kw = dict(bands=[band], clearance=cl * vs, window=w * vs, slope_base=s * vs, max_step=2 * vs, max_slope_deg=30.0, min_support=9, radius=R * vs, lut=lut)
    with contextlib.redirect_stdout(quiet):
        e = m.export_submap()
    got = m.nav_terrain(**kw)
    rk = dict(clearance=cl, window=w, slope_base=s, max_step=got["max_step_units"], max_slope2=got["max_slope2"], min_support=9, R=R, lut=lut)
    ref.assert_equal(got, ref.nav_terrain(e, m.N, m.Nz, vs, [band], **rk), name, keys=PLANES)
    u = e["indices"].astype(np.int64) + np.array([m.N // 2, m.N // 2, m.Nz // 2])
    bricks = np.unique(u >> 4, axis=0)
    utop = min(band[1] + m.Nz // 2 + cl, m.Nz - 1)
    met = int((bricks[:, 2] * 16 <= utop).sum())
    n = [int((got["cls"] == c).sum()) for c in (ref.FREE, ref.OCCUPIED, ref.UNKNOWN)]
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {vs} m, {m.bricks_in_use()} bricks, {bricks.shape[0]} of them hold an observed voxel, {met} of those lie at or under "
                 f"layer {utop - m.Nz // 2} (band {band}, clearance {cl}); {int((got['col'] == 0).sum())} supports, {int((got['slope2'] != ref.NO_SLOPE).sum())} valid slopes; "
                 f"{n[0]} free, {n[1]} occupied, {n[2]} unknown cells (every plane equal to the numpy restatement)")
    kids = [k for _, k in STAGES]
    st = stage_ms(m, kids, lambda: m.nav_terrain(device=True, **kw))
    lines.append(f"{name}: one band, window {w}, slope_base {s}, R = {R}: stages  " + "  ".join(f"{t} {st[k] * 1e3:8.1f} us" for t, k in STAGES) + f"  sum {sum(st.values()) * 1e3:8.1f} us")
    model = met * 4096 * 5
    tp = st[_lib.K_NAV_TERRAIN_COLUMNS] * 1e-3
    lines.append(f"{name}: column-walk model {model / 1e6:8.3f} MB (5 bytes per voxel of {met} bricks) in {tp * 1e6:8.1f} us = {model / tp / 1e9:8.1f} GB/s, "
                 f"{100.0 * model / tp / HBM_PEAK:5.2f} % of the 8 TB/s HBM peak (plus {m.N * m.N} cells of int16 heights and u8 col written)")

    def dev_call():
        m.nav_terrain(device=True, **kw)
        torch.cuda.synchronize()
    dev, dev_min = median_ms(dev_call, WARMUP, REPEATS, m.sync)
    host, host_min = median_ms(lambda: m.nav_terrain(**kw), WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: device call {dev:8.3f} ms (min {dev_min:8.3f})  host call (eight planes copied back) {host:8.3f} ms (min {host_min:8.3f})")

    def host_route():
        with contextlib.redirect_stdout(quiet):
            ex = m.export_submap()
        return ref.nav_terrain(ex, m.N, m.Nz, vs, [band], **rk)
    hr, hr_min = median_ms(host_route, 0, HOST_REPEATS, m.sync)
    with contextlib.redirect_stdout(quiet):
        ex, _ = median_ms(m.export_submap, 1, HOST_REPEATS, m.sync)
    lines.append(f"{name}: the host route export_submap + numpy restatement {hr:10.3f} ms (min {hr_min:10.3f}), of that export_submap {ex:8.3f} ms; "
                 f"host route / host call {hr / host:8.1f}x, / device call {hr / dev:8.1f}x")
    # 8 bands in one call against 8 one-band calls
    h8 = m.Nz // 8
    bands8 = [(-(m.Nz // 2) + h8 * b, -(m.Nz // 2) + h8 * b + h8 - 1) for b in range(8)]
    k8 = dict(kw, device=True)
    del k8["bands"]
    s8 = stage_ms(m, kids, lambda: m.nav_terrain(bands=bands8, **k8))
    s1 = stage_ms(m, kids, lambda: [m.nav_terrain(bands=[b], **k8) for b in bands8])
    lines.append(f"{name}: 8 bands of {h8} layers: one call          " + "  ".join(f"{t} {s8[k] * 1e3:8.1f} us" for t, k in STAGES) + f"  sum {sum(s8.values()) * 1e3:8.1f} us")
    lines.append(f"{name}: 8 bands of {h8} layers: 8 one-band calls  " + "  ".join(f"{t} {s1[k] * 1e3:8.1f} us" for t, k in STAGES) + f"  sum {sum(s1.values()) * 1e3:8.1f} us; "
                 f"column walk, one call of 8 bands / the one band above {s8[_lib.K_NAV_TERRAIN_COLUMNS] / st[_lib.K_NAV_TERRAIN_COLUMNS]:5.2f}x")

    def both():
        m.nav_terrain(bands=bands8, **k8)
        torch.cuda.synchronize()

    def each():
        for b in bands8:
            m.nav_terrain(bands=[b], **k8)
        torch.cuda.synchronize()
    w8, _ = median_ms(both, WARMUP, REPEATS, m.sync)
    w1, _ = median_ms(each, WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: 8 bands, wall: one device call {w8:8.3f} ms, 8 device calls {w1:8.3f} ms")
    # the window pass at three sizes
    for ws in (1, 4, 16):
        sw = stage_ms(m, kids[1:2], lambda: m.nav_terrain(device=True, **dict(kw, window=ws * vs, slope_base=ws * vs)))
        lines.append(f"{name}: window pass at window = slope_base = {ws:2d}: {sw[_lib.K_NAV_TERRAIN_WINDOW] * 1e3:8.1f} us ({m.N * m.N} cells, tiles of 32 x 32 with a halo of {ws})")
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_terrain.txt"))
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_nav_terrain.py: medians of {REPEATS} after {WARMUP} warm-up calls (host route: median of {HOST_REPEATS}); one MI355X, one process",
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

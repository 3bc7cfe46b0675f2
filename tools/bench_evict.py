"""Time of brick eviction (tsl_evict.hip, DenseTSDF.evict / restore_bricks) on two maps: the config-2 scene of taichislam_amd/utils/bench_configs.py after 20
frames of the sphere-room stream (512^3 / 2 cm) and the room of the tests (tests/render_view_scenes.py: four 320 x 240 frames, 256^3 / 4 cm).

Per map the half of the bricks on the low-x side of a brick plane is evicted (keep_box) and put back (restore_bricks), so that every repeat starts from the
same content.  Medians of REPEATS after WARMUP:
  the bricks and bytes packed and moved;
  the pack launch and the compaction's launches through the handle's profiler (HIP events around them; a snapshot runs the pack alone, an eviction without a
  payload the compaction alone);
  the whole device call tsl_tsdf_evict_dev into buffers made beforehand (events on the caller's stream around the asynchronous call, and wall time), and
  the host call DenseTSDF.evict with its copy;
  restore, the round trip, and clear_box without a payload;
against two references measured in the same run: a plain hipMemcpyAsync device-to-device of the same number of bytes (packed + moved), and the only route
the library had before: export_submap() + reset() + load_numpy() of the kept voxels.  The round trip is checked byte for byte before anything is timed.
No threshold is set.  Writes the table to --out (default profiles/evict.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import contextlib
import ctypes as C
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

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3
BRICK_BYTES = 4096 * (4 + 1 + 1)
PLANES = ("keys", "tw", "obs", "occ")


def med(v):
    return statistics.median(v), min(v)


def signed(t):
    """a tensor through the signed type of its width (comparisons of the unsigned 16 and 32-bit types are not implemented everywhere)"""
    import torch
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16) if t.element_size() == 2 else t


def same(a, b):
    return all(a[k].shape == b[k].shape and bool((signed(a[k]) == signed(b[k])).all()) for k in PLANES)


def case(lines, name, m):
    import torch
    quiet = io.StringIO()
    dev = torch.device(f"cuda:{m.device}")
    stream = torch.cuda.current_stream(dev)
    keys = m.brick_keys()
    _, bi, _, _ = m.brick_key_ijk(keys)
    bx = int(np.median(bi))
    h = 2 ** 20
    keep = ((16 * bx - m.N // 2, -h, -h), (h, h, h))                  # keep_box: the bricks with bi < bx go
    clear = ((-h, -h, -h), (16 * bx - m.N // 2 - 1, h, h))             # clear_box: the same bricks, wholly inside
    full = m.snapshot_bricks(sid=-1, device=True)
    ev = m.evict(keep_box=keep, device=True)
    E, moved, top = ev["stats"]["selected"], ev["stats"]["moved"], ev["stats"]["bricks_before"]
    assert E == int((bi < bx).sum()) and m.bricks_in_use() == top - E
    assert m.restore_bricks(ev)["restored"] == E and same(m.snapshot_bricks(sid=-1, device=True), full), "round trip"
    nbytes = (E + moved) * BRICK_BYTES
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {m.voxel_scale} m, {top} bricks in use; plane at brick {bx} of the x axis: {E} bricks packed "
                 f"({E * BRICK_BYTES / 1e6:.1f} MB), {moved} moved ({moved * BRICK_BYTES / 1e6:.1f} MB); round trip equal byte for byte")

    # ---- the pack launch and the compaction's launches, each alone, through the profiler
    m.enable_profiling(True)
    pack, compact = [], []
    for i in range(WARMUP + REPEATS):
        m.kernel_time(_lib.K_EVICT)
        snap = m.snapshot_bricks(keep_box=keep, device=True)
        tp, _ = m.kernel_time(_lib.K_EVICT)
        m.evict(keep_box=keep, payload=False)
        tc, _ = m.kernel_time(_lib.K_EVICT)
        m.restore_bricks(snap)
        if i >= WARMUP:
            pack.append(tp); compact.append(tc)
    m.enable_profiling(False)
    (pk, pk_min), (cp, cp_min) = med(pack), med(compact)

    # ---- a plain device-to-device copy of the same number of bytes
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    copy = []
    for i in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        dst.copy_(src)                                               # contiguous, same type, same device: torch issues one hipMemcpyAsync device-to-device
        b.record(stream)
        torch.cuda.synchronize()
        if i >= WARMUP:
            copy.append(a.elapsed_time(b))
    del src, dst
    cy, cy_min = med(copy)
    lines.append(f"{name}: kernels  pack {pk * 1e3:9.1f} us (min {pk_min * 1e3:9.1f})  compact {cp * 1e3:9.1f} us (min {cp_min * 1e3:9.1f})  "
                 f"plain hipMemcpyAsync of {nbytes / 1e6:.1f} MB {cy * 1e3:9.1f} us (min {cy_min * 1e3:9.1f})  (pack + compact) / copy {(pk + cp) / cy:6.2f}x")

    # ---- the whole device call into buffers made beforehand, and restore
    cfg = _lib.EvictCfg()
    cfg.rule, cfg.sid, cfg.release = _lib.EVICT_KEEP_BOX, -1, 1
    for a in range(3):
        cfg.lo[a], cfg.hi[a] = keep[0][a], keep[1][a]
    bufs = {"keys": torch.empty(E, dtype=torch.int32, device=dev), "tw": torch.empty((E, 4096), dtype=torch.int32, device=dev),
            "obs": torch.empty((E, 4096), dtype=torch.int8, device=dev), "occ": torch.empty((E, 4096), dtype=torch.int8, device=dev)}
    st = _lib.EvictStats()
    ev_ms, wall_ms, rs_ms = [], [], []
    for i in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        _lib.check(m.L.tsl_tsdf_evict_dev(m.h, C.byref(cfg), None, 0, *(bufs[k].data_ptr() for k in PLANES), None, E, C.byref(st), stream.cuda_stream))
        b.record(stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert st.selected == E
        rst = _lib.EvictStats()
        _lib.check(m.L.tsl_tsdf_restore_bricks_dev(m.h, *(bufs[k].data_ptr() for k in PLANES), None, E, -1, 0, C.byref(rst), stream.cuda_stream))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert rst.restored == E
        if i >= WARMUP:
            ev_ms.append(a.elapsed_time(b)); wall_ms.append((t1 - t0) * 1e3); rs_ms.append((t2 - t1) * 1e3)
    assert same(m.snapshot_bricks(sid=-1, device=True), full)
    (de, de_min), (dw, dw_min), (rs, rs_min) = med(ev_ms), med(wall_ms), med(rs_ms)
    lines.append(f"{name}: device call tsl_tsdf_evict_dev  events {de:8.3f} ms (min {de_min:8.3f})  wall {dw:8.3f} ms (min {dw_min:8.3f});  "
                 f"tsl_tsdf_restore_bricks_dev wall {rs:8.3f} ms (min {rs_min:8.3f});  round trip {dw + rs:8.3f} ms")

    # ---- the host call with its copy, and clear_box without a payload
    host, clr = [], []
    for i in range(WARMUP + REPEATS):
        m.sync()
        t0 = time.perf_counter()
        hv = m.evict(keep_box=keep)
        t1 = time.perf_counter()
        m.restore_bricks(hv)
        snap = m.snapshot_bricks(clear_box=clear, device=True)
        m.sync(); torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert m.evict(clear_box=clear, payload=False)["stats"]["selected"] == E
        t3 = time.perf_counter()
        m.restore_bricks(snap)
        if i >= WARMUP:
            host.append((t1 - t0) * 1e3); clr.append((t3 - t2) * 1e3)
    assert same(m.snapshot_bricks(sid=-1, device=True), full)
    (ho, ho_min), (cl, cl_min) = med(host), med(clr)
    lines.append(f"{name}: host call DenseTSDF.evict (numpy payload, {E * BRICK_BYTES / 1e6:.1f} MB to the host) {ho:9.3f} ms (min {ho_min:9.3f});  "
                 f"evict(clear_box, payload=False) {cl:8.3f} ms (min {cl_min:8.3f})")

    # ---- the only route without the feature: export_submap() + reset() + load_numpy() of the kept voxels (it keeps the observed voxels only, with obs = 1)
    route = []
    for i in range(HOST_REPEATS):
        m.sync()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            e = m.export_submap()
        kept = ((e["indices"][:, 0].astype(np.int64) + m.N // 2) >> 4) >= bx
        m.reset()
        m.load_numpy(0, e["indices"][kept], e["TSDF"][kept], e["W_TSDF"][kept], e["occupy"][kept], None)
        m.sync()
        route.append((time.perf_counter() - t0) * 1e3)
        assert m.bricks_in_use() <= top - E
        m.reset()
        m.restore_bricks(full)
    ro, ro_min = med(route)
    lines.append(f"{name}: the route without the feature, export_submap + reset + load_numpy of the kept voxels {ro:10.3f} ms (min {ro_min:10.3f}); "
                 f"route / host call {ro / ho:6.1f}x, route / device call {ro / dw:6.1f}x")
    for ln in lines[-5:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evict.txt"))
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_evict.py: medians of {REPEATS} after {WARMUP} warm-up calls (the route without the feature: median of {HOST_REPEATS}); one MI355X, one process",
             "kernels = HIP events around the pack launch / the compaction's launches (tsl_tsdf_prof_query, id TSL_K_EVICT); calls in wall time unless marked events"]
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

"""Time of the depth conditioner (tsl_depth.hip, mapping.DepthConditioner) on 640 x 480 frames of the sphere-room stream with sensor-like noise, batches
of 1 and 8, at the default configuration (radius 2, erode 1) and at the largest halo (radius 4, erode 3).  Medians of REPEATS after WARMUP:
  the device call tsl_depth_condition_dev into buffers made beforehand, HIP events on the caller's stream around the asynchronous call, and wall time;
  the same rules (a) in numpy after a copy to the host (tests/depth_condition_ref.py) and (b) written with torch on the device (padded shifts);
  the per-frame cost beside the steady per-frame time of recast_depth_to_map on the same stream, measured in the same run, and the integration rate of
  level-1 frames (320 x 240, utils.halved_intrinsics) against level-0 frames;
  the share of the peak HBM bandwidth the call reaches, counting one read and one write of every pixel;
  what track_depth does on a noisy frame raw and conditioned (a finding, not a gate).
Kernel times come from a profiler run of its own: `--kernel-loop` only launches (run it under the profiler's kernel trace), `--kernel-stats FILE` appends
the rows of that run's statistics to the table.  Whatever was not measured is written as "not measured".  No threshold is set.  Writes the table to --out
(default profiles/depth_condition.txt) and prints it.  One process; run it under `timeout`."""
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
from taichislam_amd.mapping import DenseTSDF, DepthConditioner
from taichislam_amd.utils import halved_intrinsics
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 3, 21, 3
H, W = 480, 640
PEAK_TBS = 8.0                  # MI355X HBM3E peak, TB/s
CASES = (("default (radius 2, erode 1)", dict(radius=2, erode=1)), ("largest halo (radius 4, erode 3)", dict(radius=4, erode=3)))
NOISE_MM = 6


def med(v):
    return statistics.median(v), min(v)


def frames(n, noise=NOISE_MM):
    return np.stack([d for _, _, d in syn.sphere_room_stream(n, noise_mm=noise)])


def dev_i16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def cfg_of(n, levels=0, **kw):
    import depth_condition_ref as ref
    c = dict(ref.DEFAULTS, levels=levels, **kw)
    return _lib.DepthCfg(n, H, W, c["d_min_mm"], c["d_max_mm"], c["min_support"], c["erode"], c["radius"], c["flags"], c["levels"], c["min_valid"], 0)


def torch_condition(d16, tol, ws, wr, c):
    """the status and smoothing rules with torch on the device: int64 planes, padded shifts"""
    import torch
    import torch.nn.functional as F
    P = 4
    d = d16.to(torch.int64) & 0xffff
    n, h, w = d.shape

    def sh(a, dy, dx):
        return F.pad(a, (P, P, P, P), value=0)[:, P + dy:P + dy + h, P + dx:P + dx + w]
    tol_t = torch.from_numpy(tol.astype(np.int64)).cuda()
    rq_t = torch.clamp((16 << 16) // tol_t, max=65535)
    wr_t = torch.from_numpy(wr.astype(np.int64)).cuda()
    hole = d == 0
    rng = ~hole & ((d < c["d_min_mm"]) | (d > c["d_max_mm"]))
    cand = (~hole & ~rng).to(torch.int64)
    t = tol_t[d >> 8]
    cnt = torch.zeros_like(d)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                cnt += sh(cand, dy, dx) * ((sh(d, dy, dx) - d).abs() <= t)
    sparse = (cand == 1) & (cnt < c["min_support"])
    seed = (sparse | hole if c["flags"] & 1 else sparse).to(torch.int64)
    e = c["erode"]
    near = torch.zeros_like(d)
    for dy in range(-e, e + 1):
        for dx in range(-e, e + 1):
            near += sh(seed, dy, dx)
    edge = (cand == 1) & ~sparse & (near > 0) & (e > 0)
    status = torch.zeros_like(d)
    status[hole], status[rng], status[sparse], status[edge] = 1, 2, 3, 4
    kept = (status == 0).to(torch.int64)
    num, den = torch.zeros_like(d), torch.zeros_like(d)
    r = c["radius"]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            diff = sh(d, dy, dx) - d
            a = diff.abs()
            m = kept * sh(kept, dy, dx) * (a <= t)
            qi = torch.clamp((a * rq_t[d >> 8]) >> 16, max=16)
            wgt = m * int(ws[abs(dy), abs(dx)]) * wr_t[qi]
            num += wgt * diff
            den += wgt
    off = torch.div(2 * num + den, torch.clamp(2 * den, min=1), rounding_mode="floor")
    out = torch.where(kept == 1, torch.clamp(d + off, 1, 65535), torch.zeros_like(d))
    return out, status


def time_dev_call(dc, cfg, d, out, st, cnt, lv):
    import torch
    stream = torch.cuda.current_stream()
    ev, wall = [], []
    lp = [a.data_ptr() for a in lv] + [None] * (3 - len(lv))
    for i in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record(stream)
        _lib.check(dc.L.tsl_depth_condition_dev(dc.h, C.byref(cfg), d.data_ptr(), out.data_ptr(), st.data_ptr(), cnt.data_ptr(), *lp, stream.cuda_stream))
        b.record(stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= WARMUP:
            ev.append(a.elapsed_time(b) * 1e3); wall.append((t1 - t0) * 1e6)
    return med(ev), med(wall)


def buffers(n, levels=0):
    import torch
    return (torch.empty((n, H, W), dtype=torch.int16, device="cuda"), torch.empty((n, H, W), dtype=torch.uint8, device="cuda"),
            torch.empty((n, 5), dtype=torch.int64, device="cuda"), [torch.empty((n, H >> l, W >> l), dtype=torch.int16, device="cuda") for l in range(1, levels + 1)])


def kernel_loop(dc):
    import torch
    for n in (1, 8):
        d = dev_i16(frames(n))
        for _, kw in CASES:
            out, st, cnt, lv = buffers(n, 1)
            cfg = cfg_of(n, 1, **kw)
            for _ in range(WARMUP + REPEATS):
                _lib.check(dc.L.tsl_depth_condition_dev(dc.h, C.byref(cfg), d.data_ptr(), out.data_ptr(), st.data_ptr(), cnt.data_ptr(), lv[0].data_ptr(), None, None,
                                                        torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()


def integration_rate(K, imgs, poses, what):
    import torch
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(K)
    warm = 8
    for i in range(warm):
        m.recast_depth_to_map(*poses[i], imgs[i], None)
    m.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, len(imgs)):
        m.recast_depth_to_map(*poses[i], imgs[i], None)
    m.sync()
    us = (time.perf_counter() - t0) * 1e6 / (len(imgs) - warm)
    return us, f"{what}: {us:8.1f} us per frame over {len(imgs) - warm} frames after {warm} ({m.bricks_in_use()} bricks)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_condition.txt"))
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    import torch
    import depth_condition_ref as ref
    dc = DepthConditioner(0)
    if args.kernel_loop:
        return kernel_loop(dc)
    if args.kernel_stats:
        rows = [ln.strip() for ln in open(args.kernel_stats) if "k_depth" in ln or ln.startswith('"Name"')] if os.path.exists(args.kernel_stats) else []
        with open(args.out, "a") as f:
            f.write("kernel times, a profiler run of its own (kernel trace with statistics over tools/bench_depth_condition.py --kernel-loop; levels = 1; ns):\n")
            f.write(("\n".join("  " + r for r in rows) if rows else "  not measured") + "\n")
        return
    lines = [f"tools/bench_depth_condition.py: medians of {REPEATS} after {WARMUP} warm-up calls (numpy: median of {HOST_REPEATS}); one MI355X, one process; "
             f"640 x 480 frames of the sphere-room stream, noise_mm = {NOISE_MM}"]
    per_frame = {}
    for n in (1, 8):
        raw = frames(n)
        d = dev_i16(raw)
        for name, kw in CASES:
            c = dict(ref.DEFAULTS, **kw)
            out, st, cnt, _ = buffers(n)
            (ev, ev_min), (wl, wl_min) = time_dev_call(dc, cfg_of(n, **kw), d, out, st, cnt, [])
            want = ref.condition_np(raw, dc.tol, dc.ws, dc.wr, **kw)
            ok = np.array_equal(out.cpu().numpy().view(np.uint16), want["depth"]) and np.array_equal(st.cpu().numpy(), want["status"]) and \
                np.array_equal(cnt.cpu().numpy(), want["counts"])
            gbs = n * H * W * 4 / (ev * 1e-6) / 1e9
            per_frame[(n, name)] = ev / n
            lines.append(f"n = {n}, {name}: tsl_depth_condition_dev events {ev:8.1f} us (min {ev_min:8.1f}), wall {wl:8.1f} us (min {wl_min:8.1f}); per frame {ev / n:7.1f} us; "
                         f"{gbs:7.1f} GB/s of depth read + written = {100 * gbs / (PEAK_TBS * 1e3):5.2f} % of {PEAK_TBS} TB/s; equal to the restatement: {ok}; "
                         f"kept {int(want['counts'][:, 0].sum())} of {n * H * W}")
            (e3, _), _ = time_dev_call(dc, cfg_of(n, 3, **kw), d, *buffers(n, 3))
            lines.append(f"n = {n}, {name}: with three levels {e3:8.1f} us ({e3 - ev:+7.1f} us for the three halving launches)")
            try:
                host = []
                for _ in range(HOST_REPEATS):
                    t0 = time.perf_counter()
                    ref.condition_np(d.cpu().numpy().view(np.uint16), dc.tol, dc.ws, dc.wr, **kw)
                    host.append((time.perf_counter() - t0) * 1e6)
                to, tst = torch_condition(d, dc.tol, dc.ws, dc.wr, c)
                same = bool((to == (out.to(torch.int64) & 0xffff)).all()) and bool((tst == st.to(torch.int64)).all())
                tt = []
                for i in range(2 + 5):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    torch_condition(d, dc.tol, dc.ws, dc.wr, c)
                    torch.cuda.synchronize()
                    if i >= 2:
                        tt.append((time.perf_counter() - t0) * 1e6)
                lines.append(f"n = {n}, {name}: (a) numpy after a copy to the host {med(host)[0]:10.1f} us = {med(host)[0] / wl:7.1f}x the call; (b) torch on the device "
                             f"{med(tt)[0]:10.1f} us = {med(tt)[0] / wl:7.1f}x the call (equal to the kernel: {same})")
            except Exception as ex:                                  # noqa: BLE001
                lines.append(f"n = {n}, {name}: numpy / torch restatements not measured ({type(ex).__name__}: {ex})")
    one, eight = per_frame[(1, CASES[0][0])], 8 * per_frame[(8, CASES[0][0])]
    lines.append(f"launch-sized? no: one default frame takes {one:.1f} us, several empty launches' worth, at well under 1 % of the peak bandwidth: the stages' arithmetic "
                 f"and LDS traffic bound it, not the bytes.  One frame is 150 workgroups on 256 CUs, so eight frames cost {eight / one:4.2f}x one frame, not 8x")
    # ---- integration beside it: level-0 and level-1 frames into a config-2 map
    try:
        nf = 48
        stream = list(syn.sphere_room_stream(nf, noise_mm=0))
        poses = [(R, T) for R, T, _ in stream]
        lv0 = [dev_i16(d) for _, _, d in stream]
        r = dc.condition(dev_i16(np.stack([d for _, _, d in stream])), levels=1)
        lv1 = [x.contiguous() for x in r["levels"][0]]
        us0, l0 = integration_rate(syn.K_DEPTH, lv0, poses, "recast_depth_to_map, 640 x 480 device frames (level 0), config-2 map")
        us1, l1 = integration_rate(halved_intrinsics(syn.K_DEPTH, 1), lv1, poses, "recast_depth_to_map, 320 x 240 level-1 frames, halved intrinsics, config-2 map")
        lines += [l0, l1, f"level-1 frames integrate {us0 / us1:5.2f}x as fast as level-0 frames"]
        for (n, name), us in per_frame.items():
            lines.append(f"conditioning per frame / integration per frame, n = {n}, {name}: {us:7.1f} us / {us0:7.1f} us = {us / us0:5.2f}")
    except Exception as ex:                                          # noqa: BLE001
        lines.append(f"integration rates not measured ({type(ex).__name__}: {ex})")
    # ---- a finding: track_depth on a noisy frame, raw against conditioned
    try:
        m = DenseTSDF(**C2)
        m.set_dep_camera_intrinsic(syn.K_DEPTH)
        for R, T, d in syn.sphere_room_stream(12):
            m.recast_depth_to_map(R, T, d, None)
        m.sync()
        Rt, Tt = syn.camera_pose(6)
        for noise in (10, 40):
            img = syn.sphere_room_depth(Rt, Tt, noise_mm=noise, seed=99)
            cond = dc.condition(img)
            res = []
            for what, im in (("raw", img), ("conditioned", cond["depth"])):
                R1, T1, info = m.track_depth(im, Rt, Tt + np.array([0.01, 0.0, 0.0]))
                res.append(f"{what}: |T - T_true| {1e3 * np.linalg.norm(T1 - Tt):6.2f} mm, status {info['status']}, {info['iterations']} linearisations")
            lines.append(f"track_depth, frame 6 with noise_mm = {noise}, start 10 mm off, kept {int(cond['counts'][0])} of {H * W}: " + "; ".join(res))
    except Exception as ex:                                          # noqa: BLE001
        lines.append(f"track_depth raw against conditioned: not measured ({type(ex).__name__}: {ex})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

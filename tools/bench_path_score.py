"""Time of the path scoring (tsl_path_score.hip, DenseTSDF.score_paths) on two maps: the room of the frontier tests (tests/render_view_scenes.py: four
320 x 240 frames, 256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames of the sphere-room stream (512^3 / 2 cm),
each with an ESDF of reach 2 m.

Per map: 1 024 and 16 384 paths of K = 17 waypoints -- walks of 15 cm steps that start in observed free space -- at sub = 4 (S = 65 samples, two chunks
of a wave, the second with one sample), at sub = 1 (S = 17, 47 of 64 lanes idle) and at sub = 16 (S = 257, five chunks), trilinear, radius 0.25 m, unknown and outside blocking.  Medians of
REPEATS after WARMUP: the kernel through the handle's profiler (HIP events around the launch) and the device call in wall time (torch tensors in and out,
ending in a synchronise), each with and without the stop flag.  Baseline, what a caller does without this kernel: torch builds the same sample positions
on the device, query_esdf (device form) answers them, torch reduces distances and statuses to first_stop, the three counts and min_dist; same wall clock.
Both ways are compared (first_stop, counts, min_dist as bits) before anything is timed.  No threshold is set.  Writes the table to --out (default
profiles/path_score.txt) and prints it.  --counters runs only the kernel, 16 384 paths at S = 65 on the room, a few times: the run to put under a counter
collection.  One process; run it under `timeout`."""
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

WARMUP, REPEATS = 3, 15
K = 17
RADIUS, MARGIN = 0.25, 0.15
PATHS = (1024, 16384)
SUBS = (4, 1, 16)                       # S = 65 and 17 are the cases compared; S = 257 shows the stop flag where a path has chunks to skip


def median_ms(fn, sync):
    ms = []
    for i in range(WARMUP + REPEATS):
        sync()
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def kernel_ms(m, fn):
    """median of the profiler's time of the path-score kernel for one call of fn"""
    rows = []
    m.enable_profiling(True, only=[_lib.K_PATH_SCORE])
    for i in range(WARMUP + REPEATS):
        m.kernel_time(_lib.K_PATH_SCORE)
        fn()
        m.sync()
        t, _ = m.kernel_time(_lib.K_PATH_SCORE)
        if i >= WARMUP:
            rows.append(t)
    m.enable_profiling(False)
    return statistics.median(rows)


def walks(m, n, rng):
    """n walks of K waypoints, 15 cm per step with a heading that drifts, from observed voxels at least 0.4 m from a surface"""
    idx, val = m.export_esdf()
    free = idx[val > 0.4].astype(np.float64) * m.voxel_scale
    wp = np.empty((n, K, 3))
    wp[:, 0] = free[rng.integers(0, len(free), n)]
    head = rng.normal(size=(n, 3))
    for k in range(1, K):
        head = head / np.linalg.norm(head, axis=1, keepdims=True) + 0.3 * rng.normal(size=(n, 3))
        wp[:, k] = wp[:, k - 1] + 0.15 * head / np.linalg.norm(head, axis=1, keepdims=True)
    return wp.astype(np.float32)


def torch_way(m, wp_t, sub, torch):
    """the caller's way without the kernel: sample positions, query_esdf, reductions -- all on the device"""
    n = wp_t.shape[0]
    S = (K - 1) * sub + 1
    j = np.arange(S)
    seg = torch.from_numpy(j // sub).to(wp_t.device)
    nxt = torch.from_numpy(np.minimum(j // sub + 1, K - 1)).to(wp_t.device)
    t = torch.from_numpy(((j % sub).astype(np.float32) / np.float32(sub)).astype(np.float32)).to(wp_t.device)[None, :, None]
    whole = torch.from_numpy(j % sub == 0).to(wp_t.device)[None, :, None]

    def run():
        a, b = wp_t[:, seg], wp_t[:, nxt]
        p = torch.where(whole, a, a + t * (b - a))
        d, _, st = m.query_esdf(p.reshape(-1, 3), interpolate=True, gradient=False, refresh=False)
        d, st = d.view(n, S), st.view(n, S)
        ok = st == 0
        hit, unk, outs = ok & (d < RADIUS), st == 1, st == 2
        jj = torch.arange(S, device=d.device)[None, :]
        first = torch.where(hit | unk | outs, jj, S).min(1).values
        first = torch.where(first == S, -1, first)
        md = torch.where(ok, d, float("inf")).min(1).values
        return first, hit.sum(1), unk.sum(1), outs.sum(1), md
    return run


def case(lines, name, m, torch):
    rng = np.random.default_rng(5)
    first_line = len(lines)
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {m.voxel_scale} m, {m.bricks_in_use()} bricks, ESDF reach 2 m; paths of {K} waypoints, radius {RADIUS} m")
    per_sample = {}
    for n in PATHS:
        wp = walks(m, n, rng)
        wp_t = torch.from_numpy(wp).cuda()
        for sub in SUBS:
            S = (K - 1) * sub + 1
            kw = dict(margin=MARGIN, sub=sub, refresh=False)
            base = torch_way(m, wp_t, sub, torch)
            got = {k: v.cpu().numpy() for k, v in m.score_paths(wp_t, RADIUS, **kw).items()}
            first, nh, nu, no, md = (x.cpu().numpy() for x in base())
            assert np.array_equal(got["first_stop"], first) and np.array_equal(got["n_hit"], nh) and np.array_equal(got["n_unknown"], nu)
            assert np.array_equal(got["n_outside"], no) and np.array_equal(got["min_dist"].view(np.uint32), md.view(np.uint32))
            blocked = (first >= 0).mean()
            res = {}
            for stop in (False, True):
                def call():
                    m.score_paths(wp_t, RADIUS, stop=stop, **kw)
                    torch.cuda.synchronize()
                res[stop] = (kernel_ms(m, call), median_ms(call, m.sync))

            def base_call():
                base()
                torch.cuda.synchronize()
            bt, bt_min = median_ms(base_call, m.sync)
            per_sample[(n, sub)] = res[False][0] * 1e6 / (n * S)
            for stop in (False, True):
                kt, (ct, ct_min) = res[stop]
                lines.append(f"{name}: {n:6d} paths  S {S:3d}  stop {'on ' if stop else 'off'}  kernel {kt * 1e3:9.1f} us ({kt * 1e6 / (n * S):7.3f} ns / sample)  "
                             f"device call {ct:8.3f} ms (min {ct_min:8.3f})  torch + query_esdf {bt:8.3f} ms (min {bt_min:8.3f})  ratio {bt / ct:6.2f}x")
            lines.append(f"{name}: {n:6d} paths  S {S:3d}  both ways equal (first_stop, counts, min_dist); {100 * blocked:5.1f} % of the paths block, "
                         f"median first_stop of those {int(np.median(first[first >= 0])) if blocked else -1}")
        lines.append(f"{name}: {n:6d} paths  kernel time per sample, stop off: S = 17 {per_sample[(n, 1)]:7.3f} ns, S = 65 {per_sample[(n, 4)]:7.3f} ns, "
                     f"S = 17 / S = 65 {per_sample[(n, 1)] / per_sample[(n, 4)]:5.2f}x")
    for ln in lines[first_line:]:
        print(ln, flush=True)


def room():
    import render_view_scenes as rv
    from util import SMALL
    Kc, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(Kc)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.update_esdf(max_dist=2.0)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_score.txt"))
    ap.add_argument("--counters", action="store_true")
    args = ap.parse_args()
    import torch
    m = room()
    if args.counters:
        wp_t = torch.from_numpy(walks(m, 16384, np.random.default_rng(5))).cuda()
        for _ in range(5):
            m.score_paths(wp_t, RADIUS, margin=MARGIN, sub=4, refresh=False)
        torch.cuda.synchronize()
        return
    lines = [f"tools/bench_path_score.py: medians of {REPEATS} after {WARMUP} warm-up calls; one MI355X, one process",
             "kernel = HIP events around the launch (tsl_tsdf_prof_query); calls in wall time around a device synchronise, tensors on the device on both sides",
             "ratio = the caller's way without the kernel (torch sample positions + query_esdf device form + torch reductions) / the device call"]
    case(lines, "room", m, torch)
    del m
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(20):
        m.recast_depth_to_map(R, T, d, None)
    m.update_esdf(max_dist=2.0)
    case(lines, "config-2", m, torch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

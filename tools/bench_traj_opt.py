"""Time of the B-spline trajectory descent (tsl_traj_opt.hip, DenseTSDF.traj_optimize) on two maps: the room of the frontier tests
(tests/render_view_scenes.py: four 320 x 240 frames, 256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames of the
sphere-room stream (512^3 / 2 cm), each with an ESDF of reach 2 m.

Per map: 1, 64, 1 024 and 16 384 trajectories of K = 24 control points -- walks of 10 cm steps that start in observed free space 0.1 to 0.6 m from a
surface -- at sub = 4 (S = 85 samples: two chunks of a wave, the second with 21 samples, so 43 of 128 lane slots idle), clearance 0.4 m, 50 iterations with
the defaults of traj_optimize.  Medians of REPEATS after WARMUP of HIP events around the asynchronous device call (torch tensors in and out, nothing
waits in between); the call with iters = 0 is timed too, so that (t50 - t0) / 50 is the time of one iteration.  Baseline, the loop the call replaces,
written with torch on the device: per iteration a basis matmul for the sample positions, query_esdf (device form, with gradient), index_add_ of the
weighted sample gradients onto the control points, the smoothness stencil and the same momentum update, in f32 without the fixed point -- so the two ways
agree to rounding, not bit for bit: after ONE iteration they are compared (control points within 1e-5 m) before anything is timed.  No threshold is set.
Writes the table to --out (default profiles/traj_opt.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import bspline_basis
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS = 2, 7
K, SUB, ITERS = 24, 4, 50
CLEAR = 0.4
SIZES = (1, 64, 1024, 16384)
OPT = dict(w_collision=1.0, w_smooth=1.0, step=0.05, momentum=0.8, fix_ends=3)


def event_ms(fn, torch, repeats=REPEATS):
    """median and least time of fn between two events on the current stream"""
    ms = []
    for i in range(WARMUP + repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def walks(m, n, rng):
    """n control polygons of K points, 10 cm per step with a heading that drifts, from observed voxels 0.1 to 0.6 m from a surface"""
    idx, val = m.export_esdf()
    near = idx[(val > 0.1) & (val < 0.6)].astype(np.float64) * m.voxel_scale
    c = np.empty((n, K, 3))
    c[:, 0] = near[rng.integers(0, len(near), n)]
    head = rng.normal(size=(n, 3))
    for k in range(1, K):
        head = head / np.linalg.norm(head, axis=1, keepdims=True) + 0.3 * rng.normal(size=(n, 3))
        c[:, k] = c[:, k - 1] + 0.10 * head / np.linalg.norm(head, axis=1, keepdims=True)
    return c.astype(np.float32)


def torch_loop(m, c_t, iters, max_move, torch):
    """the loop the call replaces: every step on the device, several launches per iteration"""
    n = c_t.shape[0]
    S = (K - 3) * SUB + 1
    j = np.arange(S)
    seg = np.minimum(j // SUB, K - 4)
    w = bspline_basis(SUB)[j - seg * SUB]                             # [S, 4]
    B = np.zeros((S, K), np.float32)
    for i in range(4):
        B[j, seg + i] = w[:, i]
    dev = c_t.device
    B_t, w_t = torch.from_numpy(B).to(dev), torch.from_numpy(w).to(dev)
    rows = [torch.from_numpy(seg + i).to(dev) for i in range(4)]
    lo, hi = OPT["fix_ends"], K - OPT["fix_ends"]

    def run():
        c = c_t.clone()
        v = torch.zeros_like(c)
        for _ in range(iters):
            p = torch.matmul(B_t, c)                                  # [n, S, 3]
            d, g, st = m.query_esdf(p.reshape(-1, 3), interpolate=True, gradient=True, refresh=False)
            cl = torch.clamp(CLEAR - d, max=1024.0)
            pen = (st == 0) & (cl > 0)
            Gp = (torch.where(pen, -2.0 * cl, 0.0)[:, None] * g).view(n, S, 3)
            gc = torch.zeros_like(c)
            for i in range(4):
                gc.index_add_(1, rows[i], w_t[None, :, i:i + 1] * Gp)
            a = c[:, :-2] - 2.0 * c[:, 1:-1] + c[:, 2:]
            gs = torch.zeros_like(c)
            gs[:, :-2] += 2.0 * a
            gs[:, 1:-1] -= 4.0 * a
            gs[:, 2:] += 2.0 * a
            v[:, lo:hi] = torch.clamp(OPT["momentum"] * v[:, lo:hi] - OPT["step"] * (OPT["w_collision"] * gc[:, lo:hi] + OPT["w_smooth"] * gs[:, lo:hi]),
                                      -max_move, max_move)
            c[:, lo:hi] += v[:, lo:hi]
        return c
    return run


def case(lines, name, m, torch):
    rng = np.random.default_rng(5)
    first_line = len(lines)
    S = (K - 3) * SUB + 1
    chunks = (S + 63) // 64
    max_move = 0.5 * m.voxel_scale
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {m.voxel_scale} m, {m.bricks_in_use()} bricks, ESDF reach 2 m; {K} control points, sub {SUB}: S = {S} samples "
                 f"in {chunks} chunks of 64 lanes, {100.0 * (chunks * 64 - S) / (chunks * 64):.1f} % of the lane slots idle; clearance {CLEAR} m, {ITERS} iterations")
    for n in SIZES:
        c_t = torch.from_numpy(walks(m, n, rng)).cuda()
        kw = dict(sub=SUB, refresh=False, **OPT)
        one = m.traj_optimize(c_t, CLEAR, iters=1, **kw)["ctrl"]
        diff = (one - torch_loop(m, c_t, 1, max_move, torch)()).abs()
        diff = float(diff[torch.isfinite(diff)].max())
        assert diff < 1e-5, diff
        end = {k: v.cpu().numpy() for k, v in m.traj_optimize(c_t, CLEAR, iters=ITERS, **kw).items()}
        start = {k: v.cpu().numpy() for k, v in m.traj_linearize(c_t, CLEAR, sub=SUB, gradients=False, refresh=False).items()}
        t50, t50_min = event_ms(lambda: m.traj_optimize(c_t, CLEAR, iters=ITERS, **kw), torch)
        t0, _ = event_ms(lambda: m.traj_optimize(c_t, CLEAR, iters=0, **kw), torch)
        loop = torch_loop(m, c_t, ITERS, max_move, torch)
        bt, bt_min = event_ms(loop, torch, repeats=3 if n >= 16384 else REPEATS)
        lines.append(f"{name}: {n:6d} trajectories  traj_optimize {t50:9.3f} ms (min {t50_min:9.3f}; iters = 0: {t0:7.3f} ms; per iteration {(t50 - t0) / ITERS * 1e3:9.2f} us, "
                     f"{(t50 - t0) / ITERS * 1e6 / (n * S):8.2f} ns / sample)  torch loop {bt:10.3f} ms (min {bt_min:10.3f})  ratio {bt / t50:7.2f}x")
        lines.append(f"{name}: {n:6d} trajectories  after one iteration both ways agree within {diff:.2e} m; penalised at the start {int((start['n_pen'] > 0).sum())}, "
                     f"at the end {int((end['n_pen'] > 0).sum())}; with unknown samples at the end {int((end['n_unknown'] > 0).sum())}")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_opt.txt"))
    args = ap.parse_args()
    import torch
    lines = [f"tools/bench_traj_opt.py: medians of {REPEATS} after {WARMUP} warm-up calls (the torch loop at 16 384: of 3); one MI355X, one process",
             "times = HIP events on the current stream around the asynchronous device call (tensors on the device on both sides, no host wait in between)",
             "ratio = the loop the call replaces (torch: basis matmul + query_esdf device form with gradient + index_add_ + update, per iteration) / traj_optimize"]
    m = room()
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

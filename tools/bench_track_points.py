"""Time of scan-to-model alignment (tsl_align_points.hip, k_align_points_linearize) on two maps: the room of the tests (tests/track_scenes.py: six 320 x 240
frames, 256^3 / 4 cm) with the spherical scan of tests/track_points_scenes.py (5760 points), and the config-2 scene (512^3 / 2 cm, 20 frames of the
synthetic room stream) with frame 10 (640 x 480) back-projected into a cloud of 307 200 points, at a pose 1 cm / 0.5 deg off its own.

Per map, at point strides 1 and 8, medians of REPEATS after WARMUP: the kernel through the handle's profiler (HIP events around the launch) -- with the
sums, counts only (what the gathers alone cost) and with the per-point outputs -- and the wall time of the host call (copy of the cloud, launch, copy back, wait).  The kernel time per
visited point is set against k_align_linearize per visited pixel on the same map and pose (image strides 1 and 3; on the config-2 map the cloud at
stride 1 is the image's own pixels, so the two kernels sample the same points).  Then a whole default track_points against a whole default
track_depth, in wall time.  On config 2 the cloud's integers are compared with the image's before anything is timed.  No threshold is set.  Writes the table to --out (default profiles/track_points.txt) and prints it.  One process; run it under `timeout`."""
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

WARMUP, REPEATS = 3, 7
FRAMES, TRACKED = 20, 10
WIDE = dict(d_min=1e-3, d_max=1e3)


def off_pose(R, T, metres=0.01, deg=0.5):
    th = np.deg2rad(deg)
    a = np.array([0.36, -0.48, 0.8])
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return (np.eye(3) + np.sin(th) * S + (1.0 - np.cos(th)) * (S @ S)) @ R, T + metres * np.array([0.6, 0.64, -0.48])


def back_project(depth, K):
    """f32 [h * w, 3]: every pixel with the f32 expressions of k_align_linearize (a pixel without depth becomes the origin, which the range gate drops)"""
    F = np.float32
    h, w = depth.shape
    fx, fy, cx, cy = (F(K[i]) for i in (0, 4, 2, 5))
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dep = depth.astype(F) / F(1000.0)
    return np.stack([(ii.astype(F) - cx) * dep / fx, (jj.astype(F) - cy) * dep / fy, dep], -1).reshape(-1, 3).astype(F)


def kernel_us(m, kid, fn):
    """median and minimum of the profiler's time of one launch of kernel `kid` in one call of fn, microseconds"""
    rows = []
    m.enable_profiling(True, only=[kid])
    for i in range(WARMUP + REPEATS):
        m.kernel_time(kid)                                 # a query clears the total
        fn()
        m.sync()
        t, launches = m.kernel_time(kid)
        assert launches == 1, launches
        if i >= WARMUP:
            rows.append(t * 1e3)
    m.enable_profiling(False)
    return statistics.median(rows), min(rows)


def wall_ms(m, fn):
    rows = []
    for i in range(WARMUP + REPEATS):
        m.sync()
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            rows.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(rows), min(rows)


def scene_room():
    import track_points_scenes as tps
    import track_scenes as ts
    from util import SMALL
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(ts.intrinsics())
    for R, T, d in ts.map_frames():
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    _, _, depth = ts.tracked_frame()
    R, T = ts.perturbed_poses()[0]
    return "room 256^3 / 4 cm, spherical scan", m, np.array(tps.scan()), depth, ts.intrinsics(), R, T, {}


def scene_c2():
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    frames = list(syn.sphere_room_stream(FRAMES))
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    Rt, Tt, depth = frames[TRACKED]
    R, T = off_pose(Rt, Tt)
    return "config 2 512^3 / 2 cm, frame %d as a cloud" % TRACKED, m, back_project(depth, syn.K_DEPTH), depth, syn.K_DEPTH, R, T, WIDE


def run(scene, lines):
    import torch
    name, m, cloud, depth, K, R, T, gates = scene
    dev = torch.from_numpy(cloud).cuda()
    dev_depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).cuda()
    n = cloud.shape[0]
    lines.append(f"{name}: {n} points, image {depth.shape[1]} x {depth.shape[0]}, {m.bricks_in_use()} bricks")
    # on config 2 the cloud is the image
    if gates:
        img, pts = m.align_linearize(depth, R, T, K=K), m.align_points_linearize(cloud, R, T, **gates)
        keep = [i for i in range(33) if i != 29]
        assert np.array_equal(img["sums"][keep], pts["sums"][keep]), "the cloud does not restate the image"
    lines.append(f"  {'':34s}{'visited':>9s}{'used':>9s}{'kernel us':>11s}{'min':>8s}{'ns/sample':>11s}")

    def row(label, visited, used, us):
        lines.append(f"  {label:34s}{visited:9d}{used:9d}{us[0]:11.2f}{us[1]:8.2f}{1e3 * us[0] / max(visited, 1):11.3f}")

    for stride in (1, 8):
        s = m.align_points_linearize(cloud, R, T, stride=stride, **gates)
        v = -(-n // stride)
        for label, kw in (("", {}), (", counts only", dict(counts_only=True)), (", per-point outputs", dict(per_point=True))):
            row(f"points stride {stride}{label}", v, s["n_used"], kernel_us(m, _lib.K_ALIGN_POINTS, lambda: m.align_points_linearize(dev, R, T, stride=stride, device=True, **kw, **gates)))
    for stride in (1, 3):
        s = m.align_linearize(depth, R, T, K=K, stride=stride)
        v = -(-depth.shape[0] // stride) * -(-depth.shape[1] // stride)
        for label, kw in (("", {}), (", counts only", dict(counts_only=True))):
            row(f"image stride {stride}{label}", v, s["n_used"], kernel_us(m, _lib.K_ALIGN, lambda: m.align_linearize(dev_depth, R, T, K=K, stride=stride, device=True, **kw)))
    lines.append(f"  {'wall time of a call':34s}{'':18s}{'median ms':>11s}{'min':>8s}")

    def wrow(label, ms):
        lines.append(f"  {label:34s}{'':18s}{ms[0]:11.4f}{ms[1]:8.4f}")

    for stride in (1, 8):
        wrow(f"points stride {stride}, host form", wall_ms(m, lambda: m.align_points_linearize(cloud, R, T, stride=stride, **gates)))
        wrow(f"points stride {stride}, host form, per point", wall_ms(m, lambda: m.align_points_linearize(cloud, R, T, stride=stride, per_point=True, **gates)))
    wrow("image stride 1, host form", wall_ms(m, lambda: m.align_linearize(depth, R, T, K=K)))
    info = {}

    def track_points(x):
        info["p"] = m.track_points(x, R, T, **gates)

    def track_depth(x):
        info["d"] = m.track_depth(x, R, T, K=K)

    wrow("track_points, default levels", wall_ms(m, lambda: track_points(cloud)))
    wrow("track_points, device cloud", wall_ms(m, lambda: track_points(dev)))
    wrow("track_depth, default levels", wall_ms(m, lambda: track_depth(depth)))
    wrow("track_depth, device image", wall_ms(m, lambda: track_depth(dev_depth)))
    for k, what in (("p", "track_points"), ("d", "track_depth")):
        inf = info[k][2]
        lines.append(f"  {what}: status {inf['status']}, {inf['iterations']} linearisations, used per linearisation {[r['n_used'] for r in inf['records']]}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_points.txt"))
    args = ap.parse_args()
    lines = [f"tools/bench_track_points.py: medians of {REPEATS} after {WARMUP}; kernel times by HIP events around the launch, wall times around the call", ""]
    for scene in (scene_room, scene_c2):
        run(scene(), lines)
    text = "\n".join(lines)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

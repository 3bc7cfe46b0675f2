"""Time of the depth-and-colour alignment (tsl_align_rgbd.hip, k_align_rgbd_linearize) beside the depth-only alignment (k_align_linearize) on the same
samples, on two textured maps: the C2 scene (512^3 / 2 cm, 20 frames of the synthetic room stream with a synthetic texture, a 640 x 480 frame at a pose
1 cm / 0.5 deg off its own) and the box room of the tests (256^3 / 4 cm, six 320 x 240 frames).  Per scene and stride: the kernel alone (HIP events
around the launch: tsl_tsdf_prof_query), median and minimum of 7 after a warm-up, with the sums and counts only -- counts only leaves both sets of
products and both reductions out, so the difference is what the two reductions cost and the rest what the 24 gathers cost; torch events around the
asynchronous device call; a whole default track_rgbd beside track_depth in wall time.  One process; run it under `timeout`.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from taichislam_amd import _lib
from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import synthetic as syn

C2 = dict(map_scale=[10.24, 10.24], voxel_scale=0.02, num_voxel_per_blk_axis=16, max_ray_length=5.0, min_ray_length=0.3, internal_voxels=10, recast_step=2,
          texture_enabled=True)
ROOM = dict(C2, voxel_scale=0.04)
FRAMES, WARMUP, ITERS, TRACKED = 20, 3, 7, 10
BOX_LO, BOX_HI = np.array([-2.2, -2.0, -0.8]), np.array([2.6, 2.4, 0.9])


def off_pose(R, T, metres=0.01, deg=0.5):
    th = np.deg2rad(deg)
    a = np.array([0.36, -0.48, 0.8])
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return (np.eye(3) + np.sin(th) * S + (1.0 - np.cos(th)) * (S @ S)) @ R, T + metres * np.array([0.6, 0.64, -0.48])


def colour_of(p):
    """uint8 [..., 3]: an analytic texture over space, wavelengths of 0.6 to 1.1 m"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    c = np.stack([0.5 + 0.2 * np.sin(2.0 * np.pi * (x + y) / 0.9) + 0.2 * np.sin(2.0 * np.pi * z / 0.7),
                  0.5 + 0.2 * np.sin(2.0 * np.pi * (y - x) / 1.1 + 1.0) + 0.2 * np.sin(2.0 * np.pi * (z + x) / 0.8),
                  0.5 + 0.2 * np.sin(2.0 * np.pi * (x + z) / 1.0 + 2.0) + 0.2 * np.sin(2.0 * np.pi * y / 0.6)], -1)
    return np.clip(np.rint(255.0 * c), 0, 255).astype(np.uint8)


def frame_colour(R, T, depth, K):
    """the texture at the point every pixel of a depth image (uint16 millimetres) sees"""
    h, w = depth.shape
    K = np.asarray(K, np.float64).reshape(-1)
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = depth.astype(np.float64) / 1000.0
    pc = np.stack([(ii - K[2]) / K[0] * z, (jj - K[5]) / K[4] * z, z], -1)
    return np.ascontiguousarray(colour_of(pc @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(T, np.float64).reshape(3)))


def box_depth(R, T, h, w, K):
    K = np.asarray(K, np.float64).reshape(-1)
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(ii - K[2]) / K[0], (jj - K[5]) / K[4], np.ones_like(ii)], -1) @ np.asarray(R, np.float64).reshape(3, 3).T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (BOX_HI - T) / d, np.where(d < 0, (BOX_LO - T) / d, np.inf)).min(-1)
    return np.clip(np.rint(1000.0 * t), 0, 65535).astype(np.uint16)


def kernel_us(m, kid, fn):
    """median and minimum of the profiler's time of the launches of kernel `kid` in one call of fn, microseconds, and the launches"""
    rows, launches = [], 0
    m.enable_profiling(True, only=[kid])
    for i in range(WARMUP + ITERS):
        m.kernel_time(kid)                                 # a query clears the total
        fn()
        m.sync()
        t, launches = m.kernel_time(kid)
        if i >= WARMUP:
            rows.append(t * 1e3)
    m.enable_profiling(False)
    return {"us": round(statistics.median(rows), 2), "min_us": round(min(rows), 2), "launches": int(launches)}


def device_ms(fn):
    ms = []
    for i in range(WARMUP + ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def wall_ms(fn):
    ms = []
    for i in range(WARMUP + ITERS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def scene(name, cfg, K, frames, tracked):
    m = DenseTSDF(**cfg)
    m.set_dep_camera_intrinsic(K)
    m.set_color_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, frame_colour(R, T, d, K))
    m.sync()
    Rt, Tt, depth = tracked
    rgb = frame_colour(Rt, Tt, depth, K)
    dd, dc = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(rgb).cuda()
    R, T = off_pose(Rt, Tt)
    out = {"scene": name, "image": "%d x %d" % depth.shape[::-1], "bricks": m.bricks_in_use()}
    for stride in (1, 2):
        s = m.align_rgbd_linearize(depth, rgb, R, T, stride=stride)
        px = -(-depth.shape[0] // stride) * -(-depth.shape[1] // stride)
        row = {"pixels": px, "geo_used": s["geo"]["n_used"], "col_used": s["col"]["n_used"], "col_far": s["col"]["n_far"], "col_grad": s["col"]["n_grad"]}
        row["rgbd_kernel"] = kernel_us(m, _lib.K_ALIGN_RGBD, lambda: m.align_rgbd_linearize(dd, dc, R, T, stride=stride, device=True))
        row["rgbd_kernel_counts_only"] = kernel_us(m, _lib.K_ALIGN_RGBD, lambda: m.align_rgbd_linearize(dd, dc, R, T, stride=stride, device=True, counts_only=True))
        row["depth_kernel"] = kernel_us(m, _lib.K_ALIGN, lambda: m.align_linearize(dd, R, T, stride=stride, device=True))
        row["depth_kernel_counts_only"] = kernel_us(m, _lib.K_ALIGN, lambda: m.align_linearize(dd, R, T, stride=stride, device=True, counts_only=True))
        row["rgbd_ns_per_pixel"] = round(1e3 * row["rgbd_kernel"]["us"] / px, 4)
        row["depth_ns_per_pixel"] = round(1e3 * row["depth_kernel"]["us"] / px, 4)
        row["rgbd_over_depth"] = round(row["rgbd_kernel"]["us"] / row["depth_kernel"]["us"], 3)
        row["reductions_share"] = round(1.0 - row["rgbd_kernel_counts_only"]["us"] / row["rgbd_kernel"]["us"], 3)
        row["rgbd_device_call"] = device_ms(lambda: m.align_rgbd_linearize(dd, dc, R, T, stride=stride, device=True))
        row["depth_device_call"] = device_ms(lambda: m.align_linearize(dd, R, T, stride=stride, device=True))
        out[f"stride{stride}"] = row
    info = {}

    def track(colour):
        info["c" if colour else "d"] = m.track_rgbd(dd, dc, R, T) if colour else m.track_depth(dd, R, T)
    out["track_rgbd_wall"] = wall_ms(lambda: track(True))
    out["track_depth_wall"] = wall_ms(lambda: track(False))
    for k, label in (("c", "track_rgbd"), ("d", "track_depth")):
        Rf, Tf, inf = info[k]
        D = Rf @ Rt.T
        out[label] = {"status": inf["status"], "linearisations": inf["iterations"], "error_m": round(float(np.linalg.norm(Tf - Tt)), 6),
                      "error_deg": round(float(np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0)))), 5)}
    out["track_rgbd"]["lambda"] = round(info["c"][2]["lambda"], 4)
    return out


def main():
    frames = list(syn.sphere_room_stream(FRAMES))
    out = {"probe": "track_rgbd", "iters": ITERS, "scenes": [scene("C2 textured: 512^3 / 2 cm, %d frames" % FRAMES, C2, syn.K_DEPTH, frames, frames[TRACKED])]}
    K = syn.scaled_intrinsics(240, 320)
    poses = [syn.camera_pose(f, start_deg=40.0, deg_per_frame=3.0) for f in range(6)]
    Rt, Tt = syn.camera_pose(2.5, start_deg=40.0, deg_per_frame=3.0)
    out["scenes"].append(scene("box room textured: 256^3 / 4 cm, 6 frames", ROOM, K, [(R, T, box_depth(R, T, 240, 320, K)) for R, T in poses],
                               (Rt, Tt, box_depth(Rt, Tt, 240, 320, K))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

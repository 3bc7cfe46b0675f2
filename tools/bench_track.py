"""Time of frame-to-model alignment (tsl_align.hip, k_align_linearize) on the C2 scene (512^3 / 2 cm, 20 frames of the synthetic room stream), a
640 x 480 depth image (frame 10) at a pose 1 cm / 0.5 deg off its own: one linearisation at stride 1 and stride 2, device form, torch events around
one call, median of 7 after a warm-up -- with the sums and counts only (the gathers without the products and their reduction); the host form of the
same call in wall time (launch, copy back of the 33 integers, wait: the round trip every iteration of the tracker pays); a whole default
track_depth in wall time; render_view at the same pose for scale.  One process; run it under `timeout`.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import synthetic as syn

C2 = dict(map_scale=[10.24, 10.24], voxel_scale=0.02, num_voxel_per_blk_axis=16, max_ray_length=5.0, min_ray_length=0.3, internal_voxels=10, recast_step=2)
FRAMES, WARMUP, ITERS, TRACKED = 20, 3, 7, 10


def off_pose(R, T, metres=0.01, deg=0.5):
    th = np.deg2rad(deg)
    a = np.array([0.36, -0.48, 0.8])
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return (np.eye(3) + np.sin(th) * S + (1.0 - np.cos(th)) * (S @ S)) @ R, T + metres * np.array([0.6, 0.64, -0.48])


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


def main():
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    frames = list(syn.sphere_room_stream(FRAMES))
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    Rt, Tt, depth = frames[TRACKED]
    dev = torch.from_numpy(depth.view(np.int16)).cuda()
    R, T = off_pose(Rt, Tt)
    out = {"probe": "track_depth", "scene": "512^3 / 2 cm, %d frames" % FRAMES, "image": "640 x 480, frame %d, pose 1 cm / 0.5 deg off" % TRACKED, "iters": ITERS,
           "bricks": m.bricks_in_use()}
    for stride in (1, 2):
        s = m.align_linearize(depth, R, T, stride=stride)
        out[f"stride{stride}"] = dict(device_ms(lambda: m.align_linearize(dev, R, T, stride=stride, device=True)),
                                      used=s["n_used"], gate=s["n_gate"], unknown=s["n_unknown"], far=s["n_far"], grad=s["n_grad"])
        out[f"stride{stride}_counts_only"] = device_ms(lambda: m.align_linearize(dev, R, T, stride=stride, device=True, counts_only=True))
        out[f"stride{stride}_host_form_wall"] = wall_ms(lambda: m.align_linearize(depth, R, T, stride=stride))
    info = {}

    def track(image):
        info["r"] = m.track_depth(image, R, T)
    out["track_default_wall"] = wall_ms(lambda: track(depth))
    out["track_default_device_image_wall"] = wall_ms(lambda: track(dev))
    Rf, Tf, inf = info["r"]
    D = Rf @ Rt.T
    out["track_default"] = {"status": inf["status"], "linearisations": inf["iterations"], "error_m": round(float(np.linalg.norm(Tf - Tt)), 6),
                            "error_deg": round(float(np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0)))), 5),
                            "used_per_level": [r["n_used"] for r in inf["records"]]}
    out["render_view"] = device_ms(lambda: m.render_view(Rt, Tt, device=True))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Probe: throughput of DenseTSDF.query_esdf on torch tensors (tsl_esdf_query_points_dev) on the config-4 scene (512^3 / 2 cm, the synthetic
stream, ESDF with max_dist = 1 m).  Three sets of 1 M points: (a) 1 000 straight segments of 1 000 samples at 1 cm, (b) uniform in the observed
bounding box, (c) uniform in one 2 m cube; each with refresh off and on, timed with HIP events after a warm-up.  Prints one JSON line.
Kernel times: run under rocprofv3 --kernel-trace --stats (tsl::k_esdf_query<1>)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import synthetic as syn

C4 = dict(map_scale=[10.24, 10.24], voxel_scale=0.02, num_voxel_per_blk_axis=16, max_ray_length=5.0, min_ray_length=0.3, internal_voxels=10, recast_step=2)
FRAMES, WARMUP, ITERS = 16, 3, 20


def main():
    m = DenseTSDF(**C4)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(FRAMES):
        m.recast_depth_to_map(R, T, d, None)
        m.update_esdf(max_dist=1.0, wait=False)
    idx, _ = m.export_esdf()
    lo, hi = idx.min(0).astype(np.float64) * 0.02, idx.max(0).astype(np.float64) * 0.02
    rng = np.random.default_rng(0)
    start = rng.uniform(lo, hi, (1000, 3))
    dirs = rng.normal(size=(1000, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    sets = {
        "a_segments": (start[:, None, :] + dirs[:, None, :] * (0.01 * np.arange(1000))[None, :, None]).reshape(-1, 3),
        "b_bbox": rng.uniform(lo, hi, (1_000_000, 3)),
        "c_cube_2m": (lo + hi) / 2 + rng.uniform(-1.0, 1.0, (1_000_000, 3)),
    }
    out = {"probe": "esdf_query", "scene": "512^3 / 2 cm, %d frames, max_dist 1 m" % FRAMES, "observed_voxels": int(idx.shape[0]),
           "queries": 1_000_000, "iters": ITERS}
    for name, p in sets.items():
        x = torch.from_numpy(p.astype(np.float32)).cuda()
        for refresh in (False, True):
            for _ in range(WARMUP):
                r = m.query_esdf(x, refresh=refresh)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                r = m.query_esdf(x, refresh=refresh)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / ITERS
            st = r[2].cpu().numpy()
            key = f"{name}_refresh_{'on' if refresh else 'off'}"
            out[key] = {"ms_per_call": round(ms, 4), "queries_per_s": round(1e6 / (ms * 1e-3)), "status_ok": round(float((st == 0).mean()), 4),
                        "status_unknown": round(float((st == 1).mean()), 4), "status_outside": round(float((st == 2).mean()), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Time of DenseTSDF.render_view (tsl_render.hip, k_render_view) on the C2 scene (512^3 / 2 cm, 20 frames of the synthetic room stream): a 640 x 480
view at pose 10 and the all-miss view (from the origin, looking away from everything integrated), each with and without skipping, device form,
torch events around one call, median of 7 after a warm-up; next to it the integrate time per frame of the same run, for scale.  One process; run it
under `timeout`.  Prints one JSON line."""
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
FRAMES, WARMUP, ITERS = 20, 3, 7


def main():
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    frames = [(R, T, torch.from_numpy(d.view(np.int16)).cuda()) for R, T, d in syn.sphere_room_stream(FRAMES)]
    for R, T, d in frames[:4]:                                  # scratch allocation and first launches are not a frame's cost
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    m.reset()
    t0 = time.perf_counter()
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    integrate_ms = (time.perf_counter() - t0) * 1e3 / FRAMES
    R180, _ = syn.camera_pose(180)
    views = {"pose10": syn.camera_pose(10), "all_miss": (R180, np.zeros(3))}
    out = {"probe": "render_view", "scene": "512^3 / 2 cm, %d frames" % FRAMES, "view": "640 x 480, t in [0.3, 5], step 0.75 voxel", "iters": ITERS,
           "integrate_ms_per_frame": round(integrate_ms, 4), "bricks": m.bricks_in_use()}
    for name, (R, T) in views.items():
        for skip in (True, False):
            ms = []
            for i in range(WARMUP + ITERS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                r = m.render_view(R, T, device=True, skip=skip)
                b.record()
                torch.cuda.synchronize()
                if i >= WARMUP:
                    ms.append(a.elapsed_time(b))
            st = r[3].cpu().numpy()
            out[f"{name}_{'skip' if skip else 'plain'}"] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                                                            "hits": round(float(((st & 0xBF) == 0).mean()), 4), "misses": round(float((st == 1).mean()), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

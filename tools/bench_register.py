"""Time of map-to-map registration (tsl_register.hip, k_register_linearize) on the C2 scene (512^3 / 2 cm, 20 frames of the synthetic room stream) split
into two submaps of one handle: frames 0..9 in submap 0 (the destination), frames 10..19 in submap 1 (the source), both at the identity, so the true
relative pose is the identity; the guess is 1 cm / 0.5 deg off.  One linearisation at strides 1, 2 and 4, with the sums and counts only (the
compaction and the gathers without the products and their reduction): the kernel alone, HIP events around the launch (tsl_tsdf_prof_query,
TSL_K_REGISTER), median of 7 after a warm-up; the host form of the same call in wall time (the round trip every iteration pays); the band's share of
the visited voxels, which is what the compaction pass buys; one whole default register_submap in wall time.  One process; run it under `timeout`.
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from taichislam_amd import _lib
from taichislam_amd.mapping import DenseTSDF
from taichislam_amd.utils import synthetic as syn

C2 = dict(map_scale=[10.24, 10.24], voxel_scale=0.02, num_voxel_per_blk_axis=16, max_ray_length=5.0, min_ray_length=0.3, internal_voxels=10, recast_step=2)
FRAMES, WARMUP, ITERS = 20, 3, 7


def off_pose(metres=0.01, deg=0.5):
    th = np.deg2rad(deg)
    a = np.array([0.36, -0.48, 0.8])
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(th) * S + (1.0 - np.cos(th)) * (S @ S), metres * np.array([0.6, 0.64, -0.48])


def kernel_ms(m, fn):
    """median and minimum of the kernel's own time over ITERS calls of fn (one launch each)"""
    ms = []
    for i in range(WARMUP + ITERS):
        m.kernel_time(_lib.K_REGISTER)
        fn()
        t, n = m.kernel_time(_lib.K_REGISTER)
        assert n == 1, n
        if i >= WARMUP:
            ms.append(t)
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def wall_ms(m, fn):
    ms = []
    for i in range(WARMUP + ITERS):
        m.sync()
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def main():
    m = DenseTSDF(**C2, max_submap_num=2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for f, (R, T, d) in enumerate(syn.sphere_room_stream(FRAMES)):
        if f == FRAMES // 2:
            m.switch_to_next_submap()
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    R, T = off_pose()
    kw = dict(src_sid=1, dst_sid=0)
    out = {"probe": "register_submap", "scene": "512^3 / 2 cm, frames 0..9 against frames 10..19", "guess": "1 cm / 0.5 deg off", "iters": ITERS,
           "bricks": m.bricks_in_use()}
    m.enable_profiling(True, only=[_lib.K_REGISTER])
    for stride in (1, 2, 4):
        s = m.register_linearize(m, R, T, stride=stride, **kw)
        visited = int(s["sums"][28:].sum())
        out[f"stride{stride}"] = dict(kernel_ms(m, lambda: m.register_linearize(m, R, T, stride=stride, **kw)), visited=visited,
                                      band_share=round(1.0 - s["n_gate"] / max(visited, 1), 4), used=s["n_used"], gate=s["n_gate"], unknown=s["n_unknown"],
                                      far=s["n_far"], grad=s["n_grad"])
        out[f"stride{stride}_counts_only"] = kernel_ms(m, lambda: m.register_linearize(m, R, T, stride=stride, counts_only=True, **kw))
    m.enable_profiling(False)
    out["stride1_host_form_wall"] = wall_ms(m, lambda: m.register_linearize(m, R, T, **kw))
    info = {}

    def run():
        info["r"] = m.register_submap(m, R, T, **kw)
    out["register_default_wall"] = wall_ms(m, run)
    Rf, Tf, inf = info["r"]
    out["register_default"] = {"status": inf["status"], "linearisations": inf["iterations"], "error_m": round(float(np.linalg.norm(Tf)), 6),
                               "error_deg": round(float(np.degrees(np.arccos(np.clip((np.trace(Rf) - 1.0) / 2.0, -1.0, 1.0)))), 5),
                               "used_per_linearisation": [r["n_used"] for r in inf["records"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

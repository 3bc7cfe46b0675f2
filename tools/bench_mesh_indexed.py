"""Time of the indexed marching-cubes mesh (tsl_mesh_indexed.hip, MarchingCubeMesher.generate_indexed_mesh) on two maps: the room of the tests
(tests/render_view_scenes.py: four 320 x 240 frames, 256^3 / 4 cm) and the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames of the
sphere-room stream (512^3 / 2 cm).

Per map, medians of REPEATS after WARMUP: the indexed call alone (the mesh stays on the device) and with its copy to the host, its kernels through the
handle's profiler, and the two routes that existed before it: generate_mesh(1) alone, and generate_mesh(1) + get_mesh() + a numpy weld (np.unique over
the edge keys recovered from the soup's positions, tests/mesh_indexed_ref.py) -- the route to shared vertices plus an index buffer without this kernel.
Also the device-to-host bytes of both forms.  On the room the GPU result is compared with the numpy restatement before anything is timed.  No threshold
is set.  Writes the table to --out (default profiles/mesh_indexed.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import contextlib
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
from taichislam_amd.mapping import DenseTSDF, MarchingCubeMesher
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS = 2, 7, 3


def median_ms(fn, warmup, repeats, sync):
    ms = []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def kernel_ms(m, fn):
    """median of the profiler's marching-cubes bracket for one call of fn"""
    rows = []
    m.enable_profiling(True, only=[_lib.K_MESH])
    for i in range(WARMUP + REPEATS):
        m.kernel_time(_lib.K_MESH)
        fn()
        m.sync()
        t, _ = m.kernel_time(_lib.K_MESH)
        if i >= WARMUP:
            rows.append(t)
    m.enable_profiling(False)
    return statistics.median(rows)


def weld(v, nr, m):
    """shared vertices + an index buffer from a soup on the host: the rows whose edge is recoverable are welded by edge key, the others stay their own"""
    import mesh_indexed_ref as ref
    low, axis, amb = ref.edge_of_soup_vertex(v, m.voxel_scale)
    key = np.where(amb, -1 - np.arange(v.shape[0]), ref.cell_key(low, m.N, m.Nz) * 3 + axis)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    return v[first], nr[first], inv.reshape(-1, 3).astype(np.int32)


def case(lines, name, m, check):
    import mesh_indexed_ref as ref
    quiet = io.StringIO()
    mesher = MarchingCubeMesher(m, max_triangles=4_000_000, tsdf_surface_thres=5 * m.voxel_scale)
    nv, nt = mesher.generate_indexed_mesh()
    got = mesher.get_indexed_mesh()
    if check:
        with contextlib.redirect_stdout(quiet):
            e = m.export_submap()
        ref.assert_equal(got, ref.extract(e, m.N, m.Nz, m.voxel_scale, 5 * m.voxel_scale), name)
    with contextlib.redirect_stdout(quiet):
        mesher.generate_mesh(1)
    assert mesher.num_facelets[None] == nt
    per_v, per_t = 12 + 12 + 8, 12
    lines.append(f"{name}: {m.N} x {m.N} x {m.Nz} voxels of {m.voxel_scale} m, {m.bricks_in_use()} bricks; {nt} triangles, {nv} vertices "
                 f"({3 * nt / max(nv, 1):.2f} soup rows per vertex)" + (" (equal to the numpy restatement)" if check else ""))
    lines.append(f"{name}: device-to-host bytes  soup {72 * nt} (3 T rows x 24)  indexed {per_v * nv + per_t * nt} (V x {per_v} + T x {per_t})  "
                 f"ratio {72 * nt / max(per_v * nv + per_t * nt, 1):.2f}x")
    ik = kernel_ms(m, mesher.generate_indexed_mesh)
    idev, idev_min = median_ms(mesher.generate_indexed_mesh, WARMUP, REPEATS, m.sync)

    def indexed_host():
        mesher.generate_indexed_mesh()
        mesher.get_indexed_mesh()
    ihost, ihost_min = median_ms(indexed_host, WARMUP, REPEATS, m.sync)
    lines.append(f"{name}: indexed  kernels {ik * 1e3:8.1f} us  call {idev:8.3f} ms (min {idev_min:8.3f})  call + copy to the host {ihost:8.3f} ms (min {ihost_min:8.3f})")
    with contextlib.redirect_stdout(quiet):
        sk = kernel_ms(m, lambda: mesher.generate_mesh(1))
        sdev, sdev_min = median_ms(lambda: mesher.generate_mesh(1), WARMUP, REPEATS, m.sync)

        def soup_host():
            mesher.generate_mesh(1)
            mesher.get_mesh()
        shost, shost_min = median_ms(soup_host, WARMUP, REPEATS, m.sync)

        def parent_route():
            mesher.generate_mesh(1)
            v, nr, _ = mesher.get_mesh()
            return weld(v, nr, m)
        pr, pr_min = median_ms(parent_route, 0, HOST_REPEATS, m.sync)
        wv, _, wt = parent_route()
    lines.append(f"{name}: soup     kernels {sk * 1e3:8.1f} us  call {sdev:8.3f} ms (min {sdev_min:8.3f})  call + copy to the host {shost:8.3f} ms (min {shost_min:8.3f})")
    lines.append(f"{name}: the route before: generate_mesh(1) + get_mesh() + numpy weld {pr:10.3f} ms (min {pr_min:10.3f}), {wv.shape[0]} welded rows; "
                 f"route / indexed call + copy {pr / ihost:8.1f}x; indexed call / soup call {idev / sdev:6.2f}x")
    for ln in lines[-5:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_indexed.txt"))
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_mesh_indexed.py: medians of {REPEATS} after {WARMUP} warm-up calls (the route before: median of {HOST_REPEATS}); one MI355X, one process",
             "kernels = HIP events around the call's launches (tsl_tsdf_prof_query); calls in wall time, each ends with the counts on the host"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "room", m, True)
    del m
    m = DenseTSDF(**C2)
    m.set_dep_camera_intrinsic(syn.K_DEPTH)
    for R, T, d in syn.sphere_room_stream(20):
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    case(lines, "config-2", m, False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

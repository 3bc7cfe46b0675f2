"""Time of the free-space topology graph (tsl_topo.hip, mapping/topo_graph.py: TopoGraphGen) on the room of the other tool benches
(tests/render_view_scenes.py, 256^3 / 4 cm) and on the config-2 scene of taichislam_amd/utils/bench_configs.py after 20 frames (512^3 / 2 cm), with the
reference's defaults (coll_det_num 128, max_raycast_dist 2 m) from the first camera position: one node expansion, and a whole graph of up to 100 frontiers.

Beside each: the route a caller had before -- the serial Python loop over DenseTSDF.raycast / is_pos_* for the map part and numpy over all triangles for the
facelets, which is tests/topo_graph_ref.py run on the GPU map instead of the oracle.  The two graphs are compared first (nodes, facelets, frontiers, edges,
bit for bit).  The share of the device calls (launch + wait + copies, as the host sees them: detect_collisions, add_poly, rays, read_facelets), of the hull
(scipy's Qhull) and of the rest of the Python is taken by wrapping those methods with a wall clock; the kernel alone is timed with events around
tsl_topo_rays_dev for one expansion's rays on the finished graph.  Medians of REPEATS after WARMUP (the old route: median of HOST_REPEATS whole graphs).  No threshold
is set.  Writes the table to --out (default profiles/topo_graph.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from taichislam_amd.mapping import DenseTSDF, TopoGraphGen
from taichislam_amd.utils import synthetic as syn
from taichislam_amd.utils.bench_configs import C2

WARMUP, REPEATS, HOST_REPEATS, MAX_FRONTIERS = 2, 7, 3, 100
PARTS = ("detect_collisions", "add_poly", "rays", "read_facelets", "_hull")


class MapAsOracle:
    """what tests/topo_graph_ref.py asks of a map, answered by the DenseTSDF: the old route's map part"""

    def __init__(self, m):
        self.m, self.voxel_scale = m, m.voxel_scale

    def raycast(self, pos, dir, max_dist):
        return self.m.raycast(pos, dir, max_dist)

    def query_points(self, mode, xyz, param=0):
        return self.m.is_pos_unobserved(xyz) if mode == 1 else self.m.is_pos_occupy(xyz)


def timed(fn, n, warm):
    ms = []
    for i in range(warm + n):
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def same_graph(t, r):
    from topo_graph_ref import bits
    got, want = t.read_facelets(), r.facelets()
    ok = len(t.nodes()["master_idx"]) == len(r.node_fl) and t.num_frontiers[None] == len(r.frontier)
    ok = ok and all(np.array_equal(bits(got[a]), bits(want[b])) for a, b in (("tri_vertices", "tri"), ("normal", "normal"), ("center", "center")))
    ok = ok and all(np.array_equal(bits(t.frontiers()[k]) if v.dtype == np.float32 else t.frontiers()[k], bits(v) if v.dtype == np.float32 else v) for k, v in r.frontiers().items())
    return ok and np.array_equal(t.edge_index(), np.array(r.edge_idx, np.int32).reshape(-1, 2)) and np.array_equal(bits(t.nodes()["center"]), bits(r.nodes()["center"]))


def map_case(lines, name, m, start):
    import torch
    from topo_graph_ref import RefTopo
    first = len(lines)
    t = TopoGraphGen(m)
    r = RefTopo(MapAsOracle(m), coll_det_num=128, max_raycast_dist=2)
    n = t.generate_topo_graph(start, max_nodes=MAX_FRONTIERS)
    r.generate_topo_graph(start, MAX_FRONTIERS)
    assert same_graph(t, r), f"{name}: the graph differs from the old route's"
    assert n >= 1, f"{name}: the first expansion was refused ({t.stats}): nothing to time"
    lines.append(f"{name}: start {np.round(np.asarray(start, float), 2).tolist()}; {n} nodes, {t.num_facelets[None]} facelets, {t.num_frontiers[None]} frontiers "
                 f"({t.search_frontiers_idx[None]} examined), {len(t.edge_index())} edges; {t.stats}; equal to the old route's graph")

    def one_expansion():
        t.reset()
        t.node_expansion(start)

    def whole():
        t.reset()
        t.generate_topo_graph(start, max_nodes=MAX_FRONTIERS)

    def old_expansion():
        r.reset()
        r.node_expansion(start)

    def old_whole():
        r.reset()
        r.generate_topo_graph(start, MAX_FRONTIERS)
    e, e_min = timed(one_expansion, REPEATS, WARMUP)
    w, w_min = timed(whole, REPEATS, WARMUP)
    oe, _ = timed(old_expansion, HOST_REPEATS, 1)
    ow, _ = timed(old_whole, HOST_REPEATS, 0)
    lines.append(f"{name}: one node expansion {e:9.3f} ms (min {e_min:9.3f}); old route {oe:10.3f} ms ({oe / e:7.1f} x)")
    lines.append(f"{name}: whole graph        {w:9.3f} ms (min {w_min:9.3f}); old route {ow:10.3f} ms ({ow / w:7.1f} x)")
    # where the time of a whole graph goes: the wrapped methods' wall clock
    acc = {k: 0.0 for k in PARTS}
    calls = {k: 0 for k in PARTS}

    def wrap(k):
        f = getattr(t, k)

        def g(*a, **kw):
            t0 = time.perf_counter()
            out = f(*a, **kw)
            acc[k] += (time.perf_counter() - t0) * 1e3
            calls[k] += 1
            return out
        return g
    for k in PARTS:
        setattr(t, k, wrap(k))
    t0 = time.perf_counter()
    whole()
    total = (time.perf_counter() - t0) * 1e3
    for k in PARTS:
        delattr(t, k)
    dev = acc["detect_collisions"] + acc["add_poly"] + acc["rays"] + acc["read_facelets"]
    ncalls = sum(calls[k] for k in PARTS if k != "_hull")
    lines.append(f"{name}: one whole graph {total:9.3f} ms = device calls {dev:8.3f} ({ncalls} calls, {1e3 * dev / max(ncalls, 1):7.1f} us each: collide {acc['detect_collisions']:7.3f} / "
                 f"{calls['detect_collisions']}, add_poly {acc['add_poly']:7.3f} / {calls['add_poly']}, rays {acc['rays']:7.3f} / {calls['rays']}, read_facelets "
                 f"{acc['read_facelets']:7.3f} / {calls['read_facelets']}) + hull {acc['_hull']:8.3f} ({calls['_hull']}) + other Python {total - dev - acc['_hull']:8.3f}")
    # the kernel alone: one expansion's rays against the finished graph, events around the asynchronous form
    d = torch.device(f"cuda:{m.device}")
    pos = torch.from_numpy(np.repeat(np.asarray(start, np.float32)[None, :], 128, 0)).to(d)
    dirs = torch.from_numpy(t.sample_dirs).to(d)
    ms = []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t.rays_dev(pos, dirs, 2.0)
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    lines.append(f"{name}: tsl_topo_rays_dev, 128 rays from the start against {t.num_facelets[None]} facelets in {t.num_nodes[None]} nodes: {statistics.median(ms) * 1e3:8.1f} us "
                 f"(min {min(ms) * 1e3:8.1f}) between events on the caller's stream")
    for ln in lines[first:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topo_graph.txt"))
    ap.add_argument("--skip-config2", action="store_true")
    args = ap.parse_args()
    import render_view_scenes as rv
    from util import SMALL
    lines = [f"tools/bench_topo_graph.py: medians of {REPEATS} after {WARMUP} warm-up runs (old route: median of {HOST_REPEATS}); one MI355X, one process",
             f"TopoGraphGen defaults (coll_det_num 128, max_raycast_dist 2 m), at most {MAX_FRONTIERS} frontiers examined; wall clock of the host unless said otherwise"]
    K, frames = rv.room_scene()
    m = DenseTSDF(**SMALL)
    m.set_dep_camera_intrinsic(K)
    for R, T, d in frames:
        m.recast_depth_to_map(R, T, d, None)
    m.sync()
    map_case(lines, "room", m, frames[0][1])
    del m
    if not args.skip_config2:
        m = DenseTSDF(**C2)
        m.set_dep_camera_intrinsic(syn.K_DEPTH)
        first = None
        for R, T, d in syn.sphere_room_stream(20):
            first = (np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64)) if first is None else first
            m.recast_depth_to_map(R, T, d, None)
        m.sync()
        # at the first camera itself nothing is within 2 m and the first expansion is refused: the nearest point ahead of it, in steps of 0.5 m, where one succeeds
        probe = TopoGraphGen(m)
        ahead = next((a for a in (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0) if probe.test_detect_collisions(first[1] + first[0] @ np.array([0.0, 0.0, a]))), None)
        assert ahead is not None, "config-2: no start point ahead of the first camera has a black ray"
        del probe
        lines.append(f"config-2: the start is {ahead} m ahead of the first camera")
        map_case(lines, "config-2", m, first[1] + first[0] @ np.array([0.0, 0.0, ahead]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

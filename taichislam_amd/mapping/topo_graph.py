"""TopoGraphGen (taichi_slam/mapping/topo_graph.py, reference root): the skeleton graph of free space, convex polyhedra grown around sample points of a
DenseTSDF.  The rays and the facelets run in csrc/tsl_topo.hip; what stays here is serial and small: the hull (scipy's Qhull, as in the reference), the region
growing, the construction of the frontiers and the loop.

The result is ONE defined answer, the sequential reading of the reference (include/taichislam_hip.h, "free-space topology graph"): every loop
in ascending index order, f32 arithmetic in the order the source writes it.  Where this differs from what the reference's parallel loops may give:
  * blacks, the centre sum and the neighbour nodes come in ray / facelet order; neighbour nodes are de-duplicated through the connection set, there is no
    fixed-size neighbor_node_ids list to overflow, and the region queue is a list (a facelet may enter it more than once before it is visited, as in the
    reference, and then counts more than once in the frontier's means);
  * an expansion with fewer than 4 black rays, or whose points Qhull refuses, fails and adds no node (the reference raises there and its thread wrapper
    swallows the error);
  * max_nodes of generate_topo_graph bounds the frontiers EXAMINED, not the nodes made (as written in the reference);
  * at max_map_node (4096) nodes the generation stops and `full` is set;
  * tri_colors come from a seeded generator (the reference's are np.random.rand): their shape [3 * facelets][4] and the two alpha values are all that is stated.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ._sides import _vp, device_side
from .fields import ScalarField, device_view

MAX_MAP_NODE = 4096
F32 = np.float32


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)


def _normalized(v):
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _ray_triangle(v0, e1, e2, P, w):
    """Facelet.rayTriangleIntersect (:52-70) on f32 vectors"""
    q = _cross(w, e2)
    a = _dot(e1, q)
    if not abs(a) > F32(0.00001):
        return False, F32(0.0)
    s = (P - v0) / a
    r = _cross(s, e1)
    b0, b1 = _dot(s, q), _dot(r, w)
    b2 = (F32(1.0) - b0) - b1
    return not (b0 < 0 or b1 < 0 or b2 < 0), _dot(e2, r)


class _ArrayField:
    """A field-like over a getter: .to_numpy() the rows in use; .to_torch() the same on the map's device (a zero-copy view where the data lives there)."""

    def __init__(self, getter, dev=None, name="field"):
        self._get, self._dev, self._name = getter, dev, name

    def to_numpy(self):
        return self._get()

    def to_torch(self):
        if self._dev is not None:
            return self._dev()
        import torch
        return torch.from_numpy(np.ascontiguousarray(self._get()))

    def __repr__(self):
        return f"<topo field {self._name}>"


class TopoGraphGen:
    def __init__(self, mapping, coll_det_num=128, max_raycast_dist=2, max_facelets=1024 * 1024, thres_size=0.5, transparent=0.7, transparent_frontier=0.6,
                 frontier_creation_threshold=0.5, frontier_verify_threshold=0.5, frontier_backward_check=-0.2, frontier_combine_angle_threshold=40):
        self.mapping = mapping
        self.L = _lib.lib()
        self.coll_det_num = int(coll_det_num)
        self.max_raycast_dist = max_raycast_dist
        self.max_facelets = int(max_facelets)
        h = C.c_void_p()
        _lib.check(self.L.tsl_topo_create(mapping.h, self.coll_det_num, float(max_raycast_dist), self.max_facelets, C.byref(h)))      # refuses coll_det_num outside 4 .. 512
        self.h = h
        self.generate_uniform_sample_points(self.coll_det_num)
        self.thres_size = thres_size
        self.transparent, self.transparent_frontier = transparent, transparent_frontier
        self.colormap = np.random.default_rng(0).random((MAX_MAP_NODE, 4)).astype(F32)
        self.colormap[:, 3] = transparent
        self.frontier_creation_threshold = frontier_creation_threshold
        self.frontier_verify_threshold = frontier_verify_threshold
        self.frontier_normal_dot_threshold = np.cos(np.deg2rad(frontier_combine_angle_threshold))
        self.check_frontier_small_distance = 0.1
        self.frontier_backward_check = frontier_backward_check
        self.tri_vertices = _ArrayField(self._read_tri_vertices, self._tri_vertices_dev, "tri_vertices")
        self.tri_colors = _ArrayField(self._tri_colors, None, "tri_colors")
        self.edges = _ArrayField(lambda: np.array(self._edges, F32).reshape(-1, 3), None, "edges")
        self.edge_num = ScalarField(lambda: 2 * len(self._edge_index), None, "edge_num")
        self.num_facelets = ScalarField(lambda: self._num_facelets, None, "num_facelets")
        self.num_nodes = ScalarField(lambda: len(self._nodes), None, "num_nodes")
        self.num_frontiers = ScalarField(lambda: self._num_frontiers, None, "num_frontiers")
        self.search_frontiers_idx = ScalarField(lambda: self._search_idx, None, "search_frontiers_idx")
        self._clear()

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None:
                self.L.tsl_topo_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _clear(self):
        self._nodes, self._frontiers, self._num_frontiers, self._num_facelets, self._search_idx = [], [], 0, 0, 0
        self._edges, self._edge_index, self._connected = [], [], set()
        self._frontier_flags, self._node_of_facelets = [], []
        self.full = False
        self.stats = {"expansions": 0, "refused_by_collisions": 0, "refused_by_hull": 0, "frontiers_retracted": 0, "frontiers_valid": 0, "frontiers_invalid": 0}

    def reset(self):
        _lib.check(self.L.tsl_topo_reset(self.h))
        self._clear()

    def generate_uniform_sample_points(self, npoints):
        phi = np.pi * (3 - np.sqrt(5))
        ret = []
        for i in range(npoints):
            y = 1 - 2 * (i / (npoints - 1))
            radius = np.sqrt(1 - y * y)
            theta = phi * i
            ret.append([np.cos(theta) * radius, y, np.sin(theta) * radius])
        self.sample_dirs = np.ascontiguousarray(np.array(ret, dtype=F32))
        return self.sample_dirs

    # ---- device calls ------------------------------------------------------------------------------------------------------------------------
    def rays(self, pos, dir, max_dist, skip_idx=None, backward=-0.01, facelets_only=False):
        """A batch of combined rays (TopoGraphGen.raycast :490-507; facelets_only: detect_collision_facelets alone): returns (hit bool [n], type u8 [n],
        position f32 [n, 3], length f32 [n], poly int32 [n])."""
        pos = np.ascontiguousarray(np.asarray(pos, F32).reshape(-1, 3))
        dir = np.ascontiguousarray(np.asarray(dir, F32).reshape(-1, 3))
        assert pos.shape == dir.shape
        n = pos.shape[0]
        skip = None if skip_idx is None else np.ascontiguousarray(np.broadcast_to(np.asarray(skip_idx, np.int32), (n,)))
        hit, typ = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        end, ln, poly = np.zeros((n, 3), F32), np.zeros(n, F32), np.zeros(n, np.int32)
        _lib.check(self.L.tsl_topo_rays(self.h, _vp(pos), _vp(dir), _vp(skip), n, float(F32(max_dist)), float(F32(backward)), 1 if facelets_only else 0, _vp(hit),
                                        _vp(typ), _vp(end), _vp(ln), _vp(poly)))
        return hit.astype(bool), typ, end, ln, poly

    def rays_dev(self, pos, dir, max_dist, skip_idx=None, backward=-0.01, facelets_only=False):
        """rays() on torch tensors of the map's device, asynchronously, ordered with torch's current stream"""
        import torch
        p = pos.reshape(-1, 3).contiguous().float(); d = dir.reshape(-1, 3).contiguous().float()
        assert p.shape == d.shape and p.is_cuda and d.is_cuda
        n = p.shape[0]
        sk = None if skip_idx is None else skip_idx.reshape(-1).contiguous().to(torch.int32)
        side = device_side(p.device)
        hit, typ, end, ln, poly = side.out(n, "u1"), side.out(n, "u1"), side.out((n, 3), "f4"), side.out(n, "f4"), side.out(n, "i4")
        side.call(self.L.tsl_topo_rays, self.L.tsl_topo_rays_dev, self.h, side.ptr(p), side.ptr(d), side.ptr(sk), n, float(F32(max_dist)), float(F32(backward)),
                  1 if facelets_only else 0, side.ptr(hit), side.ptr(typ), side.ptr(end), side.ptr(ln), side.ptr(poly))
        return hit.bool(), typ, end, ln, poly

    def detect_collisions(self, start_pt):
        """:444-470: returns (succ, black positions, black unit directions, black lengths, white count, node_size)"""
        n = self.coll_det_num
        start = np.ascontiguousarray(np.asarray(start_pt, F32).reshape(3))
        succ, nb, nw, size = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
        bpos, bdir, blen = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, F32)
        _lib.check(self.L.tsl_topo_collide(self.h, _vp(start), _vp(self.sample_dirs), float(F32(self.thres_size)), C.byref(succ), C.byref(nb), _vp(bpos), _vp(bdir),
                                           _vp(blen), C.byref(nw), None, C.byref(size)))
        k = nb.value
        return bool(succ.value), bpos[:k], bdir[:k], blen[:k], nw.value, F32(size.value)

    def add_poly(self, tris, start_pt, max_dist=None):
        """One node from triangles f32 [nf, 3, 3] (tsl_topo_add_poly): returns (node index, centre, is_frontier bool [nf], reason u8 [nf], neigh int32 [nf]).  The
        graph's own bookkeeping (nodes(), edges, frontiers) is NOT touched: node_expansion does that; this is the door for hand-built stores."""
        tris = np.ascontiguousarray(np.asarray(tris, F32).reshape(-1, 3, 3))
        nf = tris.shape[0]
        start = np.ascontiguousarray(np.asarray(start_pt, F32).reshape(3))
        md = self.frontier_creation_threshold if max_dist is None else max_dist
        fr, why, neigh, centre, node = np.zeros(nf, np.uint8), np.zeros(nf, np.uint8), np.zeros(nf, np.int32), np.zeros(3, F32), C.c_int32()
        _lib.check(self.L.tsl_topo_add_poly(self.h, _vp(tris), nf, _vp(start), float(F32(md)), _vp(fr), _vp(why), _vp(neigh), _vp(centre), C.byref(node)))
        return node.value, centre, fr.astype(bool), why, neigh

    def read_facelets(self, first=0, n=None):
        """the facelet store as a dictionary of arrays: tri_vertices [n, 3, 3], v0, edge1, edge2, normal, center [n, 3], poly_idx [n]"""
        total, nn = C.c_int64(), C.c_int32()
        _lib.check(self.L.tsl_topo_counts(self.h, C.byref(total), C.byref(nn)))
        n = total.value - first if n is None else n
        out = {"tri_vertices": np.zeros((n, 3, 3), F32), "poly_idx": np.zeros(n, np.int32)}
        for k in ("v0", "edge1", "edge2", "normal", "center"):
            out[k] = np.zeros((n, 3), F32)
        _lib.check(self.L.tsl_topo_read_facelets(self.h, first, n, _vp(out["tri_vertices"]), _vp(out["v0"]), _vp(out["edge1"]), _vp(out["edge2"]), _vp(out["normal"]),
                                                 _vp(out["center"]), _vp(out["poly_idx"])))
        return out

    # ---- fields ----------------------------------------------------------------------------------------------------------------------------------
    def _read_tri_vertices(self):
        return self.read_facelets()["tri_vertices"].reshape(-1, 3)

    def _tri_vertices_dev(self):
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self.L.tsl_topo_buffers_dev(self.h, C.byref(p), None, None, None, C.byref(n), None))
        return device_view(p.value, (n.value * 3, 3), "<f4", keep=self, device=getattr(self.mapping, "device", 0))

    def _tri_colors(self):
        out = np.zeros((self._num_facelets * 3, 4), F32)
        if self._num_facelets:
            col = self.colormap[np.concatenate(self._node_of_facelets)].copy()
            col[np.concatenate(self._frontier_flags), 3] = self.transparent_frontier
            out[:] = np.repeat(col, 3, axis=0)
        return out

    def nodes(self):
        """the nodes as arrays: center f32 [n, 3], master_idx, start_facelet_idx, end_facelet_idx int32 [n] (idx is the row)"""
        n = len(self._nodes)
        return {"center": np.array([x["center"] for x in self._nodes], F32).reshape(n, 3), "master_idx": np.array([x["master_idx"] for x in self._nodes], np.int32),
                "start_facelet_idx": np.array([x["start"] for x in self._nodes], np.int32), "end_facelet_idx": np.array([x["end"] for x in self._nodes], np.int32)}

    def frontiers(self):
        """the num_frontiers frontiers as arrays; next_node_initial and is_valid are those of verify_frontier (zero before it ran)"""
        fr = self._frontiers[:self._num_frontiers]
        n = len(fr)
        out = {k: np.array([x[k] for x in fr], F32).reshape(n, 3) for k in ("avg_center", "outwards_unit_normal", "projected_center", "projected_normal", "next_node_initial")}
        out["master_idx"] = np.array([x["master_idx"] for x in fr], np.int32)
        out["is_valid"] = np.array([x["is_valid"] for x in fr], np.int32)
        return out

    def edge_index(self):
        """int32 [E, 2]: the two nodes of every edge, in the order of `edges` (rows 2 e and 2 e + 1 of it are their centres)"""
        return np.array(self._edge_index, np.int32).reshape(-1, 2)

    # ---- the graph -------------------------------------------------------------------------------------------------------------------------------
    def node_expansion(self, start_pt, show=False, last_node_idx=-1):
        """:245-252; True when a node was added"""
        start = np.asarray(start_pt, F32).reshape(3)
        self.stats["expansions"] += 1
        if len(self._nodes) >= MAX_MAP_NODE:
            self.full = True
            return False
        succ, bpos, bdir, blen, nw, size = self.detect_collisions(start)
        if not succ:
            self.stats["refused_by_collisions"] += 1
            return False
        hull = self._hull(bdir)
        if hull is None:
            self.stats["refused_by_hull"] += 1
            return False
        vertices = (hull.points * blen.astype(np.float64)[:, None] + start.astype(np.float64)).astype(F32)          # :296-303
        self._add_mesh(vertices[hull.simplices], hull.neighbors, start, int(last_node_idx))
        return True

    def test_detect_collisions(self, start_pt):
        """:509-511"""
        return self.detect_collisions(start_pt)[0]

    def node_expansion_benchmark(self, start_pt, show=False, run_num=100):
        """:233-243: the two halves of an expansion timed apart; the graph is left as it was found"""
        import time
        s = time.time()
        for _ in range(run_num):
            succ, _, bdir, _, _, _ = self.detect_collisions(start_pt)
        print(f"avg detect_collisions time {(time.time() - s) * 1000 / run_num:.3f}ms")
        s = time.time()
        for _ in range(run_num):
            self._hull(bdir)
        print(f"avg gen convex cost time {(time.time() - s) * 1000 / run_num:.3f}ms")

    def _hull(self, black_dirs):
        """the convex hull of the black unit directions (:305-307), or None with fewer than 4 of them or when Qhull refuses them"""
        from scipy.spatial import ConvexHull, QhullError
        if black_dirs.shape[0] < 4:
            return None
        try:
            return ConvexHull(black_dirs.astype(np.float64))
        except QhullError:
            return None

    def _add_edge(self, a, b):
        self._edges.append(self._nodes[a]["center"]); self._edges.append(self._nodes[b]["center"])
        self._edge_index.append((a, b))

    def _add_mesh(self, tris, neighbors, start, last_node_idx):
        """:380-442"""
        first = self._num_facelets
        node, centre, is_frontier, why, neigh = self.add_poly(tris, start)
        nf = tris.shape[0]
        assert node == len(self._nodes)
        self._nodes.append({"center": centre, "master_idx": last_node_idx, "start": first, "end": first + nf})
        self._num_facelets += nf
        self._frontier_flags.append(is_frontier); self._node_of_facelets.append(np.full(nf, node, np.int64))
        if last_node_idx >= 0:
            self._add_edge(last_node_idx, node)
            self._connected.add((node, last_node_idx)); self._connected.add((last_node_idx, node))
        for nb in neigh:
            nb = int(nb)
            if nb >= 0 and (node, nb) not in self._connected:
                self._connected.add((node, nb)); self._connected.add((nb, node))
                self._add_edge(nb, node)
        if not is_frontier.any():
            return
        fl = self.read_facelets(first, nf)
        normal = fl["normal"]
        thr = F32(self.frontier_normal_dot_threshold)
        assigned = np.zeros(nf, bool)
        for i in range(nf):
            if assigned[i] or not is_frontier[i]:
                continue
            queue, at = [i], 0
            while at < len(queue):
                cur = queue[at]; at += 1
                assigned[cur] = True
                for j in range(3):
                    nb = int(neighbors[cur, j])
                    if is_frontier[nb] and not assigned[nb] and _dot(normal[i], normal[nb]) > thr:
                        queue.append(nb)
            self._construct_frontier(node, fl, queue)

    def _construct_frontier(self, node, fl, queue):
        """:344-378"""
        center, normal = np.zeros(3, F32), np.zeros(3, F32)
        for q in queue:
            center = center + fl["center"][q]
            normal = normal + fl["normal"][q]
        size = F32(len(queue))
        center = center / size
        normal = _normalized(normal / size)
        fr = {"master_idx": node, "avg_center": center, "outwards_unit_normal": normal, "projected_center": np.zeros(3, F32), "projected_normal": np.zeros(3, F32),
              "next_node_initial": np.zeros(3, F32), "is_valid": 0}
        succ, t = False, F32(0.0)
        for q in queue:
            succ, t = _ray_triangle(fl["v0"][q], fl["edge1"][q], fl["edge2"][q], center, normal)
            projected_normal = fl["normal"][q]
            if succ:
                break
        if not succ:                                     # the frontier is retracted: its slot goes to the next one
            self.stats["frontiers_retracted"] += 1
            return
        fr["projected_center"] = center + t * normal
        fr["projected_normal"] = projected_normal.copy()
        del self._frontiers[self._num_frontiers:]
        self._frontiers.append(fr)
        self._num_frontiers += 1

    def verify_frontier(self, frontier_idx):
        """:255-282"""
        fr = self._frontiers[frontier_idx]
        normal, pc = fr["projected_normal"], fr["projected_center"]
        small, thr = F32(self.check_frontier_small_distance), F32(self.frontier_verify_threshold)
        hit, _, _, ln, _ = self.rays(pc + normal * small, normal, F32(self.max_raycast_dist * 2))
        succ, _len = bool(hit[0]), ln[0]
        valid = False
        if not (succ and _len < thr):
            hit2, _, _, ln2, _ = self.rays(pc - normal * small, normal, thr, skip_idx=fr["master_idx"], backward=self.frontier_backward_check, facelets_only=True)
            succ2, _len2 = bool(hit2[0]), ln2[0]
            if not (succ2 and _len2 < thr):
                if not succ or succ2 and _len2 < _len:
                    _len = _len2
                valid = True
                fr["next_node_initial"] = pc + normal * _len / F32(2)
        fr["is_valid"] = int(valid)
        self.stats["frontiers_valid" if valid else "frontiers_invalid"] += 1
        return valid

    def generate_topo_graph(self, start_pt, max_nodes=100, show=False):
        """:284-294; max_nodes bounds the frontiers examined, not the nodes made"""
        self.node_expansion(start_pt, show)
        while self._search_idx < self._num_frontiers and self._search_idx < max_nodes and not self.full:
            if self.verify_frontier(self._search_idx):
                fr = self._frontiers[self._search_idx]
                self.node_expansion(fr["next_node_initial"], show, last_node_idx=fr["master_idx"])
            self._search_idx += 1
        return len(self._nodes)

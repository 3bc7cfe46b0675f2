"""The sequential restatement of TopoGraphGen (taichi_slam/mapping/topo_graph.py, reference root) that tests/test_topo_graph_cpu.py holds against hand-worked
numbers and tests/test_topo_graph_gpu.py holds the HIP kernels against, bit for bit.  It states the definition of include/taichislam_hip.h ("free-space topology
graph") and DESIGN.md 4.20 a second time and shares no code with taichislam_amd/mapping/topo_graph.py: the map is the CPU oracle's (one raycast / point query
at a time), every ray is tested against ALL triangles of every node inside the reach, and the winner is picked from the whole list.

All arithmetic is numpy float32, one rounding per operation, in the order the reference writes it:
  cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)      dot(a, b) = (a0 b0 + a1 b1) + a2 b2      normalized(v) = v / sqrt((x x + y y) + z z)
"""
import numpy as np

F32 = np.float32
QNAN = np.array([0x7fc00000], np.uint32).view(F32)[0]
MAX_MAP_NODE = 4096


def bits(a):
    """the bit patterns of an f32 array (so that -0.0 != 0.0 and NaN == the same NaN)"""
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalized(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]


def ray_triangles(v0, e1, e2, P, w):
    """rayTriangleIntersect (:52-70) of one ray against F triangles: (succ bool [F], t f32 [F])"""
    with np.errstate(all="ignore"):
        q = cross(w[None, :], e2)
        a = dot(e1, q)
        ok = np.abs(a) > F32(0.00001)
        s = (P[None, :] - v0) / a[:, None]
        r = cross(s, e1)
        b0, b1 = dot(s, q), dot(r, w[None, :])
        b2 = (F32(1.0) - b0) - b1
        t = dot(e2, r)
        succ = ok & ~((b0 < 0) | (b1 < 0) | (b2 < 0))
    return succ, np.where(ok, t, F32(0.0))


def uniform_sample_points(npoints):
    """generate_uniform_sample_points (:211-224)"""
    phi = np.pi * (3 - np.sqrt(5))
    out = []
    for i in range(npoints):
        y = 1 - 2 * (i / (npoints - 1))
        radius = np.sqrt(1 - y * y)
        out.append([np.cos(phi * i) * radius, y, np.sin(phi * i) * radius])
    return np.array(out, dtype=F32)


class RefTopo:
    def __init__(self, oracle, coll_det_num=128, max_raycast_dist=2, thres_size=0.5, frontier_creation_threshold=0.5, frontier_verify_threshold=0.5,
                 frontier_backward_check=-0.2, frontier_combine_angle_threshold=40):
        assert 4 <= coll_det_num <= 512
        self.o = oracle
        self.vs = F32(oracle.voxel_scale)
        self.coll_det_num, self.max_raycast_dist, self.thres_size = coll_det_num, max_raycast_dist, thres_size
        self.creation, self.verify, self.backward_check = frontier_creation_threshold, frontier_verify_threshold, frontier_backward_check
        self.dot_thr = F32(np.cos(np.deg2rad(frontier_combine_angle_threshold)))
        self.dirs = uniform_sample_points(coll_det_num)
        self.reset()

    def reset(self):
        self.node_fl = []            # per node: dict of its facelets' arrays
        self.node_center, self.node_master, self.node_range = [], [], []
        self.nfacelets = 0
        self.frontier = []           # the num_frontiers frontiers
        self.search_idx = 0
        self.edges, self.edge_idx, self.connected = [], [], set()
        self.full = False
        self.count = {"expansions": 0, "refused_by_collisions": 0, "refused_by_hull": 0, "frontiers_retracted": 0, "frontiers_valid": 0, "frontiers_invalid": 0}

    # ---- rays ----------------------------------------------------------------------------------------------------------------------------------
    def collide_facelets(self, pos, dir, max_dist, backward, skip):
        """detect_collision_facelets (:472-488): (succ, position, t, poly)"""
        max_dist, backward = F32(max_dist), F32(backward)
        reach = max_dist + F32(self.max_raycast_dist)
        best_t, best_poly, succ = max_dist, -1, False
        for k in range(len(self.node_fl)):
            if k == skip:
                continue
            d = pos - self.node_center[k]
            with np.errstate(all="ignore"):
                if not np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < reach:
                    continue
            fl = self.node_fl[k]
            ok, t = ray_triangles(fl["v0"], fl["edge1"], fl["edge2"], pos, dir)
            with np.errstate(all="ignore"):
                cand = ok & (backward < t) & (t < best_t)
            if cand.any():
                tmin = t[cand].min()
                first = int(np.nonzero(cand & (t == tmin))[0][0])      # the lowest index among equal t: what `t < best_t` in ascending order keeps
                best_t, best_poly, succ = t[first], int(fl["poly"][first]), True
        with np.errstate(all="ignore"):
            x = pos + dir * best_t
        return succ, x, best_t, best_poly

    def map_walk(self, pos, dir, max_dist):
        """BaseMap.raycast as the oracle walks it; a length below 0 makes no step (hit False, position and length 0)"""
        if not max_dist >= 0:
            return False, np.zeros(3, F32), F32(0.0)
        hit, end, ln = self.o.raycast(pos[None, :], dir[None, :], float(max_dist))
        return bool(hit[0]), end[0], ln[0]

    def ray(self, pos, dir, max_dist, skip=-1, backward=-0.01, facelets_only=False):
        """raycast (:490-507): (hit, type, position f32 [3], length, poly)"""
        pos, dir, max_dist = np.asarray(pos, F32), np.asarray(dir, F32), F32(max_dist)
        sp, x, lc, poly = self.collide_facelets(pos, dir, max_dist, backward, skip)
        hit, typ, ln = sp, 1, lc
        if not facelets_only:
            sm, xm, lm = self.map_walk(pos, dir, lc if sp else max_dist)
            if (not sp) or (sm and lm < lc):
                hit, typ, x, ln = sm, 0, xm, lm
        x = np.where(np.isnan(x), QNAN, x).astype(F32)
        return hit, typ, x, F32(ln), poly

    def rays(self, pos, dir, max_dist, skip=None, backward=-0.01, facelets_only=False):
        pos, dir = np.asarray(pos, F32).reshape(-1, 3), np.asarray(dir, F32).reshape(-1, 3)
        n = pos.shape[0]
        skip = np.full(n, -1) if skip is None else np.broadcast_to(np.asarray(skip), (n,))
        r = [self.ray(pos[i], dir[i], max_dist, int(skip[i]), backward, facelets_only) for i in range(n)]
        return (np.array([x[0] for x in r], bool), np.array([x[1] for x in r], np.uint8), np.array([x[2] for x in r], F32).reshape(n, 3),
                np.array([x[3] for x in r], F32), np.array([x[4] for x in r], np.int32))

    # ---- nodes ---------------------------------------------------------------------------------------------------------------------------------
    def add_poly(self, tris, start, max_dist=None):
        """add_mesh up to the node (:380-405): returns (node, centre, is_frontier bool [nf], reason u8 [nf], neigh int32 [nf]); reason 1 the centre is
        unobserved, 2 the voxel in front is occupied, 3 the frontier ray hit"""
        tris, start = np.asarray(tris, F32).reshape(-1, 3, 3), np.asarray(start, F32).reshape(3)
        max_dist = self.creation if max_dist is None else max_dist
        nf, node = tris.shape[0], len(self.node_fl)
        fl = {k: np.zeros((nf, 3), F32) for k in ("v0", "edge1", "edge2", "normal", "center")}
        fl["poly"] = np.full(nf, node, np.int32)
        fl["tri"] = tris.copy()
        is_frontier, reason, neigh = np.zeros(nf, bool), np.zeros(nf, np.uint8), np.full(nf, -1, np.int32)
        csum, count = np.zeros(3, F32), F32(0.0)
        for i in range(nf):
            v0, v1, v2 = tris[i, 0], tris[i, 1], tris[i, 2]
            s = (v0 + v1) + v2
            csum = csum + s
            count = count + F32(3.0)
            naive = normalized(s - F32(3.0) * start)
            e1, e2 = v1 - v0, v2 - v0
            normal = normalized(cross(e1, e2))
            if dot(normal, naive) < 0:
                normal = -normal
            center = s / F32(3.0)
            fl["v0"][i], fl["edge1"][i], fl["edge2"][i], fl["normal"][i], fl["center"][i] = v0, e1, e2, normal, center
            # detect_facelet_frontier (:324-342); is_near_pos_occupy(center, 0) loops over range(-0, 0): false
            if self.o.query_points(1, center[None, :])[0]:
                reason[i] = 1
            else:
                p = center + normal * self.vs
                if self.o.query_points(0, p[None, :])[0]:
                    reason[i] = 2
                else:
                    hit, typ, _, _, poly = self.ray(p, normal, max_dist)          # the nodes before this one: node_fl is appended below
                    if hit:
                        reason[i] = 3
                        if typ == 1:
                            neigh[i] = poly
            is_frontier[i] = reason[i] == 0
        fl["is_frontier"], fl["reason"] = is_frontier, reason
        centre = csum / count
        self.node_fl.append(fl)
        self.node_center.append(centre)
        self.node_master.append(-1)
        self.node_range.append((self.nfacelets, self.nfacelets + nf))
        self.nfacelets += nf
        return node, centre, is_frontier, reason, neigh

    def collide(self, start):
        """detect_collisions (:444-470)"""
        start = np.asarray(start, F32).reshape(3)
        bpos, bdir, blen, nw, total = [], [], [], 0, F32(0.0)
        for i in range(self.coll_det_num):
            hit, _, x, ln, _ = self.ray(start, self.dirs[i], self.max_raycast_dist)
            if hit:
                bpos.append(x); bdir.append(self.dirs[i]); blen.append(ln)
                total = total + ln
            else:
                nw += 1
        with np.errstate(all="ignore"):
            size = total / F32(len(blen))
        succ = not (len(blen) == 0 or (nw == 0 and size < F32(self.thres_size)))
        return succ, np.array(bpos, F32).reshape(-1, 3), np.array(bdir, F32).reshape(-1, 3), np.array(blen, F32), nw, size

    def node_expansion(self, start, last=-1):
        from scipy.spatial import ConvexHull, QhullError
        start = np.asarray(start, F32).reshape(3)
        self.count["expansions"] += 1
        if len(self.node_fl) >= MAX_MAP_NODE:
            self.full = True
            return False
        succ, _, bdir, blen, _, _ = self.collide(start)
        if not succ:
            self.count["refused_by_collisions"] += 1
            return False
        try:
            if bdir.shape[0] < 4:
                raise QhullError("fewer than 4 points")
            hull = ConvexHull(bdir.astype(np.float64))
        except QhullError:
            self.count["refused_by_hull"] += 1
            return False
        verts = np.zeros((bdir.shape[0], 3), F32)
        for i in range(bdir.shape[0]):
            for a in range(3):
                verts[i, a] = F32(float(hull.points[i, a]) * float(blen[i]) + float(start[a]))
        tris, nbr = verts[hull.simplices], hull.neighbors
        node, centre, is_frontier, _, neigh = self.add_poly(tris, start)
        self.node_master[node] = last
        if last >= 0:
            self.edges += [self.node_center[last], centre]; self.edge_idx.append((last, node))
            self.connected |= {(node, last), (last, node)}
        for nb in neigh:
            if nb >= 0 and (node, int(nb)) not in self.connected:
                self.connected |= {(node, int(nb)), (int(nb), node)}
                self.edges += [self.node_center[int(nb)], centre]; self.edge_idx.append((int(nb), node))
        fl = self.node_fl[node]
        assigned = [False] * tris.shape[0]
        for i in range(tris.shape[0]):
            if assigned[i] or not is_frontier[i]:
                continue
            queue, head = [i], 0
            while head < len(queue):
                cur = queue[head]; head += 1
                assigned[cur] = True
                for j in range(3):
                    n2 = int(nbr[cur, j])
                    if is_frontier[n2] and not assigned[n2] and dot(fl["normal"][i], fl["normal"][n2]) > self.dot_thr:
                        queue.append(n2)
            self.construct_frontier(node, fl, queue)
        return True

    def construct_frontier(self, node, fl, queue):
        """:344-378"""
        center, normal = np.zeros(3, F32), np.zeros(3, F32)
        for q in queue:
            center = center + fl["center"][q]
            normal = normal + fl["normal"][q]
        center = center / F32(len(queue))
        normal = normalized(normal / F32(len(queue)))
        succ, t, pn = False, F32(0.0), None
        for q in queue:
            s, tt = ray_triangles(fl["v0"][q:q + 1], fl["edge1"][q:q + 1], fl["edge2"][q:q + 1], center, normal)
            succ, t, pn = bool(s[0]), tt[0], fl["normal"][q]
            if succ:
                break
        if not succ:
            self.count["frontiers_retracted"] += 1
            return
        self.frontier.append({"master_idx": node, "avg_center": center, "outwards_unit_normal": normal, "projected_center": center + t * normal,
                              "projected_normal": pn.copy(), "next_node_initial": np.zeros(3, F32), "is_valid": 0})

    def verify_frontier(self, idx):
        """:255-282"""
        fr = self.frontier[idx]
        n, pc, thr = fr["projected_normal"], fr["projected_center"], F32(self.verify)
        succ, _, _, ln, _ = self.ray(pc + n * F32(0.1), n, F32(self.max_raycast_dist * 2))
        valid = False
        if not (succ and ln < thr):
            succ2, _, _, ln2, _ = self.ray(pc - n * F32(0.1), n, thr, fr["master_idx"], self.backward_check, facelets_only=True)
            if not (succ2 and ln2 < thr):
                if (not succ) or (succ2 and ln2 < ln):
                    ln = ln2
                valid = True
                fr["next_node_initial"] = pc + (n * ln) / F32(2.0)
        fr["is_valid"] = int(valid)
        self.count["frontiers_valid" if valid else "frontiers_invalid"] += 1
        return valid

    def generate_topo_graph(self, start, max_nodes=100):
        """:284-294"""
        self.node_expansion(start)
        while self.search_idx < len(self.frontier) and self.search_idx < max_nodes and not self.full:
            if self.verify_frontier(self.search_idx):
                fr = self.frontier[self.search_idx]
                self.node_expansion(fr["next_node_initial"], fr["master_idx"])
            self.search_idx += 1
        return len(self.node_fl)

    # ---- what the tests compare ------------------------------------------------------------------------------------------------------------------
    def facelets(self):
        keys = ("tri", "v0", "edge1", "edge2", "normal", "center", "poly", "is_frontier", "reason")
        if not self.node_fl:
            return dict({k: np.zeros((0, 3), F32) for k in keys[1:6]}, tri=np.zeros((0, 3, 3), F32), poly=np.zeros(0, np.int32), is_frontier=np.zeros(0, bool),
                        reason=np.zeros(0, np.uint8))
        return {k: np.concatenate([fl[k] for fl in self.node_fl]) for k in keys}

    def nodes(self):
        n = len(self.node_fl)
        return {"center": np.array(self.node_center, F32).reshape(n, 3), "master_idx": np.array(self.node_master, np.int32),
                "start_facelet_idx": np.array([r[0] for r in self.node_range], np.int32), "end_facelet_idx": np.array([r[1] for r in self.node_range], np.int32)}

    def frontiers(self):
        n = len(self.frontier)
        out = {k: np.array([f[k] for f in self.frontier], F32).reshape(n, 3) for k in ("avg_center", "outwards_unit_normal", "projected_center", "projected_normal",
                                                                                     "next_node_initial")}
        out["master_idx"] = np.array([f["master_idx"] for f in self.frontier], np.int32)
        out["is_valid"] = np.array([f["is_valid"] for f in self.frontier], np.int32)
        return out

"""SubmapMapping -- keyframe-stepped submaps over a DenseTSDF / Octomap collection, fused into one global map.

Written against this package's map classes for the orchestration the reference keeps in taichi_slam/mapping/submap_mapping.py:9-267
(the caller of the hot path in swarm mode): same constructor, method and attribute names, same call sequence into the map classes
-- tests/test_reference_callers.py drives the reference's own file and this class through one scenario and compares the traces.

    frames --recast_*_by_frame--> [PGO re-anchoring] -> submap collection (one active submap)
                                     every `keyframe_step` keyframes: export + send the finished submap, open the next, fuse -> global map
    remote submaps / trajectories --input_remote_*--> collection / pose table -> fuse -> global map

Differences from the reference, all opt-in or harmless: `autosave_path` replaces the hard-coded /home/xuhao/... save (:144-145; None =
no autosave), the send handles default to no-ops, and `recast_depth_to_map(R, T, ...)` (stale in the reference: it calls
need_create_new_submap with the wrong arity, :205-210) treats every frame as a keyframe."""
import time

import numpy as np

from . import wire
from .dense_tsdf import DenseTSDF
from .taichi_octomap import Octomap

_COMMON = dict(voxel_scale=0.05, texture_enabled=False, min_ray_length=0.3, max_ray_length=3.0, max_disp_particles=1024 * 1024)
# per map type: (extra keywords of the submap collection, extra keywords of the global map)   submap_mapping.py:13-34, :60-82
_TYPE_OPTS = {
    "tsdf": (dict(num_voxel_per_blk_axis=10, max_submap_num=1000), dict(num_voxel_per_blk_axis=10, max_submap_num=1024)),
    "octo": (dict(K=2, max_submap_num=1000), dict(K=2, max_submap_num=1000)),
}


class _Anchor:
    """Ego-motion -> pose-graph frame.  Poses from the odometry drift; whenever the pose graph publishes an optimised pose for a frame
    the odometry has also seen, later frames are re-expressed relative to that frame (submap_mapping.py:163-170, :106-111)."""

    def __init__(self):
        self.ego, self.pgo, self.last = {}, {}, None

    def note_optimised(self, frame_id):
        if frame_id in self.ego and (self.last is None or frame_id > self.last):
            self.last = frame_id

    def __call__(self, frame_id, R, T):
        self.ego[frame_id] = (R, T)
        if self.last is None:
            return R, T
        Re, Te = self.ego[self.last]
        Rp, Tp = self.pgo[self.last]
        A = Rp @ Re.T
        return A @ R, A @ (T - Te) + Tp


class SubmapMapping:
    def __init__(self, submap_type=DenseTSDF, keyframe_step=20, sub_opts={}, global_opts={}, autosave_path=None):
        self.submap_type = submap_type
        self._kind = "octo" if (isinstance(submap_type, type) and issubclass(submap_type, Octomap)) else "tsdf"
        self.keyframe_step = keyframe_step
        self.autosave_path = autosave_path
        self.sub_opts = dict(_COMMON, map_scale=[10, 10], **_TYPE_OPTS[self._kind][0])
        self.sub_opts.update(sub_opts)
        self.submaps = {}                         # frame id of a submap's first frame -> submap id in the collection / global pose table
        self.frame_count = 0
        self.first_init = True
        self.active_submap_frame_id = 0
        self.exporting_global = False
        self.export_TSDF_xyz = self.export_color = self.export_x = None
        self.post_local_to_global_callback = None
        self.map_send_handle = lambda buf: None
        self.traj_send_handle = lambda buf: None
        self._anchor = _Anchor()
        self.opened = {}                          # frame id of an own submap -> the pose (R, T) it was opened at: the odometry edges of optimize_poses
        self.constraints = []                     # add_constraint: (frame_a, frame_b, R, T, information)
        self._pose_graph = None
        self.submap_collection = submap_type(**self.sub_opts)
        self.global_map = self.create_globalmap(global_opts)
        self.enable_texture = self.global_map.enable_texture
        self.set_exporting_global()

    # the reference exposes these three dicts / the frame id as plain attributes (scripts/taichislam_node.py reads them)
    ego_motion_poses = property(lambda self: self._anchor.ego)
    pgo_poses = property(lambda self: self._anchor.pgo)
    last_frame_id = property(lambda self: self._anchor.last)

    def create_globalmap(self, global_opts={}):
        opts = dict(_COMMON, map_scale=[100, 100], is_global_map=True, **_TYPE_OPTS[self._kind][1])
        opts.update(global_opts)
        return self.submap_type(**opts)

    # ---- camera / export selection ---------------------------------------------------------------------------------------------------
    def set_dep_camera_intrinsic(self, K):
        self.submap_collection.set_dep_camera_intrinsic(K)

    def set_color_camera_intrinsic(self, K):
        self.submap_collection.set_color_camera_intrinsic(K)

    def set_export_submap(self, new_submap):
        self.export_color = new_submap.export_color
        if self._kind == "tsdf":
            self.export_TSDF_xyz, self.num_TSDF_particles = new_submap.export_TSDF_xyz, new_submap.num_TSDF_particles
        else:
            self.export_x, self.num_export_particles = new_submap.export_x, new_submap.num_export_particles

    def set_exporting_global(self):
        self.exporting_global = True
        self.set_export_submap(self.global_map)

    def set_exporting_local(self):
        self.exporting_global = False
        self.set_export_submap(self.submap_collection)

    # ---- pose graph --------------------------------------------------------------------------------------------------------------------
    def set_frame_poses(self, frame_poses, from_remote=False):
        """Optimised poses {frame_id: (R, T)}: re-anchor the odometry and move the base poses of the submaps that start on these frames."""
        self._anchor.pgo.update(frame_poses)
        moved = {}
        for fid, (R, T) in ((f, (p[0], p[1])) for f, p in frame_poses.items()):
            self._anchor.note_optimised(fid)
            sid = self.submaps.get(fid)
            if sid is not None:
                self.global_map.set_base_pose_submap(sid, R, T)
                moved[fid] = frame_poses[fid]
        if not from_remote:                      # our own optimisation: tell the other agents which submaps moved
            self.send_traj(moved)

    def convert_by_pgo(self, frame_id, R, T):
        return self._anchor(frame_id, R, T)

    def register_submaps(self, frame_a, frame_b, **kw):
        """Register the collection's submap that starts on frame_a (source) against the one that starts on frame_b (destination): whether the two
        agree where they overlap, as a constraint for the pose graph.  The guess is P_b^-1 P_a from the global map's pose table; returns (R, T, info),
        the refined pose taking submap a's coordinates to submap b's and DenseTSDF.register_submap's info with "information" (the 6 x 6 matrix H of
        the last linearisation, float64, twist order (v, omega) in submap b's frame), "guess" (R, T) and "submaps" (sid_a, sid_b).  Nothing moves: no
        base pose, no map and not the active submap.  kw: the keywords of DenseTSDF.register_submap.  (Not in the reference, which has no registration;
        TSDF collections only.)"""
        return self._constrain("register_submaps", "register_submap", frame_a, frame_b, kw)

    def search_submaps(self, frame_a, frame_b, **kw):
        """register_submaps with DenseTSDF.register_search in place of register_submap: for a pose table that may have drifted past the basin of
        the registration (a loop closure).  The same guess P_b^-1 P_a, the same return (R, T, info) with "information", "guess" and "submaps";
        info["search"] is the search's report.  Nothing moves.  kw: the keywords of DenseTSDF.register_search."""
        return self._constrain("search_submaps", "register_search", frame_a, frame_b, kw)

    def _constrain(self, who, method, frame_a, frame_b, kw):
        """register_submaps / search_submaps: the guess from the pose table, the collection's `method` on the two submaps, the fields of the constraint"""
        if self._kind != "tsdf":
            raise TypeError(f"{who} needs a DenseTSDF collection")
        sa, sb = self.submaps[frame_a], self.submaps[frame_b]
        g = self.global_map
        Ra, Ta, Rb, Tb = g.submaps_base_R_np[sa], g.submaps_base_T_np[sa], g.submaps_base_R_np[sb], g.submaps_base_T_np[sb]
        R0, T0 = Rb.T @ Ra, Rb.T @ (Ta - Tb)
        col = self.submap_collection
        R, T, info = getattr(col, method)(col, R0, T0, src_sid=sa, dst_sid=sb, **kw)
        info["information"] = info["records"][-1]["H_f"].copy() if info["records"] else np.zeros((6, 6))
        info["guess"], info["submaps"] = (R0, T0), (sa, sb)
        return R, T, info

    def add_constraint(self, frame_a, frame_b, R, T, information):
        """Append a pose-graph constraint: P_b^-1 P_a was measured as (R, T) with the 6 x 6 information matrix `information` (twist order (v, omega), the left
        twist in b's frame) -- exactly what register_submaps(frame_a, frame_b) / search_submaps return as R, T and info["information"].  Returns its index
        in self.constraints."""
        R, T, L = np.array(R, np.float64).reshape(3, 3), np.array(T, np.float64).reshape(3), np.array(information, np.float64).reshape(6, 6)
        if frame_a == frame_b:
            raise ValueError("add_constraint: a constraint joins two different submaps")
        self.constraints.append((frame_a, frame_b, R, T, L))
        return len(self.constraints) - 1

    def _graph(self, odom_information, fixed):
        """The pose graph as arrays.  Nodes: the known submaps in ascending frame id, at the global map's base poses.  Edges: first an odometry edge between
        every two consecutive own submaps, measured from the poses they were opened at (a = the later one), then the constraints in the order they were
        added.  fixed: frame ids, None = the first own submap."""
        from ..utils.pose import pose_information
        frames = sorted(self.submaps)
        at = {f: n for n, f in enumerate(frames)}
        g = self.global_map
        sid = [self.submaps[f] for f in frames]
        R, T = np.array(g.submaps_base_R_np[sid], np.float64), np.array(g.submaps_base_T_np[sid], np.float64)
        own = sorted(f for f in self.opened if f in at)
        if fixed is None:
            if not own:
                raise ValueError("optimize_poses: no own submap to fix; name the fixed frames")
            fixed = [own[0]]
        fx = np.zeros(len(frames), np.uint8)
        fx[[at[f] for f in fixed]] = 1
        Lo = pose_information(0.05, 0.02) if odom_information is None else np.array(odom_information, np.float64).reshape(6, 6)
        ij, Rz, Tz, L = [], [], [], []
        for prev, nxt in zip(own[:-1], own[1:]):
            (Rp, Tp), (Rn, Tn) = self.opened[prev], self.opened[nxt]
            ij.append((at[nxt], at[prev])); Rz.append(Rp.T @ Rn); Tz.append(Rp.T @ (Tn - Tp)); L.append(Lo)
        n_odom = len(ij)
        for fa, fb, Rc, Tc, Lc in self.constraints:
            if fa not in at or fb not in at:
                raise KeyError(f"a constraint names frame {fa if fa not in at else fb}, which opens no known submap")
            ij.append((at[fa], at[fb])); Rz.append(Rc); Tz.append(Tc); L.append(Lc)
        if not ij:
            raise ValueError("optimize_poses: the graph has no edge")
        return frames, R, T, fx, np.array(ij, np.int32), np.array(Rz), np.array(Tz), np.array(L), n_odom

    def _solver(self, n, e, b):
        """a PoseGraph with room for n poses, e edges and b variants on the global map's device, kept and regrown by doubling"""
        from .pose_graph import PoseGraph
        pg = self._pose_graph
        if pg is None or pg.max_poses < n or pg.max_edges < e or pg.max_variants < b:
            def cap(x, lo):
                return max(lo, 1 << (int(x) - 1).bit_length())
            self._pose_graph = pg = PoseGraph(cap(n, 64), cap(e, 256), cap(b, 1), device=getattr(self.global_map, "device", 0))
        return pg

    def optimize_poses(self, odom_information=None, fixed=None, apply=False, **solver_kw):
        """Solve the pose graph of the known submaps (see _graph for its nodes and edges; odom_information: the 6 x 6 information of an odometry edge, None =
        utils.pose_information(0.05, 0.02)).  Returns ({frame_id: (R, T)}, report): the optimised base poses and {"status" (PoseGraph.STATUS_NAMES index),
        "iterations", "cost", "records", "edge_cost" (r^T L r per edge at the result), "edges" [(frame_a, frame_b)], "n_odometry"}.  apply=True passes the
        poses to set_frame_poses; otherwise nothing moves.  solver_kw: the keywords of PoseGraph.solve."""
        from .pose_graph import pack_measurements
        frames, R, T, fx, ij, Rz, Tz, L, n_odom = self._graph(odom_information, fixed)
        out = self._solver(len(frames), len(ij), 1).solve(R, T, fx, ij, pack_measurements(Rz, Tz), L, **solver_kw)
        rep = out["report"][0]
        poses = {f: (out["R"][0, n].copy(), out["T"][0, n].copy()) for n, f in enumerate(frames)}
        report = {"status": int(rep["status"]), "iterations": int(rep["iterations"]), "cost": float(rep["cost"]), "records": rep["it"][:int(rep["iterations"])].copy(),
                  "edge_cost": out["edge_cost"][0].copy(), "edges": [(frames[a], frames[b]) for a, b in ij], "n_odometry": n_odom}
        if apply:
            self.set_frame_poses(poses)
        return poses, report

    def check_constraints(self, odom_information=None, fixed=None, **solver_kw):
        """Leave-one-out over the constraints, all in one launch: the graph is solved with every edge and once without each constraint, and constraint k is
        read under the solution that did not see it.  Returns {"loo_cost" [K], "full_cost" [K], "status" [1 + K], "order": the constraints from the most
        to the least consistent (ascending loo_cost)}.  The costs are raw r^T L r values to compare and rank: odometry drift loosens the prediction and L is
        not its covariance, so they are no chi-square to threshold.  A constraint whose removal cuts the graph (status 4) reads inf.  Nothing moves."""
        from .pose_graph import pack_measurements
        if not self.constraints:
            raise ValueError("check_constraints: no constraint")
        frames, R, T, fx, ij, Rz, Tz, L, n_odom = self._graph(odom_information, fixed)
        K = len(self.constraints)
        out = self._solver(len(frames), len(ij), 1 + K).leave_one_out(R, T, fx, ij, pack_measurements(Rz, Tz), L, n_odom + np.arange(K), **solver_kw)
        status = out["report"]["status"].astype(np.int32)
        loo = np.where(status[1:] == 4, np.inf, out["loo_cost"])
        return {"loo_cost": loo, "full_cost": out["full_cost"], "status": status, "order": np.argsort(loo, kind="stable")}

    # ---- submap life cycle -----------------------------------------------------------------------------------------------------------------
    def need_create_new_submap(self, is_keyframe, R=None, T=None):
        return self.frame_count == 0 or (bool(is_keyframe) and self.frame_count % self.keyframe_step == 0)

    def create_new_submap(self, frame_id, R, T):
        col = self.submap_collection
        if self.first_init:
            self.first_init = False
        else:                                    # close the active submap: ship it, open the next slot, refresh the global map
            self.send_submap(col.export_submap())
            col.switch_to_next_submap()
            col.clear_last_TSDF_exporting = True
            self.local_to_global()
        sid = col.get_active_submap_id()
        for m in (self.global_map, col):
            m.set_base_pose_submap(sid, R, T)
        self.submaps[frame_id] = sid
        self.opened[frame_id] = (np.array(R, np.float64), np.array(T, np.float64).reshape(3))
        self._anchor.pgo[frame_id] = (R, T)
        self.active_submap_frame_id = frame_id
        print(f"[SubmapMapping] frame {frame_id} opens submap {sid} ({sid + 1} local submaps)")
        if self.autosave_path and sid % 2 == 0:
            self.saveMap(self.autosave_path)
        return col

    def local_to_global(self):
        self.global_map.fuse_submaps(self.submap_collection)
        if self.post_local_to_global_callback is not None:
            self.post_local_to_global_callback(self.global_map)

    def _frame(self, frame_id, is_keyframe, pose, ext):
        """Common part of the two by-frame entry points: anchored body pose, submap roll-over, camera pose."""
        R, T = self._anchor(frame_id, pose[0], pose[1])
        if self.need_create_new_submap(is_keyframe, R, T):
            self.create_new_submap(frame_id, R, T)
        return R @ ext[0], T + R @ ext[1]

    def recast_depth_to_map_by_frame(self, frame_id, is_keyframe, pose, ext, depthmap, texture):
        Rc, Tc = self._frame(frame_id, is_keyframe, pose, ext)
        self.submap_collection.recast_depth_to_map(Rc, Tc, depthmap, texture)
        self.frame_count += 1

    def recast_pcl_to_map_by_frame(self, frame_id, is_keyframe, pose, ext, pcl, rgb_array):
        Rc, Tc = self._frame(frame_id, is_keyframe, pose, ext)
        self.submap_collection.recast_pcl_to_map(Rc, Tc, pcl, rgb_array)
        self.frame_count += 1

    def recast_depth_to_map(self, R, T, depthmap, texture):
        if self.need_create_new_submap(True, R, T):
            self.create_new_submap(self.frame_count, R, T)          # no frame ids from the caller: the frame counter stands in
        self.submap_collection.recast_depth_to_map(R, T, depthmap, texture)
        self.frame_count += 1

    # ---- visualisation exports ---------------------------------------------------------------------------------------------------------------
    def _shown(self):
        return self.global_map if self.exporting_global else self.submap_collection

    def cvt_TSDF_to_voxels_slice(self, z):
        self._shown().cvt_TSDF_to_voxels_slice(z)

    def cvt_TSDF_surface_to_voxels(self):
        if not self.submaps:
            return
        self._shown().cvt_TSDF_surface_to_voxels()
        if self.exporting_global:                # the active submap is not fused yet: append it to the global map's particles
            g = self.global_map
            self.submap_collection.cvt_TSDF_surface_to_voxels_to(g.num_TSDF_particles, g.max_disp_particles, self.export_TSDF_xyz, self.export_color)

    def cvt_occupy_to_voxels(self, level):
        self._shown().cvt_occupy_to_voxels(level)
        if self.exporting_global:
            g = self.global_map
            self.submap_collection.cvt_occupy_voxels_to(level, g.num_export_particles, g.max_disp_particles, self.export_x, self.export_color)

    # ---- exchange with the other agents ----------------------------------------------------------------------------------------------------------
    def send_submap(self, submap):
        submap["frame_id"] = self.active_submap_frame_id
        submap["pose"] = self._anchor.pgo[self.active_submap_frame_id]
        t0 = time.time()
        buf, raw = wire.pack(submap)
        self.map_send_handle(buf)
        print(f"[SubmapMapping] submap sent: {raw / 1024.0:.1f} kB -> {len(buf) / 1024:.1f} kB on the wire, packed in {(time.time() - t0) * 1000:.1f} ms")

    def send_traj(self, traj):
        t0 = time.time()
        buf, raw = wire.pack(traj)
        self.traj_send_handle(buf)
        print(f"[SubmapMapping] trajectory sent: {len(traj)} poses, {len(buf) / 1024:.1f} kB on the wire ({(time.time() - t0) * 1000:.1f} ms)")

    def input_remote_submap(self, buf):
        submap = wire.unpack(buf)
        print(f"[SubmapMapping] remote submap of frame {submap['frame_id']}: {len(buf) / 1024:.1f} kB on the wire, {len(submap['TSDF']) if 'TSDF' in submap else 0} voxels")
        sid = self.submap_collection.input_remote_submap(submap)
        self.global_map.set_base_pose_submap(sid, submap["pose"][0], submap["pose"][1])
        self.local_to_global()
        self.submaps[submap["frame_id"]] = sid

    def input_remote_traj(self, buf):
        traj = wire.unpack(buf)
        self.set_frame_poses(traj, True)
        print(f"[SubmapMapping] remote trajectory: {len(traj)} poses ({len(buf) / 1024.0:.1f} kB)")

    def saveMap(self, filename):
        self.global_map.saveMap(filename)

    def export_submap(self):
        return self.submap_collection.export_submap()

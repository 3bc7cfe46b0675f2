"""ctypes loader of libtaichislam_hip.so (include/taichislam_hip.h).  There is NO CPU fallback: if the HIP
library cannot be loaded, importing the mapping classes raises."""
import ctypes as C
import os

from . import build as _build

TSL_OK = 0
K_VOXELIZE, K_SORT, K_RAYS, K_INTEGRATE, K_FINALIZE, K_MESH, K_SEGMENTS, K_BIN, K_ESDF, K_FUSE, K_REGISTER, K_REGISTER_SCORE = range(12)
K_FRONTIER_MARK, K_FRONTIER_LABEL, K_FRONTIER_JOIN, K_FRONTIER_SUM, K_FRONTIER_EMIT = range(12, 17)
K_VIEW_GAIN, K_ALIGN, K_ALIGN_POINTS, K_PATH_SCORE = 17, 18, 19, 20
K_NAV_PROJECT, K_NAV_EDT, K_NAV_EDT_ROWS = 21, 22, 23
K_NAV_FIELD_SEED, K_NAV_FIELD_ROUND, K_NAV_FIELD_PARENT, K_NAV_FIELD_PATHS = 24, 25, 26, 27
K_NAV_TERRAIN_COLUMNS, K_NAV_TERRAIN_WINDOW = 28, 29
K_ALIGN_RGBD = 30
K_EVICT = 31
KERNEL_NAMES = {K_VOXELIZE: "voxelize", K_SORT: "sort", K_RAYS: "build_rays", K_INTEGRATE: "integrate",
                K_FINALIZE: "finalize", K_MESH: "marching_cubes", K_SEGMENTS: "segments", K_BIN: "bin", K_ESDF: "esdf", K_FUSE: "fuse", K_REGISTER: "register",
                K_REGISTER_SCORE: "register_score", K_FRONTIER_MARK: "frontier_mark", K_FRONTIER_LABEL: "frontier_label", K_FRONTIER_JOIN: "frontier_join",
                K_FRONTIER_SUM: "frontier_sum", K_FRONTIER_EMIT: "frontier_emit", K_VIEW_GAIN: "view_gain", K_ALIGN: "align", K_ALIGN_POINTS: "align_points",
                K_PATH_SCORE: "path_score", K_NAV_PROJECT: "nav_project", K_NAV_EDT: "nav_edt", K_NAV_EDT_ROWS: "nav_edt_rows",
                K_NAV_FIELD_SEED: "nav_field_seed", K_NAV_FIELD_ROUND: "nav_field_round", K_NAV_FIELD_PARENT: "nav_field_parent",
                K_NAV_FIELD_PATHS: "nav_field_paths", K_NAV_TERRAIN_COLUMNS: "nav_terrain_columns", K_NAV_TERRAIN_WINDOW: "nav_terrain_window", K_ALIGN_RGBD: "align_rgbd", K_EVICT: "evict"}


class TsdfCfg(C.Structure):
    _fields_ = [("map_size_xy", C.c_double), ("map_size_z", C.c_double), ("voxel_scale", C.c_double),
                ("num_voxel_per_blk_axis", C.c_int32), ("max_ray_length", C.c_double), ("min_ray_length", C.c_double),
                ("internal_voxels", C.c_int32), ("max_submap_num", C.c_int32), ("is_global_map", C.c_int32),
                ("texture_enabled", C.c_int32), ("disp_ceiling", C.c_double), ("disp_floor", C.c_double),
                ("recast_step", C.c_int32), ("color_same_proj", C.c_int32), ("max_disp_particles", C.c_int64),
                ("max_bricks", C.c_int32), ("max_frame_bricks", C.c_int32), ("max_points", C.c_int32)]


class OctoCfg(C.Structure):
    _fields_ = [("map_size_xy", C.c_double), ("map_size_z", C.c_double), ("voxel_scale", C.c_double),
                ("min_occupy_thres", C.c_double), ("texture_enabled", C.c_int32),
                ("min_ray_length", C.c_double), ("max_ray_length", C.c_double), ("K", C.c_int32),
                ("max_submap_num", C.c_int32), ("disp_ceiling", C.c_double), ("disp_floor", C.c_double),
                ("is_global_map", C.c_int32), ("recast_step", C.c_int32), ("color_same_proj", C.c_int32),
                ("max_disp_particles", C.c_int64), ("max_bricks", C.c_int32), ("max_points", C.c_int32)]


class FrameStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("p_used", "p_valid", "p_oob", "v_pcl", "v_skipped", "steps",
                                          "steps_oob", "unique", "bricks")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class EsdfStats(C.Structure):
    _fields_ = [("incremental", C.c_int32), ("dirty_bricks", C.c_int32), ("changed_bricks", C.c_int32), ("region_bricks", C.c_int32), ("total_bricks", C.c_int32),
                ("brick_relaxations", C.c_int64), ("voxel_pushes", C.c_int64), ("rounds", C.c_int32), ("max_passes", C.c_int32), ("raise_sets", C.c_int32), ("passes", C.c_int64), ("voxels_raised", C.c_int64), ("max_raise_sets", C.c_int32), ("reserved_", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class EsdfTotals(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("updates", "incremental", "dirty_bricks", "region_bricks", "brick_relaxations", "voxel_pushes", "passes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ViewCfg(C.Structure):
    """tsl_view_cfg (tsl_tsdf_render_view): a zero K / t_min / t_max / dt means the map's default"""
    _fields_ = [("K", C.c_double * 9), ("h", C.c_int32), ("w", C.c_int32), ("t_min", C.c_float), ("t_max", C.c_float), ("dt", C.c_float),
                ("flags", C.c_int32)]


class AlignCfg(C.Structure):
    """tsl_align_cfg (tsl_tsdf_align_linearize, tsl_tsdf_track_depth): a zero K / d_min / d_max / r_max / g_max means the default, huber 0 = off"""
    _fields_ = [("K", C.c_double * 9), ("h", C.c_int32), ("w", C.c_int32), ("stride", C.c_int32), ("d_min", C.c_float), ("d_max", C.c_float),
                ("r_max", C.c_float), ("g_max", C.c_float), ("huber", C.c_float), ("flags", C.c_int32)]


class AlignPointsCfg(C.Structure):
    """tsl_align_points_cfg (tsl_tsdf_align_points_linearize, tsl_tsdf_track_points): a zero d_min / d_max / r_max / g_max means the default, huber 0 = off"""
    _fields_ = [("stride", C.c_int32), ("d_min", C.c_float), ("d_max", C.c_float), ("r_max", C.c_float), ("g_max", C.c_float), ("huber", C.c_float),
                ("flags", C.c_int32)]


class AlignSums(C.Structure):
    """tsl_align_sums: the normal equations in 2^-20 fixed point and the five pixel counts, 33 x int64"""
    _fields_ = [("H", C.c_int64 * 21), ("b", C.c_int64 * 6)] + [(n, C.c_int64) for n in ("e", "n_used", "n_gate", "n_unknown", "n_far", "n_grad")]


class RegisterCfg(C.Structure):
    """tsl_register_cfg (tsl_tsdf_register_linearize, tsl_tsdf_register_submap): a zero band / r_max / g_max means the default, w_min 0 = every weight, huber 0 = off"""
    _fields_ = [("stride", C.c_int32), ("w_min", C.c_float), ("band", C.c_float), ("r_max", C.c_float), ("g_max", C.c_float), ("huber", C.c_float),
                ("flags", C.c_int32)]


class TrackCfg(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("stride", C.c_int32 * 4), ("iters", C.c_int32 * 4), ("min_used", C.c_int32), ("min_step", C.c_double),
                ("damping", C.c_double)]


class TrackIter(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("xi", C.c_double * 6), ("sums", AlignSums)]


class TrackReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("it", TrackIter * 64)]


class AlignRgbdCfg(C.Structure):
    """tsl_align_rgbd_cfg (tsl_tsdf_align_rgbd_linearize, tsl_tsdf_track_rgbd): a tsl_align_cfg and the colour gates; a zero rc_max / gc_max means the default, huber_c 0 = off"""
    _fields_ = [("a", AlignCfg), ("rc_max", C.c_float), ("gc_max", C.c_float), ("huber_c", C.c_float)]


class AlignRgbdSums(C.Structure):
    """tsl_align_rgbd_sums: the geometric and the colour tsl_align_sums, 66 x int64"""
    _fields_ = [("geo", AlignSums), ("col", AlignSums)]


class TrackRgbdIter(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("xi", C.c_double * 6), ("sums", AlignRgbdSums)]


class TrackRgbdReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("lam", C.c_double), ("it", TrackRgbdIter * 64)]


class RegisterScore(C.Structure):
    """tsl_register_score (tsl_tsdf_register_score): e and four of the five counts of a linearisation, 24 bytes"""
    _fields_ = [("e", C.c_int64), ("n_used", C.c_int32), ("n_unknown", C.c_int32), ("n_far", C.c_int32), ("n_grad", C.c_int32)]


class RegisterGate(C.Structure):
    """tsl_register_gate: the pose-independent part of a score call"""
    _fields_ = [(n, C.c_int64) for n in ("n_gate", "n_pass", "sum_i", "sum_j", "sum_k")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SearchCfg(C.Structure):
    """tsl_search_cfg (tsl_tsdf_register_search): half-counts and steps of the lattice, the pivot (flags bit 0: given), the scoring stride, miss, min_used"""
    _fields_ = [("n_t", C.c_int32 * 3), ("step_t", C.c_double * 3), ("n_r", C.c_int32 * 3), ("step_r", C.c_double * 3), ("pivot", C.c_double * 3),
                ("flags", C.c_int32), ("stride", C.c_int32), ("miss", C.c_float), ("min_used", C.c_int32)]


class SearchReport(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_candidates", C.c_int32), ("n_valid", C.c_int32), ("best", C.c_int32), ("J_best", C.c_int64),
                ("score_best", RegisterScore), ("pivot", C.c_double * 3), ("R_best", C.c_double * 9), ("T_best", C.c_double * 3), ("gate", RegisterGate)]


class FrontierCfg(C.Structure):
    """tsl_frontier_cfg (tsl_tsdf_frontier_extract): free_thres 0 = the map's surface threshold, k_min > k_max = no height limit, min_unknown /
    connectivity / min_cluster 0 = 1 / 26 / 1, flags bit 0 = no occupied voxel among the 26 neighbours"""
    _fields_ = [("free_thres", C.c_float), ("k_min", C.c_int32), ("k_max", C.c_int32), ("min_unknown", C.c_int32), ("connectivity", C.c_int32),
                ("min_cluster", C.c_int32), ("flags", C.c_int32)]


class FrontierCluster(C.Structure):
    """tsl_frontier_cluster: 64 bytes, the layout of FRONTIER_CLUSTER_DTYPE"""
    _fields_ = [("key", C.c_int32), ("count", C.c_int32), ("sum", C.c_int64 * 3), ("nsum", C.c_int32 * 3), ("lo", C.c_int16 * 3), ("hi", C.c_int16 * 3),
                ("reserved_", C.c_int32 * 2)]


class GainCfg(C.Structure):
    """tsl_gain_cfg (tsl_tsdf_view_gain): a zero K / t_min / t_max / dt / free_thres means the map's default, unknown_run 0 = no cut, flags bit 0 = every
    sample is evaluated"""
    _fields_ = [("K", C.c_double * 9), ("h", C.c_int32), ("w", C.c_int32), ("t_min", C.c_float), ("t_max", C.c_float), ("dt", C.c_float),
                ("free_thres", C.c_float), ("unknown_run", C.c_int32), ("flags", C.c_int32)]


class ViewGain(C.Structure):
    """tsl_view_gain: 64 bytes per pose, the layout of VIEW_GAIN_DTYPE"""
    _fields_ = [("n_unknown", C.c_int64), ("n_free", C.c_int64), ("vol_unknown", C.c_int64), ("vol_free", C.c_int64), ("n_hit", C.c_int32),
                ("n_range", C.c_int32), ("n_cut", C.c_int32), ("n_frontier", C.c_int32), ("reserved_", C.c_int32 * 4)]


class PathScore(C.Structure):
    """tsl_path_score: 40 bytes per path, the layout of PATH_SCORE_DTYPE"""
    _fields_ = [("n_samples", C.c_int32), ("first_stop", C.c_int32), ("n_hit", C.c_int32), ("n_unknown", C.c_int32), ("n_outside", C.c_int32),
                ("argmin", C.c_int32), ("min_dist", C.c_float), ("short_update", C.c_int32), ("cost", C.c_int64)]


class TrajScore(C.Structure):
    """tsl_traj_score: 48 bytes per trajectory, the layout of TRAJ_SCORE_DTYPE"""
    _fields_ = [("n_samples", C.c_int32), ("n_pen", C.c_int32), ("n_unknown", C.c_int32), ("n_outside", C.c_int32), ("argmin", C.c_int32),
                ("min_dist", C.c_float), ("short_update", C.c_int32), ("iters_done", C.c_int32), ("cost_collision", C.c_int64), ("cost_smooth", C.c_int64)]


class TrajOpt(C.Structure):
    """tsl_traj_opt (tsl_esdf_traj_optimize): flags bit 0 = stop at the first linearisation without a penalised sample"""
    _fields_ = [("clearance", C.c_float), ("w_collision", C.c_float), ("w_smooth", C.c_float), ("step", C.c_float), ("momentum", C.c_float),
                ("max_move", C.c_float), ("sub", C.c_int32), ("iters", C.c_int32), ("fix_head", C.c_int32), ("fix_tail", C.c_int32), ("flags", C.c_int32),
                ("reserved_", C.c_int32)]


class NavCfg(C.Structure):
    """tsl_nav_cfg (tsl_tsdf_nav_grid): n_bands bands of voxel layers k_min[b] .. k_max[b]; free_thres 0 = the map's surface threshold, min_occ / min_free
    0 = 1, max_unknown < 0 = no limit, radius in voxels, flags bit 0 = unknown cells are obstacles, bit 1 = so is the wall of the volume"""
    _fields_ = [("n_bands", C.c_int32), ("k_min", C.c_int32 * 16), ("k_max", C.c_int32 * 16), ("free_thres", C.c_float), ("min_occ", C.c_int32),
                ("min_free", C.c_int32), ("max_unknown", C.c_int32), ("radius", C.c_int32), ("flags", C.c_int32), ("cost_unknown", C.c_uint8),
                ("reserved_", C.c_uint8 * 3)]


class NavFieldCfg(C.Structure):
    """tsl_nav_field_cfg (tsl_tsdf_nav_field, tsl_tsdf_nav_field_paths): B planes of H x W cells; neutral and lethal in 1 .. 255, connectivity 4 or 8, max_rounds
    0 = 4 * tiles + 64, rounds_fixed > 0 = that many rounds and no host read, check_every 0 = 8"""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("neutral", C.c_int32), ("lethal", C.c_int32), ("connectivity", C.c_int32),
                ("max_rounds", C.c_int32), ("rounds_fixed", C.c_int32), ("check_every", C.c_int32), ("reserved_", C.c_int32)]


class NavFieldStats(C.Structure):
    """tsl_nav_field_stats"""
    _fields_ = [("converged", C.c_int32), ("rounds", C.c_int32), ("tile_visits", C.c_int64), ("n_bad_seeds", C.c_int32), ("reserved_", C.c_int32)]


NAV_UNREACHED = 0xffffffff


class NavField3Cfg(C.Structure):
    """tsl_nav_field3_cfg (tsl_tsdf_nav_field3, tsl_tsdf_nav_field3_paths): a volume of D layers of H x W cells; neutral and lethal in 1 .. 255, connectivity
    6, 18 or 26, max_rounds 0 = min(4 * tiles + 64, 65536), rounds_fixed > 0 = that many rounds and no host read, check_every 0 = 8"""
    _fields_ = [("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("neutral", C.c_int32), ("lethal", C.c_int32), ("connectivity", C.c_int32),
                ("max_rounds", C.c_int32), ("rounds_fixed", C.c_int32), ("check_every", C.c_int32), ("reserved_", C.c_int32)]


class NavField3Stats(C.Structure):
    """tsl_nav_field3_stats (the layout of tsl_nav_field_stats)"""
    _fields_ = [("converged", C.c_int32), ("rounds", C.c_int32), ("tile_visits", C.c_int64), ("n_bad_seeds", C.c_int32), ("reserved_", C.c_int32)]


NAV3_SEED = 26                  # TSL_NAV3_SEED: the parent code of a goal cell of DenseTSDF.nav_field3d


class NavCorridorCfg(C.Structure):
    """tsl_nav_corridor_cfg (tsl_tsdf_nav_boxes, tsl_tsdf_nav_corridor): a volume of D layers of H x W cells; a cell is free when cost < free_below (1 ..
    255); ext_k, ext_i, ext_j in 0 .. 127: the reach of a box from its seed; max_boxes in 1 .. L (the corridor forms only)"""
    _fields_ = [("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("free_below", C.c_int32), ("ext_k", C.c_int32), ("ext_i", C.c_int32),
                ("ext_j", C.c_int32), ("max_boxes", C.c_int32)]


BOX_BLOCKED, BOX_OUTSIDE = 1, 2     # TSL_BOX_*: the flags of DenseTSDF.nav_boxes


class NavTerrainCfg(C.Structure):
    """tsl_nav_terrain_cfg (tsl_tsdf_nav_terrain): the bands and free_thres of tsl_nav_cfg; clearance and free_run in layers above the support, pick 0 = the
    lowest / 1 = the highest standable layer, window and slope_base in cells, max_step in sixteenths of a voxel, max_slope2 = (tan * 128 * slope_base)^2
    (2^32 - 1 = no limit); radius, flags and cost_unknown as in tsl_nav_cfg"""
    _fields_ = [("n_bands", C.c_int32), ("k_min", C.c_int32 * 16), ("k_max", C.c_int32 * 16), ("free_thres", C.c_float), ("clearance", C.c_int32),
                ("free_run", C.c_int32), ("pick", C.c_int32), ("window", C.c_int32), ("slope_base", C.c_int32), ("max_step", C.c_int32),
                ("min_support", C.c_int32), ("max_slope2", C.c_uint32), ("radius", C.c_int32), ("flags", C.c_int32), ("cost_unknown", C.c_uint8),
                ("reserved_", C.c_uint8 * 3)]


TERRAIN_NO_HEIGHT, TERRAIN_NO_STAT, TERRAIN_NO_SLOPE = 32767, 65535, 0xffffffff


EVICT_KEEP_BOX, EVICT_CLEAR_BOX, EVICT_KEYS = 0, 1, 2      # TSL_EVICT_*: the selection rules of DenseTSDF.evict
RESTORE_SKIP, RESTORE_OVERWRITE = 0, 1                      # TSL_RESTORE_*


class EvictCfg(C.Structure):
    """tsl_evict_cfg (tsl_tsdf_evict): the rule, the slot of the box rules (-1 = every slot), the inclusive voxel box, release 1 = give the bricks back"""
    _fields_ = [("rule", C.c_int32), ("sid", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("release", C.c_int32), ("reserved_", C.c_int32)]


class EvictStats(C.Structure):
    """tsl_evict_stats"""
    _fields_ = [(n, C.c_int32) for n in ("selected", "missing", "moved", "bricks_before", "bricks_after", "restored", "skipped", "reserved_")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved_"}


class DepthCfg(C.Structure):
    """tsl_depth_cfg (tsl_depth_condition): the batch n x h x w, the range gate in mm, min_support 0 .. 8, erode 0 .. 3, radius 0 .. 4, flags bit 0 = holes
    erode too, levels 0 .. 3, min_valid 1 .. 4"""
    _fields_ = [(n, C.c_int32) for n in ("n", "h", "w", "d_min_mm", "d_max_mm", "min_support", "erode", "radius", "flags", "levels", "min_valid", "reserved_")]


DEPTH_KEPT, DEPTH_HOLE, DEPTH_RANGE, DEPTH_SPARSE, DEPTH_EDGE = range(5)      # TSL_DEPTH_*: the status codes of DepthConditioner.condition


class PgoCfg(C.Structure):
    """tsl_pgo_cfg (tsl_pgo_solve): iters 0 .. 64, pcg_max 0 .. 100000, huber 0 = off"""
    _fields_ = [("iters", C.c_int32), ("pcg_max", C.c_int32)] + [(n, C.c_double) for n in ("damping", "damping_up", "damping_down", "damping_min", "damping_max",
                                                                                             "pcg_tol", "min_step", "rel_tol", "huber")]


PGO_STATUS = ("converged", "iterations", "stalled", "singular", "unanchored", "flipped")      # tsl_pgo_report.status
# tsl_pgo_report as a numpy record: 2576 bytes per variant
PGO_ITER_FIELDS = [("cost_before", "<f8"), ("cost_after", "<f8"), ("max_step", "<f8"), ("damping", "<f8"), ("pcg_iters", "<i4"), ("accepted", "<i4")]
PGO_REPORT_FIELDS = [("status", "<i4"), ("iterations", "<i4"), ("cost", "<f8"), ("it", PGO_ITER_FIELDS, (64,))]


class TslError(RuntimeError):
    pass


_LIB = None

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
dp = C.POINTER(C.c_double)
pi32, pi64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

# name -> (restype, argtypes); every symbol declared in include/taichislam_hip.h
SIGNATURES = {
    "tsl_version": (C.c_char_p, []),
    "tsl_last_error": (C.c_char_p, []),
    "tsl_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "tsl_selftest": (C.c_int, [C.c_int, C.POINTER(C.c_int64)]),
    "tsl_tsdf_create": (C.c_int, [C.POINTER(TsdfCfg), C.c_int, C.POINTER(vp)]),
    "tsl_tsdf_destroy": (None, [vp]),
    "tsl_tsdf_get_dims": (C.c_int, [vp, pi32, pi32, pi32, pi32]),
    "tsl_tsdf_sync": (C.c_int, [vp]),
    "tsl_tsdf_reset": (C.c_int, [vp]),
    "tsl_tsdf_memory_bytes": (C.c_int, [vp, pi64]),
    "tsl_tsdf_bricks_in_use": (C.c_int, [vp, pi32]),
    "tsl_tsdf_set_intrinsics": (C.c_int, [vp, dp, dp]),
    "tsl_tsdf_set_base_pose": (C.c_int, [vp, dp, dp]),
    "tsl_tsdf_set_base_pose_submap": (C.c_int, [vp, C.c_int, dp, dp]),
    "tsl_tsdf_get_active_submap": (C.c_int, [vp, pi32]),
    "tsl_tsdf_set_active_submap": (C.c_int, [vp, i32]),
    "tsl_tsdf_set_colormap": (C.c_int, [vp, vp]),
    "tsl_tsdf_integrate_depth": (C.c_int, [vp, dp, dp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]),
    "tsl_tsdf_integrate_depth_dev": (C.c_int, [vp, dp, dp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]),
    "tsl_tsdf_integrate_points": (C.c_int, [vp, dp, dp, vp, vp, i64]),
    "tsl_tsdf_integrate_points_dev": (C.c_int, [vp, dp, dp, vp, vp, i64]),
    "tsl_tsdf_input_stream": (C.c_int, [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]),
    "tsl_tsdf_integrate_depth_stream": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsl_tsdf_queued_frames": (C.c_int, [vp, pi32]),
    "tsl_tsdf_frames_consumed": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsl_tsdf_last_frame_stats": (C.c_int, [vp, C.POINTER(FrameStats)]),
    "tsl_tsdf_count_active": (C.c_int, [vp, pi64]),
    "tsl_tsdf_export_sparse": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, pi64]),
    "tsl_tsdf_import_sparse": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, i64]),
    "tsl_tsdf_export_occupied": (C.c_int, [vp, vp, vp, i64, pi64]),
    "tsl_tsdf_evict": (C.c_int, [vp, C.POINTER(EvictCfg), vp, i64, vp, vp, vp, vp, vp, i64, C.POINTER(EvictStats)]),
    "tsl_tsdf_evict_dev": (C.c_int, [vp, C.POINTER(EvictCfg), vp, i64, vp, vp, vp, vp, vp, i64, C.POINTER(EvictStats), vp]),
    "tsl_tsdf_restore_bricks": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, C.c_int, C.c_int, C.POINTER(EvictStats)]),
    "tsl_tsdf_restore_bricks_dev": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, C.c_int, C.c_int, C.POINTER(EvictStats), vp]),
    "tsl_tsdf_brick_keys": (C.c_int, [vp, vp, i64, pi32]),
    "tsl_tsdf_brick_keys_dev": (C.c_int, [vp, vp, i64, pi32, vp]),
    "tsl_tsdf_surface_voxels": (C.c_int, [vp, vp, C.c_int, pi32]),
    "tsl_tsdf_slice_voxels": (C.c_int, [vp, f32, f32, C.c_int, pi32]),
    "tsl_tsdf_read_exports": (C.c_int, [vp, vp, vp, vp, i64]),
    "tsl_tsdf_exports_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pi32]),
    "tsl_tsdf_set_export_row": (C.c_int, [vp, C.c_int, i64, vp]),
    "tsl_tsdf_pack_pointcloud2": (C.c_int, [vp, C.c_int, i64, vp]),
    "tsl_tsdf_num_particles": (C.c_int, [vp, pi32]),
    "tsl_tsdf_set_num_particles": (C.c_int, [vp, i32]),
    "tsl_tsdf_fuse_submaps": (C.c_int, [vp, vp]),
    "tsl_comm_unique_id": (C.c_int, [C.c_char_p]),
    "tsl_comm_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "tsl_comm_destroy": (None, [vp]),
    "tsl_comm_handle": (vp, [vp]),
    "tsl_tsdf_allreduce_merge": (C.c_int, [vp, vp, vp, pi64]),
    "tsl_tsdf_merge_mask_bytes": (C.c_int, [vp, pi64]),
    "tsl_tsdf_merge_begin": (C.c_int, [vp, vp, vp, i64]),
    "tsl_tsdf_merge_union": (C.c_int, [vp, vp, pi32]),
    "tsl_tsdf_merge_pack": (C.c_int, [vp, vp, vp]),
    "tsl_tsdf_merge_finish": (C.c_int, [vp, vp, vp]),
    "tsl_tsdf_merge_record_bytes": (C.c_int, [pi64]),
    "tsl_tsdf_merge_finalize_slice": (C.c_int, [vp, vp, vp, i32, vp]),
    "tsl_tsdf_merge_finish_records": (C.c_int, [vp, vp]),
    "tsl_mesh_generate": (C.c_int, [vp, C.c_int, f32, i64, pi32]),
    "tsl_mesh_read": (C.c_int, [vp, vp, vp, vp, i64]),
    "tsl_mesh_buffers_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pi32]),
    "tsl_mesh_generate_indexed": (C.c_int, [vp, f32, i64, i64, pi64, pi64]),
    "tsl_mesh_read_indexed": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i64]),
    "tsl_mesh_indexed_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pi64, pi64]),
    "tsl_tsdf_query_points": (C.c_int, [vp, C.c_int, C.c_int, vp, i64, vp]),
    "tsl_tsdf_query_raycast": (C.c_int, [vp, vp, vp, f32, i64, vp, vp, vp]),
    "tsl_tsdf_query_points_dev": (C.c_int, [vp, C.c_int, C.c_int, vp, i64, vp, vp]),
    "tsl_tsdf_query_raycast_dev": (C.c_int, [vp, vp, vp, f32, i64, vp, vp, vp, vp]),
    "tsl_esdf_update": (C.c_int, [vp, f32, f32, pi32]),
    "tsl_esdf_last_stats": (C.c_int, [vp, C.POINTER(EsdfStats)]),
    "tsl_esdf_totals": (C.c_int, [vp, C.POINTER(EsdfTotals)]),
    "tsl_esdf_export": (C.c_int, [vp, vp, vp, i64, pi64]),
    "tsl_esdf_export_dev": (C.c_int, [vp, i64, C.POINTER(vp), C.POINTER(vp), pi64]),
    "tsl_esdf_slice": (C.c_int, [vp, f32, pi32]),
    "tsl_esdf_read_slice": (C.c_int, [vp, vp, vp, i64]),
    "tsl_esdf_slice_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), pi32]),
    "tsl_esdf_query_points": (C.c_int, [vp, C.c_int, f32, vp, i64, vp, vp, vp]),
    "tsl_esdf_query_points_dev": (C.c_int, [vp, C.c_int, f32, vp, i64, vp, vp, vp, vp]),
    "tsl_esdf_score_paths": (C.c_int, [vp, C.c_int, f32, vp, vp, i64, i32, i32, f32, f32, i32, vp, vp, vp]),
    "tsl_esdf_score_paths_dev": (C.c_int, [vp, C.c_int, f32, vp, vp, i64, i32, i32, f32, f32, i32, vp, vp, vp, vp]),
    "tsl_esdf_traj_linearize": (C.c_int, [vp, f32, vp, vp, i64, i32, i32, f32, vp, vp, vp]),
    "tsl_esdf_traj_linearize_dev": (C.c_int, [vp, f32, vp, vp, i64, i32, i32, f32, vp, vp, vp, vp]),
    "tsl_esdf_traj_optimize": (C.c_int, [vp, f32, vp, vp, i64, i32, C.POINTER(TrajOpt), vp, vp, vp]),
    "tsl_esdf_traj_optimize_dev": (C.c_int, [vp, f32, vp, vp, i64, i32, C.POINTER(TrajOpt), vp, vp, vp, vp]),
    "tsl_tsdf_render_view": (C.c_int, [vp, dp, dp, C.POINTER(ViewCfg), vp, vp, vp, vp]),
    "tsl_tsdf_render_view_dev": (C.c_int, [vp, dp, dp, C.POINTER(ViewCfg), vp, vp, vp, vp, vp]),
    "tsl_tsdf_align_linearize": (C.c_int, [vp, dp, dp, C.POINTER(AlignCfg), vp, C.POINTER(AlignSums)]),
    "tsl_tsdf_align_linearize_dev": (C.c_int, [vp, dp, dp, C.POINTER(AlignCfg), vp, vp, vp]),
    "tsl_align_solve": (C.c_int, [C.POINTER(AlignSums), C.c_double, dp, pi32]),
    "tsl_pose_retract": (C.c_int, [dp, dp, dp]),
    "tsl_tsdf_track_depth": (C.c_int, [vp, dp, dp, C.POINTER(AlignCfg), C.POINTER(TrackCfg), vp, dp, dp, C.POINTER(TrackReport)]),
    "tsl_tsdf_track_depth_dev": (C.c_int, [vp, dp, dp, C.POINTER(AlignCfg), C.POINTER(TrackCfg), vp, dp, dp, C.POINTER(TrackReport), vp]),
    "tsl_tsdf_align_rgbd_linearize": (C.c_int, [vp, dp, dp, C.POINTER(AlignRgbdCfg), vp, vp, C.POINTER(AlignRgbdSums)]),
    "tsl_tsdf_align_rgbd_linearize_dev": (C.c_int, [vp, dp, dp, C.POINTER(AlignRgbdCfg), vp, vp, vp, vp]),
    "tsl_align_rgbd_solve": (C.c_int, [C.POINTER(AlignRgbdSums), C.c_double, C.c_double, dp, pi32]),
    "tsl_tsdf_track_rgbd": (C.c_int, [vp, dp, dp, C.POINTER(AlignRgbdCfg), C.POINTER(TrackCfg), C.c_double, C.c_double, vp, vp, dp, dp, C.POINTER(TrackRgbdReport)]),
    "tsl_tsdf_track_rgbd_dev": (C.c_int, [vp, dp, dp, C.POINTER(AlignRgbdCfg), C.POINTER(TrackCfg), C.c_double, C.c_double, vp, vp, dp, dp,
                                          C.POINTER(TrackRgbdReport), vp]),
    "tsl_tsdf_align_points_linearize": (C.c_int, [vp, dp, dp, C.POINTER(AlignPointsCfg), vp, C.c_int64, C.POINTER(AlignSums), vp, vp]),
    "tsl_tsdf_align_points_linearize_dev": (C.c_int, [vp, dp, dp, C.POINTER(AlignPointsCfg), vp, C.c_int64, vp, vp, vp, vp]),
    "tsl_tsdf_track_points": (C.c_int, [vp, dp, dp, C.POINTER(AlignPointsCfg), C.POINTER(TrackCfg), vp, C.c_int64, dp, dp, C.POINTER(TrackReport)]),
    "tsl_tsdf_track_points_dev": (C.c_int, [vp, dp, dp, C.POINTER(AlignPointsCfg), C.POINTER(TrackCfg), vp, C.c_int64, dp, dp, C.POINTER(TrackReport), vp]),
    "tsl_tsdf_register_linearize": (C.c_int, [vp, C.c_int, vp, C.c_int, dp, dp, C.POINTER(RegisterCfg), C.POINTER(AlignSums)]),
    "tsl_tsdf_register_submap": (C.c_int, [vp, C.c_int, vp, C.c_int, dp, dp, C.POINTER(RegisterCfg), C.POINTER(TrackCfg), dp, dp, C.POINTER(TrackReport)]),
    "tsl_tsdf_register_score": (C.c_int, [vp, C.c_int, vp, C.c_int, dp, dp, i32, C.POINTER(RegisterCfg), C.POINTER(RegisterScore), C.POINTER(RegisterGate)]),
    "tsl_tsdf_register_score_tile": (C.c_int, [vp, i64, i32]),
    "tsl_tsdf_register_search": (C.c_int, [vp, C.c_int, vp, C.c_int, dp, dp, C.POINTER(RegisterCfg), C.POINTER(SearchCfg), C.POINTER(TrackCfg), dp, dp,
                                           C.POINTER(SearchReport), C.POINTER(TrackReport), C.POINTER(RegisterScore)]),
    "tsl_tsdf_frontier_extract": (C.c_int, [vp, C.POINTER(FrontierCfg), pi32, pi32]),
    "tsl_tsdf_frontier_read": (C.c_int, [vp, vp, vp, vp, vp, i64, i64]),
    "tsl_tsdf_frontier_dev": (C.c_int, [vp, C.POINTER(FrontierCfg), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pi32, pi32, vp]),
    "tsl_tsdf_view_gain": (C.c_int, [vp, dp, dp, i32, C.POINTER(GainCfg), vp, vp, vp]),
    "tsl_tsdf_view_gain_dev": (C.c_int, [vp, dp, dp, i32, C.POINTER(GainCfg), vp, vp, vp, vp]),
    "tsl_tsdf_nav_grid": (C.c_int, [vp, C.POINTER(NavCfg), vp, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_grid_dev": (C.c_int, [vp, C.POINTER(NavCfg), vp, vp, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_field": (C.c_int, [vp, C.POINTER(NavFieldCfg), vp, vp, i32, vp, vp, C.POINTER(NavFieldStats)]),
    "tsl_tsdf_nav_field_dev": (C.c_int, [vp, C.POINTER(NavFieldCfg), vp, vp, i32, vp, vp, vp, vp]),
    "tsl_tsdf_nav_field_paths": (C.c_int, [vp, C.POINTER(NavFieldCfg), vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "tsl_tsdf_nav_field_paths_dev": (C.c_int, [vp, C.POINTER(NavFieldCfg), vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_field3": (C.c_int, [vp, C.POINTER(NavField3Cfg), vp, vp, i32, vp, vp, C.POINTER(NavField3Stats)]),
    "tsl_tsdf_nav_field3_dev": (C.c_int, [vp, C.POINTER(NavField3Cfg), vp, vp, i32, vp, vp, vp, vp]),
    "tsl_tsdf_nav_field3_paths": (C.c_int, [vp, C.POINTER(NavField3Cfg), vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "tsl_tsdf_nav_field3_paths_dev": (C.c_int, [vp, C.POINTER(NavField3Cfg), vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_boxes": (C.c_int, [vp, C.POINTER(NavCorridorCfg), vp, vp, i32, vp, vp]),
    "tsl_tsdf_nav_boxes_dev": (C.c_int, [vp, C.POINTER(NavCorridorCfg), vp, vp, i32, vp, vp, vp]),
    "tsl_tsdf_nav_corridor": (C.c_int, [vp, C.POINTER(NavCorridorCfg), vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_corridor_dev": (C.c_int, [vp, C.POINTER(NavCorridorCfg), vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_terrain": (C.c_int, [vp, C.POINTER(NavTerrainCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tsl_tsdf_nav_terrain_dev": (C.c_int, [vp, C.POINTER(NavTerrainCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tsl_topo_create": (C.c_int, [vp, i32, f32, i64, C.POINTER(vp)]),
    "tsl_topo_destroy": (None, [vp]),
    "tsl_topo_reset": (C.c_int, [vp]),
    "tsl_topo_counts": (C.c_int, [vp, pi64, pi32]),
    "tsl_topo_rays": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, i32, vp, vp, vp, vp, vp]),
    "tsl_topo_rays_dev": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, i32, vp, vp, vp, vp, vp, vp]),
    "tsl_topo_collide": (C.c_int, [vp, vp, vp, f32, pi32, pi32, vp, vp, vp, pi32, vp, C.POINTER(C.c_float)]),
    "tsl_topo_add_poly": (C.c_int, [vp, vp, i32, vp, f32, vp, vp, vp, vp, pi32]),
    "tsl_topo_buffers_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pi64, pi32]),
    "tsl_topo_read_facelets": (C.c_int, [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp]),
    "tsl_depth_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "tsl_depth_destroy": (None, [vp]),
    "tsl_depth_set_tables": (C.c_int, [vp, vp, vp, vp]),
    "tsl_depth_condition": (C.c_int, [vp, C.POINTER(DepthCfg), vp, vp, vp, vp, vp, vp, vp]),
    "tsl_depth_condition_dev": (C.c_int, [vp, C.POINTER(DepthCfg), vp, vp, vp, vp, vp, vp, vp, vp]),
    "tsl_pgo_create": (C.c_int, [C.c_int, i32, i32, i32, C.POINTER(vp)]),
    "tsl_pgo_destroy": (None, [vp]),
    "tsl_pgo_linearize": (C.c_int, [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp]),
    "tsl_pgo_linearize_dev": (C.c_int, [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp]),
    "tsl_pgo_solve": (C.c_int, [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, C.POINTER(PgoCfg), vp, vp, vp, vp, vp]),
    "tsl_pgo_solve_dev": (C.c_int, [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, C.POINTER(PgoCfg), vp, vp, vp, vp, vp, vp]),
    "tsl_tsdf_set_option": (C.c_int, [vp, C.c_char_p, C.c_int]),
    "tsl_tsdf_get_option": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_int)]),
    "tsl_tsdf_prof_enable": (C.c_int, [vp, C.c_int]),
    "tsl_tsdf_prof_query": (C.c_int, [vp, C.c_int, dp, pi64]),
    "tsl_octo_create": (C.c_int, [C.POINTER(OctoCfg), C.c_int, C.POINTER(vp)]),
    "tsl_octo_destroy": (None, [vp]),
    "tsl_octo_get_dims": (C.c_int, [vp, pi32, pi32, pi32, pi32, dp]),
    "tsl_octo_sync": (C.c_int, [vp]),
    "tsl_octo_reset": (C.c_int, [vp]),
    "tsl_octo_set_intrinsics": (C.c_int, [vp, dp, dp]),
    "tsl_octo_set_base_pose_submap": (C.c_int, [vp, C.c_int, dp, dp]),
    "tsl_octo_get_active_submap": (C.c_int, [vp, pi32]),
    "tsl_octo_set_active_submap": (C.c_int, [vp, i32]),
    "tsl_octo_integrate_depth": (C.c_int, [vp, dp, dp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]),
    "tsl_octo_integrate_depth_dev": (C.c_int, [vp, dp, dp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]),
    "tsl_octo_integrate_points": (C.c_int, [vp, dp, dp, vp, vp, i64]),
    "tsl_octo_integrate_points_dev": (C.c_int, [vp, dp, dp, vp, vp, i64]),
    "tsl_octo_last_frame_stats": (C.c_int, [vp, C.POINTER(FrameStats)]),
    "tsl_octo_export_leaves": (C.c_int, [vp, vp, vp, vp, i64, pi64]),
    "tsl_octo_occupied_voxels": (C.c_int, [vp, vp, C.c_int, C.c_int, pi32]),
    "tsl_octo_read_exports": (C.c_int, [vp, vp, vp, i64]),
    "tsl_octo_exports_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), pi32]),
    "tsl_octo_pack_pointcloud2": (C.c_int, [vp, C.c_int, i64, vp]),
    "tsl_octo_num_particles": (C.c_int, [vp, pi32]),
    "tsl_octo_fuse_submaps": (C.c_int, [vp, vp]),
}


def library_path():
    return _build.LIB


def lib():
    """Load (building first if the sources are newer and hipcc exists) the HIP library.  Raises if unavailable."""
    global _LIB
    if _LIB is None:
        # TSL_LIB: developer aid, an alternative build of the same library (e.g. a -DTSL_TIMING build for tools/timing_probe*.py)
        path = os.environ.get("TSL_LIB") or _build.build_library()
        if not os.path.exists(path):
            raise TslError("libtaichislam_hip.so is missing; run `python -m taichislam_amd.build`")
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here = the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    if rc != TSL_OK:
        raise TslError(f"taichislam_hip error {rc}: {lib().tsl_last_error().decode()}")


def device_count():
    n = C.c_int(0)
    lib().tsl_device_count(C.byref(n))
    return n.value


_HOST_FN = None


_OCTO_DEV_FN = None


def octo_integrate_depth_dev_fn():
    """tsl_octo_integrate_depth_dev with integer pointer arguments (no ctypes pointer objects per call): the per-frame path of a device-resident stream into the
    Octomap, which the library only queues -- the host side of a call is what a frame costs."""
    global _OCTO_DEV_FN
    if _OCTO_DEV_FN is None:
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int)
        _OCTO_DEV_FN = proto(("tsl_octo_integrate_depth_dev", lib()))
    return _OCTO_DEV_FN


def integrate_depth_host_fn():
    """tsl_tsdf_integrate_depth bound a second time with integer pointer arguments (no ctypes pointer objects per call): the per-frame path of
    a host-image stream, see DenseTSDF.recast_depth_to_map."""
    global _HOST_FN
    if _HOST_FN is None:
        lib()
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int)
        _HOST_FN = proto(("tsl_tsdf_integrate_depth", lib()))
    return _HOST_FN

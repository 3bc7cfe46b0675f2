/*
 * taichislam_hip.h -- C-ABI of the MI355X-native dense-mapping backend (libtaichislam_hip.so).
 *
 * The reference (xuhao1/TaichiSLAM) has no FFI seam: its callers use the Python classes of
 * taichi_slam/mapping directly.  This ABI is what taichislam_amd/mapping/ *.py (ctypes shims that
 * keep those class surfaces) binds, and what any C/C++ host would bind.  Each entry point cites the
 * reference method it replaces (paths relative to the reference root).
 *
 * Conventions: opaque handles; plain pointers and sizes; int status return (0 = TSL_OK, <0 = error,
 * text via tsl_last_error()); no exceptions cross the boundary.  One handle = one device + one HIP
 * stream; a handle is NOT thread-safe, distinct handles are independent.  Pointers named *_dev are
 * device pointers (e.g. torch tensor .data_ptr()); all others are caller-owned host buffers.
 * Integration calls are asynchronous on the handle's stream; every call that returns data to the
 * host synchronises.  R/T are row-major float64 camera-to-world poses (scripts/taichislam_node.py:381).
 */
#ifndef TAICHISLAM_HIP_H
#define TAICHISLAM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSL_OK              0
#define TSL_ERR_ARG        -1
#define TSL_ERR_HIP        -2
#define TSL_ERR_CAPACITY   -3   /* brick pool / frame scratch / output buffer exhausted */
#define TSL_ERR_NO_DEVICE  -4

typedef struct tsl_tsdf tsl_tsdf;   /* DenseTSDF                 taichi_slam/mapping/dense_tsdf.py:12      */
typedef struct tsl_octo tsl_octo;   /* Octomap                   taichi_slam/mapping/taichi_octomap.py:12  */

/* DenseTSDF.__init__ kwargs (dense_tsdf.py:13-16) + backend sizing knobs (0 = default). */
typedef struct {
    double  map_size_xy, map_size_z;
    double  voxel_scale;
    int32_t num_voxel_per_blk_axis;
    double  max_ray_length, min_ray_length;
    int32_t internal_voxels;
    int32_t max_submap_num;
    int32_t is_global_map;
    int32_t texture_enabled;
    double  disp_ceiling, disp_floor;
    int32_t recast_step;
    int32_t color_same_proj;
    int64_t max_disp_particles;
    /* backend sizing */
    int32_t max_bricks;          /* 16^3 brick pool capacity (24 KiB each)                */
    int32_t max_frame_bricks;    /* bricks one frame may touch (64 KiB scratch each)      */
    int32_t max_points;          /* pixels/points per integrate call                       */
} tsl_tsdf_cfg;

typedef struct {
    int64_t p_used;      /* pixels / points visited                                   */
    int64_t p_valid;     /* passed the range gate and inside the sensor-centred grid  */
    int64_t p_oob;       /* passed the gate but outside the sensor-centred grid       */
    int64_t v_pcl;       /* sensor-grid voxels with count>0 (= rays)                  */
    int64_t v_skipped;   /* degenerate rays skipped                                   */
    int64_t steps;       /* ray-steps applied (S)                                     */
    int64_t steps_oob;   /* ray-steps outside the map volume (skipped)                */
    int64_t unique;      /* distinct voxels touched this frame (U)                    */
    int64_t bricks;      /* distinct 16^3 bricks touched this frame                   */
} tsl_frame_stats;

/* kernel ids for tsl_tsdf_prof_query */
enum { TSL_K_VOXELIZE = 0, TSL_K_SORT = 1, TSL_K_RAYS = 2, TSL_K_INTEGRATE = 3, TSL_K_FINALIZE = 4,
       TSL_K_MESH = 5, TSL_K_SEGMENTS = 6, TSL_K_BIN = 7, TSL_K_ESDF = 8, TSL_K_FUSE = 9, TSL_K_REGISTER = 10,
       TSL_K_REGISTER_SCORE = 11, TSL_K_FRONTIER_MARK = 12, TSL_K_FRONTIER_LABEL = 13, TSL_K_FRONTIER_JOIN = 14, TSL_K_FRONTIER_SUM = 15,
       TSL_K_FRONTIER_EMIT = 16, TSL_K_VIEW_GAIN = 17, TSL_K_ALIGN = 18, TSL_K_ALIGN_POINTS = 19, TSL_K_PATH_SCORE = 20,
       TSL_K_NAV_PROJECT = 21, TSL_K_NAV_EDT = 22, TSL_K_NAV_EDT_ROWS = 23,
       TSL_K_NAV_FIELD_SEED = 24, TSL_K_NAV_FIELD_ROUND = 25, TSL_K_NAV_FIELD_PARENT = 26, TSL_K_NAV_FIELD_PATHS = 27,
       TSL_K_NAV_TERRAIN_COLUMNS = 28, TSL_K_NAV_TERRAIN_WINDOW = 29,
       TSL_K_COUNT };
/* the ids added since: the first enum ends where it always did, prof_query takes every id below TSL_K_END */
enum { TSL_K_ALIGN_RGBD = 30, TSL_K_EVICT = 31 /* tsl_tsdf_evict: the pack launch, and the compaction's four launches */, TSL_K_END = 32 };

const char* tsl_version(void);
const char* tsl_last_error(void);
int  tsl_device_count(int* n);
/* Exhaustive device check (all 2^32 float patterns) of an arithmetic shortcut the kernels rely on for bit-exactness:
   which = 0: three-instruction round-half-away == ti.round (mapping_common.py:263-266, dense_tsdf.py:254);
   which = 1: rescale-free correctly rounded sqrt == sqrtf on [2^-96, inf);
   which = 2 (2^32 pseudo-random operand pairs, not exhaustive): the division-free quotient of the sequential replay's saturated voxels
              (reciprocal product + two FMA residual corrections) == IEEE division.  *mismatches must come back 0. */
int  tsl_selftest(int which, int64_t* mismatches);

/* ---- lifecycle -------------------------------------------------------------------------- */
int  tsl_tsdf_create(const tsl_tsdf_cfg* cfg, int device, tsl_tsdf** out);        /* dense_tsdf.py:13-50,52-118 */
void tsl_tsdf_destroy(tsl_tsdf* m);
int  tsl_tsdf_get_dims(const tsl_tsdf* m, int32_t* N, int32_t* Nz, int32_t* block_num_xy, int32_t* block_num_z);
int  tsl_tsdf_sync(tsl_tsdf* m);
int  tsl_tsdf_reset(tsl_tsdf* m);                                                    /* dense_tsdf.py:309-310 */
int  tsl_tsdf_memory_bytes(const tsl_tsdf* m, int64_t* bytes);
int  tsl_tsdf_bricks_in_use(tsl_tsdf* m, int32_t* n);

/* ---- poses / camera ------------------------------------------------------------------------ */
int  tsl_tsdf_set_intrinsics(tsl_tsdf* m, const double Kdep[9], const double Kcol[9]);   /* mapping_common.py:25-29 */
int  tsl_tsdf_set_base_pose(tsl_tsdf* m, const double R[9], const double T[3]);           /* mapping_common.py:141-147 */
int  tsl_tsdf_set_base_pose_submap(tsl_tsdf* m, int sid, const double R[9], const double T[3]);   /* mapping_common.py:121-131 */
int  tsl_tsdf_get_active_submap(const tsl_tsdf* m, int32_t* sid);                         /* mapping_common.py:113-114 */
int  tsl_tsdf_set_active_submap(tsl_tsdf* m, int32_t sid);                                /* mapping_common.py:116-119 */
int  tsl_tsdf_set_colormap(tsl_tsdf* m, const float rgb[1024 * 3]);                       /* mapping_common.py:158-163 */

/* ---- integration (the hot path) --------------------------------------------------------------
 * recast_depth_to_map(R, T, depthmap, texture)  dense_tsdf.py:162-165,188-270
 * depth: uint16 millimetres [h][w] C-contiguous; tex: uint8 [th][tw][3] or NULL. */
int  tsl_tsdf_integrate_depth(tsl_tsdf* m, const double R[9], const double T[3],
                              const uint16_t* depth, int h, int w, const uint8_t* tex, int th, int tw);
int  tsl_tsdf_integrate_depth_dev(tsl_tsdf* m, const double R[9], const double T[3],
                                  const void* depth_dev, int h, int w, const void* tex_dev, int th, int tw);
/* recast_pcl_to_map(R, T, xyz_array, rgb_array)  dense_tsdf.py:157-160,167-186; xyz f32 [n][3] */
int  tsl_tsdf_integrate_points(tsl_tsdf* m, const double R[9], const double T[3],
                               const float* xyz, const uint8_t* rgb, int64_t n);
int  tsl_tsdf_integrate_points_dev(tsl_tsdf* m, const double R[9], const double T[3],
                                   const void* xyz_dev, const void* rgb_dev, int64_t n);
/* Stream that will read the device buffers of the next integrate_*_dev call (points: 0 depth image, 1 point cloud).  With `ordered`,
 * that stream is made to wait (when the frame's batch is issued) for everything queued so far on `producer` (the hipStream_t the caller fills its buffers on; NULL =
 * the default stream): the reference's recast_* calls are synchronous (dense_tsdf.py:157-165), so the Python shim does this for torch
 * tensors with torch's current stream. */
int  tsl_tsdf_input_stream(tsl_tsdf* m, int points, int ordered, void* producer, void** hip_stream);
/* The three calls a caller with device buffers makes per frame, as one: input_stream(ordered, producer) + integrate_depth_dev +
 * frames_consumed (the shim's per-frame path for torch tensors: one FFI crossing instead of three). */
int  tsl_tsdf_integrate_depth_stream(tsl_tsdf* m, const double R[9], const double T[3], const void* depth_dev, int h, int w,
                                     const void* tex_dev, int th, int tw, void* producer, int64_t* queued_total, int64_t* consumed);
/* frames queued by integrate_* calls and not yet issued to the device: a device buffer handed to integrate_*_dev is read by kernels
 * that are only enqueued once this has dropped back to 0 (or any synchronising call was made) */
int  tsl_tsdf_queued_frames(const tsl_tsdf* m, int32_t* n);
/* Lifetime of device input buffers without synchronising: *queued_total = frames handed to integrate_* since the handle was created
 * (the frame of the latest call has index queued_total - 1), *consumed = how many of them the device has certainly finished reading.
 * The buffers of frame i may be reused or freed once consumed > i.  Host-side bookkeeping only (no device query, never blocks): the
 * library never queues more than eight batches (64 frames) ahead of the device -- the integrate call that would exceed that waits for
 * the oldest batch -- and that wait, like every synchronising call, advances the count. */
int  tsl_tsdf_frames_consumed(tsl_tsdf* m, int64_t* queued_total, int64_t* consumed);
/* The integrate calls only QUEUE the frame (host buffers are copied before they return -- the visited pixels of a depth image, the points, the texture,
 * into a pinned buffer of the frame's working set, from where ONE copy kernel per batch takes them to device memory at the head of the batch;
 * device buffers must stay unchanged until the next call that returns data, or tsl_tsdf_sync).  A batch that could not be issued (an allocation
 * or launch failure) is reported by the next call that returns data or synchronises -- never by a map that silently lacks its frames.  Queued frames are issued eight at a time (four for the first two batches after the pipeline ran dry), or as soon
 * as any other call needs the map (option "adaptive": also as soon as the device is ready for them), so results never depend on the queueing; frames still queued when a handle is destroyed are dropped. */
/* counters of the most recent integrate call (synchronises) */
int  tsl_tsdf_last_frame_stats(tsl_tsdf* m, tsl_frame_stats* out);

/* ---- sparse export / import  (dense_tsdf.py:412-498) -------------------------------------------- */
int  tsl_tsdf_count_active(tsl_tsdf* m, int64_t* n);                                       /* :412-423 */
int  tsl_tsdf_export_sparse(tsl_tsdf* m, int16_t* idx, uint16_t* tsdf_h, uint16_t* w_h, int8_t* occ,
                            uint16_t* color_h, int64_t cap, int64_t* n);                   /* to_numpy :425-440 */
int  tsl_tsdf_import_sparse(tsl_tsdf* m, int sid, const int16_t* idx, const uint16_t* tsdf_h,
                            const uint16_t* w_h, const int8_t* occ, const uint16_t* color_h, int64_t n);   /* load_numpy :442-454 */
int  tsl_tsdf_export_occupied(tsl_tsdf* m, int16_t* idx, int8_t* occ, int64_t cap, int64_t* n);

/* ---- evict and restore bricks: bounded pool memory for long missions (no counterpart in the reference, whose map is a dense field) -----------
 * The brick pool hands out 16^3 bricks and, until these calls, only tsl_tsdf_reset gave any back.  tsl_tsdf_evict selects bricks, copies their raw
 * planes out (the PAYLOAD) and, with release = 1, gives their pool slots back; tsl_tsdf_restore_bricks puts payload rows into a map of the same
 * geometry.  A payload is lossless: what an evict + restore round trip leaves is, brick for brick, the bytes that were there.
 *   Brick key: key = s * nb3 + b, s the submap slot (0 on a global map), b = (bi * nbx + bj) * nbz + bk, nbx = ceil(N / 16), nbz = ceil(Nz / 16),
 *     nb3 = nbx * nbx * nbz.  Brick (bi, bj, bk) holds the voxels 16 * bi - N / 2 .. 16 * bi + 15 - N / 2 of the map-centred index i of
 *     tsl_tsdf_export_sparse (j alike, k with Nz / 2); where N is no multiple of 16 the last bricks reach past the volume.  The voxel with local
 *     offsets (li, lj, lk) is element (li << 8) | (lj << 4) | lk of a plane row.
 *   Selection (tsl_evict_cfg.rule), all integer, evaluated on the device over the bricks in use:
 *     TSL_EVICT_KEEP_BOX   every brick of the chosen slots whose voxel range does NOT intersect the inclusive voxel box lo <= (i, j, k) <= hi
 *     TSL_EVICT_CLEAR_BOX  every brick of the chosen slots whose voxel range lies wholly inside the box
 *                          (a brick the box cuts through stays under both rules; lo > hi on an axis is an argument error)
 *     TSL_EVICT_KEYS       the bricks named by keys_in[0 .. nkeys): a key listed twice counts once, a key whose brick is absent counts (once) in
 *                          stats.missing, a key outside [0, max_submap_num * nb3) is an argument error and nothing changes
 *     sid (box rules): a submap slot, or -1 = every slot; on a global map 0 and -1 mean the same.  The keys rule does not read it.
 *   Payload: one row per selected brick in ASCENDING KEY order, whatever order the pool holds them in: keys int32 [n], tw uint32 [n][4096] (lo16 the
 *     TSDF f16 bits, hi16 the weight f16 bits), obs int8 [n][4096], occ int8 [n][4096], col uint16 [n][4096][4] (f16 r, g, b and the pad lane;
 *     textured maps only, ignored otherwise).  Two maps with the same content give the same bytes.  A null plane is not written.  All planes null
 *     and release = 0: the call only counts.  All planes null and release = 1: the selection is discarded without a copy (clearing a region).
 *     cap = rows the buffers hold; cap < stats.selected with any plane given: TSL_ERR_CAPACITY, stats.selected is set, nothing changes.
 *   Release (release = 1): with top bricks in use and E selected, new_top = top - E; the HOLES (selected pool indices < new_top, ascending) are
 *     filled by the MOVERS (kept pool indices >= new_top, ascending), mover k into hole k, so the pool stays dense and its order after the call is a
 *     function of its order before and the selection alone.  Every evicted key leaves the brick table, every slot in [new_top, top) is zero again,
 *     tsl_tsdf_bricks_in_use gives new_top.  With E > 0 the ESDF is invalidated exactly as tsl_tsdf_reset and tsl_tsdf_import_sparse do (the next
 *     update is a full one; tsl_esdf_query_points refuses until then); with E = 0 nothing is touched.  release = 0 is a snapshot: the map is untouched.
 *   Before anything else the queued frames are issued and waited for (tsl_tsdf_sync) and a running ESDF update is finished; a capacity error of
 *     those frames is returned AFTER the call has done its work, as tsl_tsdf_reset returns it.  Between tsl_tsdf_merge_begin and the merge's finish the
 *     calls are refused (TSL_ERR_ARG): the merge's sums and its union list name pool bricks.  They work under semantics 0 and 1.
 *   stats: selected, missing, moved (movers), bricks_before, bricks_after; restore: restored, skipped.
 * tsl_tsdf_restore_bricks: rows keys[0 .. n) with their planes (tw, obs, occ required; col read on textured maps when given) go back in.  sid = -1:
 *   every row goes to its own key; sid >= 0: to brick key % nb3 of that slot.  The keys (of the slot they go to) must ascend strictly and lie in
 *   range, else TSL_ERR_ARG.  A row whose brick exists is a CONFLICT: on_conflict TSL_RESTORE_SKIP drops the row (stats.skipped),
 *   TSL_RESTORE_OVERWRITE replaces the brick's planes.  All or nothing: the absent bricks are counted first, and when they do not fit max_bricks
 *   the call returns TSL_ERR_CAPACITY and the map is unchanged.  New bricks are claimed as integration claims them, so their pool order is not
 *   defined; the content by key is.  The ESDF is invalidated as by tsl_tsdf_import_sparse when a row went in.
 * tsl_tsdf_brick_keys: the keys of the bricks in use in pool order, *n = their number (keys NULL: only the number; cap < *n: TSL_ERR_CAPACITY).
 * The _dev forms take device pointers (payload planes 16-byte aligned), run on the handle's stream behind what user_stream has queued, and make
 * user_stream wait for them; they still wait for the selection's counts, which the host needs for stats and the capacity check. */
#define TSL_EVICT_KEEP_BOX     0
#define TSL_EVICT_CLEAR_BOX    1
#define TSL_EVICT_KEYS         2
#define TSL_RESTORE_SKIP       0
#define TSL_RESTORE_OVERWRITE  1
typedef struct {
    int32_t rule;            /* TSL_EVICT_*                                               */
    int32_t sid;             /* box rules: submap slot, -1 = every slot                   */
    int32_t lo[3], hi[3];    /* box rules: inclusive voxel box                            */
    int32_t release;         /* 1 = give the selected bricks back, 0 = snapshot           */
    int32_t reserved_;
} tsl_evict_cfg;
typedef struct {
    int32_t selected, missing, moved, bricks_before, bricks_after, restored, skipped, reserved_;
} tsl_evict_stats;
int  tsl_tsdf_evict(tsl_tsdf* m, const tsl_evict_cfg* cfg, const int32_t* keys_in, int64_t nkeys, int32_t* keys, uint32_t* tw, int8_t* obs, int8_t* occ,
                    uint16_t* col, int64_t cap, tsl_evict_stats* stats);
int  tsl_tsdf_evict_dev(tsl_tsdf* m, const tsl_evict_cfg* cfg, const void* keys_in_dev, int64_t nkeys, void* keys_dev, void* tw_dev, void* obs_dev,
                        void* occ_dev, void* col_dev, int64_t cap, tsl_evict_stats* stats, void* user_stream);
int  tsl_tsdf_restore_bricks(tsl_tsdf* m, const int32_t* keys, const uint32_t* tw, const int8_t* obs, const int8_t* occ, const uint16_t* col, int64_t n,
                             int sid, int on_conflict, tsl_evict_stats* stats);
int  tsl_tsdf_restore_bricks_dev(tsl_tsdf* m, const void* keys_dev, const void* tw_dev, const void* obs_dev, const void* occ_dev, const void* col_dev,
                                 int64_t n, int sid, int on_conflict, tsl_evict_stats* stats, void* user_stream);
int  tsl_tsdf_brick_keys(tsl_tsdf* m, int32_t* keys, int64_t cap, int32_t* n);
int  tsl_tsdf_brick_keys_dev(tsl_tsdf* m, void* keys_dev, int64_t cap, int32_t* n, void* user_stream);

/* ---- visualisation exports (device-resident result buffers, max_disp_particles rows) ---------- */
/* cvt_TSDF_surface_to_voxels[_to]  dense_tsdf.py:323-365.  add_to_cur: keep the current count and
 * append (the `_to` form); the true count is returned even when it exceeds the capacity. */
int  tsl_tsdf_surface_voxels(tsl_tsdf* m, tsl_tsdf* dst /* NULL = m itself */, int add_to_cur, int32_t* n);
/* cvt_TSDF_to_voxels_slice(z, dz, clear_last)  dense_tsdf.py:367-389 */
int  tsl_tsdf_slice_voxels(tsl_tsdf* m, float z, float dz, int clear_last, int32_t* n);
/* read back export_TSDF_xyz / export_color / export_TSDF (any may be NULL), rows [0, n) */
int  tsl_tsdf_read_exports(tsl_tsdf* m, float* xyz, float* rgb, float* val, int64_t n);
/* the same three buffers as DEVICE pointers (f32 [max_disp_particles][3] / [3] / [1], valid for the lifetime of the handle) + the count
 * of the last cvt_* call: the form taichislam_node.py:350-351 would use if its consumer stayed on the GPU.  Synchronises. */
int  tsl_tsdf_exports_dev(tsl_tsdf* m, void** xyz_dev, void** rgb_dev, void** val_dev, int32_t* n);
/* export_TSDF_xyz[row] = v (field 0) / export_color[row] = v (field 1): callers append marker points to the particle list (tests/gen_topo_graph.py:64-65) */
int  tsl_tsdf_set_export_row(tsl_tsdf* m, int field, int64_t row, const float v[3]);
/* the first n exported particles as the data block of a sensor_msgs/PointCloud2: interleaved float32 rows x y z [r g b], point_step 12 / 24
 * (what utils/ros_pcl_transfer.py:96-136 builds from the numpy copies, scripts/taichislam_node.py:420-425) -- interleaved on the device */
int  tsl_tsdf_pack_pointcloud2(tsl_tsdf* m, int has_rgb, int64_t n, void* out_host);
int  tsl_tsdf_num_particles(tsl_tsdf* m, int32_t* n);
int  tsl_tsdf_set_num_particles(tsl_tsdf* m, int32_t n);

/* ---- submap fusion  (dense_tsdf.py:272-318) ------------------------------------------------------ */
int  tsl_tsdf_fuse_submaps(tsl_tsdf* global, tsl_tsdf* submaps);
/* ---- multi-GPU global-map merge: one submap collection per GPU, one exchange at merge time -------------------------------------
 * Swarm counterpart of submap_mapping.py:226-253 + utils/communication.py:9-43 (agents ship zlib'd numpy submaps over LCM and every
 * agent fuses them, dense_tsdf.py:272-318): every rank splats its own submaps into exact 2^-24 fixed-point sums per touched 16^3
 * brick, the union of touched bricks is all-reduced (RCCL over xGMI) and every rank writes the same global TSDF.  Integer sums: the
 * result is bit-identical for any number of ranks and equal to one GPU fusing every submap.  The global map's pose table must hold the
 * base pose of every submap id used by any rank (tsl_tsdf_set_base_pose_submap), as for tsl_tsdf_fuse_submaps. */
typedef struct tsl_comm tsl_comm;                                  /* an RCCL communicator (RCCL is bound at run time, dlopen) */
int   tsl_comm_unique_id(char id[128]);                            /* ncclGetUniqueId on one rank; ship the 128 bytes to the others */
int   tsl_comm_create(const char id[128], int nranks, int rank, int device, tsl_comm** out);   /* ncclCommInitRank (collective) */
void  tsl_comm_destroy(tsl_comm* c);
void* tsl_comm_handle(tsl_comm* c);                                /* the ncclComm_t */
/* one call: splat, all-reduce the touched-brick mask (MAX) and the packed union bricks (SUM) on `rccl_comm` (an ncclComm_t from
 * tsl_comm_handle or the caller's own; NULL = this rank alone), finalise.  bytes_per_rank (nullable) = payload all-reduced. */
int   tsl_tsdf_allreduce_merge(tsl_tsdf* global, tsl_tsdf* submaps, void* rccl_comm, int64_t* bytes_per_rank);
/* the same in steps, for callers that run the two reductions themselves (torch.distributed, MPI); *_dev buffers are the caller's:
 *   merge_begin  : reset `global`, splat `submaps`, write the touched-brick byte mask (tsl_tsdf_merge_mask_bytes bytes)
 *   -> all-reduce(MAX) the mask
 *   merge_union  : ascending list of the union bricks, *nunion of them
 *   merge_pack   : acc_dev int64 [nunion][4096][2] = {sum w*tsdf, sum w}, cnt_dev int32 [nunion][4096] = contributions * 65536 + occupancy
 *   -> all-reduce(SUM) both
 *   merge_finish : write the global map from the sums */
int   tsl_tsdf_merge_mask_bytes(const tsl_tsdf* global, int64_t* n);
int   tsl_tsdf_merge_begin(tsl_tsdf* global, tsl_tsdf* submaps, void* mask_dev, int64_t mask_bytes);
int   tsl_tsdf_merge_union(tsl_tsdf* global, const void* mask_dev, int32_t* nunion);
int   tsl_tsdf_merge_pack(tsl_tsdf* global, void* acc_dev, void* cnt_dev);
int   tsl_tsdf_merge_finish(tsl_tsdf* global, const void* acc_dev, const void* cnt_dev);
/* The second form of the exchange: REDUCE-SCATTER the packed planes (pad them to whole bricks per rank with zeros), every rank turns the
 * `nbricks` bricks of sums it received into finalised records -- per brick tsl_tsdf_merge_record_bytes = 20 992 bytes: f16 {TSDF, W} words, occupancy bytes, a
 * "written" bit per voxel (dense_tsdf.py:272-280 applied once per voxel) -- and with the records of all union bricks ALL-GATHERED (union order) the map is written:
 *   merge_begin -> all-reduce(MAX) -> merge_union -> merge_pack -> reduce-scatter(SUM) x2 -> merge_finalize_slice -> all-gather -> merge_finish_records.
 * 5.1 bytes per union voxel travel in the second half instead of the 20 an all-reduce sends round again.  tsl_tsdf_allreduce_merge takes this form with
 * option "merge_exchange" = 1 on the global map (ncclReduceScatter / ncclAllGather). */
int   tsl_tsdf_merge_record_bytes(int64_t* n);
int   tsl_tsdf_merge_finalize_slice(tsl_tsdf* global, const void* acc_dev, const void* cnt_dev, int32_t nbricks, void* rec_dev);
int   tsl_tsdf_merge_finish_records(tsl_tsdf* global, const void* rec_dev);

/* ---- marching cubes  (marching_cube_mesher.py:127-193) ------------------------------------------- */
/* generate_mesh(step): result stays on the device in the map's mesh buffers (3*max_tri rows each);
 * n_tri is the true triangle count.  read with tsl_mesh_read. */
int  tsl_mesh_generate(tsl_tsdf* m, int step, float surface_thres, int64_t max_tri, int32_t* n_tri);
int  tsl_mesh_read(tsl_tsdf* m, float* verts, float* normals, float* colors, int64_t n_vertices);
/* mesh_vertices / mesh_normals / mesh_colors (marching_cube_mesher.py:16-22) as DEVICE pointers, f32 [3 * max_triangles][3] (colours NULL
 * for untextured maps), + num_facelets of the last generate: taichislam_node.py:342 without the host copy */
int  tsl_mesh_buffers_dev(tsl_tsdf* m, void** verts_dev, void** normals_dev, void** colors_dev, int32_t* n_tri);
/* ---- indexed mesh: the mesh of tsl_mesh_generate(step 1) with welded vertices, in a canonical order (DESIGN.md "Indexed marching-cubes mesh") ----
 * The same cells, validity rule (own voxel observed and < surface_thres, all eight corners observed), case table, sign (value < 0) and eps snap as the
 * soup; the soup's buffers and tsl_mesh_generate are not touched.  With u = (i + N/2, j + N/2, k + Nz/2) a voxel's unsigned coordinates, its brick
 * b = ((u.x >> 4) * nbx + (u.y >> 4)) * nbz + (u.z >> 4) (+ submap slot * bricks per submap) and l = (u.x & 15) << 8 | (u.y & 15) << 4 | (u.z & 15), its
 * cell key is c = b * 4096 + l.
 *   vertices   one row per GRID EDGE (lower-corner voxel, axis a = 0 / 1 / 2) that the case of at least one valid cell names, in ascending edge key c * 3 + a.
 *              Welded by edge identity, never by position: two edges whose vertices coincide through the eps snap stay two rows.  The order is
 *              brick-major and does not depend on the order in which the brick pool was filled.
 *              position: vertexInterp walked from the lower corner (p0) to the upper one (p1), times voxel_scale -- bit for bit the soup's vertex
 *              wherever the soup's cell walks the edge that way (table edges 2, 3, 6, 7 walk it the other way and differ by up to 2^-11 voxel);
 *              normal: the f16 generate_normal at that position; colour (textured maps): vertexInterp_color with the same p0 / p1 and mu;
 *              edge record: int16 (i, j, k, axis), the signed voxel index of the lower corner.
 *   triangles  int32[3] vertex rows, in ascending cell key, then in the order of the case's table row; the corners keep the table's order.  As many as the soup has.
 * tsl_mesh_generate_indexed issues the queued frames first, runs on the handle's stream and waits for the counts.  n_vertices / n_triangles are the TRUE
 * counts; every row below its capacity (max_vertices, max_triangles: both > 0) holds exactly the canonical row, nothing is written beyond it -- a stored
 * triangle may then name a vertex row that is not stored.  The buffers live on the handle and only grow. */
int  tsl_mesh_generate_indexed(tsl_tsdf* m, float surface_thres, int64_t max_vertices, int64_t max_triangles, int64_t* n_vertices, int64_t* n_triangles);
/* the first n_vertices rows of verts f32[.][3], normals f32[.][3], colors f32[.][3] (left alone for an untextured map), edges int16[.][4] and the first n_triangles
 * rows of indices int32[.][3] of the last tsl_mesh_generate_indexed; any pointer may be NULL.  Refused: more rows than that call stored (min(count, capacity)). */
int  tsl_mesh_read_indexed(tsl_tsdf* m, float* verts, float* normals, float* colors, int16_t* edges, int32_t* indices, int64_t n_vertices, int64_t n_triangles);
/* the same five arrays as DEVICE pointers (colours NULL for an untextured map) and the true counts of the last tsl_mesh_generate_indexed; the pointers
 * change when a later call asks for a larger capacity.  Any pointer may be NULL. */
int  tsl_mesh_indexed_dev(tsl_tsdf* m, void** verts_dev, void** normals_dev, void** colors_dev, void** edges_dev, void** indices_dev, int64_t* n_vertices, int64_t* n_triangles);

/* ---- coordinates that are not finite ----------------------------------------------------------------------------------------------
 * A coordinate that is not finite (NaN, +-inf), or whose cell index rnd(x / voxel) does not fit an int, lies OUTSIDE every map.  The entry points that
 * take coordinates from a caller without a range gate say so with an explicit test, never with a float-to-int conversion (which is undefined in C
 * and turns NaN into cell 0 on gfx950):
 *   - Octomap inserts (points, depth pixels) and tsl_octo_fuse_submaps: the point / leaf counts in p_oob and touches no leaf;
 *   - tsl_tsdf_query_points[_dev]: the voxel reads as outside -- TSDF 0, unobserved: modes 0 and 1 give 1, mode 2 gives 1 for param > 0;
 *   - tsl_tsdf_query_raycast[_dev]: a step whose position is not finite reads as outside, so the ray "hits" there; a NaN component of end_xyz is
 *     written as the quiet NaN 0x7fc00000 (which NaN an invalid operation produces differs between processors);
 *   - tsl_tsdf_integrate_points[_dev]: the point fails the gate `len < max_ray_length` and counts in no statistic but p_used.
 * The CPU oracle states the same (oracle/tsl_oracle.h); tests/test_octomap_limits_gpu.py and tests/test_query_edges_gpu.py hold both to it.
 * (Poses and intrinsics that are not finite are refused by the newer entry points; on the ones above they are the caller's business.) */

/* ---- batched map queries  (mapping_common.py:165-204, dense_tsdf.py:148-155; consumers: topo_graph.py:444-507) ---------- */
/* mode 0: is_pos_occupy, 1: is_pos_unobserved, 2: is_near_pos_occupy(param voxels, 0 .. 16); xyz f32 [n][3] in the active submap's frame */
int  tsl_tsdf_query_points(tsl_tsdf* m, int mode, int param, const float* xyz, int64_t n, uint8_t* out);
/* raycast(pos, dir, max_dist) per query: hit flag, last evaluated position, length travelled; (int)(max_dist / voxel) steps of one voxel.
 * TSL_ERR_ARG, before anything is launched or written, for a max_dist that is negative or not finite (its step count would never end). */
int  tsl_tsdf_query_raycast(tsl_tsdf* m, const float* pos, const float* dir, float max_dist, int64_t n, uint8_t* hit, float* end_xyz, float* len);
/* the same with DEVICE buffers, asynchronous: launched on the handle's stream (behind every queued frame) after the work already queued
 * on `user_stream` (a hipStream_t, e.g. torch's current stream; NULL = the legacy default stream), and `user_stream` waits for the
 * result -- no host round trip per 64-128-ray node expansion (topo_graph.py:444-507). */
int  tsl_tsdf_query_points_dev(tsl_tsdf* m, int mode, int param, const void* xyz_dev, int64_t n, void* out_u8_dev, void* user_stream);
int  tsl_tsdf_query_raycast_dev(tsl_tsdf* m, const void* pos_dev, const void* dir_dev, float max_dist, int64_t n,
                                void* hit_u8_dev, void* end_xyz_dev, void* len_dev, void* user_stream);

/* ---- ESDF  (dense_esdf.py:228-333 as the definition) -----------------------------------------------------------------
 * |TSDF| < gamma: ESDF = TSDF; elsewhere the 26-neighbour quasi-Euclidean distance (edge cost |dir| * voxel) to that band along voxels
 * of the same sign, capped at max_dist.  tsl_esdf_update is INCREMENTAL: the integrate kernels mark the bricks they write, an update
 * re-initialises and relaxes only those bricks dilated by max_dist (device-side work lists, no host synchronisation inside) and
 * yields exactly the map a full recompute yields.  The first update, one after reset / import / fusion or with other parameters, and
 * every update when option "esdf_full" is set, covers all bricks.  n_relaxed (nullable) = brick relaxations performed. */
typedef struct {
    int32_t incremental;         /* 0: all bricks were recomputed */
    int32_t dirty_bricks;        /* bricks written since the previous update */
    int32_t changed_bricks;      /* ... of which the ESDF inputs (observed / sign / band membership / band value of a voxel) changed */
    int32_t region_bricks;       /* bricks re-initialised and relaxed (dirty bricks dilated by max_dist) */
    int32_t total_bricks;        /* bricks of the handle */
    int64_t brick_relaxations;   /* LDS relaxations run (a brick is revisited when its surroundings change) */
    int64_t voxel_pushes;        /* voxel values lowered by the sweeps (a voxel may be lowered more than once) */
    int32_t rounds, max_passes;  /* relaxation rounds that had work; most sweep sets (six concurrent directional sweeps) one brick relaxation needed */
    int32_t raise_sets;          /* esdf_mode 1: sets of raise sweeps (parent links re-derived) over all brick visits */
    int64_t passes;              /* sweep sets over all brick relaxations */
    int64_t voxels_raised;       /* esdf_mode 1: of voxel_pushes, the values re-derived through their parent link by the raise sweeps (the rest was lowered) */
    int32_t max_raise_sets, reserved_;
} tsl_esdf_stats;
/* sums over the updates of the handle that have completed */
typedef struct {
    int64_t updates, incremental, dirty_bricks, region_bricks, brick_relaxations, voxel_pushes, passes;
} tsl_esdf_totals_t;
/* n_relaxed != NULL: waits for the update and returns its brick relaxations.  n_relaxed == NULL: ASYNCHRONOUS -- the update is only
 * enqueued (behind everything queued on the handle so far; up to 4 may be in flight; the per-frame hook of dense_esdf.py:400-402 uses this form), nothing is
 * waited for.  last_stats / totals / export wait for the outstanding updates first, so what they return is always complete. */
int  tsl_esdf_update(tsl_tsdf* m, float gamma, float max_dist, int32_t* n_relaxed);
int  tsl_esdf_last_stats(tsl_tsdf* m, tsl_esdf_stats* out);
int  tsl_esdf_totals(tsl_tsdf* m, tsl_esdf_totals_t* out);
int  tsl_esdf_export(tsl_tsdf* m, int16_t* idx, float* esdf, int64_t cap, int64_t* n);
/* the same compaction left on the device: *idx_dev = int16 [min(n, cap)][3], *val_dev = f32 [min(n, cap)] in the handle's staging buffer
 * (valid until the next exporting / importing / host-buffer query call on the handle) */
int  tsl_esdf_export_dev(tsl_tsdf* m, int64_t cap, void** idx_dev, void** val_dev, int64_t* n);
/* cvt_ESDF_to_voxels_slice(z)  dense_esdf.py:498-509: ESDF of the voxel layer at height z of the active submap -> export_ESDF_xyz /
 * export_ESDF (max_disp_particles rows on the device), *n = num_export_ESDF_particles; read back with tsl_esdf_read_slice or take the
 * device pointers (valid for the lifetime of the handle) with tsl_esdf_slice_dev */
int  tsl_esdf_slice(tsl_tsdf* m, float z, int32_t* n);
int  tsl_esdf_read_slice(tsl_tsdf* m, float* xyz, float* val, int64_t n);
int  tsl_esdf_slice_dev(tsl_tsdf* m, void** xyz_dev, void** val_dev, int32_t* n);
/* batched ESDF point queries for planners (tsl_esdf_query.hip).  xyz f32 [n][3] in the frame of the submap the ESDF was last updated for
 * (the frame of tsl_tsdf_query_points).  A voxel is KNOWN when it is in the volume, its brick is allocated and it is observed; its value is
 * the one tsl_esdf_export reports, with gamma / max_dist of the last update.
 *   mode 0: the nearest voxel (rnd_i(x / voxel), as tsl_tsdf_query_points); no gradient (grad must be NULL).
 *   mode 1: trilinear over the 8 corners of the cell floor(x / voxel), all of which must be known; grad (nullable) f32 [n][3] = the
 *           gradient of that interpolant (per metre), in the fixed f32 evaluation order DESIGN.md gives.
 * status u8 [n]: 0 ok, 1 a needed voxel is unknown, 2 a needed voxel is outside the volume or a coordinate is not finite (2 wins over 1);
 * for 1 and 2 dist = unknown_value and grad = 0.  | 0x80: the values come from an update that stopped before converging (only the device
 * form can see one; the next call that waits repairs it).  Errors: mode not 0 / 1, grad with mode 0, a null buffer, no update since the
 * map was created, reset or imported, or an active submap other than the one of the last update.  n = 0 does nothing.
 * The host form waits for the updates in flight first (never sees a short one); the device form is ASYNCHRONOUS like
 * tsl_tsdf_query_points_dev: launched on the handle's stream behind every queued frame and the latest update, after the work queued on
 * `user_stream`, which then waits for the result. */
int  tsl_esdf_query_points(tsl_tsdf* m, int mode, float unknown_value, const float* xyz, int64_t n,
                           float* dist, float* grad, uint8_t* status);
int  tsl_esdf_query_points_dev(tsl_tsdf* m, int mode, float unknown_value, const void* xyz_dev, int64_t n,
                               void* dist_dev, void* grad_dev, void* status_dev, void* user_stream);
/* batches of candidate paths scored against the ESDF in one launch (tsl_path_score.hip): which of these motions is free, how close does each come,
 * what does each cost.  Read-only, one wave per path.  Definition (tests/path_score_ref.py restates it in numpy bit for bit):
 *   Inputs.  waypoints f32 [n][K][3] in the frame of tsl_esdf_query_points; lengths int32 [n], nullable (NULL: every path has K waypoints), each in
 *     1 .. K -- the waypoints behind a path's length are never read and may hold anything; sub >= 1 sub-samples per segment; radius, margin f32, finite
 *     and >= 0; mode 0 / 1 and unknown_value as in tsl_esdf_query_points; flags below.
 *   Samples.  A path of length L has S = (L - 1) * sub + 1 samples j = 0 .. S-1; seg = j / sub, m = j % sub.  For m == 0 the sample is waypoint seg
 *     itself, bit for bit; otherwise p = a + t * (b - a) per component with t = (float)m / (float)sub, a = waypoint seg, b = waypoint seg + 1 (all f32,
 *     no contraction, correctly rounded division).  S_max = (K - 1) * sub + 1.
 *   Value and status of a sample: exactly what tsl_esdf_query_points returns for p in that mode, except that a sample of status 0 whose value is NaN,
 *     or that reads a voxel whose TSDF is NaN (one that came in through tsl_tsdf_import_sparse: the query reports sign(NaN) = 0 times the magnitude
 *     for it, so the value alone does not show it), counts as status 1 everywhere below.
 *   Classes.  hit: status 0 and d < radius; unknown: status 1; outside: status 2.  A sample BLOCKS when it is a hit, when it is unknown and flags & 2,
 *     or when it is outside and flags & 4.  first_stop = the least blocking index, or -1.
 *   Counted samples.  flags & 1 clear: every sample.  flags & 1 set (stop at the first blocking sample): the samples 0 .. first_stop inclusive; all of
 *     them when nothing blocks.
 *   tsl_path_score (40 bytes, one per path): n_samples, the counted samples; first_stop; n_hit, n_unknown, n_outside over the counted samples; argmin and
 *     min_dist over the counted samples of status 0: the minimum of the pair (key(d), j) in lexicographic order, key(d) = the monotone uint32 image of
 *     the float's bits (bits ^ 0xffffffff when the sign bit is set, else bits ^ 0x80000000: -0.0 sorts before +0.0, ties go to the lowest index),
 *     min_dist = the value at argmin bit for bit; without such a sample argmin = -1 and min_dist = +inf.  short_update: 0, or 0x80 when the values come
 *     from an update that stopped before converging (the flag of tsl_esdf_query_points; only the device form can see one).  cost: the sum over the
 *     counted samples of status 0 with c > 0 of (int64)(int32)(c * 1048576.0f), truncated toward zero, c = fminf(rm - d, 1024.0f), rm = radius + margin
 *     rounded to f32 once on the host: a 2^-20 fixed point, order-free, at most 2^30 per term.
 *   Optional per-sample outputs, each nullable on its own: sample_dist f32 [n][S_max] and sample_status u8 [n][S_max].  A counted sample gets the
 *     query's dist and status (0 / 1 / 2, without the 0x80 flag, which is in the record; a NaN-valued sample: unknown_value and 1); every other entry of
 *     the row gets unknown_value and 0xff.
 * TSL_ERR_ARG, before anything is launched or written: whatever tsl_esdf_query_points refuses (no update since the map was created, reset or imported;
 * the active submap changed; a bad mode); null waypoints or out with n > 0; n outside 0 .. 2^20; K outside 1 .. 4096; sub outside 1 .. 256; S_max > 2^20;
 * n * S_max >= 2^31 with a per-sample output; radius or margin negative or not finite; flags with bits other than 1, 2, 4; and, in the host form, a
 * length outside 1 .. K -- the device form cannot look and CLAMPS every length into 1 .. K.  n = 0 does nothing.
 * The host form copies in through the handle's staging buffer and waits for the updates in flight first (never sees a short one); the device form is
 * ASYNCHRONOUS and ordered like tsl_esdf_query_points_dev (lengths_dev nullable; out_dev holds n records, as int32 [n][10]).  out_dev
 * must be aligned to 8 bytes (the int64 cost lies at offset 32 of the 40-byte record), waypoints_dev, lengths_dev and sample_dist_dev to 4.  With
 * profiling on, tsl_tsdf_prof_query(m, TSL_K_PATH_SCORE) returns the time of the kernel alone. */
typedef struct { int32_t n_samples, first_stop, n_hit, n_unknown, n_outside, argmin; float min_dist; int32_t short_update; int64_t cost; } tsl_path_score;
int  tsl_esdf_score_paths(tsl_tsdf* m, int mode, float unknown_value, const float* waypoints, const int32_t* lengths, int64_t n, int32_t K, int32_t sub,
                          float radius, float margin, int32_t flags, tsl_path_score* out, float* sample_dist, uint8_t* sample_status);
int  tsl_esdf_score_paths_dev(tsl_tsdf* m, int mode, float unknown_value, const void* waypoints_dev, const void* lengths_dev, int64_t n, int32_t K,
                              int32_t sub, float radius, float margin, int32_t flags, void* out_dev, void* sample_dist_dev, void* sample_status_dev,
                              void* user_stream);
/* batches of uniform cubic B-spline trajectories optimised against the ESDF in one launch (tsl_traj_opt.hip): the collision and smoothness costs of
 * every trajectory with their gradients over the control points (linearize), and a momentum descent on them that runs all of its iterations inside the
 * kernel (optimize).  Read-only on the map, one wave per trajectory.  Definition (tests/traj_opt_ref.py restates it in numpy bit
 * for bit); every f32 product, sum and quotient below is rounded on its own, nothing is fused, divisions are correctly rounded:
 *   Inputs.  ctrl f32 [n][K][3], control points in the frame of tsl_esdf_query_points; lengths int32 [n], nullable (NULL: every trajectory has K points),
 *     each in 4 .. K -- the linearisation never reads the rows past a length; sub in 1 .. 64; clearance finite and >= 0; unknown_value as in
 *     tsl_esdf_query_points.  n in 0 .. 2^20, K in 4 .. 256.
 *   Samples.  A trajectory of length L has S = (L - 3) * sub + 1 samples j = 0 .. S-1: seg = min(j / sub, L - 4), m = j - seg * sub (the last sample has
 *     m = sub).  u = (float)m / (float)sub, v = 1 - u, u2 = u * u, u3 = u2 * u; b0 = (v * v) * v, b1 = (3 u3 - 6 u2) + 4, b2 = ((3 u2 - 3 u3) + 3 u) + 1,
 *     b3 = u3; w_i = b_i / 6.0f; per axis p = ((w0 c0 + w1 c1) + w2 c2) + w3 c3 with c_i = ctrl[seg + i].
 *   Value of a sample: tsl_esdf_query_points mode 1 (trilinear, with its gradient g) at p.  A sample of status 0 counts as status 1 (unknown) when its
 *     value or a component of g is not finite, or when it reads a voxel whose TSDF is NaN (as in tsl_esdf_score_paths).  A p that is not finite is
 *     status 2.
 *   q(t) = (int64)(int32)(fminf(fmaxf(t, -1024.0f), 1024.0f) * 1048576.0f), truncated toward zero: the 2^-20 fixed point of every gradient term.
 *   Collision term, per sample of status 0: c = fminf(clearance - d, 1024.0f); the sample is PENALISED when c > 0, and then
 *     cost_collision += (int64)((c * c) * 1048576.0f) (truncated) and, per axis a and i = 0 .. 3, Gp = -((2.0f * c) * g_a),
 *     grad_collision[seg + i][a] += q(w_i * Gp).
 *   Smoothness term, for i = 0 .. L - 3 and per axis: a = (c_i - (c_{i+1} + c_{i+1})) + c_{i+2}; a term whose a is not finite is skipped; otherwise with
 *     ac = fminf(fmaxf(a, -1024.0f), 1024.0f): cost_smooth += (int64)((ac * ac) * 1048576.0f), grad_smooth[i] += q(2.0f * a),
 *     grad_smooth[i + 1] += q(-4.0f * a), grad_smooth[i + 2] += q(2.0f * a).
 *   tsl_traj_score (48 bytes, one per trajectory): n_samples = S; n_pen, the penalised samples; n_unknown and n_outside, the samples of status 1 and 2;
 *     argmin / min_dist over the samples of status 0 by the (key(d), j) rule of tsl_path_score (-1 / +inf without one); short_update as there;
 *     iters_done; cost_collision, cost_smooth.  All sums are integers: every field is independent of the schedule.
 *   Descent (tsl_traj_opt; every f32 finite and >= 0, iters in 0 .. 1024, fix_head, fix_tail >= 0, flags bit 0 = stop at the first free
 *     linearisation).  Velocities start at 0.  For k = 0 .. iters - 1: linearise the control points as they stand; with flags & 1 and n_pen == 0 stop,
 *     iters_done = k; otherwise, for every control point i in fix_head .. L - 1 - fix_tail and every axis: gcf = (float)grad_collision *
 *     9.5367431640625e-07f, gsf likewise (int64 -> f32 rounds to nearest even), g = w_collision * gcf + w_smooth * gsf,
 *     v = momentum * v - step * g, a v that is not finite becomes 0, v = fminf(fmaxf(v, -max_move), max_move), c = c + v.  Without a stop
 *     iters_done = iters.  The record (and the gradients of linearize) is the linearisation of the control points as they stand at the end, so iters = 0
 *     is the pure linearisation and returns ctrl bit for bit; the rows past a length are copied through to ctrl_out.
 *   history (nullable) int64 [n][iters + 1][2]: (cost_collision, cost_smooth) of linearisation k = 0 .. iters_done, -1 in the entries behind it.
 *   grad_collision, grad_smooth (nullable, each on its own) int64 [n][K][3]; the rows past a length are 0.  out is nullable too.
 * TSL_ERR_ARG, before anything is launched or written: whatever tsl_esdf_query_points refuses (no update since the map was created, reset or imported;
 * the active submap changed); null ctrl (or ctrl_out, for optimize) with n > 0; n, K, sub, iters outside their ranges; a clearance, weight, step,
 * momentum or max_move that is negative or not finite; fix_head or fix_tail negative, fix_head + fix_tail > K; flags with bits other than 1; and, in
 * the host forms, a length outside 4 .. K -- the device forms CLAMP every length into 4 .. K.  n = 0 does nothing.
 * The host forms stage through the handle's staging buffer and wait for the updates in flight first; the device forms are ASYNCHRONOUS and ordered like
 * tsl_esdf_score_paths_dev.  out_dev, the gradient planes and history_dev must be aligned to 8 bytes, the rest to 4.  ctrl_out may not overlap ctrl. */
typedef struct { int32_t n_samples, n_pen, n_unknown, n_outside, argmin; float min_dist; int32_t short_update, iters_done; int64_t cost_collision, cost_smooth; } tsl_traj_score;
typedef struct { float clearance, w_collision, w_smooth, step, momentum, max_move; int32_t sub, iters, fix_head, fix_tail, flags, reserved_; } tsl_traj_opt;
int  tsl_esdf_traj_linearize(tsl_tsdf* m, float unknown_value, const float* ctrl, const int32_t* lengths, int64_t n, int32_t K, int32_t sub, float clearance,
                             tsl_traj_score* out, int64_t* grad_collision, int64_t* grad_smooth);
int  tsl_esdf_traj_linearize_dev(tsl_tsdf* m, float unknown_value, const void* ctrl_dev, const void* lengths_dev, int64_t n, int32_t K, int32_t sub,
                                 float clearance, void* out_dev, void* grad_collision_dev, void* grad_smooth_dev, void* user_stream);
int  tsl_esdf_traj_optimize(tsl_tsdf* m, float unknown_value, const float* ctrl, const int32_t* lengths, int64_t n, int32_t K, const tsl_traj_opt* opt,
                            float* ctrl_out, tsl_traj_score* out, int64_t* history);
int  tsl_esdf_traj_optimize_dev(tsl_tsdf* m, float unknown_value, const void* ctrl_dev, const void* lengths_dev, int64_t n, int32_t K, const tsl_traj_opt* opt,
                                void* ctrl_out_dev, void* out_dev, void* history_dev, void* user_stream);

/* ---- view rendering (tsl_render.hip): what a camera at a pose would see of the TSDF -- depth, normal and colour per pixel.  It stands beside
 * BaseMap.raycast (mapping_common.py:165-178; tsl_tsdf_query_raycast above), which steps a whole voxel at a time and returns the last stepped
 * position; the reference has no renderer.  R (row-major) / T: the camera-to-map pose in the frame of tsl_tsdf_query_points (the active submap's;
 * submap 0 on a global map), given as doubles and rounded to f32 once.  Definition (all f32, in this order):
 *   pixel (u, v): dc = ((u - cx) / fx, (v - cy) / fy, 1), d = R dc -- NOT normalised: the ray parameter is the optical-axis depth, the unit of
 *   the depth images.  Samples n = 0 .. S-1, S = (int)((t_max - t_min) / dt) + 1, at t_n = t_min + n * dt, p_n = T + t_n d.  A sample's value is the
 *   trilinear interpolant of the stored TSDF over the 8 corners of the cell floor(p / voxel) (the interpolant of tsl_esdf_query_points mode 1);
 *   it is KNOWN when all 8 are in the volume, in allocated bricks and observed.  Two consecutive known samples with s_prev > 0 >= s_n are a hit
 *   (front face): t* = t_prev + dt * (s_prev / (s_prev - s_n)); with s_prev <= 0 < s_n a back face, which ends the ray.  An unknown sample only
 *   forgets the previous one.
 * Outputs, row-major [h][w]: depth f32 = t* (0 unless hit); normal (nullable) f32 x 3 = the gradient of the interpolant at T + t* d divided by
 * its length, pointing from the surface into free space, in the map frame; rgb (nullable, textured maps only) f32 x 3 = the colour of the voxel
 * rnd_i(p* / voxel) as the surface export reports it (0 when that voxel is unknown); status u8: 0 hit, 1 miss, 2 back face, | 0x40 a hit whose
 * normal could not be formed (a corner of p*'s cell is unknown or the gradient is 0): the normal is 0.
 * tsl_view_cfg: K row-major intrinsics (all 9 zero = the map's depth intrinsics), t_min / t_max (0 = the map's min / max_ray_length), dt (0 =
 * 0.75 * voxel: about one voxel of path per sample at the corners of the field of view; the negative band behind a surface is internal_voxels
 * deep, so a front face cannot be stepped over), flags bit 0 = evaluate every sample (by default a ray jumps over unallocated bricks and the
 * space outside the volume; the result is the same bit for bit -- the A/B switch).
 * TSL_ERR_ARG: a null handle / pose / cfg / depth / status, rgb on an untextured map, a non-finite pose, intrinsic or range, h or w outside
 * 1 .. 32768, t_max <= t_min or dt <= 0 after the defaults, more than 2^24 samples per ray.
 * The host form issues the queued frames, renders on the handle's stream, waits and copies back; the device form is ASYNCHRONOUS like
 * tsl_tsdf_query_raycast_dev: launched on the handle's stream behind every queued frame, after the work queued on `user_stream`, which then
 * waits for the result.  Neither reads or updates the ESDF. */
typedef struct { double K[9]; int32_t h, w; float t_min, t_max, dt; int32_t flags; } tsl_view_cfg;
int  tsl_tsdf_render_view(tsl_tsdf* m, const double R[9], const double T[3], const tsl_view_cfg* v,
                          float* depth, float* normal, float* rgb, uint8_t* status);
int  tsl_tsdf_render_view_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_view_cfg* v,
                              void* depth_dev, void* normal_dev, void* rgb_dev, void* status_dev, void* user_stream);

/* ---- frame-to-model alignment (tsl_align.hip): a depth frame against the TSDF, Gauss-Newton on the signed distance -- minimise the sum of
 * s(R p_i + T)^2 over the camera-to-map pose (Bylow et al. 2013; Canelhas' SDF tracker).  The reference takes its poses from a VIO and has no
 * tracker.  R (row-major) / T: the camera-to-map pose in the frame of tsl_tsdf_query_points (the active submap's; submap 0 on a global map),
 * given as doubles and rounded to f32 once.  depth: uint16 millimetres [h][w], C-contiguous.
 * Definition (all f32, no contraction, in this order).  Visited pixels (i, j) = (ii * stride, jj * stride), ii < ceil(w /
 * stride), jj < ceil(h / stride); each lands in exactly one bucket, tested in this order:
 *   n_gate     d == 0, (float)d > d_max * 1000 or (float)d < d_min * 1000.  Otherwise dep = (float)d / 1000, px = ((float)i - cx) * dep / fx,
 *              py = ((float)j - cy) * dep / fy, pz = dep and p[a] = ((R[a][0] * px + R[a][1] * py) + R[a][2] * pz) + T[a]
 *   n_unknown  the sample at p is not KNOWN in the sense of tsl_tsdf_render_view (8 corners in the volume, in allocated bricks and observed, p
 *              finite).  Otherwise s = the trilinear interpolant, g = its gradient per metre (the expressions of tsl_esdf_query_points mode 1)
 *   n_far      not |s| <= r_max: |s| > r_max, or s is a NaN
 *   n_grad     gg = (g0 * g0 + g1 * g1) + g2 * g2 is not in (0, g_max * g_max]: 0, above it, or a NaN
 *   n_used     c = p x g, J = (g0, g1, g2, c0, c1, c2), wgt = huber > 0 && |s| > huber ? huber / |s| : 1, wJ[a] = wgt * J[a]; the 28 products
 *              H_ab = wJ[a] * J[b] (a <= b, row-major upper triangle), b_a = wJ[a] * s, e = (wgt * s) * s
 * Every product x is added as the integer rint(x * 2^20) (round half to even) into an int64 sum, so the sums are the same for any schedule.
 * Stored values that are not finite (tsl_tsdf_import_sparse writes any f16 bit pattern; a submap from another robot may hold one): a NaN or inf
 * corner makes the interpolant or the gradient of its cell a NaN or an inf (0 * inf is a NaN), and such a sample is far or grad, never used -- no
 * value that is not finite reaches a product, so the sums stay defined and the overflow refusal holds.  The per-point s of a far sample whose
 * interpolant is a NaN is that NaN as it stands (which NaN is not specified).  The readers that return floats (tsl_tsdf_render_view, the ESDF
 * queries, the meshing) pass such a value through.
 * tsl_align_cfg: K row-major intrinsics (all 9 zero = the map's depth intrinsics), stride >= 1, d_min / d_max (0 = the map's min / max_ray_length),
 * r_max (0 = internal_voxels * voxel, the depth of the negative band), g_max (0 = 4), huber (0 = off), flags bit 0 = counts only: the
 * products and their reduction are left out, H, b and e are 0 (what the gathers alone cost: the A/B switch of tools/bench_track.py; a tracker needs 0).
 * The call is refused unless M^2 * 2^20 * visited <= 2^62, M = max(2 L g_max, g_max, r_max), L the largest absolute coordinate of the volume: no
 * sum can overflow.
 * tsl_tsdf_align_linearize issues the queued frames, runs on the handle's stream, waits and returns the 33 integers.  The device form is
 * ASYNCHRONOUS like tsl_tsdf_render_view_dev: sums_dev (int64[40]: the 33 integers in the order of tsl_align_sums, the rest 0) is zeroed and
 * filled on the handle's stream behind every queued frame, after the work queued on `user_stream`, which then waits for the result.
 * Step (pure host, float64, fixed order, no libm call but sqrt): Hd = H * 2^-20, bd = b * 2^-20, Hd_aa += damping * Hd_aa, Cholesky L L^T
 * without pivoting; a pivot <= 0 or not finite (or a non-finite solution) is singular: *singular = 1 and xi = 0; else xi = (v, omega) = -Hd^-1 bd.
 * Retraction (pure host, in place): the Cayley map, a = omega / 2, C = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a); R <- C R, T <- C T + v.
 * Tracking: up to 4 levels (stride, iters), at most 64 iterations in all.  An iteration linearises at the current pose, solves and retracts; a
 * level ends early when sqrt(|v|^2 + |omega|^2) < min_step.  status 0: the last level ended by the threshold, 1: its iterations were exhausted,
 * 2: lost -- a linearisation had n_used < min_used (0 = 6), 3: singular.  On 2 and 3 the pose returned is the last one that gave a step, or the
 * guess.  Every linearisation leaves a record: the float64 pose, the sums, xi (0 where there was no step); `iterations` counts the records.
 * tsl_tsdf_track_depth_dev first makes the handle's stream wait for the work queued on `user_stream`, then runs as the host form and returns
 * when it is done.
 * TSL_ERR_ARG (the text names the entry point): a null handle / pose / cfg / depth / out, a non-finite pose, intrinsic or parameter, h or w outside
 * 1 .. 32768, stride < 1, d_max <= d_min after the defaults, a negative r_max / g_max / huber / damping / min_step, the overflow bound, more
 * than 4 levels or 64 iterations. */
typedef struct { double K[9]; int32_t h, w, stride; float d_min, d_max, r_max, g_max, huber; int32_t flags; } tsl_align_cfg;
typedef struct { int64_t H[21], b[6], e, n_used, n_gate, n_unknown, n_far, n_grad; } tsl_align_sums;
typedef struct { int32_t n_levels, stride[4], iters[4], min_used; double min_step, damping; } tsl_track_cfg;
typedef struct { double R[9], T[3], xi[6]; tsl_align_sums sums; } tsl_track_iter;
typedef struct { int32_t status, iterations; tsl_track_iter it[64]; } tsl_track_report;
int  tsl_tsdf_align_linearize(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_cfg* c, const uint16_t* depth, tsl_align_sums* out);
int  tsl_tsdf_align_linearize_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_cfg* c, const void* depth_dev,
                                  void* sums_dev, void* user_stream);
int  tsl_align_solve(const tsl_align_sums* s, double damping, double xi[6], int32_t* singular);
int  tsl_pose_retract(const double xi[6], double R[9], double T[3]);
int  tsl_tsdf_track_depth(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_cfg* c, const tsl_track_cfg* t, const uint16_t* depth,
                          double R_out[9], double T_out[3], tsl_track_report* rep);
int  tsl_tsdf_track_depth_dev(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_cfg* c, const tsl_track_cfg* t, const void* depth_dev,
                              double R_out[9], double T_out[3], tsl_track_report* rep, void* user_stream);

/* ---- depth-and-colour alignment (tsl_align_rgbd.hip): the problem of the section above with a second residual, the
 * luminance the textured map stores at the warped pixel minus the luminance of the image (Bylow, Olsson, Kahl, "Robust camera tracking by combining
 * color and depth measurements", ICPR 2014).  Signed distance says nothing in the directions in which the geometry does not change (a flat wall
 * leaves three degrees of freedom, a corridor one); the texture of the surface does.  The map must be textured (texture_enabled).
 * depth: uint16 millimetres [h][w]; rgb: uint8 [h][w][3], registered to the depth image (the same h, w and intrinsics), both C-contiguous.
 * Definition (all f32, no contraction, in this order).  The visited pixels, the depth gate, the back-projection, p, the KNOWN test, s and g are
 * those of tsl_tsdf_align_linearize, and the GEOMETRIC sums (geo) are exactly its 33 integers.
 *   voxel luminance   yv = ((77 * r + 150 * g) + 29 * b) / 256 of the three stored f16 channels converted to f32
 *   image luminance   yi = (float)(77 * R + 150 * G + 29 * B) / 65280.0f (the integer is exact)
 *   map luminance     Y = the trilinear interpolant and gY = its gradient per metre of the eight yv, over the same eight corners and with the
 *                     same cell fractions as s (a KNOWN cell of a textured map has all eight)
 * The COLOUR sums (col) are a second tsl_align_sums; every visited pixel lands in exactly one of its buckets, tested in this order:
 *   n_gate     the geometric gate
 *   n_unknown  the geometric unknown
 *   n_far      not |s| <= r_max (off the surface, where the colour means nothing), or rc = Y - yi is not |rc| <= rc_max (a NaN is far)
 *   n_grad     (gY0 * gY0 + gY1 * gY1) + gY2 * gY2 is not in (0, gc_max * gc_max]
 *   n_used     J = (gY, p x gY), wgt = huber_c > 0 && |rc| > huber_c ? huber_c / |rc| : 1 and the 28 products of the section above with rc in place
 *              of s, each added as rint(x * 2^20)
 * The colour buckets do not depend on the geometric n_grad.  A stored colour that is not finite (tsl_tsdf_import_sparse writes any bit pattern)
 * makes Y or gY of its cells a NaN or an inf: such a sample is colour-far or colour-grad, no such value reaches a product, and the geometric half is
 * untouched.
 * tsl_align_rgbd_cfg: a (tsl_align_cfg: everything of the section above, flags bit 0 = counts only for both halves), rc_max (0 = 1), gc_max (0 =
 * 1 / voxel, formed once in f32), huber_c (0 = off).  Each half has its own overflow refusal: the geometric bound as it stands, and
 * Mc^2 * 2^20 * visited <= 2^62 with Mc = max(2 L gc_max, gc_max, rc_max).
 * tsl_tsdf_align_rgbd_linearize issues the queued frames, runs on the handle's stream, waits and returns the 66 integers.  The device form is
 * ASYNCHRONOUS like tsl_tsdf_align_linearize_dev, with its stream ordering: sums_dev is int64[80], geo in [0, 33), col in [40, 73), the rest 0.
 * Step (pure host, float64, fixed order): Hd = Hg * 2^-20 + lambda * (Hc * 2^-20), bd likewise; then the damping, the Cholesky factorisation and
 * the solution of tsl_align_solve.  With lambda = 0 the step equals tsl_align_solve on the geometric half bit for bit.
 * Tracking iterates as tsl_tsdf_track_depth does, with the same tsl_track_cfg, statuses and returned pose.  lambda >= 0 is the weight of the
 * colour term; lambda < 0 means automatic: at the first linearisation of the track lambda = balance * (Hg_00 + Hg_11 + Hg_22) / (Hc_00 + Hc_11 +
 * Hc_22), from the integers converted to float64 and added in this order, 0 when the denominator is 0 (an untextured view falls back to pure
 * geometry) -- the two terms are then equally stiff in translation.  The value is held for the whole call and returned in the report (0 when
 * nothing was linearised).  A track is lost when the GEOMETRIC n_used < min_used (0 = 6): colour alone does not fix depth.
 * With profiling on, tsl_tsdf_prof_query(m, TSL_K_ALIGN_RGBD) returns the time of the kernel alone.
 * TSL_ERR_ARG before anything is launched: everything tsl_tsdf_align_linearize refuses, a null rgb, an untextured map, a negative or non-finite
 * rc_max / gc_max / huber_c / balance, a non-finite lambda (tsl_align_rgbd_solve: a negative one too), either overflow bound. */
typedef struct { tsl_align_cfg a; float rc_max, gc_max, huber_c; } tsl_align_rgbd_cfg;
typedef struct { tsl_align_sums geo, col; } tsl_align_rgbd_sums;
typedef struct { double R[9], T[3], xi[6]; tsl_align_rgbd_sums sums; } tsl_track_rgbd_iter;
typedef struct { int32_t status, iterations; double lambda; tsl_track_rgbd_iter it[64]; } tsl_track_rgbd_report;
int  tsl_tsdf_align_rgbd_linearize(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_rgbd_cfg* c, const uint16_t* depth,
                                   const uint8_t* rgb, tsl_align_rgbd_sums* out);
int  tsl_tsdf_align_rgbd_linearize_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_rgbd_cfg* c, const void* depth_dev,
                                       const void* rgb_dev, void* sums_dev, void* user_stream);
int  tsl_align_rgbd_solve(const tsl_align_rgbd_sums* s, double lambda, double damping, double xi[6], int32_t* singular);
int  tsl_tsdf_track_rgbd(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_rgbd_cfg* c, const tsl_track_cfg* t, double lambda,
                         double balance, const uint16_t* depth, const uint8_t* rgb, double R_out[9], double T_out[3], tsl_track_rgbd_report* rep);
int  tsl_tsdf_track_rgbd_dev(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_rgbd_cfg* c, const tsl_track_cfg* t, double lambda,
                             double balance, const void* depth_dev, const void* rgb_dev, double R_out[9], double T_out[3], tsl_track_rgbd_report* rep,
                             void* user_stream);

/* ---- scan-to-model alignment (tsl_align_points.hip): a point cloud against the TSDF -- the problem of the section above for sensors whose data is
 * no pinhole image (a spinning or solid-state lidar, a merged multi-camera cloud, an undistorted depth image): minimise the sum of s(R p_i + T)^2
 * over the sensor-to-map pose, p_i the points of the cloud in the sensor frame.  R (row-major) / T: the sensor-to-map pose in the frame of
 * tsl_tsdf_query_points (the active submap's; submap 0 on a global map), given as doubles and rounded to f32 once.  xyz: f32 [n][3],
 * C-contiguous, 0 <= n <= 2^30.
 * Definition (all f32, no contraction, in this order).  Visited point k is point k * stride, k < visited = ceil(n /
 * stride); each lands in exactly one bucket, tested in this order:
 *   n_gate     x, y or z is not finite, or l2 = (x * x + y * y) + z * z is > dmax2 or < dmin2, with dmax2 = d_max * d_max and dmin2 = d_min * d_min
 *              formed once in f32 (an l2 that overflows to inf is gated).  Otherwise p[a] = ((R[a][0] * x + R[a][1] * y) + R[a][2] * z) + T[a]
 *   n_unknown, n_far, n_grad, n_used   as in the section above, with the same 28 products and the same integer sums.
 * tsl_align_points_cfg: stride >= 1, d_min / d_max (the range gate in metres; 0 = the map's min / max_ray_length), r_max, g_max, huber and flags
 * bit 0 (counts only) as in tsl_align_cfg.  The overflow bound is that of the section above with the visited points for the visited pixels.
 * Per-point outputs, each optional (null = not wanted) and indexed by k: bucket[k] (uint8) 0 used, 1 gate, 2 unknown, 3 far, 4 grad; s[k] (f32) the
 * interpolant at p for used, far and grad, +0.0f for gate and unknown: what a caller needs to drop the points of moving objects before it
 * integrates the scan.
 * tsl_tsdf_align_points_linearize issues the queued frames, runs on the handle's stream, waits and returns the 33 integers (and the per-point
 * outputs).  The device form is ASYNCHRONOUS with the stream ordering of tsl_tsdf_align_linearize_dev: sums_dev (int64[40]), bucket_dev
 * (uint8[visited]) and s_dev (f32[visited]) are filled on the handle's stream behind every queued frame, after the work queued on `user_stream`,
 * which then waits for the result.  n = 0 is legal: the sums are zero and nothing is launched.
 * tsl_tsdf_track_points iterates as tsl_tsdf_track_depth does, with the same tsl_track_cfg (stride[l] is the point stride of level l; the
 * configuration's own stride is not used) and the same tsl_track_report, statuses and returned pose; an empty cloud ends with status 2.
 * tsl_tsdf_track_points_dev first makes the handle's stream wait for the work queued on `user_stream`, then runs as the host form and returns
 * when it is done.  With profiling on, tsl_tsdf_prof_query returns the time of the linearisation kernels alone: TSL_K_ALIGN_POINTS, and TSL_K_ALIGN for
 * the image form.
 * TSL_ERR_ARG (the text names the entry point), before anything is launched or written: a null handle / pose / cfg / xyz (with n > 0) / out, a
 * non-finite pose or parameter, n < 0 or n > 2^30, stride < 1, d_max <= d_min after the defaults, a negative d_min / r_max / g_max / huber, the
 * overflow bound, the track-configuration errors of the section above. */
typedef struct { int32_t stride; float d_min, d_max, r_max, g_max, huber; int32_t flags; } tsl_align_points_cfg;
int  tsl_tsdf_align_points_linearize(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_points_cfg* c, const float* xyz, int64_t n,
                                     tsl_align_sums* out, uint8_t* bucket, float* s);
int  tsl_tsdf_align_points_linearize_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_points_cfg* c, const void* xyz_dev, int64_t n,
                                         void* sums_dev, void* bucket_dev, void* s_dev, void* user_stream);
int  tsl_tsdf_track_points(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_points_cfg* c, const tsl_track_cfg* t, const float* xyz,
                           int64_t n, double R_out[9], double T_out[3], tsl_track_report* rep);
int  tsl_tsdf_track_points_dev(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_points_cfg* c, const tsl_track_cfg* t,
                               const void* xyz_dev, int64_t n, double R_out[9], double T_out[3], tsl_track_report* rep, void* user_stream);

/* ---- map-to-map registration (tsl_register.hip): a TSDF submap against another map, Gauss-Newton on the difference of the two signed distances --
 * minimise the sum of (s(R q_i + T) - t_i)^2 over X = (R, T), q_i the voxels of the source submap near its surface, t_i the values it stores there and
 * s the trilinear interpolant of the destination.  It tells whether two submaps agree where they overlap, returns the relative pose at which they
 * do, and the normal equations behind it: a constraint for a pose graph.  The reference takes its submap poses from a pose graph outside and has no
 * counterpart.  dst / dst_sid: the destination map and submap; -1 = the frame of tsl_tsdf_query_points (the active submap; submap 0 on a global
 * map).  src / src_sid: the source map and submap; -1 = its active submap.  src and dst may be the same handle; they must live on the same device
 * and have bit-equal f32 voxel sizes (the assumption of tsl_tsdf_fuse_submaps).  R (row-major) / T take source-submap coordinates to destination
 * coordinates, given as doubles and rounded to f32 once.
 * Definition (all f32, no contraction, in this order).  Visited: the observed voxels of the source submap whose indices (i, j, k)
 * are each divisible by stride; unobserved voxels are neither visited nor counted.  Each visited voxel lands in exactly one bucket, tested in this order:
 *   n_gate     not (w >= w_min && fabsf(t) <= band), w the stored f16 weight, t the stored f16 TSDF value: a NaN weight or value is gated.  Otherwise q = ((float)i * voxel, (float)j * voxel,
 *              (float)k * voxel) and p[a] = ((R[a][0] * q0 + R[a][1] * q1) + R[a][2] * q2) + T[a]
 *   n_unknown  the sample of dst at p is not KNOWN in the sense of tsl_tsdf_render_view (8 corners in the volume, in allocated bricks of dst_sid and
 *              observed, p finite).  Otherwise s = the trilinear interpolant, g = its gradient per metre (tsl_esdf_query_points mode 1)
 *   n_far      not |s| <= r_max: |s| > r_max, or s is a NaN
 *   n_grad     gg = (g0 * g0 + g1 * g1) + g2 * g2 is not in (0, g_max * g_max]: 0, above it, or a NaN
 *   n_used     r = s - t, c = p x g, J = (g0, g1, g2, c0, c1, c2), wgt = huber > 0 && |r| > huber ? huber / |r| : 1, wJ[a] = wgt * J[a]; the 28 products
 *              H_ab = wJ[a] * J[b] (a <= b, row-major upper triangle), b_a = wJ[a] * r, e = (wgt * r) * r
 * As in the alignment, a stored value of dst that is not finite makes its cells' samples far or grad, and one of src is gated: none reaches a product.
 * Every product x is added as the integer rint(x * 2^20) into an int64 sum; the result is a tsl_align_sums, the same 33 integers in the same order,
 * so tsl_align_solve and tsl_pose_retract serve unchanged (the step is the left twist p <- p + v + omega x p).
 * tsl_register_cfg: stride 1, 2, 4, 8 or 16; w_min (0 = every weight passes); band (0 = 2 * voxel); r_max (0 = internal_voxels * voxel of dst); g_max
 * (0 = 4); huber (0 = off); flags bit 0 = counts only: the products and their reduction are left out, H, b and e are 0 (the A/B switch of
 * tools/bench_register.py).  The call is refused unless M^2 * 2^20 * V <= 2^62, M = max(2 L g_max, g_max, r_max + band), L the largest absolute
 * coordinate of dst's volume, V = min(max_bricks, bricks per submap) of src * (16 / stride)^3, an upper bound of the visited voxels: no sum can overflow.
 * tsl_tsdf_register_submap iterates linearise, solve, retract as tsl_tsdf_track_depth does, with the same tsl_track_cfg (every level's stride one of
 * 1, 2, 4, 8, 16; the Python default is (4, 4 iterations), (2, 4), (1, 6)) and the same tsl_track_report: min_used, min_step, damping, the four
 * statuses and the pose returned on lost / singular are those of tsl_tsdf_track_depth.
 * Both are host forms: they issue the queued frames of both handles, wait for the source's work (as tsl_tsdf_fuse_submaps does), run on dst's stream
 * and wait.  Neither writes to either map.  dst's export staging buffer holds the accumulator: device pointers from tsl_esdf_export_dev are invalid
 * afterwards.  With profiling on, tsl_tsdf_prof_query(dst, TSL_K_REGISTER) returns the time of the kernel alone.
 * TSL_ERR_ARG (the text names the entry point): a null handle / pose / cfg / out, a non-finite pose or parameter, a stride that is not a power of two
 * in 1 .. 16, a negative w_min / band / r_max / g_max / huber / damping / min_step, a submap id outside -1 .. max_submap_num - 1 (outside -1 .. 0 on a
 * global map), maps on different devices or with different voxel sizes, the overflow bound, more than 4 levels or 64 iterations. */
typedef struct { int32_t stride; float w_min, band, r_max, g_max, huber; int32_t flags; } tsl_register_cfg;
int  tsl_tsdf_register_linearize(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R[9], const double T[3],
                                 const tsl_register_cfg* c, tsl_align_sums* out);
int  tsl_tsdf_register_submap(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R0[9], const double T0[3],
                              const tsl_register_cfg* c, const tsl_track_cfg* t, double R_out[9], double T_out[3], tsl_track_report* rep);

/* ---- pose search for the registration (tsl_register_search.hip): many poses scored in one call; a lattice of candidates around a guess, the best
 * one refined by tsl_tsdf_register_submap.  tsl_tsdf_register_submap is local: from a guess in the basin of another minimum (a room's quarter-turn
 * alias at a loop closure) it returns a confident wrong pose.  The search scores a window of poses by brute force first.
 * tsl_tsdf_register_score: out[k] holds e, n_used, n_unknown, n_far and n_grad of the tsl_align_sums that
 * tsl_tsdf_register_linearize returns for the pose (R + 9 k, T + 3 k) with the same handles, submap ids and tsl_register_cfg: the same stride, gates,
 * buckets and their order, robust weight, f32 rounding of the pose and order of evaluation.  flags bit 0 (counts only) leaves e at 0.  gate (may be
 * null) does not depend on the pose: n_gate as in the linearisation, n_pass = the visited voxels that pass the gate, sum_i / sum_j / sum_k the integer
 * sums of their voxel indices, so (sum / n_pass) * voxel is the centroid of what is being registered.  1 <= n <= 65536.
 * It is a host form with the contract of tsl_tsdf_register_linearize: it issues the queued frames of both handles, waits for the source's work, runs on
 * dst's stream, waits, and writes neither map.  dst's export staging buffer holds the counters, the poses, the scores and the list of gated source
 * voxels (8 bytes each): device pointers from tsl_esdf_export_dev are invalid afterwards.  With profiling on, tsl_tsdf_prof_query(dst,
 * TSL_K_REGISTER_SCORE) returns the time of the scoring kernel alone (not of the two passes that build the list).
 * tsl_tsdf_register_score_tile: the entries of the list that one workgroup of the scoring kernel stages for a list of `entries` (= gate.n_pass) and n
 * poses on dst's device -- 256, halved down to 64 while tiles * ceil(n / 64) < 8 * compute units; 0 for a null handle, entries < 1 or n outside
 * 1 .. 65536.  It changes no result; tests and tools ask it which tile a case takes.
 * tsl_tsdf_register_search.  Everything below is host float64 in the written order (tests/register_search_ref.py restates it bit for bit).
 *   Candidates: n_candidates = the product of the six 2 n + 1 (n_r[0..2], n_t[0..2] are half-counts); the index k runs over (r0, r1, r2, t0, t1, t2),
 *     the last fastest; an axis' offset is (index - n) * step; omega = the three rotation offsets, v = the three translation offsets.  Tp = T0 - pivot;
 *     (R, Tp) <- tsl_pose_retract((0, 0, 0, omega), R0, Tp); T = (Tp + pivot) + v: the guess turned about the pivot by the Cayley map of omega -- an
 *     angle of 2 atan(|omega| / 2), not |omega| -- then shifted.  The candidate with all six offsets zero is (R0, T0) itself, bit for bit.
 *   Pivot: flags bit 0 = `pivot` is given (dst coordinates).  Otherwise the counting pass of a score at `stride` gives the gate; qbar[a] =
 *     ((double)sum_a / (double)n_pass) * voxel_scale, pivot[a] = ((R0[a][0] qbar0 + R0[a][1] qbar1) + R0[a][2] qbar2) + T0[a]; n_pass == 0 gives status 2.
 *   Score: one tsl_tsdf_register_score over all candidates with c's gates and flags at `stride`.  J_k = e + F * n_far + U * (n_unknown + n_grad), all
 *     int64, F = rint((r_max * r_max) * 2^20), U = rint((miss * miss) * 2^20), the squares in f32 and r_max after its default; miss 0 = r_max: a voxel
 *     that lands on unknown space costs as much as the worst admissible residual, so poses that slide the source out of the destination never win.
 *     The overflow refusal of the registration holds with M = max(2 L g_max, g_max, r_max + band, miss): no J can overflow.
 *   Rank: a candidate is valid iff n_used >= min_used (0 = 6); best = the valid candidate of the least J, ties to the least k (integer comparison).
 *     No valid candidate: status 2, R_out / T_out = the guess, trk->iterations = 0, best = -1.
 *   Refine: tsl_tsdf_register_submap from (R_best, T_best) with t and c; rep->status is that run's status 0..3, R_out / T_out and trk (may be null)
 *     are that run's.  scores (may be null): the n_candidates scores.  rep->gate, rep->pivot, n_valid, J_best and score_best describe the search.
 * TSL_ERR_ARG (the text names the entry point): everything tsl_tsdf_register_linearize / tsl_tsdf_register_submap refuse, for every pose -- a
 * non-finite pose anywhere refuses the whole call before anything runs or is written (a search refuses a candidate that is not finite -- a finite
 * guess far enough out -- before any output is written; the counting pass for an automatic pivot has run by then); n outside 1 .. 65536; a null R / T / out (score), a null
 * guess / cfg / R_out / T_out / rep (search); a negative half-count, more than 65536 candidates, a non-finite step or pivot, a step <= 0 on an axis
 * with n > 0, a negative or non-finite miss, a negative min_used, a scoring stride that is not 1, 2, 4, 8 or 16. */
typedef struct { int64_t e; int32_t n_used, n_unknown, n_far, n_grad; } tsl_register_score;
typedef struct { int64_t n_gate, n_pass, sum_i, sum_j, sum_k; } tsl_register_gate;
typedef struct { int32_t n_t[3]; double step_t[3]; int32_t n_r[3]; double step_r[3]; double pivot[3]; int32_t flags; int32_t stride; float miss;
                 int32_t min_used; } tsl_search_cfg;
typedef struct { int32_t status, n_candidates, n_valid, best; int64_t J_best; tsl_register_score score_best; double pivot[3], R_best[9], T_best[3];
                 tsl_register_gate gate; } tsl_search_report;
int  tsl_tsdf_register_score(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double* R, const double* T, int32_t n,
                             const tsl_register_cfg* c, tsl_register_score* out, tsl_register_gate* gate);
int  tsl_tsdf_register_score_tile(tsl_tsdf* dst, int64_t entries, int32_t n);
int  tsl_tsdf_register_search(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R0[9], const double T0[3],
                              const tsl_register_cfg* c, const tsl_search_cfg* s, const tsl_track_cfg* t, double R_out[9], double T_out[3],
                              tsl_search_report* rep, tsl_track_report* trk, tsl_register_score* scores);

/* ---- exploration frontiers (tsl_frontier.hip): where the known map ends -- the free voxels that border unobserved space, grouped into connected
 * clusters, the targets of an exploration planner.  The reference tests a frontier per facelet inside its topology graph (topo_graph.py), which is out
 * of scope; this is the map pass behind it, defined by the project.  Everything is integer except one f32 comparison: the
 * result depends on no schedule and tests/frontier_ref.py restates it bit for bit.  The pass reads one submap slot, the one of tsl_tsdf_query_points
 * (the active submap; submap 0 on a global map), and writes nothing to the map.
 *   Classes.  A voxel (i, j, k) inside the volume is UNKNOWN when its brick is absent or its observed count is <= 0, OCCUPIED when it is observed and its
 *     f16 TSDF value, widened to f32, is < thres (the test of tsl_tsdf_query_points mode 0), FREE otherwise.  thres = free_thres, 0 = the map's surface
 *     threshold 1.8 * voxel.  A voxel outside the volume has no class -- it is not unknown: the wall of the volume is no frontier.
 *   Frontier voxel: a free voxel with at least min_unknown (1 .. 6, 0 = 1) of its six face neighbours unknown; with flags bit 0 none of its 26 neighbours
 *     occupied (keeps targets off the grazing-angle holes next to surfaces); with k_min <= k_max also k_min <= k <= k_max (signed voxel indices; k_min >
 *     k_max = no limit -- a zeroed cfg selects the layer k = 0).  mask: bit 0 .. 5 = the face neighbour at -x, +x, -y, +y, -z, +z is unknown.
 *   Key of a voxel: ((ui * N) + uj) * Nz + uk, ui = i + N / 2, uj = j + N / 2, uk = k + Nz / 2.  The call is refused when N * N * Nz >= 2^31.
 *   Clusters: the connected components of the frontier voxels under connectivity 6, 18 or 26 (0 = 26).  tsl_frontier_cluster (64 bytes): key = the least
 *     voxel key of the cluster, count, sum = the int64 sums of i, j, k (centroid = sum / count * voxel), nsum[a] = the voxels whose +a neighbour is
 *     unknown minus those whose -a neighbour is (the direction into the unknown), lo / hi = the bounding box.  Clusters with count < min_cluster (0 = 1)
 *     are dropped, and so are their voxels.
 *   Output: the voxels sorted by key -- idx int16 [n][3], mask u8 [n], cluster int32 [n] = the row of the voxel's cluster -- and the clusters sorted by key.
 * tsl_tsdf_frontier_extract issues the queued frames, runs on the handle's stream behind them, waits, and returns the two counts; the result stays on
 * the device (buffers that grow as needed: it is never truncated) until the next extraction.  tsl_tsdf_frontier_read copies the first n_voxels /
 * n_clusters rows of it to the host (null pointers are skipped).  tsl_tsdf_frontier_dev runs the same pass after the work queued on `user_stream` and
 * returns the device pointers of the result (null for an empty one; valid until the next extraction) and the counts; `user_stream` is made to wait for
 * the result as with tsl_tsdf_render_view_dev.  The host waits for the counts, as tsl_mesh_buffers_dev does: they size the buffers.
 * With profiling on, tsl_tsdf_prof_query returns the time of the stages: TSL_K_FRONTIER_MARK, _LABEL, _JOIN (join and flatten), _SUM (numbering the
 * roots, the sums, the filter) and _EMIT (the two sorts and the output).
 * TSL_ERR_ARG (the text names the entry point): a null handle / cfg, a free_thres that is not finite, a connectivity other than 0, 6, 18, 26, a
 * min_unknown outside 0 .. 6, a negative min_cluster, a volume with N * N * Nz >= 2^31; frontier_read: no extraction yet, a negative size, more rows
 * than the last extraction produced; frontier_dev: a null count pointer.  TSL_ERR_CAPACITY: an iteration cap of the labelling was reached.  The caps
 * are true bounds of a well-formed parent array (a find: the node count, frontier bricks * 4096; a union: as many retries), so no map of any size reaches
 * them; they only keep a kernel from spinning over corrupted memory.  A refused call leaves the handle usable. */
typedef struct { float free_thres; int32_t k_min, k_max, min_unknown, connectivity, min_cluster, flags; } tsl_frontier_cfg;
typedef struct { int32_t key, count; int64_t sum[3]; int32_t nsum[3]; int16_t lo[3], hi[3]; int32_t reserved_[2]; } tsl_frontier_cluster;
int  tsl_tsdf_frontier_extract(tsl_tsdf* m, const tsl_frontier_cfg* cfg, int32_t* n_voxels, int32_t* n_clusters);
int  tsl_tsdf_frontier_read(tsl_tsdf* m, int16_t* idx, uint8_t* mask, int32_t* cluster, tsl_frontier_cluster* clusters, int64_t n_voxels, int64_t n_clusters);
int  tsl_tsdf_frontier_dev(tsl_tsdf* m, const tsl_frontier_cfg* cfg, void** idx_dev, void** mask_dev, void** cluster_dev, void** clusters_dev,
                           int32_t* n_voxels, int32_t* n_clusters, void* user_stream);

/* ---- view gain (tsl_view_gain.hip): for each of n candidate camera poses, how much unobserved space a sensor there would see before its rays hit
 * something -- the figure a next-best-view planner ranks its candidates by.  One read-only launch for all poses; every output
 * is an integer, so the result depends on no schedule and tests/view_gain_ref.py restates it bit for bit.  All f32, in the written order, no contraction.
 *   Rays.  A view is a pinhole fan of h x w rays with intrinsics K; the pose R (row-major) / T is camera-to-map in the frame of tsl_tsdf_query_points
 *     (the active submap's; submap 0 on a global map), given as doubles and rounded to f32 once on the host.  Ray (u, v): dc = ((u - cx) / fx,
 *     (v - cy) / fy, 1), d = R dc (rows summed left to right, NOT normalised: the ray parameter is the optical-axis depth, as in tsl_tsdf_render_view).
 *     Samples n = 0 .. S-1, S = (int)((t_max - t_min) / dt) + 1, t_n = t_min + (float)n * dt, p_n = T + t_n * d, u_n = p_n / voxel.
 *   Class of a sample.  Its voxel is rnd(clamp(u_n)) per axis: clamp(x) = max(min(x, 2^24), -2^24) keeps the conversion inside an int (the clamp of
 *     the renderer's cell index), rnd is the project's round-half-away-from-zero, (int)(x + copysign(0.49999997f, x)).  The sample is OUTSIDE when a
 *     coordinate of p_n is not finite or the voxel is not in the volume; otherwise it has the class tsl_tsdf_frontier_extract gives that voxel:
 *     UNKNOWN (brick absent or observed count <= 0), OCCUPIED (observed and the f16 TSDF widened to f32 < thres), FREE.  thres = free_thres, 0 = the
 *     map's surface threshold (float)(voxel * 1.8).
 *   Walk.  An OUTSIDE sample counts nothing and changes no state (the space outside the volume is not unknown).  The first OCCUPIED sample ends the ray
 *     with status 0 (hit) and is not counted.  A FREE sample adds 1 to the ray's free count, w_n to its free weight, and sets the unknown run to 0.  An
 *     UNKNOWN sample adds 1 to the unknown count, w_n to the unknown weight and 1 to the run; with unknown_run > 0 the ray ends with status 2 (cut) once
 *     the run reaches unknown_run, the sample that reaches it counted (the pessimistic model: unknown space may hide a wall).  A ray that reaches S
 *     ends with status 1 (range).  A ray "looks through a frontier" when some UNKNOWN sample's previous non-OUTSIDE sample was FREE.
 *   Weight.  w_n = rnd((t_n * t_n) * 1024.0f).  The volume element of a ray at optical depth t is t^2 dt / (fx fy), so sum(w) / 1024 * dt / (fx * fy)
 *     is the volume in cubic metres the fan sees of that class -- the left Riemann sum is the definition.  t_max <= 1024 keeps w below 2^31.
 *   tsl_view_gain (64 bytes, one per pose): the sums over the pose's rays of the unknown / free counts and weights, the rays per status, and
 *     n_frontier, the rays that look through a frontier.  Optional per-ray outputs (both or neither): ray_unknown int32 [n][h][w], the ray's unknown
 *     count, and ray_status u8 [n][h][w], the status | 0x10 for a ray that looked through a frontier.
 *   tsl_gain_cfg: K, t_min, t_max, dt with the defaults of tsl_view_cfg (all-zero K = the map's depth intrinsics, 0 = the map's min / max_ray_length,
 *     dt 0 = 0.75 voxel); flags bit 0 evaluates every sample instead of jumping over the space outside the volume and over unallocated bricks: the same
 *     result bit for bit (the A/B switch).
 * tsl_tsdf_view_gain issues the queued frames, runs on the handle's stream behind them, waits and copies back.  tsl_tsdf_view_gain_dev is
 * ASYNCHRONOUS and ordered with `user_stream` like tsl_tsdf_render_view_dev; out_dev holds n records (as int32 [n][16]).  The call reads one submap slot
 * and writes nothing to the map or the ESDF.  With profiling on, tsl_tsdf_prof_query(m, TSL_K_VIEW_GAIN) returns the time of the kernel alone.
 * TSL_ERR_ARG (the text names the entry point): a null handle, pose array, cfg or out; n outside 0 .. 65536 (n = 0 does nothing: TSL_OK); a pose,
 * intrinsic, range or threshold that is not finite; h or w outside 1 .. 4096; t_max <= t_min; dt <= 0; t_max > 1024; more than 2^24 samples per ray;
 * unknown_run < 0; exactly one of the two per-ray buffers.  A refused call leaves the handle usable. */
typedef struct { double K[9]; int32_t h, w; float t_min, t_max, dt, free_thres; int32_t unknown_run, flags; } tsl_gain_cfg;
typedef struct { int64_t n_unknown, n_free, vol_unknown, vol_free; int32_t n_hit, n_range, n_cut, n_frontier; int32_t reserved_[4]; } tsl_view_gain;
int  tsl_tsdf_view_gain(tsl_tsdf* m, const double* R /* n x 9 */, const double* T /* n x 3 */, int32_t n, const tsl_gain_cfg* cfg, tsl_view_gain* out,
                        int32_t* ray_unknown, uint8_t* ray_status);
int  tsl_tsdf_view_gain_dev(tsl_tsdf* m, const double* R, const double* T, int32_t n, const tsl_gain_cfg* cfg, void* out_dev, void* ray_unknown_dev,
                            void* ray_status_dev, void* user_stream);

/* ---- navigation grids (tsl_nav_grid.hip): height bands of the TSDF projected into 2-D grids -- per band and (x, y) column a class, the squared planar
 * distance to the nearest obstacle column and a cost: the nav_msgs/OccupancyGrid and costmap layer a ground robot, or a drone that plans in altitude
 * layers, consumes.  The reference has no such pass.  Everything is integer except the one f32 comparison of the voxel
 * classes: the result depends on no schedule and tests/nav_grid_ref.py restates it bit for bit.  The pass reads one submap slot, the one of
 * tsl_tsdf_query_points (the active submap; submap 0 on a global map), and writes nothing to the map or the ESDF.
 *   Voxel classes: those of tsl_tsdf_frontier_extract -- UNKNOWN: the brick is absent or the observed count is <= 0; OCCUPIED: observed and the f16 TSDF,
 *     widened to f32, is < thres; FREE: every other observed voxel; thres = free_thres, 0 = the map's surface threshold.  ONE difference: an observed
 *     voxel whose TSDF is a NaN (it can only come in through tsl_tsdf_import_sparse) is UNKNOWN here, while the frontier pass calls it FREE: a navigation
 *     grid must not call such a voxel free.
 *   Bands: n_bands = B in 1 .. 16; band b is the voxel layers k_min[b] <= k <= k_max[b] (signed voxel indices, both ends inclusive), inside
 *     -Nz/2 .. Nz/2 - 1, k_min <= k_max.  Bands may overlap or be equal; the map is read once however many there are.
 *   Column counts: per band and column (i, j) of the N x N footprint, n_occ, n_free, n_unknown over the band's layers (they sum to its height), and
 *     lo / hi, the lowest / highest OCCUPIED layer k of the band (32767 / -32768 when there is none).
 *   Cell class (u8), tested in this order: TSL_NAV_OCCUPIED (1) when n_occ >= min_occ; TSL_NAV_FREE (0) when n_free >= min_free and (max_unknown < 0 or
 *     n_unknown <= max_unknown); TSL_NAV_UNKNOWN (2) otherwise.  min_occ / min_free 0 = 1.
 *   Distance: with ui = i + N/2, uj = j + N/2, the obstacles of a band are its OCCUPIED cells; with flags bit 0 its UNKNOWN cells too; with flags bit 1
 *     every position just outside the grid (ui or uj equal to -1 or N: the wall of the volume).  radius = R in 0 .. 254 voxels.  d2 (uint16) is the exact
 *     squared Euclidean distance in voxels to the nearest obstacle when that is <= R * R, and R * R + 1 otherwise; an obstacle cell has d2 = 0.
 *   Cost: lut is a u8 [R * R + 2] table of the caller's (the inflation formula lives in the table, not in the kernel); cost = cost_unknown for an
 *     UNKNOWN cell, else lut[d2].
 *   Layout: every plane is [B][N][N], indexed [b][ui][uj]; counts is uint16 [B][N][N][3] = { n_occ, n_free, n_unknown }, span int16 [B][N][N][2] = { lo, hi }.
 * Every output is nullable on its own (a plane that is not asked for is not computed where that is separable: without d2 and cost the distance
 * transform does not run); cost and lut come together or not at all.  tsl_tsdf_nav_grid issues the queued frames, runs on the handle's stream behind
 * them, waits and copies back.  tsl_tsdf_nav_grid_dev takes device pointers, is ASYNCHRONOUS and ordered with `user_stream` like
 * tsl_tsdf_render_view_dev.  Scratch on the handle grows as needed.  With profiling on, tsl_tsdf_prof_query returns the time of the stages:
 * TSL_K_NAV_PROJECT (the column reduction), TSL_K_NAV_EDT_ROWS (the distance pass along j) and TSL_K_NAV_EDT (the pass along i with the cost lookup).
 * TSL_ERR_ARG, before anything is launched or written (the text names the entry point): a null handle or cfg; every output null; n_bands outside
 * 1 .. 16; a band outside the volume or with k_min > k_max; a free_thres that is not finite; a negative min_occ or min_free; radius outside 0 .. 254;
 * flag bits other than 0 and 1; cost without lut or lut without cost; N * N * n_bands >= 2^31.  A refused call leaves the handle usable. */
#define TSL_NAV_FREE 0
#define TSL_NAV_OCCUPIED 1
#define TSL_NAV_UNKNOWN 2
typedef struct { int32_t n_bands, k_min[16], k_max[16]; float free_thres; int32_t min_occ, min_free, max_unknown, radius, flags;
                 uint8_t cost_unknown, reserved_[3]; } tsl_nav_cfg;
int  tsl_tsdf_nav_grid(tsl_tsdf* m, const tsl_nav_cfg* cfg, const uint8_t* lut, uint8_t* cls, uint16_t* d2, uint8_t* cost,
                       uint16_t* counts /* [B][N][N][3] */, int16_t* span /* [B][N][N][2] */);
int  tsl_tsdf_nav_grid_dev(tsl_tsdf* m, const tsl_nav_cfg* cfg, const void* lut_dev, void* cls_dev, void* d2_dev, void* cost_dev, void* counts_dev,
                           void* span_dev, void* user_stream);

/* ---- cost-to-go fields and paths over 2-D cost planes (tsl_nav_field.hip): how expensive it is to get from every cell to the
 * nearest goal, along which cells, and which cells reach no goal -- what a 2-D planner or an exploration loop asks once it holds a cost plane.  The
 * planes are the CALLER'S: u8 [B][H][W], 1 <= H, W <= 4096, 1 <= B <= 16, usually the `cost` output of tsl_tsdf_nav_grid, possibly cropped or with
 * obstacles painted in.  The handle supplies only the device, the stream and scratch (allocated by the first call); no map is read.  Everything is
 * integer and the answer is the one minimum of a sum of positive integers: it depends on no schedule, and tests/nav_field_ref.py restates it bit for bit.
 *   Traversable: cost < lethal; lethal in 1 .. 255 (253 keeps nav_grid's cost_unknown = 255 and an inflation table's 253 / 254 as walls).
 *   Moves: connectivity 4 or 8.  Direction codes 0 .. 7 are (di, dj) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1), i the row and j the column;
 *     odd codes exist only with connectivity 8, and a diagonal move is allowed only when both cells it passes between are traversable (no corner
 *     cutting).  Step length s = 5 for an axis move, 7 for a diagonal one.
 *   Seeds: int32 [S][4] = { plane, row, col, value }, 0 <= S <= 65536, value read as uint32 (2^32 - 1 counts as 2^32 - 2).  A seed outside the planes or
 *     on a cell that is not traversable is ignored and counted in n_bad_seeds; of several seeds on one cell the least value counts; planes are
 *     independent problems.  S = 0 is no error: everything is unreached.
 *   field (uint32 [B][H][W]): the minimum over all move sequences x = c0, c1, .., cm = a seed cell through traversable cells of
 *     value(seed) + sum over t < m of s(c_t -> c_t+1) * (neutral + cost[c_t]), clipped to 2^32 - 2; TSL_NAV_UNREACHED = 2^32 - 1 where no seed is
 *     reached (walls included).  neutral in 1 .. 255.
 *   parent (u8 [B][H][W], nullable; a pass of its own after the rounds): 255 for an unreached cell; 8 for a cell whose field equals a seed value placed
 *     on it; otherwise the lowest direction code d whose move is allowed and whose neighbour n satisfies
 *     min(field[n] + s_d * (neutral + cost[x]), 2^32 - 2) == field[x].  (Only a field that did not converge has reached cells that no neighbour
 *     explains; they get 255.)
 *   Rounds: one round is one launch; a 32 x 32 tile that is marked active relaxes in LDS against a one-cell halo, writes its own cells back and marks
 *     the neighbours whose halo changed for the next round.  No workgroup waits for another and every loop in a kernel has a bound known at launch.
 *     The host ends the rounds: every check_every rounds (0 = 8) it reads 4 bytes, the marks the last round made, and stops after a round that
 *     marked nothing or at max_rounds (0 = 4 * tiles of a plane + 64).  Not converged is converged = 0 WITH TSL_OK -- the field then holds upper
 *     bounds, each the cost of a real move sequence -- and never a wait.  With rounds_fixed > 0 exactly that many rounds are enqueued and nothing is
 *     read; rounds_fixed = the `rounds` of an earlier call on the same input ends on converged = 1 (field and parent depend on no schedule; the
 *     round count can: a halo read that meets a neighbour's write-back saves work, so where not all tiles of a round run at once read converged).
 *   Statistics: converged; rounds = the last round that visited a tile, counted from 1; tile_visits; n_bad_seeds.
 * tsl_tsdf_nav_field takes host pointers, issues the queued frames, runs on the handle's stream, waits and copies back.  tsl_tsdf_nav_field_dev takes
 * device pointers (stats_dev: a tsl_nav_field_stats in device memory, nullable) and is ordered with `user_stream` like tsl_tsdf_nav_grid_dev: with
 * rounds_fixed > 0 it is ASYNCHRONOUS; with rounds_fixed = 0 it SYNCHRONISES the handle's stream at each check, and so waits for the work of
 * `user_stream` queued before it.
 *   Paths (tsl_tsdf_nav_field_paths / _dev; cfg gives B, H, W): starts int32 [P][3] = { plane, row, col }, 0 <= P <= 2^20, P * L <= 2^28.  One lane per
 *     start follows `parent` for at most L = max_len cells.  cells int16 [P][L][2] = (row, col) from the start on, rows past the end -1; length int32
 *     [P]; status u8 [P]: 0 = ended on a seed, 1 = truncated at L, 2 = the start is unreached or not traversable (or the parents lead nowhere: a plane
 *     that is not of this field), 3 = the start is outside; cost uint32 [P] = the field at the start (TSL_NAV_UNREACHED for status 3).  Every output
 *     is nullable.  The _dev form is asynchronous.
 * With profiling on, tsl_tsdf_prof_query returns the time of TSL_K_NAV_FIELD_SEED, TSL_K_NAV_FIELD_ROUND (every round of the calls), TSL_K_NAV_FIELD_PARENT
 * and TSL_K_NAV_FIELD_PATHS.
 * TSL_ERR_ARG, before anything is launched or written (the text names the entry point): a null handle, cfg, cost or field (paths: field or parent); B
 * outside 1 .. 16, H or W outside 1 .. 4096, S outside 0 .. 65536; neutral or lethal outside 1 .. 255; a connectivity other than 4 and 8; seeds null
 * while S > 0 (starts while P > 0); max_len < 1; a negative max_rounds, rounds_fixed or check_every.  A refused call leaves the handle usable. */
#define TSL_NAV_UNREACHED 0xffffffffu
typedef struct { int32_t B, H, W, neutral, lethal, connectivity, max_rounds, rounds_fixed, check_every, reserved_; } tsl_nav_field_cfg;
typedef struct { int32_t converged, rounds; int64_t tile_visits; int32_t n_bad_seeds, reserved_; } tsl_nav_field_stats;
int  tsl_tsdf_nav_field(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const uint8_t* cost, const int32_t* seeds /* [S][4] */, int32_t n_seeds, uint32_t* field,
                        uint8_t* parent, tsl_nav_field_stats* stats);
int  tsl_tsdf_nav_field_dev(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const void* cost_dev, const void* seeds_dev, int32_t n_seeds, void* field_dev,
                            void* parent_dev, void* stats_dev, void* user_stream);
int  tsl_tsdf_nav_field_paths(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const uint32_t* field, const uint8_t* parent, const int32_t* starts /* [P][3] */,
                              int32_t n_starts, int32_t max_len, int16_t* cells /* [P][L][2] */, int32_t* length, uint8_t* status, uint32_t* cost);
int  tsl_tsdf_nav_field_paths_dev(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const void* field_dev, const void* parent_dev, const void* starts_dev,
                                  int32_t n_starts, int32_t max_len, void* cells_dev, void* length_dev, void* status_dev, void* cost_dev, void* user_stream);

/* ---- cost-to-go fields and paths over 3-D cost volumes (tsl_nav_field3.hip): tsl_tsdf_nav_field carried into 3-D for platforms
 * that fly -- how expensive it is to get from every cell of a volume to the nearest goal, along which cells, and which cells reach no goal, where the
 * way may climb over a wall or drop through a stairwell.  The volume is the CALLER'S: u8 [D][H][W], indexed as layer k (z), row i (x) and column j (y) --
 * the row and column of tsl_tsdf_nav_grid's planes with the layer in front -- 1 <= D, H, W <= 1024 and D * H * W <= 2^27; usually the ESDF sampled at a
 * stride of a few voxels (DenseTSDF.flight_volume).  The handle supplies only the device, the stream and scratch (allocated by the first call, released
 * with the handle); no map is read.  Everything is integer and the answer is the one minimum of a sum of positive integers: it depends on no schedule,
 * and tests/nav_field3d_ref.py restates it bit for bit.
 *   Traversable: cost < lethal; lethal in 1 .. 255.  neutral in 1 .. 255.
 *   Moves: connectivity 6, 18 or 26.  Direction codes 0 .. 25 are (dk, di, dj): codes 0 .. 7 have dk = 0 and the (di, dj) of tsl_tsdf_nav_field's codes
 *     0 .. 7, in that order; code 8 = (1, 0, 0) and codes 9 .. 16 = (1, the same eight (di, dj)); code 17 = (-1, 0, 0) and codes 18 .. 25 = (-1, the same
 *     eight).  Connectivity 6 has the six codes with one non-zero component, 18 adds those with two, 26 has all.  Step length s = 5, 7 or 9 for one, two
 *     or three non-zero components (the <5, 7, 9> chamfer: a volume with D = 1 is tsl_tsdf_nav_field's problem).  No corner cutting: a move from x by
 *     (dk, di, dj) is allowed only when EVERY cell x + (a dk, b di, c dj) with a, b, c in {0, 1} is inside the volume and traversable -- the two other
 *     cells of the square for a face diagonal, the six other cells of the cube for a space diagonal.
 *   Seeds: int32 [S][4] = { layer, row, col, value }, 0 <= S <= 65536, value read as uint32 (2^32 - 1 counts as 2^32 - 2).  A seed outside the volume or
 *     on a cell that is not traversable is ignored and counted in n_bad_seeds; of several seeds on one cell the least value counts.  S = 0 is no error:
 *     everything is unreached.
 *   field (uint32 [D][H][W]): the minimum over all move sequences x = c0, c1, .., cm = a seed cell through traversable cells of
 *     value(seed) + sum over t < m of s(c_t -> c_t+1) * (neutral + cost[c_t]) -- the cell that is left pays -- clipped to 2^32 - 2; TSL_NAV_UNREACHED where
 *     no seed is reached (walls included).
 *   parent (u8 [D][H][W], nullable; a pass of its own after the rounds): 255 for an unreached cell; TSL_NAV3_SEED = 26 for a cell whose field equals a
 *     seed value placed on it; otherwise the lowest direction code d whose move is allowed and whose neighbour n satisfies
 *     min(field[n] + s_d * (neutral + cost[x]), 2^32 - 2) == field[x].  (Only a field that did not converge has reached cells that no neighbour
 *     explains; they get 255.)
 *   Rounds: one round is one launch; a tile (16 x 8 x 8 cells in j, i, k) that is marked active relaxes in LDS against a one-cell halo, writes its own
 *     cells back and marks the neighbours whose halo changed for the next round.  No workgroup waits for another and every loop in a kernel has a bound
 *     known at launch.  The host ends the rounds: every check_every rounds (0 = 8) it reads 4 bytes, the marks the last round made, and stops after a
 *     round that marked nothing or at max_rounds (0 = min(4 * tiles of the volume + 64, 65536)).  Not converged is converged = 0 WITH TSL_OK -- the
 *     field then holds upper bounds, each the cost of a real move sequence -- and never a wait.  With rounds_fixed > 0 exactly that many rounds are
 *     enqueued and nothing is read; rounds_fixed = the `rounds` of an earlier call on the same input ends on converged = 1 (field and parent depend on no
 *     schedule; the round count can: a halo read that meets a neighbour's write-back saves work, so where not all tiles of a round run at once read
 *     converged).
 *   Statistics: converged; rounds = the last round that visited a tile, counted from 1; tile_visits; n_bad_seeds.
 * tsl_tsdf_nav_field3 takes host pointers, runs on the handle's stream, waits and copies back.  tsl_tsdf_nav_field3_dev takes device pointers (stats_dev:
 * a tsl_nav_field3_stats in device memory, nullable) and is ordered with `user_stream` like tsl_tsdf_nav_field_dev: with rounds_fixed > 0 it is
 * ASYNCHRONOUS; with rounds_fixed = 0 it SYNCHRONISES the handle's stream at each check, and so waits for the work of `user_stream` queued before it.
 *   Paths (tsl_tsdf_nav_field3_paths / _dev; cfg gives D, H, W): starts int32 [P][3] = { layer, row, col }, 0 <= P <= 2^20, P * L <= 2^28.  One lane per
 *     start follows `parent` for at most L = max_len cells.  cells int16 [P][L][3] = (layer, row, col) from the start on, rows past the end -1; length
 *     int32 [P]; status u8 [P]: 0 = ended on a seed, 1 = truncated at L, 2 = the start is unreached or not traversable (or the parents lead nowhere: a
 *     volume that is not of this field), 3 = the start is outside; cost uint32 [P] = the field at the start (TSL_NAV_UNREACHED for status 3).  Every
 *     output is nullable.  The _dev form is asynchronous.
 * These kernels have no tsl_tsdf_prof_query id; time them with events around the _dev call with rounds_fixed set (tools/bench_nav_field3d.py).
 * TSL_ERR_ARG, before anything is launched or written (the text names the entry point): a null handle, cfg, cost or field (paths: field or parent); D, H
 * or W outside 1 .. 1024 or more than 2^27 cells; S outside 0 .. 65536 (P outside 0 .. 2^20, P * L above 2^28); neutral or lethal outside 1 .. 255; a
 * connectivity other than 6, 18 and 26; seeds null while S > 0 (starts while P > 0); max_len < 1; a negative max_rounds, rounds_fixed or check_every.  A
 * refused call leaves the handle usable. */
#define TSL_NAV3_SEED 26
typedef struct { int32_t D, H, W, neutral, lethal, connectivity, max_rounds, rounds_fixed, check_every, reserved_; } tsl_nav_field3_cfg;
typedef struct { int32_t converged, rounds; int64_t tile_visits; int32_t n_bad_seeds, reserved_; } tsl_nav_field3_stats;
int  tsl_tsdf_nav_field3(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const uint8_t* cost, const int32_t* seeds /* [S][4] */, int32_t n_seeds, uint32_t* field,
                         uint8_t* parent, tsl_nav_field3_stats* stats);
int  tsl_tsdf_nav_field3_dev(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const void* cost_dev, const void* seeds_dev, int32_t n_seeds, void* field_dev,
                             void* parent_dev, void* stats_dev, void* user_stream);
int  tsl_tsdf_nav_field3_paths(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const uint32_t* field, const uint8_t* parent, const int32_t* starts /* [P][3] */,
                               int32_t n_starts, int32_t max_len, int16_t* cells /* [P][L][3] */, int32_t* length, uint8_t* status, uint32_t* cost);
int  tsl_tsdf_nav_field3_paths_dev(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const void* field_dev, const void* parent_dev, const void* starts_dev,
                                   int32_t n_starts, int32_t max_len, void* cells_dev, void* length_dev, void* status_dev, void* cost_dev, void* user_stream);

/* ---- safe corridors: free boxes around cells and along paths (tsl_nav_corridor.hip): the step between a path of
 * tsl_tsdf_nav_field_paths / tsl_tsdf_nav_field3_paths -- a staircase of cells that hugs obstacles -- and a corridor-based trajectory optimiser, which asks
 * for a short sequence of overlapping convex free regions that contains the path.  The region is the axis-aligned box inflated around a cell until a face
 * meets an obstacle.  The volume is the CALLER'S; the handle supplies only the device, the stream and scratch (allocated by the first call, released with
 * the handle); no map is read.  Everything is integer and the face order makes the answer unique: tests/nav_corridor_ref.py restates it byte for byte.
 *   Volume: cost u8 [D][H][W]: layer k, row i, column j, the axes of tsl_tsdf_nav_field3; 1 <= D, H, W <= 4096 and D * H * W <= 2^28 (the 16 planes of 4096 x
 *     4096 of tsl_tsdf_nav_field: D is then the number of planes).  A cell is free when it is inside and cost < free_below, free_below in 1 .. 255: the
 *     `lethal` of the field, or less, to keep a margin.
 *   Extents: ext_k, ext_i, ext_j, each in 0 .. 127: the most a box may reach from its seed along that axis, in cells.  ext_k = 0 makes the layers
 *     independent planes: the 2-D case.
 *   Box of a seed cell c: c outside the volume: six times -1 and the flag TSL_BOX_OUTSIDE.  c not free: lo = hi = c and TSL_BOX_BLOCKED.  Otherwise the
 *     box starts as lo = hi = c with all six faces open and grows in rounds.  In a round the open faces are tried in the fixed order -j, +j, -i, +i, -k, +k.
 *     A try moves that face out by one cell; it succeeds when the new coordinate is within ext of c on that axis, it is inside the volume, and every cell
 *     of the new slab is free -- the slab is one cell thick and spans the box as it stands at that moment on the other two axes, including what earlier
 *     tries of the same round added.  A try that fails closes the face for good (the slab only ever gets wider).  Rounds repeat until no face is open: at
 *     most 6 * (max ext + 1) tries.  The result is a free box that contains c and that no single face move can enlarge within ext; flag 0.
 *   boxes int16 [S][6] = (k0, i0, j0, k1, i1, j1), both ends inclusive; flags u8 [S].  cells int32 [S][3] = (layer, row, col), 0 <= S <= 2^20; max_boxes is
 *     not read by tsl_tsdf_nav_boxes / _dev.
 *   Corridor of a path (tsl_tsdf_nav_corridor / _dev): cells int16 [P][L][3] = (layer, row, col), the `cells` of tsl_tsdf_nav_field3_paths (those of
 *     tsl_tsdf_nav_field_paths with the plane in front); a path is the cells 0 .. len - 1 of its row, len = min(length[p], L).  0 <= P <= 2^16, 1 <= L <=
 *     4096, P * L <= 2^22, max_boxes = Q in 1 .. L.  With B(s) the box of cell s: s_0 = 0; given s_q, B(s_q) is emitted with its seed index s_q; t_q is the
 *     largest t >= s_q such that the cells s_q .. t all lie in B(s_q), and t_q = s_q when the seed is blocked or outside; t_q = len - 1 completes the
 *     corridor: status 0; otherwise s_q+1 = t_q if t_q > s_q, else s_q + 1 (the seed index strictly increases); Q boxes without completing: status 1; len
 *     <= 0: status 2 and no box.
 *   boxes int16 [P][Q][6]; seed int32 [P][Q]; count int32 [P]; status u8 [P]; link u8 [P][Q]: 0 for a path's first box, 1 when the box shares at least one
 *     cell with the box before it, 2 when it shares none (the box of a seed outside the volume has no cells), plus 4 when its seed is blocked or outside.
 *     Rows past count: boxes and seed -1, link 255.  Link 2 happens -- t_q = s_q and the boxes of two adjacent path cells only touch: a diagonal move
 *     between two cells whose boxes each stop at the other's row, or an axis move whose first slab had already been widened by an earlier face and so held
 *     an obstacle.  The flag is the honest answer; a consumer that needs overlap splits there.
 *   Kernels: the volume is packed into one free bit per cell (row pitch ceil(W / 64) words, 64-bit ballots: D * H * ceil(W / 64) * 8 bytes of scratch, an
 *     eighth of the volume where W is a multiple of 64 and at worst, for W = 1, 8 bytes per cell -- 128 MB); one wave per seed inflates on bits -- the
 *     corridor forms inflate EVERY cell of every path, P * L independent waves -- and one wave per path chains.  No atomics, no workgroup waits for
 *     another, every loop has a bound known at launch.
 * The host forms take host pointers, run on the handle's stream, wait and copy back.  The _dev forms take device pointers, are ordered with `user_stream`
 * like tsl_tsdf_nav_field3_paths_dev and are ASYNCHRONOUS -- except that a call which has to allocate or grow the handle's scratch (the first call, and any
 * call with a larger volume or more path cells than those before it) frees and allocates device memory and so waits for the device.  Every output is nullable.  S = 0 and P = 0 are no error.  These kernels have no
 * tsl_tsdf_prof_query id; time them with events around the _dev calls (tools/bench_nav_corridor.py).
 * TSL_ERR_ARG, before anything is launched or written (the text names the entry point): a null handle, cfg or cost; D, H or W outside 1 .. 4096 or more than
 * 2^28 cells; free_below outside 1 .. 255; an ext outside 0 .. 127; S outside 0 .. 2^20; P outside 0 .. 2^16, L outside 1 .. 4096, P * L above 2^22; max_boxes
 * outside 1 .. L (corridor forms); cells null while S or P > 0; length null while P > 0.  A refused call leaves the handle usable. */
#define TSL_BOX_BLOCKED 1
#define TSL_BOX_OUTSIDE 2
typedef struct { int32_t D, H, W, free_below, ext_k, ext_i, ext_j, max_boxes; } tsl_nav_corridor_cfg;
int  tsl_tsdf_nav_boxes(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const uint8_t* cost, const int32_t* cells /* [S][3] */, int32_t n, int16_t* boxes /* [S][6] */,
                        uint8_t* flags);
int  tsl_tsdf_nav_boxes_dev(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const void* cost_dev, const void* cells_dev, int32_t n, void* boxes_dev, void* flags_dev,
                            void* user_stream);
int  tsl_tsdf_nav_corridor(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const uint8_t* cost, const int16_t* cells /* [P][L][3] */, const int32_t* length, int32_t P,
                           int32_t L, int16_t* boxes, int32_t* seed, uint8_t* link, int32_t* count, uint8_t* status);
int  tsl_tsdf_nav_corridor_dev(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const void* cost_dev, const void* cells_dev, const void* length_dev, int32_t P, int32_t L,
                               void* boxes_dev, void* seed_dev, void* link_dev, void* count_dev, void* status_dev, void* user_stream);

/* ---- free-space topology graph (tsl_topo.hip): the ray and facelet work of TopoGraphGen (taichi_slam/mapping/topo_graph.py).  A
 * tsl_topo is bound to one tsl_tsdf, reads it and never writes it, and owns two device stores that grow on demand: the facelets (structure of arrays: the three
 * vertices, v0, edge1, edge2, normal, centre, poly = the node that made it; at most max_facelets) and the nodes (centre, facelet range; at most 4096, the
 * reference's max_map_node).  The hull (scipy's Qhull), the region growing, the frontiers and the loop stay with the caller (mapping/topo_graph.py).
 *
 * DEFINITION.  The reference's top-level loops are parallel, so its black-list order, its centre sum and its neighbour list are whatever the atomics gave
 * (and neighbor_node_ids, coll_det_num slots for up to 2 * coll_det_num - 4 facelets, can overflow).  This back end defines the SEQUENTIAL reading: every loop
 * of topo_graph.py in ascending index order, all arithmetic f32 in the order the source writes it, no contraction, correctly rounded divide and sqrt.
 *   normalising   v.normalized() = v / sqrt(x * x + y * y + z * z): the sum left to right, the division per component.  cross(a, b) = (a1 b2 - a2 b1,
 *                 a2 b0 - a0 b2, a0 b1 - a1 b0), dot(a, b) = (a0 b0 + a1 b1) + a2 b2.
 *   facelet       (:36-50) edge1 = v1 - v0, edge2 = v2 - v0, centre = ((v0 + v1) + v2) / 3, normal = cross(edge1, edge2).normalized(), negated when its dot with
 *                 (((v0 + v1) + v2) - 3 * start).normalized() is < 0.
 *   ray/triangle  (:52-70) as written; |a| > 1e-5f or no hit; b2 = (1 - b0) - b1.  A NaN t fails every comparison and never wins.
 *   collision     (:472-488) over the nodes k != skip_idx with norm(pos - centre_k) < max_dist + max_raycast_dist (one f32 add) the least t with
 *                 backward < t < max_dist; among equal t the lowest facelet index (what the sequential strict `<` keeps).  Without a hit t = max_dist and
 *                 poly = -1.  The position is pos + dir * t.
 *   combined ray  (:490-507) the collision with backward = -0.01f, then the map walk of tsl_tsdf_query_raycast to max_dist -- to the facelet hit's t if there
 *                 was one; (int)(t / voxel) steps, none for a t below one voxel -- bit for bit, its rule for positions that are not finite or have no int
 *                 cell and its len and end_xyz on a miss included.  The map wins (type 0) only without a facelet hit or when it hit and len_map < t,
 *                 strictly; otherwise type 1.  poly is the facelet hit's node even when the map wins.  A NaN component of a position leaves as 0x7fc00000.
 *   collide       (:444-470) rays 0 .. coll_det_num - 1 from one start, blacks (hits) and whites compacted in ray order, node_size = the left-to-right f32 sum
 *                 of the black lengths / their count; succ = !(no black || (no white && node_size < thres_size)).
 *   add_poly      (:380-405) facelets in ascending order into the store, poly = the new node's index; per facelet (:324-342; is_near_pos_occupy(centre, 0)
 *                 has an empty loop and is false) reason 1: is_pos_unobserved(centre), else 2: is_pos_occupy(centre + normal * voxel), else 3: the combined ray
 *                 from there along the normal to max_dist hit; is_frontier = reason 0; neigh = that ray's poly when it hit with type 1, else -1.  The rays see
 *                 the nodes made before this one.  The node centre is the left-to-right f32 sum of (v0 + v1) + v2 over the facelets, divided by 3 * nf.
 * TSL_ERR_ARG, before anything is launched or written (the text names the entry point): a null handle or argument; coll_det_num outside 4 .. 512 (the
 * reference's region queue holds 1024 facelets); max_facelets outside 1 .. 2^24; a max_dist or max_raycast_dist that is negative, not finite or above 2^20
 * voxels; a NaN backward; n outside 0 .. 2^20; nf outside 1 .. 4096; a flag other than bit 0; a handle whose map was destroyed (tsl_topo_destroy is still
 * fine).  TSL_ERR_CAPACITY, with nothing changed: the facelet store would pass max_facelets, or 4096 nodes exist. */
typedef struct tsl_topo tsl_topo;
int  tsl_topo_create(tsl_tsdf* m, int32_t coll_det_num, float max_raycast_dist, int64_t max_facelets, tsl_topo** out);
void tsl_topo_destroy(tsl_topo* t);
int  tsl_topo_reset(tsl_topo* t);                       /* both stores empty; their memory stays */
int  tsl_topo_counts(tsl_topo* t, int64_t* n_facelets, int32_t* n_nodes);
/* n rays: flags bit 0 = facelets only (the collision alone, type 1; verify_frontier's second cast); skip_idx int32 [n] or NULL = -1.  Outputs (any may be NULL):
 * hit u8, type u8 (0 map, 1 facelet), end_xyz f32 [n][3], len f32, poly int32. */
int  tsl_topo_rays(tsl_topo* t, const float* pos, const float* dir, const int32_t* skip_idx, int64_t n, float max_dist, float backward, int32_t flags, uint8_t* hit,
                   uint8_t* type, float* end_xyz, float* len, int32_t* poly);
/* the same with DEVICE buffers (no output may be NULL), ordered with `user_stream` like tsl_tsdf_query_raycast_dev; nothing is waited for */
int  tsl_topo_rays_dev(tsl_topo* t, const void* pos_dev, const void* dir_dev, const void* skip_idx_dev, int64_t n, float max_dist, float backward, int32_t flags,
                       void* hit_dev, void* type_dev, void* end_xyz_dev, void* len_dev, void* poly_dev, void* user_stream);
/* the coll_det_num rays of one expansion: start f32 [3], dirs f32 [coll_det_num][3]; black_pos / black_dir f32 [coll_det_num][3], black_len f32 [coll_det_num],
 * white_pos likewise (may be NULL, as white_num and node_size) */
int  tsl_topo_collide(tsl_topo* t, const float* start, const float* dirs, float thres_size, int32_t* succ, int32_t* black_num, float* black_pos, float* black_dir,
                      float* black_len, int32_t* white_num, float* white_pos, float* node_size);
/* one node from nf triangles f32 [nf][3][3]; outputs (any may be NULL): is_frontier u8 [nf], reason u8 [nf], neigh int32 [nf], centre f32 [3], the node's index */
int  tsl_topo_add_poly(tsl_topo* t, const float* tris, int32_t nf, const float* start, float max_dist, uint8_t* is_frontier, uint8_t* reason, int32_t* neigh,
                       float* centre, int32_t* node_idx);
/* DEVICE pointers of the store (tri_vertices f32 [.][3][3], normal and centre f32 [.][3], poly int32) and the counts; the pointers change when the store grows */
int  tsl_topo_buffers_dev(tsl_topo* t, void** tri_vertices_dev, void** normal_dev, void** centre_dev, void** poly_dev, int64_t* n_facelets, int32_t* n_nodes);
/* facelets first .. first + n - 1 of the store to host arrays (any may be NULL) */
int  tsl_topo_read_facelets(tsl_topo* t, int64_t first, int64_t n, float* tri_vertices, float* v0, float* edge1, float* edge2, float* normal, float* centre,
                            int32_t* poly);

/* ---- depth conditioning (tsl_depth.hip): a batch of uint16 millimetre frames, as the sensor delivers them, loses its flying pixels
 * and speckle, has the pixels it keeps smoothed by an integer bilateral filter, and is halved into up to three coarser levels -- one launch for the batch
 * and one per level.  Every integrating and tracking entry point takes raw depth at face value; this pass is what a caller with a real camera puts in
 * front of them.  The handle is its own type: it owns the tables and knows no map, touches none and issues nobody's queued frames.  Everything is integer, so
 * the answer depends on no schedule; tests/depth_condition_ref.py restates it byte for byte.
 *
 * DEFINITION.  depth u16 [n][h][w] in millimetres, 1 <= n <= 64, 1 <= h, w <= 8192, n h w <= 2^28.
 *   Tables (tsl_depth_set_tables): tol u16 [256], every entry in 1 .. 32767: the tolerance of a pixel of depth d is t(d) = tol[d >> 8] mm; ws u8 [5][5], the
 *     spatial weight by (|dy|, |dx|); wr u8 [17], the range weight by q; ws[0][0] * wr[0] > 0.  The library derives rq[b] = min(65535, (16 << 16) / tol[b]).
 *   Status, exactly one per pixel, the rules tested in this order; a pixel outside the image never counts as anything:
 *     1 HOLE    d == 0
 *     2 RANGE   d < d_min_mm or d > d_max_mm.  A pixel that is neither HOLE nor RANGE is a CANDIDATE.
 *     3 SPARSE  fewer than min_support of the 8 neighbours are candidates q with |d_q - d| <= t(d) (the centre's tolerance)
 *     4 EDGE    a seed lies within Chebyshev distance `erode`.  Seeds: the SPARSE pixels, and the HOLE pixels when flags bit 0 is set.  RANGE pixels and the
 *               image border are no seeds.
 *     0 KEPT    everything else
 *   Output: a pixel that is not KEPT gives 0.  For a KEPT pixel p the members are the KEPT pixels q of the (2 radius + 1)^2 window with a = |d_q - d_p| <=
 *     t(d_p); qi = (a * rq[d_p >> 8]) >> 16 (at most 16; the product fits 32 bits); wgt = ws[|dy|][|dx|] * wr[qi]; num = sum wgt * (d_q - d_p), den = sum wgt
 *     (> 0: the centre is a member); off = floor((2 num + den) / (2 den)); out = clamp(d_p + off, 1, 65535).  radius 0: out = d_p.
 *   counts int64 [n][5]: the pixels per status and frame; zeroed by the call.
 *   Levels: level 0 is the output; level l + 1 has h' = h / 2, w' = w / 2 (an odd last row or column is dropped).  Of the four source pixels the non-zero
 *     ones are valid; fewer than min_valid of them give 0; otherwise ref = the smallest valid depth (the foreground wins), the members are the valid pixels
 *     with d - ref <= t(ref), m their number, out = floor((2 * sum of the members + m) / (2 m)).
 * cfg: n, h, w; d_min_mm <= d_max_mm; min_support 0 .. 8; erode 0 .. 3; radius 0 .. 4; flags bit 0 = holes are seeds; levels 0 .. 3; min_valid 1 .. 4.
 * tsl_depth_condition takes HOST pointers: it stages, runs on a stream of the handle and waits.  status, counts and the level pointers may be NULL; a level
 *   above cfg->levels is ignored; a level left out below one that is given is computed in a buffer of the handle.
 * tsl_depth_condition_dev takes DEVICE pointers and runs on `user_stream` itself, asynchronously: the result is ordered with whatever the caller queues there
 *   next, an integration of `out` included.  One handle serves one stream at a time.  depth, out and the levels must be 2-byte aligned, counts 8-byte.
 * Output and input must not overlap (equal pointers are refused).
 * TSL_ERR_ARG (the text names the entry point), before anything is launched or written: a null handle, cfg, depth or out; tables not set or out of range; a
 * configuration outside the ranges above; a level asked for that has no pixels (h >> levels or w >> levels is 0); an output that overlaps the input. */
typedef struct tsl_depth tsl_depth;
typedef struct {
    int32_t n, h, w;
    int32_t d_min_mm, d_max_mm, min_support, erode, radius, flags, levels, min_valid, reserved_;
} tsl_depth_cfg;
#define TSL_DEPTH_KEPT 0
#define TSL_DEPTH_HOLE 1
#define TSL_DEPTH_RANGE 2
#define TSL_DEPTH_SPARSE 3
#define TSL_DEPTH_EDGE 4
int  tsl_depth_create(int device, tsl_depth** out);
void tsl_depth_destroy(tsl_depth* t);
/* copies the tables to the device and waits; TSL_ERR_ARG and nothing changed when an entry is out of range */
int  tsl_depth_set_tables(tsl_depth* t, const uint16_t* tol /* [256] */, const uint8_t* ws /* [5][5] */, const uint8_t* wr /* [17] */);
int  tsl_depth_condition(tsl_depth* t, const tsl_depth_cfg* cfg, const uint16_t* depth, uint16_t* out, uint8_t* status, int64_t* counts, uint16_t* lvl1,
                         uint16_t* lvl2, uint16_t* lvl3);
int  tsl_depth_condition_dev(tsl_depth* t, const tsl_depth_cfg* cfg, const void* depth_dev, void* out_dev, void* status_dev, void* counts_dev, void* lvl1_dev,
                             void* lvl2_dev, void* lvl3_dev, void* user_stream);

/* ---- pose graph (tsl_pose_graph.hip): the poses of submaps under relative-pose constraints, solved once per VARIANT in one launch.
 * A variant is a bit mask over the edges (bit e & 63 of word e >> 6: edge e takes part); one workgroup of 256 threads runs the whole Levenberg-Marquardt
 * loop of one variant in float64, with no atomic and no library call on the device.  Every sum below has a fixed order, so a result is one defined answer:
 * tests/pose_graph_ref.py restates this text in numpy and the tests compare bit for bit.  The handle needs no map.
 *   Conventions.  A pose P_i = (R_i, T_i) takes submap coordinates to the common frame (what tsl_tsdf_set_base_pose_submap takes).  An edge (a, b, Z = (Rz,
 *   Tz), L) says that P_b^-1 P_a was measured as Z -- what tsl_tsdf_register_submap returns for source a and destination b -- with the information matrix L
 *   in twist order (v, omega), the left twist in b's frame.  A twist xi = (v, omega) acts as tsl_pose_retract does (the Cayley map): R <- C R, T <- C T + v.
 *   "dot3" and "dot6" below are sums of products added left to right: (a0 b0 + a1 b1) + a2 b2, and so on to six terms.
 *   Residual of an edge: Rx = R_b^T R_a, Tx = R_b^T (T_a - T_b), R_D = Rx Rz^T, T_D = Tx - R_D Tz (every entry a dot3 over the summed index 0, 1, 2),
 *   den = 1 + ((R_D00 + R_D11) + R_D22), r = (T_D, (2 * vee(R_D - R_D^T)) / den) with vee = (R_D21 - R_D12, R_D02 - R_D20, R_D10 - R_D01): the twist whose
 *   retraction from the identity is the error D.  An edge with den < 1 (a rotation error above 120 degrees) is FLIPPED.
 *   Cost of an edge: c = dot6(r, L r), each row of L r a dot6.  chi = sqrt(c); with huber > 0 and chi > huber the weight is wgt = huber / chi and the edge
 *   counts (2 huber) chi - huber huber in the cost, otherwise wgt = 1 and it counts c.  Lw = wgt * L entry by entry.
 *   Linearisation, every pose moved by a left twist in the common frame: with Ri = R_b^T and ti = -(R_b^T T_b), A d = (Ri v + ti x (Ri w), Ri w) for d = (v,
 *   w) and A^T m = (R_b m_v, R_b (m_w - ti x m_v)); dr/dxi_a = A, dr/dxi_b = -A, the Jacobian of the inverse retraction taken as the identity.  Per edge
 *   q_e = A^T (Lw r) and W_e = A^T Lw A, column j of it being A^T (Lw (A e_j)).  Per pose Hd_i = the sum of W_e (its upper triangle, the 21 numbers in the
 *   order of tsl_align_sums.H) and g_i = the sum of +q_e where the pose is a, -q_e where it is b, over its enabled incident edges IN ASCENDING EDGE INDEX
 *   from 0.  Rows of fixed poses are 0.
 *   Operator, for one 6-vector p_i per pose (0 for fixed poses): per enabled edge u_e = A^T (Lw (A (p_a - p_b))); per free pose y_i = (damping * Hd_i[k][k])
 *   * p_i[k], then + u_e / - u_e over the incident edges in ascending index.  Preconditioner: per free pose the Cholesky factor of Hd_i with its diagonal
 *   multiplied by (1 + damping) as tsl_align_solve does (H_kk + damping * H_kk), eliminated in tsl_align_solve's order; a pivot <= 0 or not finite is singular.
 *   Reductions: a sum over poses (or edges) is taken in 256 classes: class c adds the terms of i = c, c + 256, ... in ascending order from 0.0, then
 *   s[c] += s[c + h] for h = 128, 64, .., 1 and s[0] is the sum.  The order depends on N and E only.
 *   Linear solve, H x = -g by preconditioned conjugate gradients: x = 0, r = -g, z = M^-1 r, p = z, rz = rz0 = sum dot6(r_i, z_i).  While fewer than pcg_max
 *   iterations are done and not rz <= (pcg_tol * pcg_tol) * rz0: y = operator(p), pAp = sum dot6(p_i, y_i), stop unless pAp > 0, alpha = rz / pAp,
 *   x += alpha p, r -= alpha y, z = M^-1 r, rz' = sum dot6(r_i, z_i), beta = rz' / rz, p = z + beta p, rz = rz'.
 *   Outer loop, at most cfg.iters (<= 64) iterations: evaluate the edges at the current poses (cost = the sum over the enabled edges), gather and factor
 *   (singular: status 3, the iteration is recorded with cost_after = cost_before), solve, retract every free pose by its x_i into trial poses, evaluate them.
 *   max_step = sqrt(max dot6(x_i, x_i)).  The trial is REJECTED when an enabled edge is flipped there, its cost is not finite or not below the current cost:
 *   damping *= damping_up, status 2 once damping > damping_max.  Otherwise it is ACCEPTED: damping = max(damping / damping_down, damping_min), status 0 when
 *   max_step < min_step or cost - trial <= rel_tol * cost.  Status 1: the iterations ran out.  Status 4, decided on the host by a union-find per variant
 *   before the launch: some connected component of the enabled edges holds a free pose and no fixed one (a free pose without an enabled edge included);
 *   status 5: an enabled edge is flipped at the given poses.  Variants of status 4 and 5 are not solved and return the poses as given.
 *   Outputs per variant: the poses, for EVERY edge (enabled or not) r and c = r^T L r at the final poses -- the value of a disabled edge under the solution
 *   that did not see it is what a leave-one-out check reads: a raw cost to compare and rank, not a chi-square to threshold -- and a tsl_pgo_report with the
 *   final cost, the status, the iteration count and a record per iteration (the rest zero).
 * Capacities: max_poses <= 8192, max_edges <= 131072, max_variants <= 1024 and max_variants * (720 * max_poses + 56 * max_edges) bytes of workspace plus the
 * tables under 1 GiB (720 = the trial pose, Hd, the factor and six 6-vectors per pose; 56 = u_e and wgt per edge): 4096 poses, 32768 edges, 1 variant and 1024
 * poses, 8192 edges, 256 variants both fit.  The search direction p lives in LDS up to 1024 poses and in the workspace above; the results do not differ.
 * Arguments: R f64 [N][9] row-major, T f64 [N][3], fixed u8 [N] (linearize: may be NULL), ij i32 [E][2] = (a, b), Z f64 [E][12] = Rz row-major then Tz,
 * L f64 [E][21], masks u64 [B][ceil(E / 64)] (NULL: one variant, every edge on; B is then ignored).  Duplicate edges between one pair simply add.
 * TSL_ERR_ARG (the text names the entry point): a null pointer, N, E or B outside 1 .. the capacity, a == b or an index outside the poses, no fixed pose
 * (solve), a cfg value that is negative or not finite, iters > 64, pcg_max > 100000, damping_down = 0, and in the host forms a number that is not finite or a
 * negative diagonal of L.  The host forms copy, run and wait.  The _dev forms take R, T, Z, L and the outputs as DEVICE pointers and run asynchronously on the
 * handle's stream behind the work queued on `user_stream`, which then waits for them; ij, fixed and the masks stay HOST pointers in both forms, because the
 * incidence lists and the status-4 check are made on the host (they are copied before the call returns).  The _dev forms cannot check the values on the device. */
typedef struct tsl_pgo tsl_pgo;
typedef struct {
    int32_t iters, pcg_max;
    double  damping, damping_up, damping_down, damping_min, damping_max, pcg_tol, min_step, rel_tol, huber;
} tsl_pgo_cfg;
typedef struct { double cost_before, cost_after, max_step, damping; int32_t pcg_iters, accepted; } tsl_pgo_iter;      /* 40 bytes */
typedef struct { int32_t status, iterations; double cost; tsl_pgo_iter it[64]; } tsl_pgo_report;                       /* 2576 bytes */

int  tsl_pgo_create(int device, int32_t max_poses, int32_t max_edges, int32_t max_variants, tsl_pgo** out);
void tsl_pgo_destroy(tsl_pgo* h);
/* one mask (NULL: every edge on): per edge r f64 [E][6], cost f64 [E] = r^T L r, flipped u8 [E]; per pose Hd f64 [N][21] and g f64 [N][6].  For a caller
 * with a solver of its own. */
int  tsl_pgo_linearize(tsl_pgo* h, int32_t N, const double* R, const double* T, const uint8_t* fixed, int32_t E, const int32_t* ij, const double* Z,
                       const double* L, const uint64_t* mask, double huber, double* r, double* cost, uint8_t* flipped, double* Hd, double* g);
int  tsl_pgo_linearize_dev(tsl_pgo* h, int32_t N, const void* R_dev, const void* T_dev, const uint8_t* fixed, int32_t E, const int32_t* ij, const void* Z_dev,
                           const void* L_dev, const uint64_t* mask, double huber, void* r_dev, void* cost_dev, void* flipped_dev, void* Hd_dev, void* g_dev,
                           void* user_stream);
/* outputs: R_out f64 [B][N][9], T_out f64 [B][N][3], r f64 [B][E][6], cost f64 [B][E], reports [B] */
int  tsl_pgo_solve(tsl_pgo* h, int32_t N, const double* R, const double* T, const uint8_t* fixed, int32_t E, const int32_t* ij, const double* Z, const double* L,
                   int32_t B, const uint64_t* masks, const tsl_pgo_cfg* cfg, double* R_out, double* T_out, double* r, double* cost, tsl_pgo_report* reports);
int  tsl_pgo_solve_dev(tsl_pgo* h, int32_t N, const void* R_dev, const void* T_dev, const uint8_t* fixed, int32_t E, const int32_t* ij, const void* Z_dev,
                       const void* L_dev, int32_t B, const uint64_t* masks, const tsl_pgo_cfg* cfg, void* R_out_dev, void* T_out_dev, void* r_dev, void* cost_dev,
                       void* reports_dev, void* user_stream);

/* ---- terrain layers for ground robots (tsl_nav_terrain.hip): per height band and (x, y) column the height of the surface a robot
 * can stand on, over the robot's footprint the step and the slope of that surface, and a class, a distance and a cost in the vocabulary of
 * tsl_tsdf_nav_grid, so that tsl_tsdf_nav_field and the OccupancyGrid adapters take them unchanged.  Where nav_grid calls a column an obstacle as soon as
 * the band holds an occupied voxel, this pass tells a ramp from a wall, a kerb from a cliff and a table one fits under from a block.  The reference has
 * no such pass.  Everything is integer except the f32 comparison of the voxel classes and one f64 expression per column: the result depends on no
 * schedule and tests/nav_terrain_ref.py restates it bit for bit.  The pass reads one submap slot and writes nothing to the map.  All k are signed layers.
 *   The submap slot, the voxel classes and thres are exactly those of tsl_tsdf_nav_grid: thres = free_thres, 0 = the map's surface threshold; an observed
 *     NaN is UNKNOWN; a layer outside the volume is UNKNOWN.
 *   Bands: n_bands in 1 .. 16, k_min[b] <= k_max[b] inside the volume, as in nav_grid: the range in which the support layer is looked for.
 *   Standable layer: layer k of a column is standable when voxel k is OCCUPIED, none of the `clearance` layers k + 1 .. k + clearance is OCCUPIED, and all
 *     of the `free_run` layers k + 1 .. k + free_run are FREE.  0 <= free_run <= clearance <= Nz.  The layers tested above k may leave the band; where
 *     they leave the volume they are UNKNOWN, which is not occupied and not free.
 *   Support: the lowest standable layer of the column with k_min <= k <= k_max when pick = 0, the highest when pick = 1.
 *   col (u8): 0 = has a support; 1 = obstructed: the band holds an OCCUPIED voxel but no standable layer (a wall, a top without headroom); 2 = empty: no
 *     OCCUPIED voxel in the band.
 *   height (int16): 16 * k + q for the support layer k; 32767 where col != 0.  q in 0 .. 15 places the level set thres between the centres of layers k and
 *     k + 1.  When voxel k + 1 is FREE: r = 16.0 * ((double)thres - (double)t_k) / ((double)t_k1 - (double)t_k), the f16 values widened exactly: three
 *     correctly rounded IEEE f64 operations in this order; q = r >= 15.0 ? 15 : (r >= 0.0 ? (int)r : 0), so a NaN r (infinite voxels) gives 0.  When voxel
 *     k + 1 is not FREE, q = 0.  The height is that of the iso-level thres, which lies about thres above the zero crossing of the TSDF: a constant offset
 *     of every height (1.8 voxels = 28.8 height units at the default threshold 1.8 * voxel_scale; subtract it when absolute heights matter; steps
 *     and slopes do not see it).  In metres a height is height * voxel / 16.  A volume with Nz > 4094 is refused: height would not fit.
 *   Window statistics, for the cells with col == 0, over the (2 w + 1)^2 cells within Chebyshev distance w = window, 0 .. 16, clipped to the grid:
 *     nsup (uint16) = the number of those cells that have a support; step (uint16) = the maximum minus the minimum height over them.  Both are 65535
 *     where col != 0.
 *   slope2 (uint32): a Sobel gradient of height at stride s = slope_base, 1 .. 16.  With h(di, dj) = height[i + di][j + dj]:
 *     gx = h(s,-s) + 2 h(s,0) + h(s,s) - h(-s,-s) - 2 h(-s,0) - h(-s,s); gy the same with the roles of i and j exchanged;
 *     slope2 = min(gx^2 + gy^2, 2^32 - 2), computed in 64 bits.  It is valid only when the cell and all eight cells at stride s are inside the grid and
 *     have a support; otherwise it is 2^32 - 1.  tan of the slope = sqrt(slope2) / (128 s).
 *   cls (u8, the codes of nav_grid), tested in this order: col == 1: TSL_NAV_OCCUPIED; col == 2: TSL_NAV_UNKNOWN; step > max_step: OCCUPIED; slope2 valid
 *     and > max_slope2: OCCUPIED; nsup < min_support: UNKNOWN; otherwise TSL_NAV_FREE.  max_step is 0 .. 65534 sixteenths of a voxel; max_slope2 =
 *     2^32 - 1 switches the slope test off.
 *   d2, cost: nav_grid's own distance passes over this cls plane, with the same radius (0 .. 254), flag bits 0 and 1, lut of R * R + 2 entries and
 *     cost_unknown, and the same values.
 *   Layout: every plane is [B][N][N], indexed [b][i + N/2][j + N/2].  Every output is nullable on its own, and a plane that is not asked for is not
 *     computed where that is separable: without step, nsup, slope2, cls, d2 and cost the window pass does not run; without d2 and cost the distance
 *     passes do not run.  cost and lut come together or not at all.
 * tsl_tsdf_nav_terrain issues the queued frames, runs on the handle's stream behind them, waits and copies back.  tsl_tsdf_nav_terrain_dev takes device
 * pointers, is ASYNCHRONOUS and ordered with `user_stream` exactly like tsl_tsdf_nav_grid_dev.  Scratch lives on the handle, grows as needed and is
 * released with it.  With profiling on, tsl_tsdf_prof_query returns the time of TSL_K_NAV_TERRAIN_COLUMNS (the column walk), TSL_K_NAV_TERRAIN_WINDOW (the
 * window statistics, the slope and the class) and, for the distance passes, TSL_K_NAV_EDT_ROWS and TSL_K_NAV_EDT.
 * TSL_ERR_ARG, before anything is launched or written (the text names the entry point): a null handle or cfg; every output null; n_bands outside
 * 1 .. 16; a band that is empty or leaves the volume; a free_thres that is not finite; clearance outside 0 .. Nz; free_run outside 0 .. clearance; pick
 * other than 0 or 1; window outside 0 .. 16; slope_base outside 1 .. 16; max_step outside 0 .. 65534; a negative min_support; radius outside 0 .. 254;
 * flag bits other than 0 and 1; cost without lut or lut without cost; Nz > 4094; N * N * n_bands >= 2^31.  A refused call leaves the handle usable. */
#define TSL_TERRAIN_NO_HEIGHT 32767
#define TSL_TERRAIN_NO_SLOPE 0xffffffffu
typedef struct { int32_t n_bands, k_min[16], k_max[16]; float free_thres;
                 int32_t clearance, free_run, pick, window, slope_base, max_step, min_support; uint32_t max_slope2;
                 int32_t radius, flags; uint8_t cost_unknown, reserved_[3]; } tsl_nav_terrain_cfg;
int  tsl_tsdf_nav_terrain(tsl_tsdf* m, const tsl_nav_terrain_cfg* cfg, const uint8_t* lut, int16_t* height, uint8_t* col, uint16_t* step,
                          uint16_t* nsup, uint32_t* slope2, uint8_t* cls, uint16_t* d2, uint8_t* cost);
int  tsl_tsdf_nav_terrain_dev(tsl_tsdf* m, const tsl_nav_terrain_cfg* cfg, const void* lut_dev, void* height_dev, void* col_dev, void* step_dev,
                              void* nsup_dev, void* slope2_dev, void* cls_dev, void* d2_dev, void* cost_dev, void* user_stream);

/* backend knobs for A/B-ing kernel variants: name in
     "variant"  0|1: one global int64 atomic pair per ray step, 2 (default): brick-binned LDS accumulation
     "semantics" 0 (default): a frame's contributions to a voxel are summed exactly and applied once (order-free, oracle mode BATCHED);
                1: the reference-literal SEQUENTIAL replay of dense_tsdf.py:236-270 -- rays in Taichi's struct-for order, every ray step an f16
                read-modify-write with the W clamp, colours by last writer; on a GLOBAL map: tsl_tsdf_fuse_submaps replays fuse_submaps_kernel
                (dense_tsdf.py:272-318) the same way, submap cells in struct-for order, corners in loop order -- bit-exact with oracle FAITHFUL and
                with the maps the reference's own source produces on tools/ti_seq (tests/golden/ref_*.npz); needs variant 2 and group 1, at
                most 2^21 points per frame and maps of at most 2^17 bricks.  Integration and fusion both follow the reference's struct-for order for any
                num_voxel_per_blk_axis of the submaps, 4..32 (the fusion orders the source cells by the sorted list of the blocks their 16^3 storage bricks overlap).
                Switching the mode on allocates the replay scratch of "seq_impl" 1 (an allocation failure is reported by this call)
     "seq_impl" how semantics 1 integrates.  1 (default): on the brick pipeline, whole batches -- behind phase A every (frame, brick) gets its
                ray steps as 8-byte tuples, stably grouped by voxel in replay order (k_seq_group: persistent workgroups claim the items heavy-first; LDS sample
                sort of the brick's segments by ray rank, a counting walk, then a placing pass that evaluates every step at its replay position),
                phase B is one thread per voxel applying its runs frame after frame (k_seq_replay);
                memory: 8 bytes x "seq_tuple_cap" + 16 KiB x (max_frame_bricks + 1024) per working set, 24 working sets -- ~4.1 GB at the
                defaults -- allocated when "semantics" is set to 1 (round 5: a step is evaluated twice and written once; the first form also kept every
                step in a "stash" array in replay order, 1.5 GB more and 16 bytes of traffic per step).  0: round 3's form -- every ray step a 16-byte tuple, two global radix sorts, one frame per batch
     "seq_longest_run" (get only) the longest run of updates of one voxel in a frame, summed over the frames of the batch issued last (the voxel next
                to the sensor; a wave of its own settles it 64 updates per evaluation where its f16 state has stopped moving)
     "seq_long_voxels" (get only) voxels of the batch issued last that were replayed by a wave of their own (a run of >= 64 updates in a frame)
     "overlapped_launches" / "dry_launches" (get only) batches issued while phase B of the batch before was still pending / into a pipeline that had run
                dry: what the back-to-back parity tests assert on (tests/test_pipeline_overlap_gpu.py); "batch_shape_hash" (get only): FNV hash over the
                sizes of the batches issued so far (two runs that batched the stream alike have the same hash)
     "seq_verify_mismatches" (get only; developer aid, environment TSL_SEQ_VERIFY=1, else -1) literal mode: every (frame, brick) work item is recomputed by
                brute force behind k_seq_group and its offsets / tuples are checksummed behind k_seq_group, in front of the replay and behind it;
                the number of disagreements logged (records on stderr).  Found round 5's one-brick difference
     "seq_tuple_cap" ray steps one frame may produce under seq_impl 1 (default 2^23; a frame beyond it is dropped with TSL_ERR_CAPACITY);
                synchronises; scratch that exists already is rebuilt at the new size
     "overlap"  0 = one frame at a time on the main stream, n = frames per batch (default and maximum 8; three batch slots: phase A of up to two
                batches is in flight beside phase B of a third)
     "adaptive" 1 = queued frames are also issued as soon as phase A of the previous batch has completed (a slow sensor gets every frame
                integrated on arrival; full batches form by themselves when the producer outruns the device), 0 (default) = a batch is
                issued when it is full -- half full for the first two batches after the pipeline ran dry -- or when anything reads the map
     "ramp"     short batches issued after the pipeline ran dry before full ones are waited for (default 2; with 1 a 20-frame burst runs as 4 + 8 + 8: 18.5 k against 18.3 k frames/s in an A/B, inside the box-to-box spread, while the launches of the burst get longer per frame), "ramp_size" their length (default 4)
     "group"    1 (default) = hash grouping of the pixels of a sensor voxel, 0 = stable radix sort
     "split"    lanes per ray (divides 64; the brick-binned path uses at most 8), default 2
     "wg"       threads per workgroup of the brick integrate kernel: 512 (default) or 256 (two workgroups per CU)
     "spt"      segments per thread and step of the brick kernel: 4 (steps of 2048 segments, one 512-thread workgroup per CU) or 2 (steps of 1024,
                <= 128 VGPRs: two 512-thread workgroups = 16 waves per CU)
     "unit"     a brick whose segments of a whole batch number at most this is walked by ONE workgroup, frame after frame, with its voxels in
                registers; heavier bricks are split into parts that leave their sums in slab slots of their own, applied by k_apply_slab
     "unit_floor" the unit limit is quoted for a full batch and scaled with the frames of a shorter one, but not below this (default 4096)
     "unit_half" bricks with more segments per batch than this (and at most "unit") are walked half as a unit (their first frames) and half as
                parts (their later frames): halves the longest serial chain of a launch; >= "unit" disables the middle tier
     "chunks"   steps a part may hold (1..8, default 4)
     "bgrid"    resident workgroups of the brick kernel in percent of the slots (default 75: the rest is left to phase A of the next batch)
     "split_launch" 1 = full batches of the overlapped pipeline launch the brick kernel twice: the PARTS of the heavy bricks (they read
                their frame's rays and write slab slots of their own, never the map) on the batch's phase-A stream, beside the previous
                batch's phase B, and the UNITS + k_apply_slab on the handle's stream; 0 (default) = one launch over the whole work list.
                Measured slower (27 k against 30 k frames/s): the brick kernel is bound by the SIMDs' issue rate, two launches side by side
                slow each other by more than the shorter chain saves
     "ugrid" / "pgrid" resident workgroups of the units / parts launch in percent of the slots (defaults 75 / 25)
     "mesh_gather" 1 = marching cubes reads every value through the brick table also at step 1 (default: brick + halo staged in LDS)
     "esdf_full" 1 = every tsl_esdf_update recomputes all bricks (the reference for the incremental update)
     "esdf_mode" 0 (default) = regional recompute: the bricks whose ESDF inputs changed, dilated by max_dist, are re-initialised and relaxed;
                 1 = raise / lower wavefront with a parent direction per voxel (dense_esdf.py:96, :255-333): only the voxels whose parent chain passes
                 through a changed voxel are re-derived, then lowered -- a third of the voxel writes, the same map bit for bit, ~1.45x the time on the
                 benchmark stream (tsl_esdf.hip has the measurements); read-only "esdf_orphans" = lowered voxels without a supporting neighbour (always 0)
     "esdf_grid" n > 0 = workgroups of a relaxation round (default 0 = four per CU; developer A/B)
     "merge_exchange" (on the GLOBAL map) 0 (default) = tsl_tsdf_allreduce_merge all-reduces the packed sums of the union bricks; 1 = reduce-scatter of the
                 sums, every rank finalises its slice, all-gather of the finalised 5.1-byte voxels (the step form: tsl_tsdf_merge_finalize_slice / _finish_records)
     "fuse_window_misses" (read-only, on the GLOBAL map) corner splats of the LDS-window fusion that fell outside their 15^3 window and went straight to memory
                 (cumulative over the life of the handle.  0 for yaw-like poses, where the window holds every corner; near a body-diagonal rotation a
                 few corners per thousand leave it -- 48 of 229 376 in the case pinned by tests/test_fuse_window_cpu.py.  A miss costs time and is exact)
     "fuse_direct" (on the GLOBAL map) 1 = the fusion splat of round 5, one set of global atomics per corner (A/B); 0 (default) = sums gathered per 8^3 source
                 block in a 15^3 LDS window first.  Textured maps always take the direct form
     "esdf_overlap" 1 (default) = an update's kernels run on one of the handle's phase-A streams: the relaxation rounds of update n overlap
                    the integration of frame n + 1 (which waits only until the update has read the TSDF); 0 = on the handle's stream
     "esdf_round_cap" n > 0 = launch at most n relaxation rounds per update (test knob: an update that stops early must be repaired)
     "fastdiv"  0 = force IEEE division
     "phases"   developer timing aid: 1 = phase A only, 2 = phase B only (the map contents are then meaningless), 3 = both */
int  tsl_tsdf_set_option(tsl_tsdf* m, const char* name, int value);
int  tsl_tsdf_get_option(tsl_tsdf* m, const char* name, int* value);   /* also "fastdiv": 1 when the device verified the fma-refined division;
                                                                           read-only: "last_heavy_bricks" / "last_slab_slots" = bricks walked in parts and
                                                                           merge-slab slots handed out by the batch issued last (synchronises) */

/* ---- environment switches ------------------------------------------------------------------------
 * The product library (lib/libtaichislam_hip.so) reads ONE environment variable:
 *   TSL_SEQ_VERIFY=1   semantics = 1 only: every work item of the literal mode is recounted by brute force from its segment list and an order-free
 *                      checksum of its tuples is compared behind k_seq_group, in front of the replay and behind it; mismatches are counted in
 *                      get_option("seq_verify_mismatches").  Slows the mode down by ~10x; never changes a result.
 * Everything else is compiled only into the developer build lib/libtaichislam_hip_testhooks.so (-DTSL_TEST_HOOKS, built beside the product library
 * by taichislam_amd/build.py; load it with TSL_LIB=<path> in the Python shims):
 *   TSL_FAULT_NO_BDONE_WAIT=1   FAULT INJECTION: phase A of a batch does not wait for the phase B that still reads the batch slot's working sets --
 *                               the map becomes wrong; tests/test_pipeline_overlap_gpu.py uses it to show that the parity tests see the overlap
 *   TSL_PIN_LEGACY=1            host staging buffers without hipHostMallocCoherent (A/B of round 4's allocation)
 *   TSL_EV_SYS=1                pipeline events with the default system-scope fence (A/B of round 5's hipEventDisableSystemFence)
 *   TSL_SEQ_SPLIT_ROLES=1       the two roles of k_seq_replay as separate launches (profiling aid)
 * (the sort-grouped phase A that TSL_GROUP_SORT selected is the backend option "group" = 0.) */

/* ---- profiling: HIP-event timing of the per-frame kernels on the handle's stream ----------------- */
int  tsl_tsdf_prof_enable(tsl_tsdf* m, int on);   /* 0 off, 1 every kernel, 2*mask: only the kernel ids whose bit is set in mask */
int  tsl_tsdf_prof_query(tsl_tsdf* m, int kernel_id, double* total_ms, int64_t* launches);   /* synchronises, resets */

/* ======== Octomap hit counter (taichi_octomap.py) =================================================== */
typedef struct {
    double  map_size_xy, map_size_z, voxel_scale;
    double  min_occupy_thres;
    int32_t texture_enabled;
    double  min_ray_length, max_ray_length;
    int32_t K;
    int32_t max_submap_num;
    double  disp_ceiling, disp_floor;
    int32_t is_global_map;
    int32_t recast_step;
    int32_t color_same_proj;
    int64_t max_disp_particles;
    int32_t max_bricks;
    int32_t max_points;
} tsl_octo_cfg;

int  tsl_octo_create(const tsl_octo_cfg* cfg, int device, tsl_octo** out);        /* taichi_octomap.py:14-84 */
void tsl_octo_destroy(tsl_octo* m);
int  tsl_octo_get_dims(const tsl_octo* m, int32_t* N, int32_t* Nz, int32_t* Rxy, int32_t* Rz, double* voxel_scale);
int  tsl_octo_sync(tsl_octo* m);
int  tsl_octo_reset(tsl_octo* m);                                                    /* :210-211 */
int  tsl_octo_set_intrinsics(tsl_octo* m, const double Kdep[9], const double Kcol[9]);
int  tsl_octo_set_base_pose_submap(tsl_octo* m, int sid, const double R[9], const double T[3]);
int  tsl_octo_get_active_submap(const tsl_octo* m, int32_t* sid);
int  tsl_octo_set_active_submap(tsl_octo* m, int32_t sid);
/* host image.  Untextured: the visited pixels are copied into a pinned, device-mapped slot of a ring at once (the image may be reused on return) and the frame is
 * queued like a device-resident one: no copy call, no synchronisation per frame (30 k frames/s from numpy images).  Textured: staged and inserted at once. */
int  tsl_octo_integrate_depth(tsl_octo* m, const double R[9], const double T[3], const uint16_t* depth, int h, int w,
                              const uint8_t* tex, int th, int tw);                   /* :130-132,147-169; tex u8[th][tw][3] BGR (:120-124) or NULL */
/* device-resident depth (and texture).  Untextured frames are only QUEUED: up to eight are inserted by ONE launch (the insert is an order-free count), issued when
 * eight are queued or as soon as any other call on the handle needs the map or its stream -- invisible except in timing.  The buffers must stay unchanged until
 * tsl_octo_sync (or any call that returns map contents). */
int  tsl_octo_integrate_depth_dev(tsl_octo* m, const double R[9], const double T[3], const void* depth_dev, int h, int w,
                                  const void* tex_dev, int th, int tw);
/* recast_pcl_to_map has no range gate: a point outside the tree, or with a coordinate that is not finite (see "coordinates that are not finite"), counts in p_oob */
int  tsl_octo_integrate_points(tsl_octo* m, const double R[9], const double T[3], const float* xyz, const uint8_t* rgb, int64_t n);   /* :126-128,134-145 */
int  tsl_octo_integrate_points_dev(tsl_octo* m, const double R[9], const double T[3], const void* xyz_dev, const void* rgb_dev, int64_t n);   /* device buffers: f32 [n][3], u8 [n][3] or NULL */
/* the statistics of the last insert.  TSL_ERR_CAPACITY (once: the flag is cleared by the read, and by tsl_octo_reset) when an insert since the last read found
 * the brick pool (max_bricks) full: the points of the bricks that did not get in count in p_oob, the bricks that did hold exact counts */
int  tsl_octo_last_frame_stats(tsl_octo* m, tsl_frame_stats* out);
/* every touched leaf of the active submap: index, hit count and (textured maps; else zeros) colour f32[n][3]; rgb may be NULL */
int  tsl_octo_export_leaves(tsl_octo* m, int32_t* idx, float* cnt, float* rgb, int64_t cap, int64_t* n);
/* cvt_occupy_to_voxels(level) / cvt_occupy_voxels_to(...)  :90-114 */
int  tsl_octo_occupied_voxels(tsl_octo* m, tsl_octo* dst /* NULL = m */, int level, int add_to_cur, int32_t* n);
int  tsl_octo_read_exports(tsl_octo* m, float* xyz, float* rgb, int64_t n);
int  tsl_octo_exports_dev(tsl_octo* m, void** xyz_dev, void** rgb_dev, int32_t* n);   /* export_x / export_color as device pointers + num_export_particles (taichislam_node.py:330-333) */
/* the first n rows of export_x [+ export_color] as a sensor_msgs/PointCloud2 data block (interleaved f32 x y z [r g b]): the publisher of
 * scripts/taichislam_node.py:330-333 + utils/ros_pcl_transfer.py:96-136, interleaved on the device */
int  tsl_octo_pack_pointcloud2(tsl_octo* m, int has_rgb, int64_t n, void* out_host);
int  tsl_octo_num_particles(tsl_octo* m, int32_t* n);
int  tsl_octo_fuse_submaps(tsl_octo* global, tsl_octo* submaps);                     /* :171-199 */

#ifdef __cplusplus
}
#endif
#endif

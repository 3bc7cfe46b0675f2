// tsl_query.hip -- batched map queries used by planners on top of the TSDF map.  Replaces BaseMap.raycast /
// is_pos_occupy / is_near_pos_occupy / is_pos_unobserved (taichi_slam/mapping/mapping_common.py:165-204) and
// DenseTSDF.is_occupy / is_unobserved (dense_tsdf.py:148-155), reference root; TopoGraphGen calls them 64-128 rays at a
// time (topo_graph.py:444-507).  One thread per query, read-only gathers through the brick table.
#include "tsl_query.hpp"
#include "tsl_stage.hpp"
#include <cfloat>

namespace tsl {

// mode 0: is_pos_occupy  1: is_pos_unobserved  2: is_near_pos_occupy(param)
__global__ void __launch_bounds__(256) k_query_points(MapDev M, int s, float vs, float thres, int mode, int param, const float* __restrict__ xyz, long long n, uint8_t* out)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const float q0 = xyz[q * 3] / vs, q1 = xyz[q * 3 + 1] / vs, q2 = xyz[q * 3 + 2] / vs;
    const int i = rnd_i(q0), j = rnd_i(q1), k = rnd_i(q2);                                                   // mapping_common.py:258-266
    bool r = false;
    if (!(cell_fits(q0) && cell_fits(q1) && cell_fits(q2))) {                                                // not finite / no int cell: outside the volume, and so is every neighbour
        const bool occ = 0.0f < thres;                                                                       // (what q_read gives there: TSDF 0, unobserved)
        r = mode == 1 ? true : mode == 0 ? occ : (param > 0 && occ);
    }
    else if (mode == 0) r = q_occupied(M, s, i, j, k, thres);                                                     // :187-191
    else if (mode == 1) { float t; int o; q_read(M, s, i, j, k, &t, &o); r = o == 0; }                       // :181-185
    else { for (int a = -param; a < param; ++a) for (int b = -param; b < param; ++b) for (int c = -param; c < param; ++c) r |= q_occupied(M, s, i + a, j + b, k + c, thres); }   // :193-204
    out[q] = r ? 1 : 0;
}

// the steps of one ray (mapping_common.py:167-177); TEST = test every position for "not finite / no int cell", which reads as outside (TSDF 0)
template <bool TEST>
__device__ __forceinline__ bool ray_walk(const MapDev& M, int s, float vs_f, float vs_len, float thres, int steps, const float* __restrict__ pos, const float* __restrict__ dir, float* x, float* len)
{
    for (int jj = 0; jj < steps; ++jj) {
        const float l = (float)jj * vs_len;                                                                  // :173
        *len = l;
        for (int a = 0; a < 3; ++a) x[a] = dir[a] * l + pos[a];                                              // :174
        const float q0 = x[0] / vs_f, q1 = x[1] / vs_f, q2 = x[2] / vs_f;
        const bool occ = (!TEST || (cell_fits(q0) && cell_fits(q1) && cell_fits(q2))) ? q_occupied(M, s, rnd_i(q0), rnd_i(q1), rnd_i(q2), thres) : 0.0f < thres;
        if (occ) return true;                                                                                // :175-177
    }
    return false;
}
// raycast  mapping_common.py:165-178
__global__ void __launch_bounds__(256) k_query_raycast(MapDev M, int s, float vs_f, float vs_len, float thres, float max_dist, const float* __restrict__ pos,
                                                       const float* __restrict__ dir, long long n, uint8_t* hit, float* end_xyz, float* len)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int steps = (int)(max_dist / vs_f);                                                                // :167, range() truncates
    float x[3] = { 0.0f, 0.0f, 0.0f }, l = 0.0f;
    // The test is made once per ray where that settles it: with a finite origin and direction and |origin| + |direction| * (the ray's length) below 2e9 voxels on
    // every axis, the cell index of every step fits an int (NaN and inf fail the comparison; 2e9 leaves 7 % for the roundings) and the walk is the plain one.
    const float lmax = (float)steps * vs_len;
    bool plain = true;
    for (int a = 0; a < 3; ++a) plain = plain && (fabsf(pos[q * 3 + a]) + fabsf(dir[q * 3 + a]) * lmax) / vs_f < 2.0e9f;
    const bool succ = plain ? ray_walk<false>(M, s, vs_f, vs_len, thres, steps, pos + q * 3, dir + q * 3, x, &l)
                            : ray_walk<true>(M, s, vs_f, vs_len, thres, steps, pos + q * 3, dir + q * 3, x, &l);
    hit[q] = succ ? 1 : 0;
    for (int a = 0; a < 3; ++a) end_xyz[q * 3 + a] = x[a] != x[a] ? __uint_as_float(0x7fc00000u) : x[a];          // a NaN leaves as THE quiet NaN: which one an invalid operation makes differs between processors
    len[q] = l;
}

// ---- device-buffer forms: nothing is staged, nothing is waited for.  The queries are launched on the handle's stream -- behind every frame
// queued so far -- after what `user_stream` (a hipStream_t, e.g. torch's current stream; NULL = the legacy default stream, which is what
// torch uses unless told otherwise) has queued, and `user_stream` is made to wait for them: a planner that expands a node with 64-128
// rays (topo_graph.py:444-507) pays two event operations and one launch, no host round trip.  (Also used by tsl_esdf_query.hip.)
int order_before(tsl_tsdf* m, hipStream_t user, hipStream_t q)
{
    if (user == q) return TSL_OK;
    if (!m->in_ev[0]) for (auto& e : m->in_ev) TSL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipEvent_t e = m->in_ev[m->in_ev_next]; m->in_ev_next = (m->in_ev_next + 1) % 8;
    TSL_HIP(hipEventRecord(e, user));
    TSL_HIP(hipStreamWaitEvent(q, e, 0));
    return TSL_OK;
}
int order_after(tsl_tsdf* m, hipStream_t user, hipStream_t q)
{
    if (user == q) return TSL_OK;
    hipEvent_t e = m->in_ev[m->in_ev_next]; m->in_ev_next = (m->in_ev_next + 1) % 8;
    TSL_HIP(hipEventRecord(e, q));
    TSL_HIP(hipStreamWaitEvent(user, e, 0));
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_query_points(tsl_tsdf* m, int mode, int param, const float* xyz, int64_t n, uint8_t* out)
{
    TSL_REQUIRE(m && n >= 0 && (n == 0 || (xyz && out)), "query_points: bad argument"); TSL_REQUIRE(mode >= 0 && mode <= 2 && param >= 0 && param <= 16, "query_points: bad mode");
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_x = st.in(xyz, (size_t)n * 12), i_o = st.out(out, (size_t)n);
    int rc = st.upload(); if (rc) return rc;
    hipLaunchKernelGGL(k_query_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, m->M, m->cfg.is_global_map ? 0 : m->active, m->P.vs, m->surf_thres, mode, param,
                       st.ptr<const float>(i_x), (long long)n, st.ptr<uint8_t>(i_o));
    TSL_HIP(hipGetLastError());
    return st.download();
}

int tsl_tsdf_query_raycast(tsl_tsdf* m, const float* pos, const float* dir, float max_dist, int64_t n, uint8_t* hit, float* end_xyz, float* len)
{
    TSL_REQUIRE(m && n >= 0 && (n == 0 || (pos && dir && hit && end_xyz && len)), "query_raycast: bad argument");
    TSL_REQUIRE(max_dist >= 0.0f && max_dist <= FLT_MAX, "query_raycast: max_dist is negative or not finite");      // (int)(inf / vs) steps would never end
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    const size_t c = (size_t)n;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_pos = st.in(pos, c * 12), i_dir = st.in(dir, c * 12), i_hit = st.out(hit, c), i_end = st.out(end_xyz, c * 12), i_len = st.out(len, c * 4);
    int rc = st.upload(); if (rc) return rc;
    hipLaunchKernelGGL(k_query_raycast, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, m->M, m->cfg.is_global_map ? 0 : m->active, m->P.vs, (float)m->cfg.voxel_scale,
                       m->surf_thres, max_dist, st.ptr<const float>(i_pos), st.ptr<const float>(i_dir), (long long)n, st.ptr<uint8_t>(i_hit), st.ptr<float>(i_end),
                       st.ptr<float>(i_len));
    TSL_HIP(hipGetLastError());
    return st.download();
}

int tsl_tsdf_query_points_dev(tsl_tsdf* m, int mode, int param, const void* xyz_dev, int64_t n, void* out_dev, void* user_stream)
{
    TSL_REQUIRE(m && n >= 0 && (n == 0 || (xyz_dev && out_dev)), "query_points_dev: bad argument"); TSL_REQUIRE(mode >= 0 && mode <= 2 && param >= 0 && param <= 16, "query_points_dev: bad mode");
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    hipStream_t q = ms(m);
    int rc = order_before(m, (hipStream_t)user_stream, q); if (rc) return rc;
    hipLaunchKernelGGL(k_query_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, m->M, m->cfg.is_global_map ? 0 : m->active, m->P.vs, m->surf_thres, mode, param,
                       (const float*)xyz_dev, (long long)n, (uint8_t*)out_dev);
    TSL_HIP(hipGetLastError());
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_tsdf_query_raycast_dev(tsl_tsdf* m, const void* pos_dev, const void* dir_dev, float max_dist, int64_t n, void* hit_dev, void* end_xyz_dev, void* len_dev, void* user_stream)
{
    TSL_REQUIRE(m && n >= 0 && (n == 0 || (pos_dev && dir_dev && hit_dev && end_xyz_dev && len_dev)), "query_raycast_dev: bad argument");
    TSL_REQUIRE(max_dist >= 0.0f && max_dist <= FLT_MAX, "query_raycast_dev: max_dist is negative or not finite");
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    hipStream_t q = ms(m);
    int rc = order_before(m, (hipStream_t)user_stream, q); if (rc) return rc;
    // rays are short serial chains (max_dist / voxel steps of dependent gathers): 64 threads per workgroup spread a 128-ray batch over two CUs
    hipLaunchKernelGGL(k_query_raycast, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, q, m->M, m->cfg.is_global_map ? 0 : m->active, m->P.vs, (float)m->cfg.voxel_scale,
                       m->surf_thres, max_dist, (const float*)pos_dev, (const float*)dir_dev, (long long)n, (uint8_t*)hit_dev, (float*)end_xyz_dev, (float*)len_dev);
    TSL_HIP(hipGetLastError());
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

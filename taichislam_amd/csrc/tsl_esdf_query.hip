// tsl_esdf_query.hip -- batched ESDF distance / gradient queries for planners (trajectory samples, collision checks, the 64-128-ray node
// expansions of topo_graph.py:444-507, reference root): the counterpart of tsl_query.hip for the ESDF of tsl_esdf.hip.  One lane per query,
// read-only gathers through the brick table, no LDS, no atomics.
//
// A voxel V(i,j,k) of the submap the ESDF was last updated for is KNOWN when it lies in the volume, its brick is allocated and obs > 0; its
// value is exactly what k_esdf_export reports (esdf_value, tsl_esdf_sample.hpp).  Mode 0 reads the nearest voxel (rnd_i(x / vs), as k_query_points does);
// mode 1 interpolates the 8 corners of the cell trilinearly in a fixed f32 order and returns the gradient of that interpolant, so that
// tests/esdf_query_ref.py can restate it bit for bit in numpy.  Status per query: 0 ok, 1 a needed voxel is unknown, 2 a needed voxel is
// outside the volume (or a coordinate is not finite); | 0x80 when the values come from an update that stopped before converging.
#include "tsl_esdf_sample.hpp"      // esdf_sample: the look-up, the value and the interpolant, shared with tsl_path_score.hip
#include "tsl_stage.hpp"

namespace tsl {

template <int MODE>
__global__ void __launch_bounds__(256) k_esdf_query(MapDev M, int s, const float* __restrict__ esdf, float gamma, float max_dist, float vs, float unknown,
                                                    const int* __restrict__ ctr, int rounds, const float* __restrict__ xyz, long long n,
                                                    float* __restrict__ dist, float* __restrict__ grad, uint8_t* __restrict__ status)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int flag = esdf_short_flag(ctr, rounds);
    const float x = xyz[q * 3], y = xyz[q * 3 + 1], z = xyz[q * 3 + 2];
    float d, g0, g1, g2;
    bool nan_tsdf;                                               // not reported here: the value of such a voxel is 0 (esdf_value)
    const int st = esdf_sample<MODE>(M, M.table + (size_t)s * M.nb3, esdf, gamma, max_dist, vs, unknown, x, y, z, &d, &g0, &g1, &g2, &nan_tsdf);
    dist[q] = d;
    if (grad) { grad[q * 3] = g0; grad[q * 3 + 1] = g1; grad[q * 3 + 2] = g2; }
    status[q] = (uint8_t)(st | flag);
}

// the refusals every read of the ESDF makes about the state of the handle (the point queries here, tsl_esdf_score_paths)
int esdf_read_check(tsl_tsdf* m, const char* who)
{
    TSL_REQUIRE(m->esdf && m->esdf_query_ok, std::string(who) + ": no ESDF update since the map was created, reset or imported");
    TSL_REQUIRE(m->esdf_submap == (m->cfg.is_global_map ? 0 : m->active), std::string(who) + ": the active submap changed since the last ESDF update");
    return TSL_OK;
}

// the checks every form makes; *s = the submap the query reads
static int esdf_query_check(tsl_tsdf* m, int mode, const void* xyz, int64_t n, const void* dist, const void* grad, const void* status, const char* who)
{
    TSL_REQUIRE(m && n >= 0, std::string(who) + ": bad argument");
    TSL_REQUIRE(mode == 0 || mode == 1, std::string(who) + ": mode must be 0 (nearest voxel) or 1 (trilinear with gradient)");
    TSL_REQUIRE(!(grad && mode == 0), std::string(who) + ": the gradient needs mode 1");
    TSL_REQUIRE(n == 0 || (xyz && dist && status), std::string(who) + ": null buffer");
    return esdf_read_check(m, who);
}

// launched on the handle's stream, behind the latest update (its relaxation rounds may run on another stream: esdf_overlap)
static int esdf_query_launch(tsl_tsdf* m, hipStream_t q, int mode, float unknown, const float* xyz, int64_t n, float* dist, float* grad, uint8_t* status)
{
    if (m->esdf_last) TSL_HIP(hipStreamWaitEvent(q, m->esdf_last, 0));
    const int s = m->cfg.is_global_map ? 0 : m->active;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (mode == 0) hipLaunchKernelGGL(k_esdf_query<0>, grid, dim3(256), 0, q, m->M, s, (const float*)m->esdf, m->esdf_gamma, m->esdf_maxd, m->P.vs, unknown,
                                      (const int*)m->esdf_q_ctr, m->esdf_q_rounds, xyz, (long long)n, dist, grad, status);
    else hipLaunchKernelGGL(k_esdf_query<1>, grid, dim3(256), 0, q, m->M, s, (const float*)m->esdf, m->esdf_gamma, m->esdf_maxd, m->P.vs, unknown,
                            (const int*)m->esdf_q_ctr, m->esdf_q_rounds, xyz, (long long)n, dist, grad, status);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_esdf_query_points(tsl_tsdf* m, int mode, float unknown_value, const float* xyz, int64_t n, float* dist, float* grad, uint8_t* status)
{
    int rc = esdf_query_check(m, mode, xyz, n, dist, grad, status, "esdf_query_points"); if (rc) return rc;
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    if ((rc = esdf_finish(m))) return rc;                      // the values handed out are the fixed point of the last update
    const hipStream_t q = ms(m);
    const size_t c = (size_t)n;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_x = st.in(xyz, c * 12), i_d = st.out(dist, c * 4), i_g = st.out(grad, c * 12), i_s = st.out(status, c);
    if ((rc = st.upload())) return rc;
    if ((rc = esdf_query_launch(m, q, mode, unknown_value, st.ptr<const float>(i_x), n, st.ptr<float>(i_d), st.ptr<float>(i_g), st.ptr<uint8_t>(i_s)))) return rc;
    return st.download();
}

int tsl_esdf_query_points_dev(tsl_tsdf* m, int mode, float unknown_value, const void* xyz_dev, int64_t n, void* dist_dev, void* grad_dev, void* status_dev, void* user_stream)
{
    int rc = esdf_query_check(m, mode, xyz_dev, n, dist_dev, grad_dev, status_dev, "esdf_query_points_dev"); if (rc) return rc;
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    if (m->esdf_short && (rc = esdf_finish(m))) return rc;     // the host already knows an update stopped early: repair it first
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = esdf_query_launch(m, q, mode, unknown_value, (const float*)xyz_dev, n, (float*)dist_dev, (float*)grad_dev, (uint8_t*)status_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

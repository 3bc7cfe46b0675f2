// tsl_esdf_query.hip -- batched ESDF distance / gradient queries for planners (trajectory samples, collision checks, the 64-128-ray node
// expansions of topo_graph.py:444-507, reference root): the counterpart of tsl_query.hip for the ESDF of tsl_esdf.hip.  One lane per query,
// read-only gathers through the brick table, no LDS, no atomics.
//
// A voxel V(i,j,k) of the submap the ESDF was last updated for is KNOWN when it lies in the volume, its brick is allocated and obs > 0; its
// value is exactly what k_esdf_export reports (esdf_value below).  Mode 0 reads the nearest voxel (rnd_i(x / vs), as k_query_points does);
// mode 1 interpolates the 8 corners of the cell trilinearly in a fixed f32 order and returns the gradient of that interpolant, so that
// tests/esdf_query_ref.py can restate it bit for bit in numpy.  Status per query: 0 ok, 1 a needed voxel is unknown, 2 a needed voxel is
// outside the volume (or a coordinate is not finite); | 0x80 when the values come from an update that stopped before converging.
#include "tsl_interp.hpp"      // lerp_f, cell_floor, the corner bricks and the interpolant: shared with tsl_render.hip

namespace tsl {

#define EQ_UNKNOWN 1
#define EQ_OUTSIDE 2
#define EQ_SHORT 0x80

// the value k_esdf_export reports for an observed voxel (tsl_esdf.hip, k_esdf_export): the TSDF inside the band, elsewhere its sign times the
// relaxed magnitude (max_dist where the voxel was not observed at the last update)
__device__ __forceinline__ float esdf_value(float t, float e, float gamma, float max_dist)
{ return fabsf(t) < gamma ? t : (float)sgn_f(t) * (e != e ? max_dist : fabsf(e)); }

template <int MODE>
__global__ void __launch_bounds__(256) k_esdf_query(MapDev M, int s, const float* __restrict__ esdf, float gamma, float max_dist, float vs, float unknown,
                                                    const int* __restrict__ ctr, int rounds, const float* __restrict__ xyz, long long n,
                                                    float* __restrict__ dist, float* __restrict__ grad, uint8_t* __restrict__ status)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    // an update that stopped early (tsl_esdf.hip esdf_retire: the round after the last one still had work listed, or a raise did not settle)
    const int flag = (ctr && (ctr[2 + rounds % 3] != 0 || ctr[8] != 0)) ? EQ_SHORT : 0;
    const float x = xyz[q * 3], y = xyz[q * 3 + 1], z = xyz[q * 3 + 2];
    const int* __restrict__ T = M.table + (size_t)s * M.nb3;
    float d = unknown, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    int st = EQ_OUTSIDE;
    if (MODE == 0) {
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            const int i = rnd_i(x / vs), j = rnd_i(y / vs), k = rnd_i(z / vs);                   // k_query_points (tsl_query.hip)
            if (in_volume(M, i, j, k)) {
                int l; const int p = T[brick_of(M, i, j, k, &l)];
                const size_t v = (size_t)(p < 0 ? 0 : p) * TSL_BRK3 + l;                          // brick 0 exists: an in-bounds dummy read
                const float t = h2f((h16)(M.tw[v] & 0xffffu)); const int o = M.obs[v]; const float e = esdf[v];
                st = EQ_UNKNOWN;
                if (p >= 0 && o > 0) { d = esdf_value(t, e, gamma, max_dist); st = 0; }
            }
        }
    } else {
        const float u0 = x / vs, u1 = y / vs, u2 = z / vs;
        const int b0 = cell_floor(u0), b1 = cell_floor(u1), b2 = cell_floor(u2);
        if (isfinite(x) && isfinite(y) && isfinite(z) && in_volume(M, b0, b1, b2) && in_volume(M, b0 + 1, b1 + 1, b2 + 1)) {
            const float f0 = u0 - (float)b0, f1 = u1 - (float)b1, f2 = u2 - (float)b2;
            int l000; const int bb = brick_of(M, b0, b1, b2, &l000);
            const int li = l000 >> 8, lj = (l000 >> 4) & 15, lk = l000 & 15;
            int P[8]; cell_bricks(M, T, bb, li, lj, lk, P);                                    // the distinct bricks only; corner c = p << 2 | q << 1 | r
            // all 24 gathers are issued before any is used: two dependent latencies per query (table, then data)
            uint32_t tw[8]; int ob[8]; float e[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const size_t v = corner_voxel(P, c, li, lj, lk);
                tw[c] = M.tw[v]; ob[c] = M.obs[v]; e[c] = esdf[v];
            }
            bool known = true;
            float V[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                known = known && P[c] >= 0 && ob[c] > 0;
                V[c] = esdf_value(h2f((h16)(tw[c] & 0xffffu)), e[c], gamma, max_dist);
            }
            st = EQ_UNKNOWN;
            if (known) {
                // the order of evaluation is the contract (tsl_interp.hpp, tests/esdf_query_ref.py)
                d = tri_value(V, f0, f1, f2);
                tri_grad(V, f0, f1, f2, &g0, &g1, &g2);
                g0 = g0 / vs; g1 = g1 / vs; g2 = g2 / vs;
                st = 0;
            }
        }
    }
    dist[q] = d;
    if (grad) { grad[q * 3] = g0; grad[q * 3 + 1] = g1; grad[q * 3 + 2] = g2; }
    status[q] = (uint8_t)(st | flag);
}

// the checks every form makes; *s = the submap the query reads
static int esdf_query_check(tsl_tsdf* m, int mode, const void* xyz, int64_t n, const void* dist, const void* grad, const void* status, const char* who)
{
    TSL_REQUIRE(m && n >= 0, std::string(who) + ": bad argument");
    TSL_REQUIRE(mode == 0 || mode == 1, std::string(who) + ": mode must be 0 (nearest voxel) or 1 (trilinear with gradient)");
    TSL_REQUIRE(!(grad && mode == 0), std::string(who) + ": the gradient needs mode 1");
    TSL_REQUIRE(n == 0 || (xyz && dist && status), std::string(who) + ": null buffer");
    TSL_REQUIRE(m->esdf && m->esdf_query_ok, std::string(who) + ": no ESDF update since the map was created, reset or imported");
    TSL_REQUIRE(m->esdf_submap == (m->cfg.is_global_map ? 0 : m->active), std::string(who) + ": the active submap changed since the last ESDF update");
    return TSL_OK;
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
    const size_t c = (size_t)n, o_d = c * 12, o_g = o_d + c * 4, o_s = o_g + (grad ? c * 12 : 0);
    if ((rc = grow(&m->xbuf, &m->xbuf_bytes, o_s + c + 64))) return rc;
    char* base = (char*)m->xbuf;
    TSL_HIP(hipMemcpy(base, xyz, c * 12, hipMemcpyHostToDevice));
    const hipStream_t q = ms(m);
    if ((rc = esdf_query_launch(m, q, mode, unknown_value, (const float*)base, n, (float*)(base + o_d), grad ? (float*)(base + o_g) : nullptr, (uint8_t*)(base + o_s)))) return rc;
    TSL_HIP(hipStreamSynchronize(q));
    TSL_HIP(hipMemcpy(dist, base + o_d, c * 4, hipMemcpyDeviceToHost));
    if (grad) TSL_HIP(hipMemcpy(grad, base + o_g, c * 12, hipMemcpyDeviceToHost));
    TSL_HIP(hipMemcpy(status, base + o_s, c, hipMemcpyDeviceToHost));
    return TSL_OK;
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

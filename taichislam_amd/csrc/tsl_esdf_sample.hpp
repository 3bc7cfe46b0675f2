// tsl_esdf_sample.hpp -- the per-point ESDF sample shared by the point queries (tsl_esdf_query.hip), the path scoring (tsl_path_score.hip) and the
// trajectory optimiser (tsl_traj_opt.hip): ONE copy of the voxel / cell look-up, the value k_esdf_export reports and the interpolant with its gradient,
// so that all of them return the same bits for a point (tests/esdf_query_ref.py restates it in numpy; tests/path_score_ref.py and tests/traj_opt_ref.py
// build on that).
#pragma once
#include "tsl_interp.hpp"      // lerp_f, cell_floor, the corner bricks and the interpolant: shared with tsl_render.hip

namespace tsl {

#define EQ_UNKNOWN 1
#define EQ_OUTSIDE 2
#define EQ_SHORT 0x80

// the value k_esdf_export reports for an observed voxel (tsl_esdf.hip, k_esdf_export): the TSDF inside the band, elsewhere its sign times the
// relaxed magnitude (max_dist where the voxel was not observed at the last update)
__device__ __forceinline__ float esdf_value(float t, float e, float gamma, float max_dist)
{ return fabsf(t) < gamma ? t : (float)sgn_f(t) * (e != e ? max_dist : fabsf(e)); }

// an update that stopped early (tsl_esdf.hip esdf_retire: the round after the last one still had work listed, or a raise did not settle)
__device__ __forceinline__ int esdf_short_flag(const int* __restrict__ ctr, int rounds)
{ return (ctr && (ctr[2 + rounds % 3] != 0 || ctr[8] != 0)) ? EQ_SHORT : 0; }

// The sample at (x, y, z) of submap table T: returns the status (0, EQ_UNKNOWN, EQ_OUTSIDE; without the early-stop flag), *d = the value (`unknown`
// unless the status is 0) and, in mode 1, (*g0, *g1, *g2) = the gradient per metre (0 unless the status is 0).  *nan_tsdf: the status is 0 and a voxel
// the sample reads holds a NaN TSDF (one that came in through an import; its value is sign(NaN) = 0 times the magnitude, so the VALUE does not show it).
// The point queries ignore it; the path scoring counts such a sample as unknown.
template <int MODE>
__device__ __forceinline__ int esdf_sample(const MapDev& M, const int* __restrict__ T, const float* __restrict__ esdf, float gamma, float max_dist, float vs,
                                           float unknown, float x, float y, float z, float* dd, float* gg0, float* gg1, float* gg2, bool* nan_tsdf)
{
    float d = unknown, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    int st = EQ_OUTSIDE;
    bool tainted = false;
    if (MODE == 0) {
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            const int i = rnd_i(x / vs), j = rnd_i(y / vs), k = rnd_i(z / vs);                   // k_query_points (tsl_query.hip)
            if (in_volume(M, i, j, k)) {
                int l; const int p = T[brick_of(M, i, j, k, &l)];
                const size_t v = (size_t)(p < 0 ? 0 : p) * TSL_BRK3 + l;                          // brick 0 exists: an in-bounds dummy read
                const float t = h2f((h16)(M.tw[v] & 0xffffu)); const int o = M.obs[v]; const float e = esdf[v];
                st = EQ_UNKNOWN;
                if (p >= 0 && o > 0) { d = esdf_value(t, e, gamma, max_dist); st = 0; tainted = t != t; }
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
                const float t = h2f((h16)(tw[c] & 0xffffu));
                tainted = tainted || t != t;
                V[c] = esdf_value(t, e[c], gamma, max_dist);
            }
            st = EQ_UNKNOWN;
            if (known) {
                // the order of evaluation is the contract (tsl_interp.hpp, tests/esdf_query_ref.py)
                d = tri_value(V, f0, f1, f2);
                tri_grad(V, f0, f1, f2, &g0, &g1, &g2);
                g0 = g0 / vs; g1 = g1 / vs; g2 = g2 / vs;
                st = 0;
            }
            tainted = tainted && known;
        }
    }
    *nan_tsdf = tainted;
    *dd = d; *gg0 = g0; *gg1 = g1; *gg2 = g2;
    return st;
}

}  // namespace tsl

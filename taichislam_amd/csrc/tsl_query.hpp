// tsl_query.hpp -- the voxel reads of the map queries (tsl_query.hip) shared with the topology graph's rays (tsl_topo.hip)
#pragma once
#include "tsl_tsdf.hpp"

namespace tsl {

__device__ __forceinline__ void q_read(const MapDev& M, int s, int i, int j, int k, float* tsdf, int* obs)
{
    *tsdf = 0.0f; *obs = 0;                                   // outside the volume / inactive cell reads as 0 (A7)
    if (!in_volume(M, i, j, k)) return;
    int l; const int b = brick_of(M, i, j, k, &l);
    const int p = pool_lookup_ro(M, s, b);
    if (p < 0) return;
    const size_t v = (size_t)p * TSL_BRK3 + l;
    *tsdf = h2f((h16)(M.tw[v] & 0xffffu)); *obs = M.obs[v];
}
// is_occupy  dense_tsdf.py:153-155 (an unobserved voxel reads TSDF = 0 and therefore counts as occupied)
__device__ __forceinline__ bool q_occupied(const MapDev& M, int s, int i, int j, int k, float thres)
{ float t; int o; q_read(M, s, i, j, k, &t, &o); return t < thres; }

}  // namespace tsl

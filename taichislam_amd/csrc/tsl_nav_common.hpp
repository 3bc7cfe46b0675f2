// tsl_nav_common.hpp -- the one copy of what the two column passes share, k_nav_project (tsl_nav_grid.hip) and k_terrain_columns (tsl_nav_terrain.hip): the
// height bands, the refusals both make about them, and the voxel classes of a lane's 16 layers of a brick -- with the NaN rule, which differs from the
// frontier pass on purpose and must never differ between these two.
#pragma once
#include <cmath>
#include <string>
#include "tsl_tsdf.hpp"

namespace tsl {

#define NAV_MAX_BANDS 16

// the head of the configuration of either kernel
struct NavBands {
    int s, B;                                          // the submap slot read, the number of bands
    int uk0[NAV_MAX_BANDS], uk1[NAV_MAX_BANDS];        // the bands as unsigned layer indices k + Nz / 2; a band beyond B is empty: uk0 = 0, uk1 = -1
    float thres;
};

// A lane's 16 layers of pool brick P, voxels tid * 16 .. tid * 16 + 15: 64 contiguous bytes of tw and 16 of obs, five 16-byte loads.  mo / mf: bit lk set
// when layer lk is OCCUPIED (observed and the f16 TSDF widened to f32 < thres) / FREE (observed, not occupied, and not a NaN: a NaN is neither and stays
// UNKNOWN).  tw: the 16 words as loaded, f16 TSDF in the low half.
__device__ __forceinline__ void nav_column_load(const MapDev& M, int P, int tid, float thres, uint32_t& mo, uint32_t& mf, uint32_t tw[16])
{
    const uint4* __restrict__ tw4 = reinterpret_cast<const uint4*>(M.tw + (size_t)P * TSL_BRK3 + (size_t)tid * 16);
    const uint4 ob = *reinterpret_cast<const uint4*>(M.obs + (size_t)P * TSL_BRK3 + (size_t)tid * 16);
    const uint4 t0 = tw4[0], t1 = tw4[1], t2 = tw4[2], t3 = tw4[3];
    const uint32_t t[16] = { t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, t3.x, t3.y, t3.z, t3.w };
    const uint32_t ow[4] = { ob.x, ob.y, ob.z, ob.w };
    mo = 0u; mf = 0u;
#pragma unroll
    for (int lk = 0; lk < 16; ++lk) {
        tw[lk] = t[lk];
        const bool seen = (int8_t)((ow[lk >> 2] >> ((lk & 3) * 8)) & 0xffu) > 0;
        const float v = h2f((h16)(t[lk] & 0xffffu));
        const bool occ = seen && v < thres;                    // the test of q_occupied; false for a NaN
        const bool fre = seen && !occ && v == v;               // a NaN is neither: it stays unknown
        mo |= occ ? (1u << lk) : 0u;
        mf |= fre ? (1u << lk) : 0u;
    }
}

// The refusals nav_grid and nav_terrain share, in the order both make them, and the bands.  `mid` and `late` are the caller's own refusals, which stand
// between free_thres and radius and in front of the grid size: each returns TSL_OK or has set the error.  Cfg: tsl_nav_cfg or tsl_nav_terrain_cfg.
template <class Cfg, class Mid, class Late>
int nav_bands_check(tsl_tsdf* m, const Cfg* c, const void* lut, bool any_out, const void* cost, const std::string& w, Mid mid, Late late, NavBands* C)
{
    int rc;
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(any_out, w + ": every output is null");
    TSL_REQUIRE(c->n_bands >= 1 && c->n_bands <= NAV_MAX_BANDS, w + ": n_bands must be 1 .. 16");
    for (int b = 0; b < c->n_bands; ++b)
        TSL_REQUIRE(c->k_min[b] <= c->k_max[b] && c->k_min[b] >= -(m->Nz / 2) && c->k_max[b] <= m->Nz / 2 - 1,
                    w + ": band " + std::to_string(b) + " is empty (k_min > k_max) or leaves the volume");
    TSL_REQUIRE(std::isfinite(c->free_thres), w + ": free_thres is not finite");
    if ((rc = mid())) return rc;
    TSL_REQUIRE(c->radius >= 0 && c->radius <= 254, w + ": radius must be 0 .. 254 voxels");
    TSL_REQUIRE((c->flags & ~3) == 0, w + ": unknown flags (bits 0 and 1 are defined)");
    TSL_REQUIRE((cost != nullptr) == (lut != nullptr), w + ": cost and lut come together or not at all");
    if ((rc = late())) return rc;
    TSL_REQUIRE((long long)m->N * m->N * c->n_bands < (1ll << 31), w + ": the grids are too large (N * N * n_bands >= 2^31)");
    C->s = m->cfg.is_global_map ? 0 : m->active;
    C->B = c->n_bands;
    for (int b = 0; b < NAV_MAX_BANDS; ++b) { C->uk0[b] = b < c->n_bands ? c->k_min[b] + m->Nz / 2 : 0; C->uk1[b] = b < c->n_bands ? c->k_max[b] + m->Nz / 2 : -1; }
    C->thres = c->free_thres != 0.0f ? c->free_thres : m->surf_thres;
    return TSL_OK;
}

}  // namespace tsl

// tsl_register_common.hpp -- what the map-to-map registration (tsl_register.hip) and the pose search over it
// (tsl_register_search.hip, section 4.10) share: the per-call constants of a linearisation and the checks and defaults of a tsl_register_cfg.  One
// copy, so that a score and a linearisation gate, round and refuse alike.
#pragma once
#include <cmath>
#include <cstring>
#include "tsl_align_common.hpp"

namespace tsl {

struct RegisterDev {
    float R[9], T[3];                  // source-submap to destination coordinates, rounded to f32 once
    float vs;
    float w_min, band, r_max, gm2, huber;      // after the defaults; gm2 = g_max * g_max
    int smask;                         // stride - 1: an index is on the lattice when (index & smask) == 0 (two's complement: negative indices too)
    int flags;                         // bit 0: counts only
};

static bool rg_finite(float x) { return std::isfinite(x); }

static int rg_slot(const tsl_tsdf* m, int sid) { return m->cfg.is_global_map ? 0 : (sid < 0 ? m->active : sid); }

// r_max after its default: the truncation distance of the destination
static float rg_r_max(const tsl_tsdf* dst, const tsl_register_cfg* c)
{
    return c->r_max != 0.0f ? c->r_max : (float)((double)dst->cfg.internal_voxels * dst->cfg.voxel_scale);
}

// the checks and defaults the entry points share; `stride` replaces the configuration's (the levels of the registration).  m_min: a further lower
// bound of M in the overflow refusal (the search's cost of a miss, tsl_register_search.hip); 0 leaves the bound as section 4.9 states it
static int register_check(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R[9], const double T[3], const tsl_register_cfg* c, const void* out,
                          int stride, RegisterDev* A, const char* who, double m_min = 0.0)
{
    const std::string w(who);
    TSL_REQUIRE(dst && src, w + ": null handle");
    TSL_REQUIRE(R && T && c && out, w + ": null argument");
    TSL_REQUIRE(al_finite(R, 9) && al_finite(T, 3), w + ": the pose is not finite");
    TSL_REQUIRE(rg_finite(c->w_min) && rg_finite(c->band) && rg_finite(c->r_max) && rg_finite(c->g_max) && rg_finite(c->huber), w + ": w_min / band / r_max / g_max / huber is not finite");
    TSL_REQUIRE(stride == 1 || stride == 2 || stride == 4 || stride == 8 || stride == 16, w + ": stride must be 1, 2, 4, 8 or 16");
    TSL_REQUIRE(!(c->w_min < 0.0f) && !(c->band < 0.0f) && !(c->r_max < 0.0f) && !(c->g_max < 0.0f) && !(c->huber < 0.0f), w + ": w_min, band, r_max, g_max and huber must not be negative");
    TSL_REQUIRE(dst_sid >= -1 && (dst->cfg.is_global_map ? dst_sid <= 0 : dst_sid < dst->nsub), w + ": dst_sid out of range (-1 or 0 on a global map)");
    TSL_REQUIRE(src_sid >= -1 && (src->cfg.is_global_map ? src_sid <= 0 : src_sid < src->nsub), w + ": src_sid out of range (-1 or 0 on a global map)");
    TSL_REQUIRE(dst->device == src->device, w + ": the maps live on different devices");
    TSL_REQUIRE(std::memcmp(&dst->P.vs, &src->P.vs, sizeof(float)) == 0, w + ": the maps have different voxel sizes");
    for (int i = 0; i < 9; ++i) A->R[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) A->T[i] = (float)T[i];
    A->vs = dst->P.vs;
    A->w_min = c->w_min;
    A->band = c->band != 0.0f ? c->band : 2.0f * A->vs;
    A->r_max = rg_r_max(dst, c);
    const float gmax = c->g_max != 0.0f ? c->g_max : 4.0f;
    A->gm2 = gmax * gmax;
    A->huber = c->huber;
    A->smask = stride - 1; A->flags = c->flags;
    // no sum can overflow: a used voxel has |g_a| <= g_max, |p_a| <= L (its cell is in dst's volume), so |c_a| <= 2 L g_max, and |r| <= |s| + |t| <=
    // r_max + band; wgt <= 1.  Every product is at most M^2 in magnitude, every addend at most M^2 2^20 + 1/2.  V bounds the visited voxels without a
    // look at the device: a submap has at most min(max_bricks, nb3) bricks of (16 / stride)^3 lattice voxels.
    const double L = (double)(dst->M.hN > dst->M.hNz ? dst->M.hN : dst->M.hNz) * dst->cfg.voxel_scale;
    double Mx = 2.0 * L * (double)gmax;
    if ((double)gmax > Mx) Mx = (double)gmax;
    if ((double)A->r_max + (double)A->band > Mx) Mx = (double)A->r_max + (double)A->band;
    if (m_min > Mx) Mx = m_min;
    const double per = (double)(16 / stride), V = (double)(src->M.max_bricks < src->M.nb3 ? src->M.max_bricks : src->M.nb3) * per * per * per;
    TSL_REQUIRE(Mx * Mx * 1048576.0 * V <= 4611686018427387904.0, w + ": the sums could overflow (max(2 L g_max, g_max, r_max + band" + (m_min > 0.0 ? ", miss" : "") +
                ")^2 * 2^20 * visited voxels exceeds 2^62)");
    return TSL_OK;
}

}  // namespace tsl

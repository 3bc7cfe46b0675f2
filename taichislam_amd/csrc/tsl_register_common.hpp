// tsl_register_common.hpp -- what the map-to-map registration (tsl_register.hip) and the pose search over it
// (tsl_register_search.hip, section 4.10) share: the per-call constants of a linearisation, pass 1 over a source brick (rg_brick_origin, rg_scan_row,
// rg_push: which voxels are visited, which of them pass the gate, and their queue in LDS), the checks and defaults of a tsl_register_cfg, the grid of a
// kernel over the source's bricks and the staging of a call.  One copy, so that a score and a linearisation visit, gate, round and refuse alike.
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

// ---- pass 1: a workgroup of 256 threads over one brick of the source; thread t owns the 16 voxels of k-row t (local indices t * 16 .. t * 16 + 15) ----

// the voxel indices of the first voxel of pool brick pb; false when the brick belongs to another submap (`first` = slot * nb3).  Uniform in the workgroup.
__device__ __forceinline__ bool rg_brick_origin(const MapDev& S, int pb, int first, int* i0, int* j0, int* k0)
{
    const int b = S.owner[pb] - first;
    if (b < 0 || b >= S.nb3) return false;
    const int bk = b % S.nbz, bj = (b / S.nbz) % S.nbx, bi = b / (S.nbz * S.nbx);
    *i0 = bi * 16 - S.hN; *j0 = bj * 16 - S.hN; *k0 = bk * 16 - S.hNz;
    return true;
}

// This thread's row of brick pb: the obs and tw planes by 16-byte loads when the row is on the lattice, then f(r, seen, pass, tw) for every r of the
// row whose k is on the lattice (uniform: every lane calls f for the same r) -- seen: a visited voxel, pass: it passes the weight and band gates too.
template <class F>
__device__ __forceinline__ void rg_scan_row(const MapDev& S, const RegisterDev& A, int pb, int i0, int j0, int k0, F f)
{
    const int li = threadIdx.x >> 4, lj = threadIdx.x & 15;
    const bool row = (((i0 + li) | (j0 + lj)) & A.smask) == 0;
    uint4 ob = make_uint4(0u, 0u, 0u, 0u), t0 = ob, t1 = ob, t2 = ob, t3 = ob;
    if (row) {
        ob = *reinterpret_cast<const uint4*>(S.obs + (size_t)pb * TSL_BRK3 + threadIdx.x * 16);
        const uint4* tp = reinterpret_cast<const uint4*>(S.tw + (size_t)pb * TSL_BRK3 + threadIdx.x * 16);
        t0 = tp[0]; t1 = tp[1]; t2 = tp[2]; t3 = tp[3];
    }
    const uint32_t obw[4] = { ob.x, ob.y, ob.z, ob.w };
    const uint32_t tww[16] = { t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, t3.x, t3.y, t3.z, t3.w };
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if ((k0 + r) & A.smask) continue;                         // uniform
        const bool seen = row && (int8_t)((obw[r >> 2] >> ((r & 3) * 8)) & 0xffu) > 0;
        const uint32_t tw = tww[r];
        const float w = h2f((h16)(tw >> 16)), t = h2f((h16)(tw & 0xffffu));
        f(r, seen, seen && (w >= A.w_min) && (fabsf(t) <= A.band), tw);      // a NaN weight or value is gated
    }
}

// The lanes of m = __ballot(pass) append their voxel r to an LDS queue, as local index << 16 | t: the leader reserves the places on *counter, each
// lane takes the one of its rank.  The queue's first entry stands for the counter value q_base.
__device__ __forceinline__ void rg_push(unsigned long long m, bool pass, int r, uint32_t tw, int* counter, uint32_t* queue, int q_base)
{
    if (!m) return;
    const int leader = (int)__builtin_ctzll(m);
    int base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(counter, popc64(m));
    base = __shfl(base, leader);
    if (pass) queue[base + rank_below(m) - q_base] = ((uint32_t)(threadIdx.x * 16 + r) << 16) | (tw & 0xffffu);      // at most 4096 per brick
}

// the voxel indices of a queue entry's local index l
__device__ __forceinline__ void rg_entry_voxel(int l, int i0, int j0, int k0, int* i, int* j, int* k) { *i = i0 + (l >> 8); *j = j0 + ((l >> 4) & 15); *k = k0 + (l & 15); }

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

// the grid of a kernel whose workgroups stride over the source's pool
static int rg_grid(const tsl_tsdf* dst, const tsl_tsdf* src)
{
    int grid = src->M.max_bricks;                                  // never more workgroups than pool bricks
    if (grid > 4 * dst->ncu) grid = 4 * dst->ncu;
    return grid < 1 ? 1 : grid;
}

// issues the queued frames of both handles, waits for the source's, and leaves dst's stream with `bytes` of dst's staging buffer: the accumulator
static int register_stage(tsl_tsdf* dst, tsl_tsdf* src, size_t bytes, hipStream_t* q, long long** acc)
{
    TSL_HIP(hipSetDevice(dst->device));
    if (src != dst) { const int rc = tsl_tsdf_sync(src); if (rc) return rc; }      // as tsl_tsdf_fuse_submaps: the source is complete before dst's stream reads it
    *q = ms(dst);
    const int rc = grow(&dst->xbuf, &dst->xbuf_bytes, bytes); if (rc) return rc;
    *acc = (long long*)dst->xbuf;
    return TSL_OK;
}

}  // namespace tsl

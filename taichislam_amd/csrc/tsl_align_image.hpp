// tsl_align_image.hpp -- what the two image kernels of the Gauss-Newton family share: the depth-only alignment (tsl_align.hip) and
// the depth-and-colour alignment (tsl_align_rgbd.hip, section 4.8.2) visit the same pixels, gate and back-project them in the same f32 order, and take
// the same checks and defaults of a tsl_align_cfg.
#pragma once
#include "tsl_align_common.hpp"

namespace tsl {

struct AlignDev {
    float R[9], T[3];                  // camera-to-map pose in the frame of the point queries, rounded to f32 once
    float fx, fy, cx, cy, vs;
    float thr_min, thr_max;            // the depth gate in millimetres
    float r_max, gm2, huber;           // gm2 = g_max * g_max
    int h, w, stride, hh, ww;          // image size; visited rows / columns
    int flags;                         // bit 0: counts only
};

// The pixel of visited column ii and row jj: -1 when it is not a visited pixel, AL_GATE when its depth is gated; otherwise AL_USED, (*i, *j) the pixel
// and p its back-projection in the map frame, which the caller carries on into its sampler.  The f32 expressions and their order are the contract.
__device__ __forceinline__ int al_pixel(const AlignDev& A, const uint16_t* __restrict__ depth, int ii, int jj, int* i_out, int* j_out, float p[3])
{
    if (!(ii < A.ww && jj < A.hh)) return -1;
    const int i = ii * A.stride, j = jj * A.stride;
    *i_out = i; *j_out = j;
    const uint16_t d = depth[(size_t)j * A.w + i];
    const float df = (float)d;
    if (!(d != 0 && !(df > A.thr_max) && !(df < A.thr_min))) return AL_GATE;
    const float dep = df / 1000.0f;
    const float px = ((float)i - A.cx) * dep / A.fx, py = ((float)j - A.cy) * dep / A.fy, pz = dep;
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = ((A.R[a * 3] * px + A.R[a * 3 + 1] * py) + A.R[a * 3 + 2] * pz) + A.T[a];
    return AL_USED;
}

// the checks and defaults every form shares; `stride` replaces the configuration's (the levels of the tracker)
static int align_check(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_cfg* c, const void* depth, const void* out, int stride,
                       AlignDev* A, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(R && T && c && depth && out, w + ": null argument");
    TSL_REQUIRE(al_finite(R, 9) && al_finite(T, 3), w + ": the pose is not finite");
    TSL_REQUIRE(al_finite(c->K, 9), w + ": an intrinsic is not finite");
    TSL_REQUIRE(std::isfinite(c->d_min) && std::isfinite(c->d_max) && std::isfinite(c->r_max) && std::isfinite(c->g_max) && std::isfinite(c->huber),
                w + ": d_min / d_max / r_max / g_max / huber is not finite");
    TSL_REQUIRE(c->h > 0 && c->w > 0 && c->h <= 32768 && c->w <= 32768, w + ": the image size must be 1 .. 32768 per side");
    TSL_REQUIRE(stride >= 1, w + ": stride must be at least 1");
    TSL_REQUIRE(!(c->r_max < 0.0f) && !(c->g_max < 0.0f) && !(c->huber < 0.0f), w + ": r_max, g_max and huber must not be negative");
    for (int i = 0; i < 9; ++i) A->R[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) A->T[i] = (float)T[i];
    bool zero = true; for (int i = 0; i < 9; ++i) zero = zero && c->K[i] == 0.0;
    if (zero) { A->fx = m->P.fx; A->fy = m->P.fy; A->cx = m->P.cx; A->cy = m->P.cy; }           // the map's depth intrinsics
    else { A->fx = (float)c->K[0]; A->fy = (float)c->K[4]; A->cx = (float)c->K[2]; A->cy = (float)c->K[5]; }
    A->vs = m->P.vs;
    const double dmin = c->d_min != 0.0f ? (double)c->d_min : m->cfg.min_ray_length, dmax = c->d_max != 0.0f ? (double)c->d_max : m->cfg.max_ray_length;
    TSL_REQUIRE(dmax > dmin, w + ": d_max must exceed d_min");
    A->thr_min = (float)(dmin * 1000.0); A->thr_max = (float)(dmax * 1000.0);                     // as tsl_tsdf_create forms the integrator's gate
    A->r_max = c->r_max != 0.0f ? c->r_max : (float)((double)m->cfg.internal_voxels * m->cfg.voxel_scale);
    const float gmax = c->g_max != 0.0f ? c->g_max : 4.0f;
    A->gm2 = gmax * gmax;
    A->huber = c->huber;
    A->h = c->h; A->w = c->w; A->stride = stride; A->flags = c->flags;
    A->hh = (int)(((long long)c->h + stride - 1) / stride); A->ww = (int)(((long long)c->w + stride - 1) / stride);      // a stride near INT_MAX must not wrap
    // no sum can overflow: a used pixel has |g_a| <= g_max, |p_a| <= L (its cell is in the volume), so |c_a| <= 2 L g_max, and |s| <= r_max;
    // wgt <= 1.  Every product is at most M^2 in magnitude, M = max(2 L g_max, g_max, r_max), every addend at most M^2 2^20 + 1/2.
    const double L = (double)(m->M.hN > m->M.hNz ? m->M.hN : m->M.hNz) * m->cfg.voxel_scale;
    double Mx = 2.0 * L * (double)gmax;
    if ((double)gmax > Mx) Mx = (double)gmax;
    if ((double)A->r_max > Mx) Mx = (double)A->r_max;
    const double visited = (double)A->hh * (double)A->ww;
    TSL_REQUIRE(Mx * Mx * 1048576.0 * visited <= 4611686018427387904.0, w + ": the sums could overflow (max(2 L g_max, r_max)^2 * 2^20 * visited pixels exceeds 2^62)");
    return TSL_OK;
}

}  // namespace tsl

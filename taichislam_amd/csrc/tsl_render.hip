// tsl_render.hip -- what a camera at a given pose would see of the TSDF: depth, normal and colour per pixel (the model image of frame-to-model
// tracking, a view of the map without meshing it, the check of a map against the depth stream that built it).  It stands beside BaseMap.raycast
// (taichi_slam/mapping/mapping_common.py:165-178, reference root; tsl_query.hip), which steps a whole voxel at a time, tests the nearest voxel
// against a threshold and returns the last stepped position: a depth quantised to a voxel and no normal.  The reference has no renderer.
//
// Definition (tests/render_view_ref.py restates it in numpy and the output must equal it bit for bit).  All f32, no
// contraction, in the written order.  Pixel (u, v): dc = ((u - cx) / fx, (v - cy) / fy, 1), d = R dc (rows summed left to right, NOT normalised:
// the ray parameter is the optical-axis depth).  Samples n = 0 .. S-1 at t_n = t_min + n * dt, p_n = T + t_n * d.  The value of a sample is the
// trilinear interpolant (tsl_interp.hpp) of the stored TSDF over the cell floor(p / vs); the sample is KNOWN when its 8 corners are in the volume,
// in allocated bricks and observed.  Two consecutive known samples with s_prev > 0 >= s_n are a hit (front face), with s_prev <= 0 < s_n a back
// face, which ends the ray; an unknown sample only forgets the previous one.  At a hit t* = t_prev + dt * (s_prev / (s_prev - s_n)) is the depth,
// the normal is the normalised gradient of the interpolant at p* = T + t* d, the colour that of the voxel rnd_i(p* / vs).
//
// One lane per pixel, a wave covers an 8 x 8 pixel tile (neighbouring rays share bricks and cache lines), read-only gathers through the brick
// table with every load of a sample issued before any is used, no LDS, no atomics.
//
// Skipping (flags bit 0 switches it off; the output is the same bit for bit).  Per axis, p_n is a monotone function of n: t_n is (n -> n * dt and
// x -> t_min + x are monotone under round-to-nearest), and so are x -> T + x * d, x -> x / vs and floor.  So the samples whose base voxel lies in
// one brick -- a box -- or beyond one face of the volume -- a half space -- are a contiguous run of n: if samples n and m > n are both there,
// so is every sample between them.  A sample whose base voxel is outside the volume or in an unallocated brick is unknown (its corner 000 is).
// A ray that meets such a sample estimates the end of the run with a slab test, steps two samples back, and CHECKS that sample m with the exact
// arithmetic of the walk: if it is in the same brick / half space, n .. m are all unknown and the walk resumes at m + 1 having forgotten the
// previous sample, exactly what evaluating them one by one leaves behind; if not, it goes on to n + 1.  The estimate decides how far a ray
// jumps, never what it computes.
#include <cmath>
#include "tsl_interp.hpp"
#include "tsl_stage.hpp"

namespace tsl {

#define RV_MISS 1
#define RV_BACK 2
#define RV_NO_NORMAL 0x40

struct ViewDev {
    float R[9], T[3];                  // camera-to-map pose in the frame of the point queries, rounded to f32 once
    float fx, fy, cx, cy;
    float tmin, dt, vs;
    int h, w, S, flags;
};

// sample m of the ray: position and base voxel, with the arithmetic of the walk; false when a coordinate is not finite
__device__ __forceinline__ bool rv_sample_pos(const ViewDev& W, const float d[3], int m, float* t, float p[3], float u[3], int b[3])
{
    *t = W.tmin + (float)m * W.dt;
#pragma unroll
    for (int a = 0; a < 3; ++a) { p[a] = W.T[a] + *t * d[a]; u[a] = p[a] / W.vs; b[a] = cell_floor(u[a]); }
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// the sample index at which the ray reaches the plane `edge` (a voxel index) of axis a, as a float: an ESTIMATE (see the file comment)
__device__ __forceinline__ float rv_plane_sample(const ViewDev& W, float da, int a, int edge)
{ return ((((float)edge * W.vs - W.T[a]) / da) - W.tmin) / W.dt; }

// Sample n has its base voxel b in an unallocated brick.  Returns the next sample to evaluate: m + 1 when sample m > n was verified to lie in the
// same brick (n .. m are unknown), else n + 1.
__device__ __forceinline__ int rv_skip_brick(const MapDev& M, const ViewDev& W, const float d[3], int n, const int b[3])
{
    const int lo[3] = { ((b[0] + M.hN) & ~15) - M.hN, ((b[1] + M.hN) & ~15) - M.hN, ((b[2] + M.hNz) & ~15) - M.hNz };
    float ne = (float)(W.S - 1);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (d[a] != 0.0f) { const float nf = rv_plane_sample(W, d[a], a, d[a] > 0.0f ? lo[a] + TSL_BRK : lo[a]); if (nf < ne) ne = nf; }
    if (!(ne >= (float)(n + 4))) return n + 1;                     // nothing to gain (or the estimate is not a number)
    const int m = (int)ne - 2;                                     // rounded down, two samples of margin: the check below nearly always passes
    float t, p[3], u[3]; int c[3];
    if (!rv_sample_pos(W, d, m, &t, p, u, c)) return n + 1;
    const bool same = c[0] >= lo[0] && c[0] < lo[0] + TSL_BRK && c[1] >= lo[1] && c[1] < lo[1] + TSL_BRK && c[2] >= lo[2] && c[2] < lo[2] + TSL_BRK;
    return same ? m + 1 : n + 1;
}

// Sample n has its base voxel b outside the volume.  On an axis where it moves away from the volume (or not at all) every later sample is outside
// too: the ray is over (returns S).  Otherwise jumps towards the face it has to cross, as rv_skip_brick does.
__device__ __forceinline__ int rv_skip_outside(const MapDev& M, const ViewDev& W, const float d[3], int n, const int b[3])
{
    const int lo[3] = { -M.hN, -M.hN, -M.hNz }, hi[3] = { M.N - M.hN, M.N - M.hN, M.Nz - M.hNz };      // voxels lo .. hi - 1 are in the volume
    float ne = -1.0f; int ax = 0; bool below = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool under = b[a] < lo[a], over = b[a] >= hi[a];
        if ((under && !(d[a] > 0.0f)) || (over && !(d[a] < 0.0f))) return W.S;
        if (under || over) { const float nf = rv_plane_sample(W, d[a], a, under ? lo[a] : hi[a]); if (nf > ne) { ne = nf; ax = a; below = under; } }
    }
    if (!(ne >= (float)(n + 4))) return n + 1;
    if (ne > (float)(W.S - 1)) ne = (float)(W.S - 1);
    const int m = (int)ne - 2;
    if (m <= n) return n + 1;
    float t, p[3], u[3]; int c[3];
    if (!rv_sample_pos(W, d, m, &t, p, u, c)) return n + 1;
    const int ca = ax == 0 ? c[0] : ax == 1 ? c[1] : c[2], la = ax == 0 ? lo[0] : ax == 1 ? lo[1] : lo[2], ha = ax == 0 ? hi[0] : ax == 1 ? hi[1] : hi[2];
    return (below ? ca < la : ca >= ha) ? m + 1 : n + 1;
}

// 5 waves per SIMD: 89 VGPRs, no scratch.  Left to itself the compiler takes 147 VGPRs (3 waves) and the walk -- a chain of dependent gathers that only
// other waves can hide -- runs 1.5 times slower (profiles/render_view.txt).
__global__ void __launch_bounds__(256, 5) k_render_view(MapDev M, int s, ViewDev W, float* __restrict__ depth, float* __restrict__ normal,
                                                     float* __restrict__ rgb, uint8_t* __restrict__ status)
{
    // a wave = an 8 x 8 pixel tile, the workgroup's four waves a 16 x 16 tile
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (px >= W.w || py >= W.h) return;
    const int* __restrict__ T = M.table + (size_t)s * M.nb3;
    const float dc0 = ((float)px - W.cx) / W.fx, dc1 = ((float)py - W.cy) / W.fy, dc2 = 1.0f;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (W.R[r * 3] * dc0 + W.R[r * 3 + 1] * dc1) + W.R[r * 3 + 2] * dc2;
    const bool skip = !(W.flags & 1);

    int st = RV_MISS, n = 0;
    bool pk = false; float ps = 0.0f, pt = 0.0f, ts = 0.0f;
    while (n < W.S) {
        float t, p[3], u[3], V[8]; int b[3];
        int next = n + 1; bool kn = false; float sv = 0.0f;
        if (rv_sample_pos(W, d, n, &t, p, u, b)) {
            if (in_volume(M, b[0], b[1], b[2])) {
                int l; const int P0 = T[brick_of(M, b[0], b[1], b[2], &l)];
                if (P0 >= 0) {
                    kn = tsdf_read_cell(M, T, b[0], b[1], b[2], V);
                    if (kn) sv = tri_value(V, u[0] - (float)b[0], u[1] - (float)b[1], u[2] - (float)b[2]);
                } else if (skip) next = rv_skip_brick(M, W, d, n, b);
            } else if (skip) next = rv_skip_outside(M, W, d, n, b);
        }
        if (pk && kn) {
            if (ps > 0.0f && sv <= 0.0f) { st = 0; ts = pt + W.dt * (ps / (ps - sv)); break; }
            if (ps <= 0.0f && sv > 0.0f) { st = RV_BACK; break; }
        }
        pk = kn; ps = sv; pt = t; n = next;
    }

    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (st == 0) {
        float p[3], u[3], V[8]; int b[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { p[a] = W.T[a] + ts * d[a]; u[a] = p[a] / W.vs; b[a] = cell_floor(u[a]); }
        const bool fin = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        bool ok = fin && tsdf_read_cell(M, T, b[0], b[1], b[2], V);
        if (ok) {
            tri_grad(V, u[0] - (float)b[0], u[1] - (float)b[1], u[2] - (float)b[2], &g0, &g1, &g2);
            const float len = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
            ok = len > 0.0f;
            if (ok) { g0 = g0 / len; g1 = g1 / len; g2 = g2 / len; }
        }
        if (!ok) { g0 = 0.0f; g1 = 0.0f; g2 = 0.0f; st = RV_NO_NORMAL; }
        if (rgb && fin) {                                        // the voxel the surface export colours (tsl_tsdf.hip k_export_particles); 0 when it is unknown
            const int i = rnd_i(u[0]), j = rnd_i(u[1]), k = rnd_i(u[2]);
            if (in_volume(M, i, j, k)) {
                int l; const int P = T[brick_of(M, i, j, k, &l)];
                const size_t v = (size_t)(P < 0 ? 0 : P) * TSL_BRK3 + l;
                if (P >= 0 && M.obs[v] > 0) { c0 = h2f(M.col[v * 4]); c1 = h2f(M.col[v * 4 + 1]); c2 = h2f(M.col[v * 4 + 2]); }
            }
        }
    }
    const size_t o = (size_t)py * W.w + px;
    depth[o] = (st & ~RV_NO_NORMAL) == 0 ? ts : 0.0f;
    if (normal) { normal[o * 3] = g0; normal[o * 3 + 1] = g1; normal[o * 3 + 2] = g2; }
    if (rgb) { rgb[o * 3] = c0; rgb[o * 3 + 1] = c1; rgb[o * 3 + 2] = c2; }
    status[o] = (uint8_t)st;
}

static bool all_finite(const double* a, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false; return true; }

// the checks and defaults both forms share
static int render_check(tsl_tsdf* m, const double R[9], const double T[3], const tsl_view_cfg* v, const void* depth, const void* rgb, const void* status,
                        ViewDev* W, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(R && T && v && depth && status, w + ": null argument");
    TSL_REQUIRE(all_finite(R, 9) && all_finite(T, 3), w + ": the pose is not finite");
    TSL_REQUIRE(all_finite(v->K, 9), w + ": an intrinsic is not finite");
    TSL_REQUIRE(std::isfinite(v->t_min) && std::isfinite(v->t_max) && std::isfinite(v->dt), w + ": t_min / t_max / dt is not finite");
    TSL_REQUIRE(v->h > 0 && v->w > 0 && v->h <= 32768 && v->w <= 32768, w + ": the image size must be 1 .. 32768 per side");
    TSL_REQUIRE(!rgb || m->M.col, w + ": rgb needs a textured map");
    for (int i = 0; i < 9; ++i) W->R[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) W->T[i] = (float)T[i];
    bool zero = true; for (int i = 0; i < 9; ++i) zero = zero && v->K[i] == 0.0;
    if (zero) { W->fx = m->P.fx; W->fy = m->P.fy; W->cx = m->P.cx; W->cy = m->P.cy; }           // the map's depth intrinsics
    else { W->fx = (float)v->K[0]; W->fy = (float)v->K[4]; W->cx = (float)v->K[2]; W->cy = (float)v->K[5]; }
    W->vs = m->P.vs;
    W->tmin = v->t_min != 0.0f ? v->t_min : (float)m->cfg.min_ray_length;
    const float tmax = v->t_max != 0.0f ? v->t_max : (float)m->cfg.max_ray_length;
    W->dt = v->dt != 0.0f ? v->dt : 0.75f * W->vs;
    TSL_REQUIRE(tmax > W->tmin, w + ": t_max must exceed t_min");
    TSL_REQUIRE(W->dt > 0.0f, w + ": dt must be positive");
    const float q = (tmax - W->tmin) / W->dt;
    TSL_REQUIRE(q < 16777216.0f, w + ": more than 2^24 samples per ray");
    W->S = (int)q + 1;
    W->h = v->h; W->w = v->w; W->flags = v->flags;
    return TSL_OK;
}

static int render_launch(tsl_tsdf* m, hipStream_t q, const ViewDev& W, float* depth, float* normal, float* rgb, uint8_t* status)
{
    hipLaunchKernelGGL(k_render_view, dim3((unsigned)((W.w + 15) / 16), (unsigned)((W.h + 15) / 16)), dim3(256), 0, q, m->M, m->cfg.is_global_map ? 0 : m->active, W,
                       depth, normal, rgb, status);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_render_view(tsl_tsdf* m, const double R[9], const double T[3], const tsl_view_cfg* v, float* depth, float* normal, float* rgb, uint8_t* status)
{
    ViewDev W;
    int rc = render_check(m, R, T, v, depth, rgb, status, &W, "render_view"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames
    const size_t c = (size_t)W.h * W.w;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_d = st.out(depth, c * 4), i_n = st.out(normal, c * 12), i_c = st.out(rgb, c * 12), i_s = st.out(status, c);
    if ((rc = st.upload())) return rc;
    if ((rc = render_launch(m, q, W, st.ptr<float>(i_d), st.ptr<float>(i_n), st.ptr<float>(i_c), st.ptr<uint8_t>(i_s)))) return rc;
    return st.download();
}

int tsl_tsdf_render_view_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_view_cfg* v, void* depth_dev, void* normal_dev, void* rgb_dev,
                             void* status_dev, void* user_stream)
{
    ViewDev W;
    int rc = render_check(m, R, T, v, depth_dev, rgb_dev, status_dev, &W, "render_view_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = render_launch(m, q, W, (float*)depth_dev, (float*)normal_dev, (float*)rgb_dev, (uint8_t*)status_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

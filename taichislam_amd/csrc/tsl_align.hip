// tsl_align.hip -- frame-to-model alignment: a depth frame against the TSDF, Gauss-Newton on the signed distance (Bylow et al., "Real-Time Camera
// Tracking and 3D Reconstruction Using Signed Distance Functions", RSS 2013; Canelhas et al., "SDF Tracker", IROS 2013): minimise the sum of
// s(R p_i + T)^2 over the camera-to-map pose, s the trilinear interpolant of the stored TSDF (tsl_interp.hpp), p_i the back-projected pixels.  The
// reference takes its poses from a VIO and has no tracker; tsl_render.hip renders the model image, this file consumes a frame against the model.
//
// Definition (tests/track_ref.py restates it in numpy and every integer must equal it).  All f32, no contraction, in the
// written order.  Visited pixels (i, j) = (ii * stride, jj * stride).  A pixel with depth d (uint16 millimetres) falls into exactly one bucket:
//   gate     d == 0, (float)d > d_max * 1000 or (float)d < d_min * 1000 (the comparisons of k_voxelize_depth, tsl_tsdf.hip); otherwise
//            dep = (float)d / 1000, px = ((float)i - cx) * dep / fx, py = ((float)j - cy) * dep / fy, pz = dep, p[a] = ((R[a][0] px + R[a][1] py) + R[a][2] pz) + T[a]
//   unknown  the sample at p is not KNOWN (section 4.7); otherwise s = tri_value, g = tri_grad / vs
//   far      not |s| <= r_max (a NaN s, from a stored value that is not finite, is far)
//   grad     gg = (g0 g0 + g1 g1) + g2 g2 is not in (0, g_max * g_max]
//   used     c = p x g, J = (g, c), wgt = huber > 0 && |s| > huber ? huber / |s| : 1, wJ = wgt J; the 28 products H_ab = wJ[a] J[b] (a <= b), b_a = wJ[a] s,
//            e = (wgt s) s
// Every product x is added as the integer rint(x * 2^20) (round half to even) into int64 sums: integer sums do not depend on the order of
// the additions, so the 33 integers are the same for any schedule.
//
// Buckets unknown to used, the products and their reduction are tsl_align_common.hpp's (al_sample, al_products, al_flush), shared with
// tsl_register.hip and tsl_register_search.hip; the pixel gate, the back-projection and the checks are tsl_align_image.hpp's (al_pixel, align_check),
// shared with tsl_align_rgbd.hip; the tiling is this file's.
//
// One lane per visited pixel, a wave covers an 8 x 8 tile of them and a workgroup 16 x 16 (the tiling of k_render_view).  The 28 sums are reduced in
// the wave by a halving butterfly -- at the step over lane bit b a lane keeps one half of its values and hands the other half to its partner, 16 + 8
// + 4 + 2 + 1 + 1 = 32 exchanges instead of 28 x 6 -- the five counts by ballots, then across the four waves through LDS; one 64-bit integer
// atomic per non-zero sum per workgroup.  No float atomics.  flags bit 0 leaves the products and their reduction out (H, b, e = 0, the counts as
// usual): what the gathers cost alone (tools/bench_track.py).
#include <cmath>
#include "tsl_align_common.hpp"      // the sampler, the products, the reduction, the step, the retraction and the iteration: shared with tsl_register.hip
#include "tsl_align_image.hpp"       // the visited pixels, their gate and back-projection, the checks of a tsl_align_cfg: shared with tsl_align_rgbd.hip

namespace tsl {

__global__ void __launch_bounds__(256) k_align_linearize(MapDev M, int s, AlignDev A, const uint16_t* __restrict__ depth, long long* __restrict__ acc)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ii = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), jj = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    float sv = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f }, p[3] = { 0.0f, 0.0f, 0.0f };
    int i, j, bucket = al_pixel(A, depth, ii, jj, &i, &j, p);     // -1: not a visited pixel
    if (bucket == AL_USED) bucket = al_sample(p, M, M.table + (size_t)s * M.nb3, A.vs, A.r_max, A.gm2, &sv, g);
    const bool used = bucket == AL_USED;
    long long v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = 0;
    const bool sums = !(A.flags & 1);                             // the A/B switch: without the products and their reduction only the counts are formed
    if (used && sums) al_products(p, g, sv, A.huber, v);           // the residual is the distance itself
    const unsigned long long mu = __ballot(used);
    al_flush(v, popc64(mu), popc64(__ballot(bucket == AL_GATE)), popc64(__ballot(bucket == AL_UNKNOWN)), popc64(__ballot(bucket == AL_FAR)),
             popc64(__ballot(bucket == AL_GRAD)), mu && sums, acc);
}

// zeroes the accumulator and launches, both on q
static int align_launch(tsl_tsdf* m, hipStream_t q, const AlignDev& A, const uint16_t* depth, long long* acc)
{
    TSL_HIP(hipMemsetAsync(acc, 0, AL_SLOTS * sizeof(long long), q));
    prof_begin(m, TSL_K_ALIGN, q);
    hipLaunchKernelGGL(k_align_linearize, dim3((unsigned)((A.ww + 15) / 16), (unsigned)((A.hh + 15) / 16)), dim3(256), 0, q, m->M,
                       m->cfg.is_global_map ? 0 : m->active, A, depth, acc);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// one linearisation on q with the result on the host: launch, copy back through the pinned buffer, wait
static int align_run(tsl_tsdf* m, hipStream_t q, const AlignDev& A, const uint16_t* depth_dev, long long* acc, tsl_align_sums* out)
{
    int rc = align_launch(m, q, A, depth_dev, acc); if (rc) return rc;
    return al_read_back(m, q, acc, sizeof(tsl_align_sums), out);
}

// the accumulator and (host form) the staged image in the export staging buffer: [40 x int64 | pad to 512 | depth]
static int align_stage(tsl_tsdf* m, hipStream_t q, const tsl_align_cfg* c, const uint16_t* depth_host, long long** acc, const uint16_t** depth_dev)
{
    const size_t bytes = (size_t)c->h * c->w * sizeof(uint16_t);
    int rc = grow(&m->xbuf, &m->xbuf_bytes, 512 + (depth_host ? bytes : 0) + 64); if (rc) return rc;
    *acc = (long long*)m->xbuf;
    if (depth_host) {
        TSL_HIP(hipMemcpyAsync((char*)m->xbuf + 512, depth_host, bytes, hipMemcpyHostToDevice, q));
        *depth_dev = (const uint16_t*)((char*)m->xbuf + 512);
    }
    return TSL_OK;
}

// the iteration (al_iterate); the depth image is on the device, q has been ordered behind whatever produced it
static int track_run(tsl_tsdf* m, hipStream_t q, const double R0[9], const double T0[3], const tsl_align_cfg* c, const tsl_track_cfg* t, const uint16_t* depth_dev,
                     long long* acc, double R_out[9], double T_out[3], tsl_track_report* rep, const char* who)
{
    return al_iterate(R0, T0, t, [&](int stride, const double* R, const double* T, tsl_align_sums* s) {
        AlignDev A;
        const int rc = align_check(m, R, T, c, depth_dev, R_out, stride, &A, who); if (rc) return rc;
        return align_run(m, q, A, depth_dev, acc, s);
    }, R_out, T_out, rep);
}

// every level is checked before anything runs
static int track_prepare(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_cfg* c, const tsl_track_cfg* t, const void* depth, const void* R_out,
                         const void* T_out, const char* who)
{
    TSL_REQUIRE(m, std::string(who) + ": null handle");
    TSL_REQUIRE(R_out && T_out, std::string(who) + ": null argument");
    int rc = track_check(t, who); if (rc) return rc;
    AlignDev A;
    for (int l = 0; l < t->n_levels; ++l) if ((rc = align_check(m, R0, T0, c, depth, R_out, t->stride[l], &A, who))) return rc;
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_align_linearize(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_cfg* c, const uint16_t* depth, tsl_align_sums* out)
{
    AlignDev A;
    int rc = align_check(m, R, T, c, depth, out, c ? c->stride : 1, &A, "align_linearize"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames
    long long* acc; const uint16_t* dd = nullptr;
    if ((rc = align_stage(m, q, c, depth, &acc, &dd))) return rc;
    return align_run(m, q, A, dd, acc, out);
}

int tsl_tsdf_align_linearize_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_cfg* c, const void* depth_dev, void* sums_dev, void* user_stream)
{
    AlignDev A;
    int rc = align_check(m, R, T, c, depth_dev, sums_dev, c ? c->stride : 1, &A, "align_linearize_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = align_launch(m, q, A, (const uint16_t*)depth_dev, (long long*)sums_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_align_solve(const tsl_align_sums* s, double damping, double xi[6], int32_t* singular)
{
    TSL_REQUIRE(s && xi && singular, "align_solve: null argument");
    TSL_REQUIRE(std::isfinite(damping) && !(damping < 0.0), "align_solve: damping must be finite and not negative");
    *singular = al_solve(s, damping, xi) ? 0 : 1;
    return TSL_OK;
}

int tsl_pose_retract(const double xi[6], double R[9], double T[3])
{
    TSL_REQUIRE(xi && R && T, "pose_retract: null argument");
    TSL_REQUIRE(al_finite(xi, 6) && al_finite(R, 9) && al_finite(T, 3), "pose_retract: an argument is not finite");
    al_retract(xi, R, T);
    return TSL_OK;
}

int tsl_tsdf_track_depth(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_cfg* c, const tsl_track_cfg* t, const uint16_t* depth,
                         double R_out[9], double T_out[3], tsl_track_report* rep)
{
    int rc = track_prepare(m, R0, T0, c, t, depth, R_out, T_out, "track_depth"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    long long* acc; const uint16_t* dd = nullptr;
    if ((rc = align_stage(m, q, c, depth, &acc, &dd))) return rc;
    return track_run(m, q, R0, T0, c, t, dd, acc, R_out, T_out, rep, "track_depth");
}

int tsl_tsdf_track_depth_dev(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_cfg* c, const tsl_track_cfg* t, const void* depth_dev,
                             double R_out[9], double T_out[3], tsl_track_report* rep, void* user_stream)
{
    int rc = track_prepare(m, R0, T0, c, t, depth_dev, R_out, T_out, "track_depth_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;      // the image is whatever user_stream has queued for it
    long long* acc;
    if ((rc = align_stage(m, q, c, nullptr, &acc, nullptr))) return rc;
    return track_run(m, q, R0, T0, c, t, (const uint16_t*)depth_dev, acc, R_out, T_out, rep, "track_depth_dev");
}

}  // extern "C"

// tsl_align_points.hip -- scan-to-model alignment: a point cloud (a lidar scan, a merged multi-camera cloud, an undistorted depth image) against the
// TSDF.  The same Gauss-Newton problem as tsl_align.hip -- minimise the sum of s(R p_i + T)^2 over the sensor-to-map pose -- with the points given
// in the sensor frame instead of back-projected from an image, and with a per-point result: the bucket and the signed distance of every visited
// point at the pose, which a caller can use to drop the points of moving objects before it integrates the scan.
//
// Definition (tests/track_points_ref.py restates it in numpy and every integer, bucket and s must equal it).  All f32, no
// contraction, in the written order.  Visited point k is point k * stride of xyz (f32 [n][3]), k < visited = ceil(n / stride); it falls into
// exactly one bucket:
//   gate     x, y or z is not finite, or l2 = (x x + y y) + z z is > dmax2 or < dmin2 (dmax2 = d_max d_max, dmin2 = d_min d_min, formed once on the
//            host in f32; an l2 that overflows to inf is > dmax2); otherwise p[a] = ((R[a][0] x + R[a][1] y) + R[a][2] z) + T[a]
//   unknown, far, grad, used   al_sample at p with the residual r = s, as in tsl_align.hip
// Buckets unknown to used, the products and their reduction are tsl_align_common.hpp's (al_sample, al_products, al_flush); the gate, the transform,
// the tiling of the flat list and the per-point outputs are this file's.  bucket[k] (u8, the AL_* codes) and s[k] (f32: the interpolant for used,
// far and grad, +0.0f for gate and unknown) are optional and written by plain vector stores.
//
// One lane per visited point, 256 threads per workgroup, lanes beyond `visited` hold bucket -1.  The per-point outputs are a template parameter: the
// variant without them has no stores (67 VGPRs, no scratch, as k_align_linearize).  flags bit 0 leaves the products and their reduction out (counts only).
//
// Point loads: three dwords per lane, straight from global memory.  The alternative, the wave's span of the cloud -- (63 stride + 1) x 3 floats --
// loaded coalesced into LDS and read from there, was built and timed against it (tools/bench_track_points.py, profiles/track_points.txt): at stride
// 1 the two are level (38.6 against 39.2 us for 307 200 points, inside the spread), at stride 8 the staged form is slower (15.3 against 13.1 us
// for 38 400 visited points: it moves the same lines and adds an LDS round trip with an 8-way bank conflict).  The direct loads are kept.
#include <cmath>
#include "tsl_align_common.hpp"

namespace tsl {

struct AlignPointsDev {
    float R[9], T[3];                  // sensor-to-map pose in the frame of the point queries, rounded to f32 once
    float vs, dmin2, dmax2;            // the range gate, squared
    float r_max, gm2, huber;           // gm2 = g_max * g_max
    long long visited;                 // visited points = ceil(n / stride)
    int stride, flags;                 // bit 0: counts only
};

template <bool PP>
__global__ void __launch_bounds__(256) k_align_points_linearize(MapDev M, int sub, AlignPointsDev A, const float* __restrict__ xyz, long long* __restrict__ acc,
                                                                 uint8_t* __restrict__ bucket_out, float* __restrict__ s_out)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    int bucket = -1;                                              // not a visited point
    float sv = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f }, p[3] = { 0.0f, 0.0f, 0.0f };
    if (k < A.visited) {
        const float* q = xyz + (size_t)(k * A.stride) * 3;       // k * stride <= n - 1 < 2^30
        const float x = q[0], y = q[1], z = q[2];
        const float l2 = (x * x + y * y) + z * z;
        bucket = AL_GATE;
        if (isfinite(x) && isfinite(y) && isfinite(z) && !(l2 > A.dmax2) && !(l2 < A.dmin2)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = ((A.R[a * 3] * x + A.R[a * 3 + 1] * y) + A.R[a * 3 + 2] * z) + A.T[a];
            bucket = al_sample(p, M, M.table + (size_t)sub * M.nb3, A.vs, A.r_max, A.gm2, &sv, g);
        }
        if (PP) {
            if (bucket_out) bucket_out[k] = (uint8_t)bucket;
            if (s_out) s_out[k] = (bucket == AL_GATE || bucket == AL_UNKNOWN) ? 0.0f : sv;
        }
    }
    const bool used = bucket == AL_USED;
    long long v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = 0;
    const bool sums = !(A.flags & 1);
    if (used && sums) al_products(p, g, sv, A.huber, v);           // the residual is the distance itself
    const unsigned long long mu = __ballot(used);
    al_flush(v, popc64(mu), popc64(__ballot(bucket == AL_GATE)), popc64(__ballot(bucket == AL_UNKNOWN)), popc64(__ballot(bucket == AL_FAR)),
             popc64(__ballot(bucket == AL_GRAD)), mu && sums, acc);
}

// the checks and defaults every form shares; `stride` replaces the configuration's (the levels of the tracker)
static int points_check(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_points_cfg* c, const void* xyz, int64_t n, const void* out, int stride,
                        AlignPointsDev* A, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(R && T && c && out, w + ": null argument");
    TSL_REQUIRE(n >= 0 && n <= (int64_t)1 << 30, w + ": the number of points must be 0 .. 2^30");
    TSL_REQUIRE(xyz || n == 0, w + ": null argument");
    TSL_REQUIRE(al_finite(R, 9) && al_finite(T, 3), w + ": the pose is not finite");
    TSL_REQUIRE(std::isfinite(c->d_min) && std::isfinite(c->d_max) && std::isfinite(c->r_max) && std::isfinite(c->g_max) && std::isfinite(c->huber),
                w + ": d_min / d_max / r_max / g_max / huber is not finite");
    TSL_REQUIRE(stride >= 1, w + ": stride must be at least 1");
    TSL_REQUIRE(!(c->d_min < 0.0f) && !(c->r_max < 0.0f) && !(c->g_max < 0.0f) && !(c->huber < 0.0f), w + ": d_min, r_max, g_max and huber must not be negative");
    for (int i = 0; i < 9; ++i) A->R[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) A->T[i] = (float)T[i];
    A->vs = m->P.vs;
    const float dmin = c->d_min != 0.0f ? c->d_min : (float)m->cfg.min_ray_length, dmax = c->d_max != 0.0f ? c->d_max : (float)m->cfg.max_ray_length;
    TSL_REQUIRE(dmax > dmin, w + ": d_max must exceed d_min");
    A->dmin2 = dmin * dmin; A->dmax2 = dmax * dmax;
    A->r_max = c->r_max != 0.0f ? c->r_max : (float)((double)m->cfg.internal_voxels * m->cfg.voxel_scale);
    const float gmax = c->g_max != 0.0f ? c->g_max : 4.0f;
    A->gm2 = gmax * gmax;
    A->huber = c->huber;
    A->stride = stride; A->flags = c->flags;
    A->visited = (n + stride - 1) / stride;                      // int64: a stride near INT_MAX must not wrap
    // no sum can overflow: the bound of align_check (tsl_align.hip) with the visited points in place of the visited pixels
    const double L = (double)(m->M.hN > m->M.hNz ? m->M.hN : m->M.hNz) * m->cfg.voxel_scale;
    double Mx = 2.0 * L * (double)gmax;
    if ((double)gmax > Mx) Mx = (double)gmax;
    if ((double)A->r_max > Mx) Mx = (double)A->r_max;
    TSL_REQUIRE(Mx * Mx * 1048576.0 * (double)A->visited <= 4611686018427387904.0, w + ": the sums could overflow (max(2 L g_max, r_max)^2 * 2^20 * visited points exceeds 2^62)");
    return TSL_OK;
}

// zeroes the accumulator and launches, both on q; an empty cloud launches nothing
static int points_launch(tsl_tsdf* m, hipStream_t q, const AlignPointsDev& A, const float* xyz, long long* acc, uint8_t* bucket, float* s)
{
    TSL_HIP(hipMemsetAsync(acc, 0, AL_SLOTS * sizeof(long long), q));
    if (A.visited == 0) return TSL_OK;
    const dim3 grid((unsigned)((A.visited + 255) / 256));
    const int sub = m->cfg.is_global_map ? 0 : m->active;
    prof_begin(m, TSL_K_ALIGN_POINTS, q);
    if (bucket || s) hipLaunchKernelGGL(k_align_points_linearize<true>, grid, dim3(256), 0, q, m->M, sub, A, xyz, acc, bucket, s);
    else hipLaunchKernelGGL(k_align_points_linearize<false>, grid, dim3(256), 0, q, m->M, sub, A, xyz, acc, bucket, s);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// The export staging buffer of the host forms: [40 x int64 | pad to 512 | xyz f32 [n][3] | s f32 [per] | bucket u8 [per]], per = the visited points
// of a call that wants the per-point outputs, else 0.  The cloud is copied in on q.
struct PointsStage { long long* acc; const float* xyz; float* s; uint8_t* bucket; };

static int points_stage(tsl_tsdf* m, hipStream_t q, const float* xyz_host, int64_t n, int64_t per, PointsStage* st)
{
    const size_t cloud = xyz_host ? (size_t)n * 3 * sizeof(float) : 0;
    int rc = grow(&m->xbuf, &m->xbuf_bytes, 512 + cloud + (size_t)per * 5 + 64); if (rc) return rc;
    char* base = (char*)m->xbuf;
    st->acc = (long long*)base;
    st->xyz = (const float*)(base + 512);
    st->s = (float*)(base + 512 + cloud);
    st->bucket = (uint8_t*)(base + 512 + cloud + (size_t)per * 4);
    if (cloud) TSL_HIP(hipMemcpyAsync(base + 512, xyz_host, cloud, hipMemcpyHostToDevice, q));
    return TSL_OK;
}

// the iteration (al_iterate); the cloud is on the device, q has been ordered behind whatever produced it
static int track_points_run(tsl_tsdf* m, hipStream_t q, const double R0[9], const double T0[3], const tsl_align_points_cfg* c, const tsl_track_cfg* t,
                            const float* xyz_dev, int64_t n, long long* acc, double R_out[9], double T_out[3], tsl_track_report* rep, const char* who)
{
    return al_iterate(R0, T0, t, [&](int stride, const double* R, const double* T, tsl_align_sums* s) {
        AlignPointsDev A;
        int rc = points_check(m, R, T, c, xyz_dev, n, R_out, stride, &A, who); if (rc) return rc;
        if ((rc = points_launch(m, q, A, xyz_dev, acc, nullptr, nullptr))) return rc;
        return al_read_back(m, q, acc, sizeof(tsl_align_sums), s);
    }, R_out, T_out, rep);
}

// every level is checked before anything runs
static int track_points_prepare(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_points_cfg* c, const tsl_track_cfg* t, const void* xyz, int64_t n,
                                const void* R_out, const void* T_out, const char* who)
{
    TSL_REQUIRE(m, std::string(who) + ": null handle");
    TSL_REQUIRE(R_out && T_out, std::string(who) + ": null argument");
    int rc = track_check(t, who); if (rc) return rc;
    AlignPointsDev A;
    for (int l = 0; l < t->n_levels; ++l) if ((rc = points_check(m, R0, T0, c, xyz, n, R_out, t->stride[l], &A, who))) return rc;
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_align_points_linearize(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_points_cfg* c, const float* xyz, int64_t n,
                                    tsl_align_sums* out, uint8_t* bucket, float* s)
{
    AlignPointsDev A;
    int rc = points_check(m, R, T, c, xyz, n, out, c ? c->stride : 1, &A, "align_points_linearize"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames
    const int64_t per = (bucket || s) ? A.visited : 0;
    PointsStage st;
    if ((rc = points_stage(m, q, xyz, n, per, &st))) return rc;
    if ((rc = points_launch(m, q, A, st.xyz, st.acc, bucket ? st.bucket : nullptr, s ? st.s : nullptr))) return rc;
    if (s && per) TSL_HIP(hipMemcpyAsync(s, st.s, (size_t)per * sizeof(float), hipMemcpyDeviceToHost, q));
    if (bucket && per) TSL_HIP(hipMemcpyAsync(bucket, st.bucket, (size_t)per, hipMemcpyDeviceToHost, q));
    return al_read_back(m, q, st.acc, sizeof(tsl_align_sums), out);      // waits for q: the per-point copies are done too
}

int tsl_tsdf_align_points_linearize_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_points_cfg* c, const void* xyz_dev, int64_t n,
                                        void* sums_dev, void* bucket_dev, void* s_dev, void* user_stream)
{
    AlignPointsDev A;
    int rc = points_check(m, R, T, c, xyz_dev, n, sums_dev, c ? c->stride : 1, &A, "align_points_linearize_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = points_launch(m, q, A, (const float*)xyz_dev, (long long*)sums_dev, (uint8_t*)bucket_dev, (float*)s_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_tsdf_track_points(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_points_cfg* c, const tsl_track_cfg* t, const float* xyz, int64_t n,
                          double R_out[9], double T_out[3], tsl_track_report* rep)
{
    int rc = track_points_prepare(m, R0, T0, c, t, xyz, n, R_out, T_out, "track_points"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    PointsStage st;
    if ((rc = points_stage(m, q, xyz, n, 0, &st))) return rc;
    return track_points_run(m, q, R0, T0, c, t, st.xyz, n, st.acc, R_out, T_out, rep, "track_points");
}

int tsl_tsdf_track_points_dev(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_points_cfg* c, const tsl_track_cfg* t, const void* xyz_dev, int64_t n,
                              double R_out[9], double T_out[3], tsl_track_report* rep, void* user_stream)
{
    int rc = track_points_prepare(m, R0, T0, c, t, xyz_dev, n, R_out, T_out, "track_points_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;      // the cloud is whatever user_stream has queued for it
    PointsStage st;
    if ((rc = points_stage(m, q, nullptr, n, 0, &st))) return rc;
    return track_points_run(m, q, R0, T0, c, t, (const float*)xyz_dev, n, st.acc, R_out, T_out, rep, "track_points_dev");
}

}  // extern "C"

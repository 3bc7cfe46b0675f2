// tsl_align_rgbd.hip -- depth-and-colour alignment: a registered depth and colour frame against the textured TSDF.  The signed distance of
// tsl_align.hip says nothing in the directions in which the geometry does not change (a flat wall leaves three degrees of freedom, a corridor one);
// the colour the map stores beside every TSDF value does (Bylow, Olsson, Kahl, "Robust camera tracking by combining color and depth measurements",
// ICPR 2014): minimise sum s(R p_i + T)^2 + lambda * sum (Y(R p_i + T) - y_i)^2, Y the trilinear interpolant of the stored luminance, y_i the
// luminance of pixel i.
//
// Definition (tests/track_rgbd_ref.py restates it in numpy and every integer must equal it).  All f32, no contraction, in
// the written order.  The visited pixels, the depth gate, the back-projection, p, the KNOWN test, s and g are those of tsl_align.hip, and the
// geometric sums are exactly its 33 integers.
//   voxel luminance  yv = ((77 r + 150 g) + 29 b) / 256 of the three stored f16 channels converted to f32
//   image luminance  yi = (float)(77 R + 150 G + 29 B) / 65280.0f of the uint8 pixel (the integer is exact)
//   map luminance    Y = tri_value, gY = tri_grad / vs of the eight yv: the same eight corners and the same cell fractions as s
// The colour sums are a second tsl_align_sums; every visited pixel lands in exactly one of its buckets, tested in this order:
//   gate     the geometric gate
//   unknown  the geometric unknown
//   far      not |s| <= r_max (off the surface, where the colour means nothing), or rc = Y - yi is not |rc| <= rc_max (a NaN is far)
//   grad     (gY0 gY0 + gY1 gY1) + gY2 gY2 is not in (0, gc_max * gc_max]
//   used     J = (gY, p x gY), wgt = al_weight(rc, huber_c) and the 28 products of tsl_align.hip with rc in place of s, added as rint(x * 2^20)
// The colour buckets do not depend on the geometric grad.  A stored colour that is not finite makes Y or gY a NaN or an inf, so its samples are
// colour-far or colour-grad: no such value reaches a product, and the geometric half never sees a colour.
//
// The tiling is k_align_linearize's: one lane per visited pixel, 8 x 8 per wave, 256 threads.  The cell read issues all 24 gathers of a sample (tw,
// obs and one 8-byte colour per corner) before any is used: still two dependent latencies per sample.  The two sets of 28 sums never live at once
// -- 32 int64 are 64 VGPRs -- : the colour bucket, rc and gY (five registers) are kept, the geometric half is formed and flushed (al_flush), a
// barrier frees al_flush's LDS, and the colour half is formed in the same registers and flushed into acc + 40.  flags bit 0 leaves both sets of
// products and their reductions out (the counts as usual).
#include <cmath>
#include "tsl_align_common.hpp"
#include "tsl_align_image.hpp"

namespace tsl {

struct AlignRgbdDev {
    AlignDev a;
    float rc_max, gcm2, huber_c;       // gcm2 = gc_max * gc_max
};

__global__ void __launch_bounds__(256) k_align_rgbd_linearize(MapDev M, int s, AlignRgbdDev A, const uint16_t* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                                              long long* __restrict__ acc)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ii = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), jj = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    float sv = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f }, p[3] = { 0.0f, 0.0f, 0.0f }, rc = 0.0f, gY[3] = { 0.0f, 0.0f, 0.0f };
    int i, j, bucket = al_pixel(A.a, depth, ii, jj, &i, &j, p);   // -1: not a visited pixel
    int cb = bucket;                                              // the colour bucket
    if (bucket == AL_USED) {
        const uint8_t* c = rgb + ((size_t)j * A.a.w + i) * 3;
        const float yi = (float)(77 * (int)c[0] + 150 * (int)c[1] + 29 * (int)c[2]) / 65280.0f;
        bucket = al_sample_lum(p, M, M.table + (size_t)s * M.nb3, A.a.vs, A.a.r_max, A.a.gm2, yi, A.rc_max, A.gcm2, &sv, g, &cb, &rc, gY);
    }
    const bool sums = !(A.a.flags & 1);
    const bool used = bucket == AL_USED, cused = cb == AL_USED;
    const unsigned long long mu = __ballot(used), mc = __ballot(cused);
    long long v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = 0;
    if (used && sums) al_products(p, g, sv, A.a.huber, v);
    al_flush(v, popc64(mu), popc64(__ballot(bucket == AL_GATE)), popc64(__ballot(bucket == AL_UNKNOWN)), popc64(__ballot(bucket == AL_FAR)),
             popc64(__ballot(bucket == AL_GRAD)), mu && sums, acc);
    __syncthreads();                                              // al_flush's LDS has been read: the second flush may write it
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = 0;
    if (cused && sums) al_products(p, gY, rc, A.huber_c, v);
    al_flush(v, popc64(mc), popc64(__ballot(cb == AL_GATE)), popc64(__ballot(cb == AL_UNKNOWN)), popc64(__ballot(cb == AL_FAR)),
             popc64(__ballot(cb == AL_GRAD)), mc && sums, acc + AL_SLOTS);
}

// the checks and defaults every form shares: align_check, then the colour half's own
static int rgbd_check(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_rgbd_cfg* c, const void* depth, const void* rgb, const void* out, int stride,
                      AlignRgbdDev* A, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c && rgb, w + ": null argument");
    int rc = align_check(m, R, T, &c->a, depth, out, stride, &A->a, who); if (rc) return rc;
    TSL_REQUIRE(m->M.col, w + ": the map is not textured");
    TSL_REQUIRE(std::isfinite(c->rc_max) && std::isfinite(c->gc_max) && std::isfinite(c->huber_c), w + ": rc_max / gc_max / huber_c is not finite");
    TSL_REQUIRE(!(c->rc_max < 0.0f) && !(c->gc_max < 0.0f) && !(c->huber_c < 0.0f), w + ": rc_max, gc_max and huber_c must not be negative");
    A->rc_max = c->rc_max != 0.0f ? c->rc_max : 1.0f;
    const float gcmax = c->gc_max != 0.0f ? c->gc_max : 1.0f / A->a.vs;
    A->gcm2 = gcmax * gcmax;
    A->huber_c = c->huber_c;
    // the bound of align_check for the colour half: |gY_a| <= gc_max, |p_a| <= L, |rc| <= rc_max
    const double L = (double)(m->M.hN > m->M.hNz ? m->M.hN : m->M.hNz) * m->cfg.voxel_scale;
    double Mc = 2.0 * L * (double)gcmax;
    if ((double)gcmax > Mc) Mc = (double)gcmax;
    if ((double)A->rc_max > Mc) Mc = (double)A->rc_max;
    const double visited = (double)A->a.hh * (double)A->a.ww;
    TSL_REQUIRE(Mc * Mc * 1048576.0 * visited <= 4611686018427387904.0, w + ": the colour sums could overflow (max(2 L gc_max, rc_max)^2 * 2^20 * visited pixels exceeds 2^62)");
    return TSL_OK;
}

// zeroes the accumulator (80 slots: geo | col) and launches, both on q
static int rgbd_launch(tsl_tsdf* m, hipStream_t q, const AlignRgbdDev& A, const uint16_t* depth, const uint8_t* rgb, long long* acc)
{
    TSL_HIP(hipMemsetAsync(acc, 0, 2 * AL_SLOTS * sizeof(long long), q));
    prof_begin(m, TSL_K_ALIGN_RGBD, q);
    hipLaunchKernelGGL(k_align_rgbd_linearize, dim3((unsigned)((A.a.ww + 15) / 16), (unsigned)((A.a.hh + 15) / 16)), dim3(256), 0, q, m->M,
                       m->cfg.is_global_map ? 0 : m->active, A, depth, rgb, acc);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// one linearisation on q with the result on the host: launch, copy the 80 slots back through the pinned buffer, wait
static int rgbd_run(tsl_tsdf* m, hipStream_t q, const AlignRgbdDev& A, const uint16_t* depth_dev, const uint8_t* rgb_dev, long long* acc, tsl_align_rgbd_sums* out)
{
    int rc = rgbd_launch(m, q, A, depth_dev, rgb_dev, acc); if (rc) return rc;
    long long all[2 * AL_SLOTS];
    if ((rc = al_read_back(m, q, acc, sizeof(all), all))) return rc;
    std::memcpy(&out->geo, all, sizeof(tsl_align_sums)); std::memcpy(&out->col, all + AL_SLOTS, sizeof(tsl_align_sums));
    return TSL_OK;
}

// the accumulator and (host form) the staged images in the export staging buffer: [80 x int64 | pad to 1024 | depth | pad to 64 | rgb]
static int rgbd_stage(tsl_tsdf* m, hipStream_t q, const tsl_align_cfg* c, const uint16_t* depth_host, const uint8_t* rgb_host, long long** acc,
                      const uint16_t** depth_dev, const uint8_t** rgb_dev)
{
    const size_t px = (size_t)c->h * c->w, dbytes = (px * sizeof(uint16_t) + 63) & ~(size_t)63;
    int rc = grow(&m->xbuf, &m->xbuf_bytes, 1024 + (depth_host ? dbytes + px * 3 : 0) + 64); if (rc) return rc;
    *acc = (long long*)m->xbuf;
    if (depth_host) {
        char* base = (char*)m->xbuf + 1024;
        TSL_HIP(hipMemcpyAsync(base, depth_host, px * sizeof(uint16_t), hipMemcpyHostToDevice, q));
        TSL_HIP(hipMemcpyAsync(base + dbytes, rgb_host, px * 3, hipMemcpyHostToDevice, q));
        *depth_dev = (const uint16_t*)base; *rgb_dev = (const uint8_t*)(base + dbytes);
    }
    return TSL_OK;
}

// The iteration (al_iterate_with) on the 66 integers; the images are on the device, q has been ordered behind whatever produced them.  An automatic
// lambda is formed at the first linearisation and held.
static int track_rgbd_run(tsl_tsdf* m, hipStream_t q, const double R0[9], const double T0[3], const tsl_align_rgbd_cfg* c, const tsl_track_cfg* t, double lambda,
                          double balance, const uint16_t* depth_dev, const uint8_t* rgb_dev, long long* acc, double R_out[9], double T_out[3],
                          tsl_track_rgbd_report* rep, const char* who)
{
    double lam = lambda;
    const int rc = al_iterate_with<tsl_align_rgbd_sums>(R0, T0, t, [&](int stride, const double* R, const double* T, tsl_align_rgbd_sums* s) {
        AlignRgbdDev A;
        int r = rgbd_check(m, R, T, c, depth_dev, rgb_dev, R_out, stride, &A, who); if (r) return r;
        if ((r = rgbd_run(m, q, A, depth_dev, rgb_dev, acc, s))) return r;
        if (lam < 0.0) {
            const double num = ((double)s->geo.H[0] + (double)s->geo.H[6]) + (double)s->geo.H[11], den = ((double)s->col.H[0] + (double)s->col.H[6]) + (double)s->col.H[11];
            lam = den == 0.0 ? 0.0 : balance * num / den;
        }
        return (int)TSL_OK;
    }, [&](const tsl_align_rgbd_sums* s, double damping, double xi[6]) { return al_solve_rgbd(s, lam, damping, xi); }, R_out, T_out, rep);
    if (rep) rep->lambda = lam < 0.0 ? 0.0 : lam;
    return rc;
}

// every level is checked before anything runs
static int track_rgbd_prepare(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_rgbd_cfg* c, const tsl_track_cfg* t, double lambda, double balance,
                              const void* depth, const void* rgb, const void* R_out, const void* T_out, const char* who)
{
    TSL_REQUIRE(m, std::string(who) + ": null handle");
    TSL_REQUIRE(R_out && T_out, std::string(who) + ": null argument");
    TSL_REQUIRE(std::isfinite(lambda), std::string(who) + ": lambda is not finite");
    TSL_REQUIRE(std::isfinite(balance) && !(balance < 0.0), std::string(who) + ": balance must be finite and not negative");
    int rc = track_check(t, who); if (rc) return rc;
    AlignRgbdDev A;
    for (int l = 0; l < t->n_levels; ++l) if ((rc = rgbd_check(m, R0, T0, c, depth, rgb, R_out, t->stride[l], &A, who))) return rc;
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_align_rgbd_linearize(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_rgbd_cfg* c, const uint16_t* depth, const uint8_t* rgb,
                                  tsl_align_rgbd_sums* out)
{
    AlignRgbdDev A;
    int rc = rgbd_check(m, R, T, c, depth, rgb, out, c ? c->a.stride : 1, &A, "align_rgbd_linearize"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames
    long long* acc; const uint16_t* dd = nullptr; const uint8_t* cd = nullptr;
    if ((rc = rgbd_stage(m, q, &c->a, depth, rgb, &acc, &dd, &cd))) return rc;
    return rgbd_run(m, q, A, dd, cd, acc, out);
}

int tsl_tsdf_align_rgbd_linearize_dev(tsl_tsdf* m, const double R[9], const double T[3], const tsl_align_rgbd_cfg* c, const void* depth_dev, const void* rgb_dev,
                                      void* sums_dev, void* user_stream)
{
    AlignRgbdDev A;
    int rc = rgbd_check(m, R, T, c, depth_dev, rgb_dev, sums_dev, c ? c->a.stride : 1, &A, "align_rgbd_linearize_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = rgbd_launch(m, q, A, (const uint16_t*)depth_dev, (const uint8_t*)rgb_dev, (long long*)sums_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_align_rgbd_solve(const tsl_align_rgbd_sums* s, double lambda, double damping, double xi[6], int32_t* singular)
{
    TSL_REQUIRE(s && xi && singular, "align_rgbd_solve: null argument");
    TSL_REQUIRE(std::isfinite(damping) && !(damping < 0.0), "align_rgbd_solve: damping must be finite and not negative");
    TSL_REQUIRE(std::isfinite(lambda) && !(lambda < 0.0), "align_rgbd_solve: lambda must be finite and not negative");
    *singular = al_solve_rgbd(s, lambda, damping, xi) ? 0 : 1;
    return TSL_OK;
}

int tsl_tsdf_track_rgbd(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_rgbd_cfg* c, const tsl_track_cfg* t, double lambda, double balance,
                        const uint16_t* depth, const uint8_t* rgb, double R_out[9], double T_out[3], tsl_track_rgbd_report* rep)
{
    int rc = track_rgbd_prepare(m, R0, T0, c, t, lambda, balance, depth, rgb, R_out, T_out, "track_rgbd"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    long long* acc; const uint16_t* dd = nullptr; const uint8_t* cd = nullptr;
    if ((rc = rgbd_stage(m, q, &c->a, depth, rgb, &acc, &dd, &cd))) return rc;
    return track_rgbd_run(m, q, R0, T0, c, t, lambda, balance, dd, cd, acc, R_out, T_out, rep, "track_rgbd");
}

int tsl_tsdf_track_rgbd_dev(tsl_tsdf* m, const double R0[9], const double T0[3], const tsl_align_rgbd_cfg* c, const tsl_track_cfg* t, double lambda, double balance,
                            const void* depth_dev, const void* rgb_dev, double R_out[9], double T_out[3], tsl_track_rgbd_report* rep, void* user_stream)
{
    int rc = track_rgbd_prepare(m, R0, T0, c, t, lambda, balance, depth_dev, rgb_dev, R_out, T_out, "track_rgbd_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;      // the images are whatever user_stream has queued for them
    long long* acc;
    if ((rc = rgbd_stage(m, q, &c->a, nullptr, nullptr, &acc, nullptr, nullptr))) return rc;
    return track_rgbd_run(m, q, R0, T0, c, t, lambda, balance, (const uint16_t*)depth_dev, (const uint8_t*)rgb_dev, acc, R_out, T_out, rep, "track_rgbd_dev");
}

}  // extern "C"

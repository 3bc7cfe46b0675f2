// tsl_path_score.hip -- scores batches of candidate paths (polylines of waypoints: MPPI roll-outs, motion primitives, straight lines to view candidates)
// against the ESDF of tsl_esdf.hip in one launch: the consumer tsl_esdf_query.hip names.  The definition is in include/taichislam_hip.h and DESIGN.md
// section 4.13; tests/path_score_ref.py restates it in numpy bit for bit.
//
// One wave per path, four paths per 256-thread workgroup; lane l takes the samples j = 64 c + l of chunk c.  The value and status of a sample are
// esdf_sample's (tsl_esdf_sample.hpp, the one copy k_esdf_query uses too).  Per chunk a ballot of the blocking lanes gives first_stop, popcounts of the
// class ballots under the mask of the counted lanes give the counts; every lane keeps the minimum (key, index) pair and the fixed-point cost of its own
// counted samples, and ONE shuffle reduction behind the last chunk combines them (both are order-free, so this equals a reduction per chunk).  With the
// stop flag the wave leaves behind the chunk that holds first_stop; the branch is wave-uniform (it depends on ballots only).  No LDS, no atomics, no
// scratch, no barrier: the waves of a block never meet.  Read-only on the map.
#include "tsl_esdf_sample.hpp"
#include "tsl_stage.hpp"

namespace tsl {

#define PS_STOP 1
#define PS_UNKNOWN_BLOCKS 2
#define PS_OUTSIDE_BLOCKS 4
#define PS_MAX_N (1 << 20)
#define PS_MAX_K 4096
#define PS_MAX_SUB 256
#define PS_MAX_S (1 << 20)

struct PathDev { int K, sub, smax, flags; float radius, rm, unknown, vs, gamma, maxd; };

// the monotone uint32 image of a float's bits: -0.0 sorts before +0.0
__device__ __forceinline__ uint32_t dist_key(float d) { const uint32_t b = __float_as_uint(d); return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u); }
__device__ __forceinline__ float key_dist(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <int MODE>
__global__ void __launch_bounds__(256) k_path_score(MapDev M, int s, const float* __restrict__ esdf, PathDev W, const int* __restrict__ ctr, int rounds,
                                                    const float* __restrict__ wp, const int* __restrict__ lengths, int n, tsl_path_score* __restrict__ out,
                                                    float* __restrict__ sdist, uint8_t* __restrict__ sstat)
{
    const int lane = threadIdx.x & 63;
    const int path = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (path >= n) return;                                           // whole waves leave; nothing below synchronises the block
    int L = W.K;
    if (lengths) { L = lengths[path]; L = L < 1 ? 1 : (L > W.K ? W.K : L); }      // the device form clamps (the host form has refused already)
    const int S = (L - 1) * W.sub + 1;
    const float* __restrict__ w = wp + (size_t)path * W.K * 3;
    const int* __restrict__ T = M.table + (size_t)s * M.nb3;
    const size_t row = (size_t)path * W.smax;
    int first = -1, ns = 0, nh = 0, nu = 0, no = 0;
    unsigned long long best = ~0ull;                                 // (key << 32 | index) of the lane's counted samples of status 0
    long long cost = 0;
    int j0 = 0;
    for (; j0 < S; j0 += 64) {
        const int j = j0 + lane;
        const bool active = j < S;
        float d = W.unknown;
        int st = EQ_OUTSIDE;
        if (active) {
            const int seg = j / W.sub, m = j - seg * W.sub;
            float x = w[seg * 3], y = w[seg * 3 + 1], z = w[seg * 3 + 2];      // m == 0: the waypoint itself, bit for bit; the next one is not read
            if (m) {
                const float t = (float)m / (float)W.sub;
                x = lerp_f(x, w[seg * 3 + 3], t); y = lerp_f(y, w[seg * 3 + 4], t); z = lerp_f(z, w[seg * 3 + 5], t);
            }
            float g0, g1, g2;                                        // unused: the gradient is dead code here
            bool nan_tsdf;
            st = esdf_sample<MODE>(M, T, esdf, W.gamma, W.maxd, W.vs, W.unknown, x, y, z, &d, &g0, &g1, &g2, &nan_tsdf);
            if (st == 0 && (nan_tsdf || d != d)) { st = EQ_UNKNOWN; d = W.unknown; }      // a NaN TSDF that came in through an import, or a NaN value: unknown
        }
        const bool hit = active && st == 0 && d < W.radius, unk = active && st == EQ_UNKNOWN, outs = active && st == EQ_OUTSIDE;
        const bool blocks = hit || (unk && (W.flags & PS_UNKNOWN_BLOCKS)) || (outs && (W.flags & PS_OUTSIDE_BLOCKS));
        const unsigned long long bb = __ballot(blocks);
        if (first < 0 && bb) first = j0 + __ffsll(bb) - 1;
        const bool stop = (W.flags & PS_STOP) && first >= 0;         // then first lies in this chunk: the wave would have left behind an earlier one
        unsigned long long cm = __ballot(active);
        if (stop) cm &= (2ull << (first - j0)) - 1ull;               // the counted lanes: j <= first_stop
        ns += __popcll(cm);
        nh += __popcll(__ballot(hit) & cm); nu += __popcll(__ballot(unk) & cm); no += __popcll(__ballot(outs) & cm);
        const bool counted = (cm >> lane) & 1ull;
        if (counted && st == 0) {
            const unsigned long long kv = ((unsigned long long)dist_key(d) << 32) | (unsigned)j;
            best = kv < best ? kv : best;
            const float c = fminf(W.rm - d, 1024.0f);
            if (c > 0.0f) cost += (long long)(int)(c * 1048576.0f);
        }
        if (j < W.smax) {                                            // the row of the path: plain coalesced stores
            if (sdist) sdist[row + j] = counted ? d : W.unknown;
            if (sstat) sstat[row + j] = counted ? (uint8_t)st : (uint8_t)0xff;
        }
        if (stop) { j0 += 64; break; }
    }
    if (sdist) for (int j = j0 + lane; j < W.smax; j += 64) sdist[row + j] = W.unknown;      // the uncounted tail of the wave's own row
    if (sstat) for (int j = j0 + lane; j < W.smax; j += 64) sstat[row + j] = (uint8_t)0xff;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long ob = __shfl_xor(best, o);
        best = ob < best ? ob : best;
        cost += __shfl_xor(cost, o);
    }
    if (lane == 0) {
        tsl_path_score r;
        r.n_samples = ns; r.first_stop = first; r.n_hit = nh; r.n_unknown = nu; r.n_outside = no;
        r.argmin = best == ~0ull ? -1 : (int)(unsigned)(best & 0xffffffffull);
        r.min_dist = best == ~0ull ? __uint_as_float(0x7f800000u) : key_dist((uint32_t)(best >> 32));
        r.short_update = esdf_short_flag(ctr, rounds);
        r.cost = cost;
        out[path] = r;
    }
}

// every refusal that does not need the lengths; *go = false for n = 0
static int path_check(tsl_tsdf* m, int mode, const void* waypoints, int64_t n, int K, int sub, float radius, float margin, int flags, float unknown,
                      const void* out, bool sample_out, PathDev* W, bool* go, const char* who)
{
    const std::string w(who);
    *go = false;
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(n >= 0 && n <= PS_MAX_N, w + ": n must lie in 0 .. 2^20");
    TSL_REQUIRE(K >= 1 && K <= PS_MAX_K, w + ": K must lie in 1 .. 4096");
    TSL_REQUIRE(sub >= 1 && sub <= PS_MAX_SUB, w + ": sub must lie in 1 .. 256");
    const int64_t smax = (int64_t)(K - 1) * sub + 1;
    TSL_REQUIRE(smax <= PS_MAX_S, w + ": more than 2^20 samples per path");
    TSL_REQUIRE(!(sample_out && n * smax >= ((int64_t)1 << 31)), w + ": the per-sample outputs hold fewer than 2^31 entries");
    TSL_REQUIRE(std::isfinite(radius) && radius >= 0.0f && std::isfinite(margin) && margin >= 0.0f, w + ": radius and margin must be finite and not negative");
    TSL_REQUIRE((flags & ~(PS_STOP | PS_UNKNOWN_BLOCKS | PS_OUTSIDE_BLOCKS)) == 0, w + ": flags has bits other than 1 (stop), 2 (unknown blocks), 4 (outside blocks)");
    TSL_REQUIRE(n == 0 || (waypoints && out), w + ": null buffer");
    TSL_REQUIRE(mode == 0 || mode == 1, w + ": mode must be 0 (nearest voxel) or 1 (trilinear)");
    const int rc = esdf_read_check(m, who); if (rc) return rc;
    W->K = K; W->sub = sub; W->smax = (int)smax; W->flags = flags; W->radius = radius; W->rm = radius + margin; W->unknown = unknown;
    W->vs = m->P.vs; W->gamma = m->esdf_gamma; W->maxd = m->esdf_maxd;
    *go = n > 0;
    return TSL_OK;
}

// launched on the handle's stream, behind the latest update (its relaxation rounds may run on another stream: esdf_overlap)
static int path_launch(tsl_tsdf* m, hipStream_t q, int mode, const PathDev& W, const float* wp, const int* lengths, int n, tsl_path_score* out, float* sdist,
                       uint8_t* sstat)
{
    if (m->esdf_last) TSL_HIP(hipStreamWaitEvent(q, m->esdf_last, 0));
    const int s = m->cfg.is_global_map ? 0 : m->active;
    const dim3 grid((unsigned)((n + 3) / 4));
    prof_begin(m, TSL_K_PATH_SCORE, q);
    if (mode == 0) hipLaunchKernelGGL(k_path_score<0>, grid, dim3(256), 0, q, m->M, s, (const float*)m->esdf, W, (const int*)m->esdf_q_ctr, m->esdf_q_rounds, wp,
                                      lengths, n, out, sdist, sstat);
    else hipLaunchKernelGGL(k_path_score<1>, grid, dim3(256), 0, q, m->M, s, (const float*)m->esdf, W, (const int*)m->esdf_q_ctr, m->esdf_q_rounds, wp, lengths, n,
                            out, sdist, sstat);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_esdf_score_paths(tsl_tsdf* m, int mode, float unknown_value, const float* waypoints, const int32_t* lengths, int64_t n, int32_t K, int32_t sub,
                         float radius, float margin, int32_t flags, tsl_path_score* out, float* sample_dist, uint8_t* sample_status)
{
    PathDev W; bool go;
    int rc = path_check(m, mode, waypoints, n, K, sub, radius, margin, flags, unknown_value, out, sample_dist || sample_status, &W, &go, "esdf_score_paths");
    if (rc) return rc;
    if (lengths) for (int64_t i = 0; i < n; ++i) TSL_REQUIRE(lengths[i] >= 1 && lengths[i] <= K, "esdf_score_paths: a length outside 1 .. K");
    if (!go) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    if ((rc = esdf_finish(m))) return rc;                      // the values handed out are the fixed point of the last update
    const hipStream_t q = ms(m);
    const size_t c = (size_t)n, rows = c * (size_t)W.smax;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_wp = st.in(waypoints, c * (size_t)K * 12), i_len = st.in(lengths, c * 4), i_out = st.out(out, c * sizeof(tsl_path_score)),
              i_sd = st.out(sample_dist, rows * 4), i_ss = st.out(sample_status, rows);
    if ((rc = st.upload())) return rc;
    if ((rc = path_launch(m, q, mode, W, st.ptr<const float>(i_wp), st.ptr<const int>(i_len), (int)n, st.ptr<tsl_path_score>(i_out), st.ptr<float>(i_sd),
                          st.ptr<uint8_t>(i_ss)))) return rc;
    return st.download();
}

int tsl_esdf_score_paths_dev(tsl_tsdf* m, int mode, float unknown_value, const void* waypoints_dev, const void* lengths_dev, int64_t n, int32_t K, int32_t sub,
                             float radius, float margin, int32_t flags, void* out_dev, void* sample_dist_dev, void* sample_status_dev, void* user_stream)
{
    PathDev W; bool go;
    int rc = path_check(m, mode, waypoints_dev, n, K, sub, radius, margin, flags, unknown_value, out_dev, sample_dist_dev || sample_status_dev, &W, &go,
                        "esdf_score_paths_dev");
    if (rc || !go) return rc;
    TSL_HIP(hipSetDevice(m->device));
    if (m->esdf_short && (rc = esdf_finish(m))) return rc;     // the host already knows an update stopped early: repair it first
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = path_launch(m, q, mode, W, (const float*)waypoints_dev, (const int*)lengths_dev, (int)n, (tsl_path_score*)out_dev, (float*)sample_dist_dev,
                          (uint8_t*)sample_status_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

// tsl_traj_opt.hip -- batches of uniform cubic B-spline trajectories against the ESDF of tsl_esdf.hip: the collision and smoothness costs of every
// trajectory with their gradients over the control points (tsl_esdf_traj_linearize), and a momentum descent on them whose iterations all run inside ONE
// launch (tsl_esdf_traj_optimize).  The definition is in include/taichislam_hip.h and DESIGN.md section 4.22; tests/traj_opt_ref.py restates it in numpy
// bit for bit.
//
// One wave per trajectory, four trajectories per 256-thread workgroup.  The wave keeps its control points, its velocities and the collision gradient
// plane (int64 fixed point) in LDS: 16 bytes per control point and axis, 12 KB at K = 256, sized by K at the launch.  A linearisation strides the lanes
// over the samples in chunks of 64; the value and gradient of a sample are esdf_sample<1>'s (tsl_esdf_sample.hpp, the one copy: a sample has
// query_esdf's bits).  The collision gradient is SCATTERED: a penalised sample adds its twelve fixed-point terms to the four control points of its span
// with 64-bit LDS atomic adds -- the sums are integers, so the order the hardware takes them in does not show.  The smoothness gradient is GATHERED: a
// control point has at most three second-difference terms, which its lane recomputes from the control points in LDS, so that plane needs no LDS at all.
// Counts come from ballots; the minimum (key, index) pair and the two costs from one shuffle reduction per linearisation.  The stop depends on a ballot
// count only, so it is wave-uniform.  The waves of a block never meet: there is no block barrier, whole waves leave early, and a wave orders its own LDS
// traffic with wave_lds_sync().  No global atomics; nothing is written to the map.
#include "tsl_esdf_sample.hpp"
#include "tsl_stage.hpp"

namespace tsl {

#define TO_STOP_FREE 1
#define TO_MAX_N (1 << 20)
#define TO_MIN_K 4
#define TO_MAX_K 256
#define TO_MAX_SUB 64
#define TO_MAX_ITERS 1024
#define TO_LDS_PER_POINT 48                  // 3 axes x (int64 gradient + f32 control point + f32 velocity)

struct TrajDev { int K, sub, iters, fix_head, fix_tail, flags; float clearance, wc, wsm, step, mom, maxmove, unknown, vs, gamma, maxd; };

__device__ __forceinline__ uint32_t traj_key(float d) { const uint32_t b = __float_as_uint(d); return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u); }
__device__ __forceinline__ float traj_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// the words other lanes of this wave wrote to LDS (stores and atomic adds) are complete and visible behind this; no other wave takes part
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float clamp_f(float t, float b) { return fminf(fmaxf(t, -b), b); }
// the 2^-20 fixed point of a gradient term
__device__ __forceinline__ long long traj_q(float t) { return (long long)(int)(clamp_f(t, 1024.0f) * 1048576.0f); }

// the second difference of term t on one axis (c: the wave's control points in LDS)
__device__ __forceinline__ float smooth_a(const float* c, int t, int ax) { return (c[t * 3 + ax] - (c[t * 3 + 3 + ax] + c[t * 3 + 3 + ax])) + c[t * 3 + 6 + ax]; }

// the smoothness gradient of control point i on one axis: the terms t = i, i - 1, i - 2 that exist (0 .. L - 3) and are finite
__device__ __forceinline__ long long smooth_grad(const float* c, int L, int i, int ax)
{
    long long g = 0;
    if (i <= L - 3) { const float a = smooth_a(c, i, ax); if (isfinite(a)) g += traj_q(2.0f * a); }
    if (i >= 1 && i <= L - 2) { const float a = smooth_a(c, i - 1, ax); if (isfinite(a)) g += traj_q(-4.0f * a); }
    if (i >= 2) { const float a = smooth_a(c, i - 2, ax); if (isfinite(a)) g += traj_q(2.0f * a); }
    return g;
}

__global__ void __launch_bounds__(256) k_traj_opt(MapDev M, int s, const float* __restrict__ esdf, TrajDev W, const int* __restrict__ ctr, int rounds,
                                                  const float* __restrict__ ctrl, const int* __restrict__ lengths, int n, float* __restrict__ ctrl_out,
                                                  tsl_traj_score* __restrict__ out, long long* __restrict__ gc_out, long long* __restrict__ gs_out,
                                                  long long* __restrict__ hist)
{
    extern __shared__ long long traj_lds[];                          // [4][K][3] int64, then [4][K][3] f32 twice: every wave has a slice of each
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int traj = blockIdx.x * 4 + wave;
    if (traj >= n) return;                                           // whole waves leave; nothing below synchronises the block
    const int K3 = W.K * 3;
    long long* gc = traj_lds + wave * K3;
    float* c = (float*)(traj_lds + 4 * K3) + wave * K3;
    float* vel = (float*)(traj_lds + 4 * K3) + 4 * K3 + wave * K3;
    int L = W.K;
    if (lengths) { L = lengths[traj]; L = L < TO_MIN_K ? TO_MIN_K : (L > W.K ? W.K : L); }      // the device form clamps (the host form has refused already)
    const int L3 = L * 3, S = (L - 3) * W.sub + 1;
    const size_t base = (size_t)traj * K3;
    const int* __restrict__ T = M.table + (size_t)s * M.nb3;
    for (int e = lane; e < L3; e += 64) { c[e] = ctrl[base + e]; vel[e] = 0.0f; }
    int np = 0, nu = 0, no = 0, k = 0;
    unsigned long long best;
    long long cc, cs;
    for (;;) {
        // ---- linearise the control points as they stand
        for (int e = lane; e < L3; e += 64) gc[e] = 0;
        wave_lds_sync();                                             // the zeros and the control points, before any lane adds to or reads them
        np = 0; nu = 0; no = 0; best = ~0ull; cc = 0; cs = 0;
        for (int j0 = 0; j0 < S; j0 += 64) {
            const int j = j0 + lane;
            const bool active = j < S;
            int st = EQ_OUTSIDE, seg = 0;
            float d = W.unknown, g[3] = { 0.0f, 0.0f, 0.0f }, w[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (active) {
                seg = j / W.sub; seg = seg < L - 4 ? seg : L - 4;
                const int m = j - seg * W.sub;
                const float u = (float)m / (float)W.sub, v = 1.0f - u, u2 = u * u, u3 = u2 * u;
                w[0] = ((v * v) * v) / 6.0f;
                w[1] = ((3.0f * u3 - 6.0f * u2) + 4.0f) / 6.0f;
                w[2] = (((3.0f * u2 - 3.0f * u3) + 3.0f * u) + 1.0f) / 6.0f;
                w[3] = u3 / 6.0f;
                const float* cp = c + seg * 3;
                float p[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) p[a] = ((w[0] * cp[a] + w[1] * cp[3 + a]) + w[2] * cp[6 + a]) + w[3] * cp[9 + a];
                bool nan_tsdf;
                st = esdf_sample<1>(M, T, esdf, W.gamma, W.maxd, W.vs, W.unknown, p[0], p[1], p[2], &d, &g[0], &g[1], &g[2], &nan_tsdf);
                if (st == 0 && (nan_tsdf || !isfinite(d) || !isfinite(g[0]) || !isfinite(g[1]) || !isfinite(g[2]))) { st = EQ_UNKNOWN; d = W.unknown; }
            }
            bool pen = false;
            if (active && st == 0) {
                const unsigned long long kv = ((unsigned long long)traj_key(d) << 32) | (unsigned)j;
                best = kv < best ? kv : best;
                const float cl = fminf(W.clearance - d, 1024.0f);
                if (cl > 0.0f) {
                    pen = true;
                    cc += (long long)((cl * cl) * 1048576.0f);
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float Gp = -((2.0f * cl) * g[a]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const long long q = traj_q(w[i] * Gp);
                            if (q) atomicAdd((unsigned long long*)&gc[(seg + i) * 3 + a], (unsigned long long)q);      // seg + i <= L - 1
                        }
                    }
                }
            }
            np += __popcll(__ballot(pen)); nu += __popcll(__ballot(active && st == EQ_UNKNOWN)); no += __popcll(__ballot(active && st == EQ_OUTSIDE));
        }
        for (int e = lane; e < (L - 2) * 3; e += 64) {               // the smoothness cost: term t = e / 3 = 0 .. L - 3, axis e % 3
            const float a = smooth_a(c, e / 3, e % 3);
            if (isfinite(a)) { const float ac = clamp_f(a, 1024.0f); cs += (long long)((ac * ac) * 1048576.0f); }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const unsigned long long ob = __shfl_xor(best, o);
            best = ob < best ? ob : best;
            cc += __shfl_xor(cc, o);
            cs += __shfl_xor(cs, o);
        }
        wave_lds_sync();                                             // every lane's atomic adds, before any lane reads the plane
        if (hist && lane == 0) { long long* h = hist + ((size_t)traj * (W.iters + 1) + k) * 2; h[0] = cc; h[1] = cs; }
        if (k == W.iters || ((W.flags & TO_STOP_FREE) && np == 0)) break;      // wave-uniform: k, W and a ballot count
        // ---- one step of the descent: every velocity from the old control points first, then the moves
        for (int e = W.fix_head * 3 + lane; e < (L - W.fix_tail) * 3; e += 64) {
            const float gcf = (float)gc[e] * 9.5367431640625e-07f, gsf = (float)smooth_grad(c, L, e / 3, e % 3) * 9.5367431640625e-07f;
            const float gr = W.wc * gcf + W.wsm * gsf;
            float v = W.mom * vel[e] - W.step * gr;
            if (!isfinite(v)) v = 0.0f;
            vel[e] = clamp_f(v, W.maxmove);
        }
        wave_lds_sync();                                             // the gathers above read control points that other lanes move below
        for (int e = W.fix_head * 3 + lane; e < (L - W.fix_tail) * 3; e += 64) c[e] = c[e] + vel[e];
        ++k;
    }
    // ---- the outputs: the last linearisation's record and gradients, the control points, the rest of the history
    if (hist) for (int e = (k + 1) * 2 + lane; e < (W.iters + 1) * 2; e += 64) hist[(size_t)traj * (W.iters + 1) * 2 + e] = -1;
    if (ctrl_out) for (int e = lane; e < K3; e += 64) ctrl_out[base + e] = e < L3 ? c[e] : ctrl[base + e];
    if (gc_out) for (int e = lane; e < K3; e += 64) gc_out[base + e] = e < L3 ? gc[e] : 0;
    if (gs_out) for (int e = lane; e < K3; e += 64) gs_out[base + e] = e < L3 ? smooth_grad(c, L, e / 3, e % 3) : 0;
    if (out && lane == 0) {
        tsl_traj_score r;
        r.n_samples = S; r.n_pen = np; r.n_unknown = nu; r.n_outside = no;
        r.argmin = best == ~0ull ? -1 : (int)(unsigned)(best & 0xffffffffull);
        r.min_dist = best == ~0ull ? __uint_as_float(0x7f800000u) : traj_unkey((uint32_t)(best >> 32));
        r.short_update = esdf_short_flag(ctr, rounds);
        r.iters_done = k;
        r.cost_collision = cc; r.cost_smooth = cs;
        out[traj] = r;
    }
}

static bool ok_f(float x) { return std::isfinite(x) && x >= 0.0f; }

// every refusal that does not need the lengths; *go = false for n = 0
static int traj_check(tsl_tsdf* m, const void* ctrl, int64_t n, int K, const tsl_traj_opt* o, float unknown, bool need_ctrl_out, const void* ctrl_out,
                      TrajDev* W, bool* go, const char* who)
{
    const std::string w(who);
    *go = false;
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(o, w + ": null parameters");
    TSL_REQUIRE(n >= 0 && n <= TO_MAX_N, w + ": n must lie in 0 .. 2^20");
    TSL_REQUIRE(K >= TO_MIN_K && K <= TO_MAX_K, w + ": K must lie in 4 .. 256");
    TSL_REQUIRE(o->sub >= 1 && o->sub <= TO_MAX_SUB, w + ": sub must lie in 1 .. 64");
    TSL_REQUIRE(o->iters >= 0 && o->iters <= TO_MAX_ITERS, w + ": iters must lie in 0 .. 1024");
    TSL_REQUIRE(ok_f(o->clearance), w + ": clearance must be finite and not negative");
    TSL_REQUIRE(ok_f(o->w_collision) && ok_f(o->w_smooth) && ok_f(o->step) && ok_f(o->momentum) && ok_f(o->max_move),
                w + ": the weights, step, momentum and max_move must be finite and not negative");
    TSL_REQUIRE(o->fix_head >= 0 && o->fix_tail >= 0 && (int64_t)o->fix_head + o->fix_tail <= K, w + ": fix_head and fix_tail must be >= 0 and sum to at most K");
    TSL_REQUIRE((o->flags & ~TO_STOP_FREE) == 0, w + ": flags has bits other than 1 (stop at the first free linearisation)");
    TSL_REQUIRE(n == 0 || (ctrl && (ctrl_out || !need_ctrl_out)), w + ": null buffer");
    const int rc = esdf_read_check(m, who); if (rc) return rc;
    W->K = K; W->sub = o->sub; W->iters = o->iters; W->fix_head = o->fix_head; W->fix_tail = o->fix_tail; W->flags = o->flags;
    W->clearance = o->clearance; W->wc = o->w_collision; W->wsm = o->w_smooth; W->step = o->step; W->mom = o->momentum; W->maxmove = o->max_move;
    W->unknown = unknown; W->vs = m->P.vs; W->gamma = m->esdf_gamma; W->maxd = m->esdf_maxd;
    *go = n > 0;
    return TSL_OK;
}

static tsl_traj_opt linearize_only(int sub, float clearance)
{
    tsl_traj_opt o = {};
    o.clearance = clearance; o.sub = sub;
    return o;
}

// launched on the handle's stream, behind the latest update (its relaxation rounds may run on another stream: esdf_overlap)
static int traj_launch(tsl_tsdf* m, hipStream_t q, const TrajDev& W, const float* ctrl, const int* lengths, int n, float* ctrl_out, tsl_traj_score* out,
                       long long* gc, long long* gs, long long* hist)
{
    if (m->esdf_last) TSL_HIP(hipStreamWaitEvent(q, m->esdf_last, 0));
    const int s = m->cfg.is_global_map ? 0 : m->active;
    const dim3 grid((unsigned)((n + 3) / 4));
    const size_t lds = (size_t)4 * W.K * TO_LDS_PER_POINT;           // at most 48 KB
    hipLaunchKernelGGL(k_traj_opt, grid, dim3(256), lds, q, m->M, s, (const float*)m->esdf, W, (const int*)m->esdf_q_ctr, m->esdf_q_rounds, ctrl, lengths, n,
                       ctrl_out, out, gc, gs, hist);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

static int traj_host(tsl_tsdf* m, const TrajDev& W, const float* ctrl, const int32_t* lengths, int64_t n, float* ctrl_out, tsl_traj_score* out, int64_t* gc,
                     int64_t* gs, int64_t* hist)
{
    TSL_HIP(hipSetDevice(m->device));
    int rc;
    if ((rc = esdf_finish(m))) return rc;                      // the values read are the fixed point of the last update
    const hipStream_t q = ms(m);
    const size_t c = (size_t)n, plane = c * (size_t)W.K * 3;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_c = st.in(ctrl, plane * 4), i_len = st.in(lengths, c * 4), i_co = st.out(ctrl_out, plane * 4), i_out = st.out(out, c * sizeof(tsl_traj_score)),
              i_gc = st.out(gc, plane * 8), i_gs = st.out(gs, plane * 8), i_h = st.out(hist, c * (size_t)(W.iters + 1) * 16);
    if ((rc = st.upload())) return rc;
    if ((rc = traj_launch(m, q, W, st.ptr<const float>(i_c), st.ptr<const int>(i_len), (int)n, st.ptr<float>(i_co), st.ptr<tsl_traj_score>(i_out),
                          st.ptr<long long>(i_gc), st.ptr<long long>(i_gs), st.ptr<long long>(i_h)))) return rc;
    return st.download();
}

static int traj_dev(tsl_tsdf* m, const TrajDev& W, const void* ctrl, const void* lengths, int64_t n, void* ctrl_out, void* out, void* gc, void* gs, void* hist,
                    void* user_stream)
{
    TSL_HIP(hipSetDevice(m->device));
    int rc;
    if (m->esdf_short && (rc = esdf_finish(m))) return rc;     // the host already knows an update stopped early: repair it first
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = traj_launch(m, q, W, (const float*)ctrl, (const int*)lengths, (int)n, (float*)ctrl_out, (tsl_traj_score*)out, (long long*)gc, (long long*)gs,
                          (long long*)hist))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

static int lengths_check(const int32_t* lengths, int64_t n, int K, const char* who)
{
    if (lengths) for (int64_t i = 0; i < n; ++i) TSL_REQUIRE(lengths[i] >= TO_MIN_K && lengths[i] <= K, std::string(who) + ": a length outside 4 .. K");
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_esdf_traj_linearize(tsl_tsdf* m, float unknown_value, const float* ctrl, const int32_t* lengths, int64_t n, int32_t K, int32_t sub, float clearance,
                            tsl_traj_score* out, int64_t* grad_collision, int64_t* grad_smooth)
{
    const tsl_traj_opt o = linearize_only(sub, clearance);
    TrajDev W; bool go;
    int rc = traj_check(m, ctrl, n, K, &o, unknown_value, false, nullptr, &W, &go, "esdf_traj_linearize");
    if (rc || (rc = lengths_check(lengths, n, K, "esdf_traj_linearize")) || !go) return rc;
    return traj_host(m, W, ctrl, lengths, n, nullptr, out, grad_collision, grad_smooth, nullptr);
}

int tsl_esdf_traj_linearize_dev(tsl_tsdf* m, float unknown_value, const void* ctrl_dev, const void* lengths_dev, int64_t n, int32_t K, int32_t sub,
                                float clearance, void* out_dev, void* grad_collision_dev, void* grad_smooth_dev, void* user_stream)
{
    const tsl_traj_opt o = linearize_only(sub, clearance);
    TrajDev W; bool go;
    const int rc = traj_check(m, ctrl_dev, n, K, &o, unknown_value, false, nullptr, &W, &go, "esdf_traj_linearize_dev");
    if (rc || !go) return rc;
    return traj_dev(m, W, ctrl_dev, lengths_dev, n, nullptr, out_dev, grad_collision_dev, grad_smooth_dev, nullptr, user_stream);
}

int tsl_esdf_traj_optimize(tsl_tsdf* m, float unknown_value, const float* ctrl, const int32_t* lengths, int64_t n, int32_t K, const tsl_traj_opt* opt,
                           float* ctrl_out, tsl_traj_score* out, int64_t* history)
{
    TrajDev W; bool go;
    int rc = traj_check(m, ctrl, n, K, opt, unknown_value, true, ctrl_out, &W, &go, "esdf_traj_optimize");
    if (rc || (rc = lengths_check(lengths, n, K, "esdf_traj_optimize")) || !go) return rc;
    return traj_host(m, W, ctrl, lengths, n, ctrl_out, out, nullptr, nullptr, history);
}

int tsl_esdf_traj_optimize_dev(tsl_tsdf* m, float unknown_value, const void* ctrl_dev, const void* lengths_dev, int64_t n, int32_t K, const tsl_traj_opt* opt,
                               void* ctrl_out_dev, void* out_dev, void* history_dev, void* user_stream)
{
    TrajDev W; bool go;
    const int rc = traj_check(m, ctrl_dev, n, K, opt, unknown_value, true, ctrl_out_dev, &W, &go, "esdf_traj_optimize_dev");
    if (rc || !go) return rc;
    return traj_dev(m, W, ctrl_dev, lengths_dev, n, ctrl_out_dev, out_dev, nullptr, nullptr, history_dev, user_stream);
}

}  // extern "C"

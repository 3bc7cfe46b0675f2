// tsl_align_common.hpp -- the one copy of what the Gauss-Newton family shares: the frame-to-model alignment (tsl_align.hip), the
// depth-and-colour alignment (tsl_align_rgbd.hip, section 4.8.2: al_sample_lum, al_solve_rgbd, al_iterate_with over its 66 integers), the
// map-to-map registration (tsl_register.hip, section 4.9) and the pose scoring (tsl_register_search.hip, section 4.10).  Device side, the bit-exact
// contract that tests/track_ref.py restates (points, robust_weight): al_sample carries a map-frame point into its bucket, al_weight is the robust
// weight, al_products adds the 28 fixed-point products of a used sample, al_flush reduces them over the workgroup (the halving butterfly, LDS, one
// integer atomic per non-zero sum).  Host side: the float64 step and the Cayley retraction in their fixed order (tests/track_ref.py restates both),
// the checks of a tsl_track_cfg, the iteration over its levels and the copy of a result through the pinned buffer.
#pragma once
#include <cmath>
#include "tsl_interp.hpp"

namespace tsl {

#define AL_SLOTS 40                    // int64 slots of the device accumulator: 33 used (tsl_align_sums), the rest stay 0
#define AL_NPROD 28
#define AL_SCALE 1048576.0f            // 2^20
#define AL_USED 0
#define AL_GATE 1
#define AL_UNKNOWN 2
#define AL_FAR 3
#define AL_GRAD 4

// rint(x * 2^20) as an integer.  The product is exact in f32 (a power of two; the overflow refusal keeps it far below 2^63), so this is
// (int64) rint((double)x * 2^20).
__device__ __forceinline__ long long al_fix(float x)
{
    const float q = rintf(x * AL_SCALE);
    if (fabsf(q) < 2147483648.0f) return (long long)(int)q;
    return (long long)q;
}

// one halving step of the wave reduction: v[0 .. N-1] of this lane and of lane ^ D become v[0 .. N/2-1], the sums of the half this lane keeps
template <int N, int D>
__device__ __forceinline__ void al_halve(long long (&v)[32], int lane)
{
    const bool up = (lane & D) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const long long keep = up ? v[i + N / 2] : v[i], send = up ? v[i] : v[i + N / 2];
        v[i] = keep + __shfl_xor(send, D);
    }
}

// The bucket of the sample at the map-frame point p -- AL_UNKNOWN, AL_FAR, AL_GRAD or AL_USED -- and, for a used one, the interpolant *s and its
// gradient g per metre.  T: the table of the map's submap; gm2 = g_max * g_max.  The f32 expressions and their order are the contract.
__device__ __forceinline__ int al_sample(const float p[3], const MapDev& M, const int* __restrict__ T, float vs, float r_max, float gm2, float* s, float g[3])
{
    float u[3]; int b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { u[a] = p[a] / vs; b[a] = cell_floor(u[a]); }
    float V[8];
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && tsdf_read_cell(M, T, b[0], b[1], b[2], V))) return AL_UNKNOWN;
    const float f0 = u[0] - (float)b[0], f1 = u[1] - (float)b[1], f2 = u[2] - (float)b[2];
    *s = tri_value(V, f0, f1, f2);
    if (!(fabsf(*s) <= r_max)) return AL_FAR;                     // a NaN interpolant (a stored value that is not finite) is far
    tri_grad(V, f0, f1, f2, &g[0], &g[1], &g[2]);
    g[0] = g[0] / vs; g[1] = g[1] / vs; g[2] = g[2] / vs;
    const float gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    return (gg > 0.0f && gg <= gm2) ? AL_USED : AL_GRAD;          // a NaN or inf gradient is grad: no value that is not finite reaches a product
}

// al_sample over a textured map with the colour bucket beside the geometric one (the return value, exactly al_sample's): *cb is AL_UNKNOWN, AL_FAR,
// AL_GRAD or AL_USED in the order of DESIGN.md section 4.8.2, and for a colour-used sample *rc = Y - yi and gY is the luminance gradient per metre.
// yi: the luminance of the pixel; gcm2 = gc_max * gc_max.  The colour bucket does not depend on the geometric AL_GRAD.
__device__ __forceinline__ int al_sample_lum(const float p[3], const MapDev& M, const int* __restrict__ T, float vs, float r_max, float gm2, float yi, float rc_max,
                                             float gcm2, float* s, float g[3], int* cb, float* rc, float gY[3])
{
    float u[3]; int b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { u[a] = p[a] / vs; b[a] = cell_floor(u[a]); }
    float V[8], Y[8];
    *cb = AL_UNKNOWN;
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && tsdf_read_cell_lum(M, T, b[0], b[1], b[2], V, Y))) return AL_UNKNOWN;
    const float f0 = u[0] - (float)b[0], f1 = u[1] - (float)b[1], f2 = u[2] - (float)b[2];
    *s = tri_value(V, f0, f1, f2);
    *cb = AL_FAR;
    if (!(fabsf(*s) <= r_max)) return AL_FAR;                     // off the surface the colour means nothing
    tri_grad(V, f0, f1, f2, &g[0], &g[1], &g[2]);
    g[0] = g[0] / vs; g[1] = g[1] / vs; g[2] = g[2] / vs;
    const float gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    const int bucket = (gg > 0.0f && gg <= gm2) ? AL_USED : AL_GRAD;
    *rc = tri_value(Y, f0, f1, f2) - yi;
    if (fabsf(*rc) <= rc_max) {                                   // a NaN residual (a stored colour that is not finite) is far
        tri_grad(Y, f0, f1, f2, &gY[0], &gY[1], &gY[2]);
        gY[0] = gY[0] / vs; gY[1] = gY[1] / vs; gY[2] = gY[2] / vs;
        const float cg = (gY[0] * gY[0] + gY[1] * gY[1]) + gY[2] * gY[2];
        *cb = (cg > 0.0f && cg <= gcm2) ? AL_USED : AL_GRAD;
    }
    return bucket;
}

// the robust weight of the residual r
__device__ __forceinline__ float al_weight(float r, float huber)
{
    const float ar = fabsf(r);
    return (huber > 0.0f && ar > huber) ? huber / ar : 1.0f;
}

// adds the 28 products of a used sample to v: H_ab = wJ[a] J[b] (a <= b) in v[0 .. 20], b_a = wJ[a] r in v[21 .. 26], e = (wgt r) r in v[27]
__device__ __forceinline__ void al_products(const float p[3], const float g[3], float r, float huber, long long (&v)[32])
{
    const float J[6] = { g[0], g[1], g[2], p[1] * g[2] - p[2] * g[1], p[2] * g[0] - p[0] * g[2], p[0] * g[1] - p[1] * g[0] };
    const float wgt = al_weight(r, huber);
    float wJ[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) wJ[a] = wgt * J[a];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) v[k++] += al_fix(wJ[a] * J[c]);
#pragma unroll
    for (int a = 0; a < 6; ++a) v[21 + a] += al_fix(wJ[a] * r);
    v[27] += al_fix((wgt * r) * r);
}

// The end of a linearisation kernel of 256 threads: the sums v of every lane and the five counts of every wave (uniform in the wave) are added into
// acc[0 .. 32].  A kernel that flushes twice (tsl_align_rgbd.hip) puts a barrier between the calls: they share this LDS.  reduce: some lane of this wave holds products (it used a sample and the sums are wanted); otherwise v is zero and the butterfly is
// left out.  After the five halving steps lane l holds sum number l >> 1 over its half of the wave, the last step adds the other half.
__device__ __forceinline__ void al_flush(long long (&v)[32], int n_used, int n_gate, int n_unknown, int n_far, int n_grad, bool reduce, long long* __restrict__ acc)
{
    __shared__ long long sm[4][32];
    __shared__ int sc[4][8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (reduce) {
        al_halve<32, 32>(v, lane); al_halve<16, 16>(v, lane); al_halve<8, 8>(v, lane); al_halve<4, 4>(v, lane); al_halve<2, 2>(v, lane);
        v[0] += __shfl_xor(v[0], 1);
    }
    if (!(lane & 1)) sm[wave][lane >> 1] = v[0];
    if (lane == 0) { sc[wave][AL_USED] = n_used; sc[wave][AL_GATE] = n_gate; sc[wave][AL_UNKNOWN] = n_unknown; sc[wave][AL_FAR] = n_far; sc[wave][AL_GRAD] = n_grad; }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < AL_NPROD + 5) {
        long long sum;
        if (t < AL_NPROD) sum = (sm[0][t] + sm[1][t]) + (sm[2][t] + sm[3][t]);
        else { const int c = t - AL_NPROD; sum = ((long long)sc[0][c] + sc[1][c]) + ((long long)sc[2][c] + sc[3][c]); }      // widened before the additions
        if (sum != 0) __hip_atomic_fetch_add(acc + t, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static bool al_finite(const double* a, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false; return true; }

static long long* al_pinned(tsl_tsdf* m) { return reinterpret_cast<long long*>(m->h_ints + 128); }      // the upper part of the pinned scratch: room for 192 x int64

// `bytes` (at most 192 x int64; the widest reader takes 80) at `dev` to `out` on the host: through the pinned buffer on q; q is idle when it returns
static int al_read_back(tsl_tsdf* m, hipStream_t q, const void* dev, size_t bytes, void* out)
{
    TSL_HIP(hipMemcpyAsync(al_pinned(m), dev, bytes, hipMemcpyDeviceToHost, q));
    TSL_HIP(hipStreamSynchronize(q));
    std::memcpy(out, al_pinned(m), bytes);
    return TSL_OK;
}

// ---- the step and the retraction: host code, float64, in this order (tests/track_ref.py restates both) ----

static void al_system(const tsl_align_sums* s, double damping, double Hm[6][6], double b[6])
{
    int k = 0;
    for (int a = 0; a < 6; ++a) for (int c = a; c < 6; ++c) { const double x = (double)s->H[k++] * (1.0 / 1048576.0); Hm[a][c] = x; Hm[c][a] = x; }
    for (int a = 0; a < 6; ++a) { b[a] = (double)s->b[a] * (1.0 / 1048576.0); Hm[a][a] += damping * Hm[a][a]; }
}

// Hm = L L^T by Cholesky without pivoting, column by column (only the lower triangle of Lm is written); false when a pivot is <= 0 or not finite.
// Host and device: the pose graph (tsl_pose_graph.hip) factors its 6 x 6 blocks with the elimination order of the trackers.
__host__ __device__ static inline bool al_cholesky(const double Hm[6][6], double Lm[6][6])
{
    for (int j = 0; j < 6; ++j) {
        double d = Hm[j][j];
        for (int k = 0; k < j; ++k) d -= Lm[j][k] * Lm[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        Lm[j][j] = std::sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double t = Hm[i][j];
            for (int k = 0; k < j; ++k) t -= Lm[i][k] * Lm[j][k];
            Lm[i][j] = t / Lm[j][j];
        }
    }
    return true;
}

// x = (L L^T)^-1 c: L y = c forwards, L^T x = y backwards
__host__ __device__ static inline void al_cholesky_solve(const double Lm[6][6], const double c[6], double x[6])
{
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double t = c[i];
        for (int k = 0; k < i; ++k) t -= Lm[i][k] * y[k];
        y[i] = t / Lm[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double t = y[i];
        for (int k = i + 1; k < 6; ++k) t -= Lm[k][i] * x[k];
        x[i] = t / Lm[i][i];
    }
}

// xi = -H^-1 b of a ready system; false (xi = 0) when a pivot is <= 0 or not finite
static bool al_solve_system(const double Hm[6][6], const double b[6], double xi[6])
{
    double Lm[6][6], nb[6], x[6];
    for (int a = 0; a < 6; ++a) { xi[a] = 0.0; nb[a] = -b[a]; }
    if (!al_cholesky(Hm, Lm)) return false;
    al_cholesky_solve(Lm, nb, x);
    for (int a = 0; a < 6; ++a) if (!std::isfinite(x[a])) return false;
    for (int a = 0; a < 6; ++a) xi[a] = x[a];
    return true;
}

static bool al_solve(const tsl_align_sums* s, double damping, double xi[6])
{
    double Hm[6][6], b[6];
    al_system(s, damping, Hm, b);
    return al_solve_system(Hm, b, xi);
}

// the system of the depth-and-colour step: Hd = Hg * 2^-20 + lambda * (Hc * 2^-20), bd likewise, then the damping
static bool al_solve_rgbd(const tsl_align_rgbd_sums* s, double lambda, double damping, double xi[6])
{
    double Hg[6][6], bg[6], Hc[6][6], bc[6];
    al_system(&s->geo, 0.0, Hg, bg); al_system(&s->col, 0.0, Hc, bc);
    for (int a = 0; a < 6; ++a) {
        for (int c = 0; c < 6; ++c) Hg[a][c] = Hg[a][c] + lambda * Hc[a][c];
        bg[a] = bg[a] + lambda * bc[a];
    }
    for (int a = 0; a < 6; ++a) Hg[a][a] += damping * Hg[a][a];
    return al_solve_system(Hg, bg, xi);
}

static int64_t al_used(const tsl_align_sums& s) { return s.n_used; }
static int64_t al_used(const tsl_align_rgbd_sums& s) { return s.geo.n_used; }                 // colour alone does not fix depth

// the Cayley map of omega = xi[3..5]: R <- C R, T <- C T + v (host and device: the pose graph retracts its poses with it)
__host__ __device__ static inline void al_retract(const double xi[6], double R[9], double T[3])
{
    const double a[3] = { xi[3] * 0.5, xi[4] * 0.5, xi[5] * 0.5 };
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], den = 1.0 + aa;
    const double S[3][3] = { { 0.0, -a[2], a[1] }, { a[2], 0.0, -a[0] }, { -a[1], a[0], 0.0 } };
    double Cm[3][3], Rn[9], Tn[3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Cm[i][j] = (((i == j ? 1.0 - aa : 0.0) + (2.0 * a[i]) * a[j]) + 2.0 * S[i][j]) / den;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = (Cm[i][0] * R[j] + Cm[i][1] * R[3 + j]) + Cm[i][2] * R[6 + j];
        Tn[i] = ((Cm[i][0] * T[0] + Cm[i][1] * T[1]) + Cm[i][2] * T[2]) + xi[i];
    }
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    for (int i = 0; i < 3; ++i) T[i] = Tn[i];
}

static int track_check(const tsl_track_cfg* t, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(t, w + ": null argument");
    TSL_REQUIRE(t->n_levels >= 1 && t->n_levels <= 4, w + ": 1 .. 4 levels");
    int total = 0;
    for (int l = 0; l < t->n_levels; ++l) {
        TSL_REQUIRE(t->stride[l] >= 1, w + ": stride must be at least 1");
        TSL_REQUIRE(t->iters[l] >= 0 && t->iters[l] <= 64, w + ": at most 64 iterations");
        total += t->iters[l];
    }
    TSL_REQUIRE(total <= 64, w + ": at most 64 iterations");
    TSL_REQUIRE(t->min_used >= 0, w + ": min_used must not be negative");
    TSL_REQUIRE(std::isfinite(t->min_step) && std::isfinite(t->damping) && !(t->min_step < 0.0) && !(t->damping < 0.0), w + ": min_step and damping must be finite and not negative");
    return TSL_OK;
}

// The iteration over the levels of a checked tsl_track_cfg, for any sums type (al_used gives its count) and its report.  lin(stride, R, T, &sums)
// linearises at the float64 pose (R, T) and returns an error code; solve(&sums, damping, xi) is the step, false when singular.
template <class Sums, class Report, class Lin, class Solve>
static int al_iterate_with(const double R0[9], const double T0[3], const tsl_track_cfg* t, Lin lin, Solve solve, double R_out[9], double T_out[3], Report* rep)
{
    double R[9], T[3], Rl[9], Tl[3];                               // the current pose; the last one that gave a step
    std::memcpy(R, R0, sizeof(R)); std::memcpy(T, T0, sizeof(T)); std::memcpy(Rl, R0, sizeof(Rl)); std::memcpy(Tl, T0, sizeof(Tl));
    const int64_t min_used = t->min_used > 0 ? t->min_used : 6;
    int n = 0, status = 1;
    bool failed = false;
    for (int l = 0; l < t->n_levels && !failed; ++l) {
        status = 1;
        for (int k = 0; k < t->iters[l]; ++k) {
            Sums s; double xi[6] = { 0, 0, 0, 0, 0, 0 };
            const int rc = lin(t->stride[l], R, T, &s); if (rc) return rc;
            const bool lost = al_used(s) < min_used, singular = !lost && !solve(&s, t->damping, xi);
            if (rep) { auto& it = rep->it[n]; std::memcpy(it.R, R, sizeof(R)); std::memcpy(it.T, T, sizeof(T)); std::memcpy(it.xi, xi, sizeof(xi)); it.sums = s; }
            ++n;
            if (lost || singular) { status = lost ? 2 : 3; failed = true; break; }
            std::memcpy(Rl, R, sizeof(R)); std::memcpy(Tl, T, sizeof(T));
            al_retract(xi, R, T);
            const double n2 = ((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + xi[3] * xi[3]) + xi[4] * xi[4]) + xi[5] * xi[5];
            if (std::sqrt(n2) < t->min_step) { status = 0; break; }
        }
    }
    std::memcpy(R_out, failed ? Rl : R, sizeof(R)); std::memcpy(T_out, failed ? Tl : T, sizeof(T));
    if (rep) { rep->status = status; rep->iterations = n; }
    return TSL_OK;
}

// the iteration on the 33 integers with the step of tsl_align_solve
template <class Lin>
static int al_iterate(const double R0[9], const double T0[3], const tsl_track_cfg* t, Lin lin, double R_out[9], double T_out[3], tsl_track_report* rep)
{
    return al_iterate_with<tsl_align_sums>(R0, T0, t, lin, al_solve, R_out, T_out, rep);
}

}  // namespace tsl

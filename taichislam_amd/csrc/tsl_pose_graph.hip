// tsl_pose_graph.hip -- a pose graph over submap poses, solved once per VARIANT (a bit mask over the edges) in ONE launch: tsl_pgo_linearize and
// tsl_pgo_solve with their _dev forms.  The definition, with the order of every sum, is in include/taichislam_hip.h ("pose graph") and DESIGN.md section
// 4.25; tests/pose_graph_ref.py restates it in numpy bit for bit.
//
// One workgroup of 256 threads per variant, float64 throughout, the whole Levenberg-Marquardt loop inside the launch: evaluate the edges, gather the
// blocks, factor them, preconditioned conjugate gradients, retract, evaluate the trial, accept or reject.  Nothing is scattered and there is no atomic:
// an edge pass writes one record per edge (thread t takes the edges e = t mod 256), a pose pass GATHERS over the pose's incidence list in ascending edge
// index (the host builds the lists once per call), and every reduction is the 256-class sum of pgo_sum.  The vectors of the linear solve live in the
// variant's slice of the workspace (L2-resident: 720 bytes per pose, 56 per edge); the search direction p, the one vector other poses' threads read, is
// in LDS while 48 N bytes fit beside the 2 KB of reduction scratch (N <= 1024) and in the workspace above that.  The workgroups never meet.
#include "tsl_align_common.hpp"
#include "tsl_stage.hpp"

#define PGO_T 256
#define PGO_LDS_POSES 1024                   // p in LDS up to this many poses: 2048 + 48 * 1024 = 51200 bytes
#define PGO_WS_POSE 90                       // doubles of workspace per pose and variant: trial pose 12, Hd 21, factor 21, g x r z Ap p 6 each
#define PGO_WS_EDGE 7                        // per edge and variant: u 6, wgt 1
#define PGO_MAX_N 8192
#define PGO_MAX_E 131072
#define PGO_MAX_B 1024
#define PGO_MAX_PCG 100000
#define PGO_WS_LIMIT ((size_t)1 << 30)

struct tsl_pgo {
    int device, max_n, max_e, max_b;
    hipStream_t stream;
    hipEvent_t ev_in, ev_out, ev_up;         // user -> handle stream, handle stream -> user, "the tables of the last call are uploaded"
    double* ws;                              // [max_b][90 max_n + 7 max_e]
    char* tab; char* h_tab; size_t tab_bytes;      // the tables of a call on the device and their pinned source: ij, lists, masks, fixed, skip
    void* sbuf; size_t sbuf_bytes;           // the staging buffer of the host-pointer forms
};

namespace tsl {

struct PgoDev {
    int N, E, W, iters, pcg_max, p_in_lds, lin_only;
    double damping, up, down, dmin, dmax, tol2, min_step, rel_tol, huber;
    const double *R0, *T0, *Z, *L;
    const int *ij, *inc_ptr, *inc;
    const unsigned long long* masks;
    const uint8_t *fixed, *skip;
    double *R, *T, *r, *c;                   // outputs per variant: [B][N][9], [B][N][3], [B][E][6], [B][E]
    tsl_pgo_report* rep;
    uint8_t* flipped; double *Hd, *g;        // linearize only
    double* ws; size_t ws_stride;
};

// ---- the 6-vector algebra, every sum left to right ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// the residual of an edge and den = 1 + tr(R_D)
__device__ __forceinline__ void pgo_residual(const double* Ra, const double* Ta, const double* Rb, const double* Tb, const double* Z, double r[6], double* den)
{
    double Rx[3][3], RD[3][3], Tx[3];
    const double d0 = Ta[0] - Tb[0], d1 = Ta[1] - Tb[1], d2 = Ta[2] - Tb[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rx[i][j] = dot3(Rb[i], Ra[j], Rb[3 + i], Ra[3 + j], Rb[6 + i], Ra[6 + j]);
        Tx[i] = dot3(Rb[i], d0, Rb[3 + i], d1, Rb[6 + i], d2);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) RD[i][j] = dot3(Rx[i][0], Z[j * 3], Rx[i][1], Z[j * 3 + 1], Rx[i][2], Z[j * 3 + 2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = Tx[i] - dot3(RD[i][0], Z[9], RD[i][1], Z[10], RD[i][2], Z[11]);
    const double dn = 1.0 + ((RD[0][0] + RD[1][1]) + RD[2][2]);
    r[3] = (2.0 * (RD[2][1] - RD[1][2])) / dn;
    r[4] = (2.0 * (RD[0][2] - RD[2][0])) / dn;
    r[5] = (2.0 * (RD[1][0] - RD[0][1])) / dn;
    *den = dn;
}

// the 21 upper-triangle entries (the order of tsl_align_sums.H) times w, as a full symmetric matrix
__device__ __forceinline__ void pgo_full(const double* L21, double w, double Lf[6][6])
{
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) { const double x = w * L21[k++]; Lf[a][c] = x; Lf[c][a] = x; }
}

__device__ __forceinline__ void pgo_matvec(const double Lf[6][6], const double v[6], double m[6])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = ((((Lf[i][0] * v[0] + Lf[i][1] * v[1]) + Lf[i][2] * v[2]) + Lf[i][3] * v[3]) + Lf[i][4] * v[4]) + Lf[i][5] * v[5];
}

__device__ __forceinline__ double pgo_dot6(const double a[6], const double b[6])
{
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}

// ti = -(Rb^T Tb): the translation of P_b^-1
__device__ __forceinline__ void pgo_tinv(const double* Rb, const double* Tb, double ti[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) ti[i] = -dot3(Rb[i], Tb[0], Rb[3 + i], Tb[1], Rb[6 + i], Tb[2]);
}

// o = A d with A = Ad(P_b^-1): (Rb^T v + ti x (Rb^T w), Rb^T w)
__device__ __forceinline__ void pgo_adj(const double* Rb, const double ti[3], const double d[6], double o[6])
{
    double Rv[3], Rw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Rv[i] = dot3(Rb[i], d[0], Rb[3 + i], d[1], Rb[6 + i], d[2]);
        Rw[i] = dot3(Rb[i], d[3], Rb[3 + i], d[4], Rb[6 + i], d[5]);
    }
    o[0] = Rv[0] + (ti[1] * Rw[2] - ti[2] * Rw[1]);
    o[1] = Rv[1] + (ti[2] * Rw[0] - ti[0] * Rw[2]);
    o[2] = Rv[2] + (ti[0] * Rw[1] - ti[1] * Rw[0]);
    o[3] = Rw[0]; o[4] = Rw[1]; o[5] = Rw[2];
}

// u = A^T m: (Rb m_v, Rb (m_w - ti x m_v))
__device__ __forceinline__ void pgo_adj_t(const double* Rb, const double ti[3], const double m[6], double u[6])
{
    const double s0 = m[3] - (ti[1] * m[2] - ti[2] * m[1]), s1 = m[4] - (ti[2] * m[0] - ti[0] * m[2]), s2 = m[5] - (ti[0] * m[1] - ti[1] * m[0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u[i] = dot3(Rb[i * 3], m[0], Rb[i * 3 + 1], m[1], Rb[i * 3 + 2], m[2]);
        u[3 + i] = dot3(Rb[i * 3], s0, Rb[i * 3 + 1], s1, Rb[i * 3 + 2], s2);
    }
}

// The sum of the 256 class partials (thread t holds class t): s[c] += s[c + h] for h = 128 .. 1.  The steps h = 128 and 64 go through LDS; from h = 32 down
// every operand lies in wave 0, which folds in registers: lane c adds lane c + h's value, the same two operands in the same order, so the bits are those of
// the LDS form with four barriers in place of ten.  (Lanes c >= h add on as well; no lane that counts reads them again.)  Every thread gets the sum; s is
// free again on return.
__device__ __forceinline__ double pgo_sum(double v, double* s)
{
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    if (t < 128) s[t] = s[t] + s[t + 128];
    __syncthreads();
    if (t < 64) {
        double a = s[t] + s[t + 64];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) a = a + __shfl_down(a, h);
        if (t == 0) s[0] = a;
    }
    __syncthreads();
    const double out = s[0];
    __syncthreads();
    return out;
}

// the largest of the 256 values (no NaN takes part: a thread keeps the larger by `>`); the order does not show
__device__ __forceinline__ double pgo_max(double v, double* s)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) { const double o = __shfl_xor(v, h); v = o > v ? o : v; }
    if ((t & 63) == 0) s[t >> 6] = v;
    __syncthreads();
    double out = s[0];
#pragma unroll
    for (int w = 1; w < PGO_T / 64; ++w) out = s[w] > out ? s[w] : out;
    __syncthreads();
    return out;
}

// the mask bit of edge e, for a pose pass (the lanes of a wave hold unrelated edges)
__device__ __forceinline__ bool pgo_on(const unsigned long long* mask, int e) { return (mask[e >> 6] >> (e & 63)) & 1ull; }

// One pass over the edges at the poses (R, T): the class partial of the cost over the enabled edges, *flip set when an enabled edge is flipped.  r_out /
// c_out / wgt / flipped receive the residual, r^T L r, the robust weight and the flipped flag of EVERY edge when not null.  A wave holds 64 consecutive
// edges, so its mask word is one wave-uniform load.
__device__ __forceinline__ double pgo_edges(const PgoDev& P, const double* R, const double* T, const unsigned long long* mask, double* r_out, double* c_out,
                                            double* wgt, uint8_t* flipped, int* flip)
{
    double acc = 0.0;
    for (int e = threadIdx.x; e < P.E; e += PGO_T) {
        const unsigned long long word = mask[__builtin_amdgcn_readfirstlane(e >> 6)];
        const int a = P.ij[2 * e], b = P.ij[2 * e + 1];
        double r[6], den, Lf[6][6], m[6];
        pgo_residual(R + (size_t)a * 9, T + (size_t)a * 3, R + (size_t)b * 9, T + (size_t)b * 3, P.Z + (size_t)e * 12, r, &den);
        pgo_full(P.L + (size_t)e * 21, 1.0, Lf);
        pgo_matvec(Lf, r, m);
        const double c = pgo_dot6(r, m);
        double rho = c, w = 1.0;
        if (P.huber > 0.0) {
            const double chi = sqrt(c);
            if (chi > P.huber) { w = P.huber / chi; rho = (2.0 * P.huber) * chi - P.huber * P.huber; }
        }
        const bool fl = den < 1.0;
        if (r_out) {
#pragma unroll
            for (int k = 0; k < 6; ++k) r_out[(size_t)e * 6 + k] = r[k];
            c_out[e] = c;
        }
        if (wgt) wgt[e] = w;
        if (flipped) flipped[e] = fl ? 1 : 0;
        if ((word >> (e & 63)) & 1ull) { acc = acc + rho; if (fl) *flip = 1; }
    }
    return acc;
}

// Hd_i (21, upper triangle) and g_i of pose i at the poses (R, T): the sums over its enabled incident edges in ascending edge index; 0 for a fixed pose
__device__ __forceinline__ void pgo_gather_blocks(const PgoDev& P, int i, const double* R, const double* T, const unsigned long long* mask, const double* r,
                                                  const double* wgt, double Hd[21], double g[6])
{
#pragma unroll
    for (int k = 0; k < 21; ++k) Hd[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = 0.0;
    if (P.fixed && P.fixed[i]) return;
    for (int n = P.inc_ptr[i]; n < P.inc_ptr[i + 1]; ++n) {
        const int code = P.inc[n], e = code >> 1;
        if (!pgo_on(mask, e)) continue;
        const int b = P.ij[2 * e + 1];
        const double* Rb = R + (size_t)b * 9;
        double ti[3], Lf[6][6], re[6], m[6], q[6];
        pgo_tinv(Rb, T + (size_t)b * 3, ti);
        pgo_full(P.L + (size_t)e * 21, wgt[e], Lf);
#pragma unroll
        for (int k = 0; k < 6; ++k) re[k] = r[(size_t)e * 6 + k];
        pgo_matvec(Lf, re, m);
        pgo_adj_t(Rb, ti, m, q);
        if (code & 1) {
#pragma unroll
            for (int k = 0; k < 6; ++k) g[k] = g[k] - q[k];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) g[k] = g[k] + q[k];
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {                                // column j of W_e = A^T Lw A
            double ej[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, aj[6], wj[6];
            ej[j] = 1.0;
            pgo_adj(Rb, ti, ej, aj);
            pgo_matvec(Lf, aj, m);
            pgo_adj_t(Rb, ti, m, wj);
#pragma unroll
            for (int a = 0; a <= j; ++a) { const int k = a * 6 - (a * (a - 1)) / 2 + (j - a); Hd[k] = Hd[k] + wj[a]; }
        }
    }
}

// the factor's lower triangle (21 numbers, row by row) back as the matrix al_cholesky_solve reads
__device__ __forceinline__ void pgo_load_factor(const double* f, double Lm[6][6])
{
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Lm[i][j] = f[k++];
}

__global__ void __launch_bounds__(PGO_T) k_pose_graph(PgoDev P)
{
    extern __shared__ double pgo_lds[];                              // 256 doubles of reduction scratch, then p [N][6] when it fits
    double* red = pgo_lds;
    const int v = blockIdx.x, t = threadIdx.x, N = P.N, E = P.E;
    const unsigned long long* mask = P.masks + (size_t)v * P.W;
    double* ws = P.ws + (size_t)v * P.ws_stride;
    double *Rt = ws, *Tt = Rt + (size_t)N * 9, *Hd = Tt + (size_t)N * 3, *Lf = Hd + (size_t)N * 21, *g = Lf + (size_t)N * 21, *x = g + (size_t)N * 6,
           *rr = x + (size_t)N * 6, *z = rr + (size_t)N * 6, *Ap = z + (size_t)N * 6, *pw = Ap + (size_t)N * 6, *u = pw + (size_t)N * 6,
           *wgt = u + (size_t)E * 6;
    double* p = P.p_in_lds ? pgo_lds + PGO_T : pw;

    if (P.lin_only) {                                                // one mask; the poses are read where they are
        int flip = 0;
        (void)pgo_edges(P, P.R0, P.T0, mask, P.r, P.c, wgt, P.flipped, &flip);
        __syncthreads();
        for (int i = t; i < N; i += PGO_T) {
            double h[21], gi[6];
            pgo_gather_blocks(P, i, P.R0, P.T0, mask, P.r, wgt, h, gi);
#pragma unroll
            for (int k = 0; k < 21; ++k) P.Hd[(size_t)i * 21 + k] = h[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) P.g[(size_t)i * 6 + k] = gi[k];
        }
        return;
    }

    double* R = P.R + (size_t)v * N * 9;
    double* T = P.T + (size_t)v * N * 3;
    double* r_out = P.r + (size_t)v * E * 6;
    double* c_out = P.c + (size_t)v * E;
    tsl_pgo_report* rep = P.rep + v;
    for (int k = t; k < N * 9; k += PGO_T) R[k] = P.R0[k];
    for (int k = t; k < N * 3; k += PGO_T) T[k] = P.T0[k];
    __syncthreads();

    int status = P.skip[v], n_it = 0;                                // 0 or 4 (the host's union-find)
    double damping = P.damping;
    if (status == 0) {
        int flip = 0;
        (void)pgo_edges(P, R, T, mask, nullptr, nullptr, nullptr, nullptr, &flip);
        if (__syncthreads_or(flip)) status = 5;
    }
    if (status == 0) {
        status = 1;
        for (int it = 0; it < P.iters; ++it) {
            // ---- linearise at the current poses
            int flip = 0;
            const double cost = pgo_sum(pgo_edges(P, R, T, mask, r_out, c_out, wgt, nullptr, &flip), red);      // the barriers inside publish r and wgt
            int singular = 0;
            for (int i = t; i < N; i += PGO_T) {
                double h[21], gi[6];
                pgo_gather_blocks(P, i, R, T, mask, r_out, wgt, h, gi);
#pragma unroll
                for (int k = 0; k < 21; ++k) Hd[(size_t)i * 21 + k] = h[k];
#pragma unroll
                for (int k = 0; k < 6; ++k) g[(size_t)i * 6 + k] = gi[k];
                if (!P.fixed[i]) {
                    double Hm[6][6], Lm[6][6];
                    pgo_full(h, 1.0, Hm);
#pragma unroll
                    for (int a = 0; a < 6; ++a) Hm[a][a] += damping * Hm[a][a];
                    if (!al_cholesky(Hm, Lm)) singular = 1;
                    else {
                        int k = 0;
#pragma unroll
                        for (int a = 0; a < 6; ++a)
#pragma unroll
                            for (int c = 0; c <= a; ++c) Lf[(size_t)i * 21 + k++] = Lm[a][c];
                    }
                }
            }
            ++n_it;
            if (__syncthreads_or(singular)) {
                if (t == 0) { tsl_pgo_iter& q = rep->it[it]; q.cost_before = cost; q.cost_after = cost; q.max_step = 0.0; q.damping = damping; q.pcg_iters = 0; q.accepted = 0; }
                status = 3;
                break;
            }
            // ---- preconditioned conjugate gradients on H x = -g from x = 0; a thread owns the poses i = t mod 256
            double part = 0.0;
            for (int i = t; i < N; i += PGO_T) {
                double ri[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, zi[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
                if (!P.fixed[i]) {
                    double Lm[6][6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) ri[k] = -g[(size_t)i * 6 + k];
                    pgo_load_factor(Lf + (size_t)i * 21, Lm);
                    al_cholesky_solve(Lm, ri, zi);
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) { x[(size_t)i * 6 + k] = 0.0; rr[(size_t)i * 6 + k] = ri[k]; z[(size_t)i * 6 + k] = zi[k]; p[(size_t)i * 6 + k] = zi[k]; }
                part = part + pgo_dot6(ri, zi);
            }
            double rz = pgo_sum(part, red);                           // its barriers publish p
            const double rz0 = rz;
            int n_pcg = 0;
            while (n_pcg < P.pcg_max && !(rz <= P.tol2 * rz0)) {
                for (int e = t; e < E; e += PGO_T) {                  // edges: u_e = A^T (Lw (A (p_a - p_b)))
                    const unsigned long long word = mask[__builtin_amdgcn_readfirstlane(e >> 6)];
                    if (!((word >> (e & 63)) & 1ull)) continue;
                    const int a = P.ij[2 * e], b = P.ij[2 * e + 1];
                    const double* Rb = R + (size_t)b * 9;
                    double ti[3], d[6], o[6], m[6], ue[6], Lw[6][6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) d[k] = p[(size_t)a * 6 + k] - p[(size_t)b * 6 + k];
                    pgo_tinv(Rb, T + (size_t)b * 3, ti);
                    pgo_adj(Rb, ti, d, o);
                    pgo_full(P.L + (size_t)e * 21, wgt[e], Lw);
                    pgo_matvec(Lw, o, m);
                    pgo_adj_t(Rb, ti, m, ue);
#pragma unroll
                    for (int k = 0; k < 6; ++k) u[(size_t)e * 6 + k] = ue[k];
                }
                __syncthreads();
                part = 0.0;
                for (int i = t; i < N; i += PGO_T) {                  // poses: y_i = damping diag(Hd_i) p_i + the signed gather
                    double y[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, pi[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) pi[k] = p[(size_t)i * 6 + k];
                    if (!P.fixed[i]) {
                        const double* h = Hd + (size_t)i * 21;
                        const double dg[6] = { h[0], h[6], h[11], h[15], h[18], h[20] };
#pragma unroll
                        for (int k = 0; k < 6; ++k) y[k] = (damping * dg[k]) * pi[k];
                        for (int n = P.inc_ptr[i]; n < P.inc_ptr[i + 1]; ++n) {
                            const int code = P.inc[n], e = code >> 1;
                            if (!pgo_on(mask, e)) continue;
                            if (code & 1) {
#pragma unroll
                                for (int k = 0; k < 6; ++k) y[k] = y[k] - u[(size_t)e * 6 + k];
                            } else {
#pragma unroll
                                for (int k = 0; k < 6; ++k) y[k] = y[k] + u[(size_t)e * 6 + k];
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k) Ap[(size_t)i * 6 + k] = y[k];
                    part = part + pgo_dot6(pi, y);
                }
                const double pAp = pgo_sum(part, red);
                if (!(pAp > 0.0)) break;                              // uniform: every thread holds the same sum
                const double alpha = rz / pAp;
                part = 0.0;
                for (int i = t; i < N; i += PGO_T) {
                    double ri[6], zi[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        x[(size_t)i * 6 + k] = x[(size_t)i * 6 + k] + alpha * p[(size_t)i * 6 + k];
                        ri[k] = rr[(size_t)i * 6 + k] - alpha * Ap[(size_t)i * 6 + k];
                        rr[(size_t)i * 6 + k] = ri[k];
                    }
                    if (!P.fixed[i]) {
                        double Lm[6][6];
                        pgo_load_factor(Lf + (size_t)i * 21, Lm);
                        al_cholesky_solve(Lm, ri, zi);
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k) z[(size_t)i * 6 + k] = zi[k];
                    part = part + pgo_dot6(ri, zi);
                }
                const double rz_new = pgo_sum(part, red);
                const double beta = rz_new / rz;
                for (int i = t; i < N; i += PGO_T) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) p[(size_t)i * 6 + k] = z[(size_t)i * 6 + k] + beta * p[(size_t)i * 6 + k];
                }
                __syncthreads();                                      // p, before the next edge pass reads it
                rz = rz_new;
                ++n_pcg;
            }
            // ---- retract into the trial poses and evaluate them
            double n2max = 0.0;
            for (int i = t; i < N; i += PGO_T) {
                double Ri[9], Ti[3], xi[6];
#pragma unroll
                for (int k = 0; k < 9; ++k) Ri[k] = R[(size_t)i * 9 + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) Ti[k] = T[(size_t)i * 3 + k];
#pragma unroll
                for (int k = 0; k < 6; ++k) xi[k] = x[(size_t)i * 6 + k];
                if (!P.fixed[i]) {
                    al_retract(xi, Ri, Ti);
                    const double n2 = pgo_dot6(xi, xi);
                    n2max = n2 > n2max ? n2 : n2max;
                }
#pragma unroll
                for (int k = 0; k < 9; ++k) Rt[(size_t)i * 9 + k] = Ri[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) Tt[(size_t)i * 3 + k] = Ti[k];
            }
            const double step = sqrt(pgo_max(n2max, red));            // its barriers publish the trial poses
            flip = 0;
            const double trial = pgo_sum(pgo_edges(P, Rt, Tt, mask, nullptr, nullptr, nullptr, nullptr, &flip), red);
            const bool accept = !__syncthreads_or(flip) && isfinite(trial) && trial < cost;
            if (t == 0) {
                tsl_pgo_iter& q = rep->it[it];
                q.cost_before = cost; q.cost_after = trial; q.max_step = step; q.damping = damping; q.pcg_iters = n_pcg; q.accepted = accept ? 1 : 0;
            }
            if (accept) {
                for (int k = t; k < N * 9; k += PGO_T) R[k] = Rt[k];
                for (int k = t; k < N * 3; k += PGO_T) T[k] = Tt[k];
                __syncthreads();
                const double d = damping / P.down;
                damping = d > P.dmin ? d : P.dmin;
                if (step < P.min_step || cost - trial <= P.rel_tol * cost) { status = 0; break; }
            } else {
                damping = damping * P.up;
                if (damping > P.dmax) { status = 2; break; }
            }
        }
    }
    // ---- the outputs: every edge at the final poses, the cost over the enabled ones, the report
    int flip = 0;
    const double cost = pgo_sum(pgo_edges(P, R, T, mask, r_out, c_out, nullptr, nullptr, &flip), red);
    if (t == 0) { rep->status = status; rep->iterations = n_it; rep->cost = cost; }
    for (int k = n_it + t; k < 64; k += PGO_T) { tsl_pgo_iter& q = rep->it[k]; q.cost_before = 0.0; q.cost_after = 0.0; q.max_step = 0.0; q.damping = 0.0; q.pcg_iters = 0; q.accepted = 0; }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------

static size_t pgo_ws_doubles(int64_t n, int64_t e) { return (size_t)(PGO_WS_POSE * n + PGO_WS_EDGE * e); }
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
static size_t pgo_tab_bytes(int64_t n, int64_t e, int64_t b)
{
    return up16(8 * (size_t)e) + up16(8 * (size_t)e) + up16(4 * (size_t)(n + 1)) + up16(8 * (size_t)b * (size_t)((e + 63) / 64)) + up16((size_t)n) + up16((size_t)b);
}

static bool ok_d(double x) { return std::isfinite(x) && x >= 0.0; }

// every check that reads host memory; vals: R, T, Z and L are host arrays (the host forms) and are checked too
static int pgo_check(tsl_pgo* h, int32_t N, const void* R, const void* T, const uint8_t* fixed, int32_t E, const int32_t* ij, const void* Z, const void* L, int32_t B,
                     bool need_fixed, bool vals, const char* who)
{
    const std::string w = std::string(who) + ": ";
    TSL_REQUIRE(h, w + "null handle");
    TSL_REQUIRE(R && T && ij && Z && L, w + "null R, T, ij, Z or L");
    TSL_REQUIRE(N >= 1 && N <= h->max_n && E >= 1 && E <= h->max_e && B >= 1 && B <= h->max_b, w + "N, E or B outside 1 .. the handle's capacity");
    for (int e = 0; e < E; ++e) {
        const int a = ij[2 * e], b = ij[2 * e + 1];
        TSL_REQUIRE(a >= 0 && a < N && b >= 0 && b < N && a != b, w + "an edge joins a pose to itself or to an index outside the poses");
    }
    bool any = false;
    if (fixed) for (int i = 0; i < N; ++i) any = any || fixed[i];
    TSL_REQUIRE(!need_fixed || any, w + "no fixed pose");
    if (vals) {
        const double* Ld = (const double*)L;
        TSL_REQUIRE(al_finite((const double*)R, N * 9) && al_finite((const double*)T, N * 3) && al_finite((const double*)Z, E * 12) && al_finite(Ld, E * 21),
                    w + "a number that is not finite");
        static const int dg[6] = { 0, 6, 11, 15, 18, 20 };
        for (int e = 0; e < E; ++e) for (int k = 0; k < 6; ++k) TSL_REQUIRE(Ld[(size_t)e * 21 + dg[k]] >= 0.0, w + "a negative diagonal of L");
    }
    return TSL_OK;
}

static int pgo_cfg_check(const tsl_pgo_cfg* c, const char* who)
{
    const std::string w = std::string(who) + ": ";
    TSL_REQUIRE(c, w + "null cfg");
    TSL_REQUIRE(c->iters >= 0 && c->iters <= 64, w + "iters must be 0 .. 64");
    TSL_REQUIRE(c->pcg_max >= 0 && c->pcg_max <= PGO_MAX_PCG, w + "pcg_max must be 0 .. 100000");
    TSL_REQUIRE(ok_d(c->damping) && ok_d(c->damping_up) && ok_d(c->damping_down) && ok_d(c->damping_min) && ok_d(c->damping_max) && ok_d(c->pcg_tol) &&
                ok_d(c->min_step) && ok_d(c->rel_tol) && ok_d(c->huber), w + "a parameter that is negative or not finite");
    TSL_REQUIRE(c->damping_down > 0.0, w + "damping_down must be positive");
    return TSL_OK;
}

// The tables of a call into the pinned buffer and up to the device on the handle's stream: ij, the incidence lists (per pose its edges in ascending index,
// 2 e + 1 where the pose is b), the masks (null: one variant, every edge on), fixed, and per variant 4 when some component of its enabled edges holds a
// free pose and no fixed one (a union-find per variant).  Fills the table pointers of P.
static int pgo_tables(tsl_pgo* h, PgoDev* P, int N, int E, int B, const int32_t* ij, const uint8_t* fixed, const uint64_t* masks, bool want_skip)
{
    TSL_HIP(hipEventSynchronize(h->ev_up));                          // the last call's upload has left the pinned buffer
    const int W = (E + 63) / 64;
    const size_t o_ij = 0, o_inc = o_ij + up16(8 * (size_t)E), o_ptr = o_inc + up16(8 * (size_t)E), o_mask = o_ptr + up16(4 * (size_t)(N + 1)),
                 o_fix = o_mask + up16(8 * (size_t)B * W), o_skip = o_fix + up16((size_t)N), total = o_skip + up16((size_t)B);
    char* H = h->h_tab;
    int32_t* h_ij = (int32_t*)(H + o_ij); int32_t* h_inc = (int32_t*)(H + o_inc); int32_t* h_ptr = (int32_t*)(H + o_ptr);
    uint64_t* h_mask = (uint64_t*)(H + o_mask); uint8_t* h_fix = (uint8_t*)(H + o_fix); uint8_t* h_skip = (uint8_t*)(H + o_skip);
    std::memcpy(h_ij, ij, 8 * (size_t)E);
    for (int i = 0; i < N; ++i) h_fix[i] = fixed && fixed[i] ? 1 : 0;
    for (int i = 0; i <= N; ++i) h_ptr[i] = 0;
    for (int e = 0; e < E; ++e) { ++h_ptr[ij[2 * e] + 1]; ++h_ptr[ij[2 * e + 1] + 1]; }
    for (int i = 0; i < N; ++i) h_ptr[i + 1] += h_ptr[i];
    std::vector<int32_t> at(h_ptr, h_ptr + N);
    for (int e = 0; e < E; ++e) { h_inc[at[ij[2 * e]]++] = 2 * e; h_inc[at[ij[2 * e + 1]]++] = 2 * e + 1; }      // e ascends, so every list does
    for (int v = 0; v < B; ++v)
        for (int k = 0; k < W; ++k) {
            const uint64_t valid = (k == W - 1 && (E & 63)) ? (((uint64_t)1 << (E & 63)) - 1) : ~(uint64_t)0;
            h_mask[(size_t)v * W + k] = (masks ? masks[(size_t)v * W + k] : ~(uint64_t)0) & valid;
        }
    std::vector<int32_t> root(N);
    std::vector<uint8_t> has(N);
    for (int v = 0; v < B; ++v) {
        h_skip[v] = 0;
        if (!want_skip) continue;
        for (int i = 0; i < N; ++i) root[i] = i;
        auto find = [&](int i) { while (root[i] != i) { root[i] = root[root[i]]; i = root[i]; } return i; };
        for (int e = 0; e < E; ++e)
            if ((h_mask[(size_t)v * W + (e >> 6)] >> (e & 63)) & 1) { const int a = find(ij[2 * e]), b = find(ij[2 * e + 1]); if (a != b) root[a < b ? b : a] = a < b ? a : b; }
        for (int i = 0; i < N; ++i) has[i] = 0;
        for (int i = 0; i < N; ++i) if (h_fix[i]) has[find(i)] = 1;
        for (int i = 0; i < N; ++i) if (!h_fix[i] && !has[find(i)]) { h_skip[v] = 4; break; }
    }
    TSL_HIP(hipMemcpyAsync(h->tab, H, total, hipMemcpyHostToDevice, h->stream));
    TSL_HIP(hipEventRecord(h->ev_up, h->stream));
    P->N = N; P->E = E; P->W = W;
    P->ij = (const int*)(h->tab + o_ij); P->inc = (const int*)(h->tab + o_inc); P->inc_ptr = (const int*)(h->tab + o_ptr);
    P->masks = (const unsigned long long*)(h->tab + o_mask); P->fixed = (const uint8_t*)(h->tab + o_fix); P->skip = (const uint8_t*)(h->tab + o_skip);
    P->ws = h->ws; P->ws_stride = pgo_ws_doubles(N, E);
    P->p_in_lds = N <= PGO_LDS_POSES ? 1 : 0;
    return TSL_OK;
}

static void pgo_params(PgoDev* P, const tsl_pgo_cfg* c)
{
    P->iters = c->iters; P->pcg_max = c->pcg_max; P->damping = c->damping; P->up = c->damping_up; P->down = c->damping_down; P->dmin = c->damping_min;
    P->dmax = c->damping_max; P->tol2 = c->pcg_tol * c->pcg_tol; P->min_step = c->min_step; P->rel_tol = c->rel_tol; P->huber = c->huber;
}

static int pgo_launch(tsl_pgo* h, const PgoDev& P, int B)
{
    const size_t lds = sizeof(double) * PGO_T + (P.p_in_lds ? sizeof(double) * 6 * (size_t)P.N : 0);
    hipLaunchKernelGGL(k_pose_graph, dim3((unsigned)B), dim3(PGO_T), lds, h->stream, P);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// the handle's stream behind the work queued on `user`, and `user` behind the handle's stream
static int pgo_before(tsl_pgo* h, hipStream_t user) { TSL_HIP(hipEventRecord(h->ev_in, user)); TSL_HIP(hipStreamWaitEvent(h->stream, h->ev_in, 0)); return TSL_OK; }
static int pgo_after(tsl_pgo* h, hipStream_t user) { TSL_HIP(hipEventRecord(h->ev_out, h->stream)); TSL_HIP(hipStreamWaitEvent(user, h->ev_out, 0)); return TSL_OK; }

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_pgo_create(int device, int32_t max_poses, int32_t max_edges, int32_t max_variants, tsl_pgo** out)
{
    TSL_REQUIRE(out, "tsl_pgo_create: null out"); *out = nullptr;
    TSL_REQUIRE(max_poses >= 1 && max_poses <= PGO_MAX_N && max_edges >= 1 && max_edges <= PGO_MAX_E && max_variants >= 1 && max_variants <= PGO_MAX_B,
                "tsl_pgo_create: at most 8192 poses, 131072 edges and 1024 variants, at least one of each");
    const size_t ws_bytes = sizeof(double) * (size_t)max_variants * pgo_ws_doubles(max_poses, max_edges);
    TSL_REQUIRE(ws_bytes + pgo_tab_bytes(max_poses, max_edges, max_variants) <= PGO_WS_LIMIT,
                "tsl_pgo_create: max_variants * (720 * max_poses + 56 * max_edges) bytes of workspace must stay under 1 GiB");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available"); return TSL_ERR_NO_DEVICE; }
    TSL_REQUIRE(device >= 0 && device < ndev, "tsl_pgo_create: bad device index");
    TSL_HIP(hipSetDevice(device));
    tsl_pgo* h = new tsl_pgo();                                      // value-initialised: every pointer null
    h->device = device; h->max_n = max_poses; h->max_e = max_edges; h->max_b = max_variants;
    h->tab_bytes = pgo_tab_bytes(max_poses, max_edges, max_variants);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming) != hipSuccess ||
        hipMalloc((void**)&h->ws, ws_bytes) != hipSuccess || hipMalloc((void**)&h->tab, h->tab_bytes) != hipSuccess ||
        hipHostMalloc((void**)&h->h_tab, h->tab_bytes, hipHostMallocDefault) != hipSuccess) {
        set_error("tsl_pgo_create: the stream, the events, the workspace or the tables could not be made");
        tsl_pgo_destroy(h);
        return TSL_ERR_HIP;
    }
    *out = h;
    return TSL_OK;
}

void tsl_pgo_destroy(tsl_pgo* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    hipEvent_t evs[] = { h->ev_in, h->ev_out, h->ev_up };
    for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    void* ptrs[] = { h->ws, h->tab, h->sbuf };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (h->h_tab) (void)hipHostFree(h->h_tab);
    delete h;
}

int tsl_pgo_linearize(tsl_pgo* h, int32_t N, const double* R, const double* T, const uint8_t* fixed, int32_t E, const int32_t* ij, const double* Z, const double* L,
                      const uint64_t* mask, double huber, double* r, double* cost, uint8_t* flipped, double* Hd, double* g)
{
    int rc = pgo_check(h, N, R, T, fixed, E, ij, Z, L, 1, false, true, "tsl_pgo_linearize"); if (rc) return rc;
    TSL_REQUIRE(ok_d(huber), "tsl_pgo_linearize: huber must be finite and not negative");
    TSL_REQUIRE(r && cost && flipped && Hd && g, "tsl_pgo_linearize: null output");
    TSL_HIP(hipSetDevice(h->device));
    PgoDev P = {};
    if ((rc = pgo_tables(h, &P, N, E, 1, ij, fixed, mask, false))) return rc;
    Stage st(&h->sbuf, &h->sbuf_bytes, h->stream);
    const int i_R = st.in(R, 72 * (size_t)N), i_T = st.in(T, 24 * (size_t)N), i_Z = st.in(Z, 96 * (size_t)E), i_L = st.in(L, 168 * (size_t)E),
              i_r = st.out(r, 48 * (size_t)E), i_c = st.out(cost, 8 * (size_t)E), i_f = st.out(flipped, (size_t)E), i_H = st.out(Hd, 168 * (size_t)N),
              i_g = st.out(g, 48 * (size_t)N);
    if ((rc = st.upload())) return rc;
    P.lin_only = 1; P.huber = huber;
    P.R0 = st.ptr<const double>(i_R); P.T0 = st.ptr<const double>(i_T); P.Z = st.ptr<const double>(i_Z); P.L = st.ptr<const double>(i_L);
    P.r = st.ptr<double>(i_r); P.c = st.ptr<double>(i_c); P.flipped = st.ptr<uint8_t>(i_f); P.Hd = st.ptr<double>(i_H); P.g = st.ptr<double>(i_g);
    if ((rc = pgo_launch(h, P, 1))) return rc;
    return st.download();
}

int tsl_pgo_linearize_dev(tsl_pgo* h, int32_t N, const void* R_dev, const void* T_dev, const uint8_t* fixed, int32_t E, const int32_t* ij, const void* Z_dev,
                          const void* L_dev, const uint64_t* mask, double huber, void* r_dev, void* cost_dev, void* flipped_dev, void* Hd_dev, void* g_dev,
                          void* user_stream)
{
    int rc = pgo_check(h, N, R_dev, T_dev, fixed, E, ij, Z_dev, L_dev, 1, false, false, "tsl_pgo_linearize_dev"); if (rc) return rc;
    TSL_REQUIRE(ok_d(huber), "tsl_pgo_linearize_dev: huber must be finite and not negative");
    TSL_REQUIRE(r_dev && cost_dev && flipped_dev && Hd_dev && g_dev, "tsl_pgo_linearize_dev: null output");
    TSL_HIP(hipSetDevice(h->device));
    PgoDev P = {};
    if ((rc = pgo_tables(h, &P, N, E, 1, ij, fixed, mask, false))) return rc;
    P.lin_only = 1; P.huber = huber;
    P.R0 = (const double*)R_dev; P.T0 = (const double*)T_dev; P.Z = (const double*)Z_dev; P.L = (const double*)L_dev;
    P.r = (double*)r_dev; P.c = (double*)cost_dev; P.flipped = (uint8_t*)flipped_dev; P.Hd = (double*)Hd_dev; P.g = (double*)g_dev;
    if ((rc = pgo_before(h, (hipStream_t)user_stream)) || (rc = pgo_launch(h, P, 1))) return rc;
    return pgo_after(h, (hipStream_t)user_stream);
}

int tsl_pgo_solve(tsl_pgo* h, int32_t N, const double* R, const double* T, const uint8_t* fixed, int32_t E, const int32_t* ij, const double* Z, const double* L,
                  int32_t B, const uint64_t* masks, const tsl_pgo_cfg* cfg, double* R_out, double* T_out, double* r, double* cost, tsl_pgo_report* reports)
{
    if (!masks) B = 1;
    int rc = pgo_check(h, N, R, T, fixed, E, ij, Z, L, B, true, true, "tsl_pgo_solve"); if (rc) return rc;
    if ((rc = pgo_cfg_check(cfg, "tsl_pgo_solve"))) return rc;
    TSL_REQUIRE(R_out && T_out && r && cost && reports, "tsl_pgo_solve: null output");
    TSL_HIP(hipSetDevice(h->device));
    PgoDev P = {};
    if ((rc = pgo_tables(h, &P, N, E, B, ij, fixed, masks, true))) return rc;
    Stage st(&h->sbuf, &h->sbuf_bytes, h->stream);
    const size_t b = (size_t)B;
    const int i_R = st.in(R, 72 * (size_t)N), i_T = st.in(T, 24 * (size_t)N), i_Z = st.in(Z, 96 * (size_t)E), i_L = st.in(L, 168 * (size_t)E),
              i_Ro = st.out(R_out, b * 72 * (size_t)N), i_To = st.out(T_out, b * 24 * (size_t)N), i_r = st.out(r, b * 48 * (size_t)E),
              i_c = st.out(cost, b * 8 * (size_t)E), i_rep = st.out(reports, b * sizeof(tsl_pgo_report));
    if ((rc = st.upload())) return rc;
    pgo_params(&P, cfg);
    P.R0 = st.ptr<const double>(i_R); P.T0 = st.ptr<const double>(i_T); P.Z = st.ptr<const double>(i_Z); P.L = st.ptr<const double>(i_L);
    P.R = st.ptr<double>(i_Ro); P.T = st.ptr<double>(i_To); P.r = st.ptr<double>(i_r); P.c = st.ptr<double>(i_c); P.rep = st.ptr<tsl_pgo_report>(i_rep);
    if ((rc = pgo_launch(h, P, B))) return rc;
    return st.download();
}

int tsl_pgo_solve_dev(tsl_pgo* h, int32_t N, const void* R_dev, const void* T_dev, const uint8_t* fixed, int32_t E, const int32_t* ij, const void* Z_dev,
                      const void* L_dev, int32_t B, const uint64_t* masks, const tsl_pgo_cfg* cfg, void* R_out_dev, void* T_out_dev, void* r_dev, void* cost_dev,
                      void* reports_dev, void* user_stream)
{
    if (!masks) B = 1;
    int rc = pgo_check(h, N, R_dev, T_dev, fixed, E, ij, Z_dev, L_dev, B, true, false, "tsl_pgo_solve_dev"); if (rc) return rc;
    if ((rc = pgo_cfg_check(cfg, "tsl_pgo_solve_dev"))) return rc;
    TSL_REQUIRE(R_out_dev && T_out_dev && r_dev && cost_dev && reports_dev, "tsl_pgo_solve_dev: null output");
    TSL_HIP(hipSetDevice(h->device));
    PgoDev P = {};
    if ((rc = pgo_tables(h, &P, N, E, B, ij, fixed, masks, true))) return rc;
    pgo_params(&P, cfg);
    P.R0 = (const double*)R_dev; P.T0 = (const double*)T_dev; P.Z = (const double*)Z_dev; P.L = (const double*)L_dev;
    P.R = (double*)R_out_dev; P.T = (double*)T_out_dev; P.r = (double*)r_dev; P.c = (double*)cost_dev; P.rep = (tsl_pgo_report*)reports_dev;
    if ((rc = pgo_before(h, (hipStream_t)user_stream)) || (rc = pgo_launch(h, P, B))) return rc;
    return pgo_after(h, (hipStream_t)user_stream);
}

}  // extern "C"

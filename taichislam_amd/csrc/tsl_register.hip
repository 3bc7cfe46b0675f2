// tsl_register.hip -- map-to-map registration: a TSDF submap against another map, Gauss-Newton on the difference of the two signed distances.  The
// source's voxels near its surface are carried by X = (R, T) into the destination; there the destination's trilinear interpolant s (tsl_interp.hpp)
// should equal the value t the source stores: minimise the sum of (s(R q_i + T) - t_i)^2 over X.  The reference takes every submap pose from a pose
// graph outside and has no counterpart; this is the constraint such a graph consumes, and what re-anchors a tracked submap before it is fused.
//
// Definition (tests/register_ref.py restates it in numpy and every integer must equal it).  All f32, no contraction, in the
// written order.  Visited: the observed voxels (obs > 0) of the source submap whose indices (i, j, k) are each divisible by stride (1, 2, 4, 8 or 16).
// A visited voxel with the stored word tw falls into exactly one bucket:
//   gate     w = h2f(tw >> 16) fails w >= w_min, or |t| > band, t = h2f(tw & 0xffff); otherwise q = ((float)i vs, (float)j vs, (float)k vs),
//            p[a] = ((R[a][0] q0 + R[a][1] q1) + R[a][2] q2) + T[a]
//   unknown  the destination's sample at p is not KNOWN (section 4.7); otherwise s = tri_value, g = tri_grad / vs
//   far      |s| > r_max
//   grad     gg = (g0 g0 + g1 g1) + g2 g2 is 0 or > g_max * g_max
//   used     r = s - t, c = p x g, J = (g, c), wgt = huber > 0 && |r| > huber ? huber / |r| : 1, wJ = wgt J; the 28 products H_ab = wJ[a] J[b] (a <= b),
//            b_a = wJ[a] r, e = (wgt r) r, each added as rint(x * 2^20) into int64 sums (al_fix): the 33 integers of tsl_align_sums.
//
// k_register_linearize: one workgroup per source brick, the workgroups stride over the pool.  Only a thin band of a brick passes the gate, so the
// work is compaction first: pass 1 reads the brick's obs and tw planes with 16-byte loads (a thread owns the 16 voxels of one k-row), applies the
// lattice, weight and band tests and queues the survivors in LDS by wave ballot and prefix rank (the idiom of wave_reserve, on an LDS counter);
// pass 2 hands the queue to the lanes densely, 64 live lanes per wave until the tail, and each lane samples the destination (tsdf_read_cell: all 16
// gathers issued before the first use) and adds its 28 products into int64 accumulators of its own.  The queue holds 4096 entries -- a brick can lie
// in the band whole -- of 4 bytes each: local index << 16 | t.  The accumulators live across every brick a workgroup takes; the halving butterfly
// (al_halve) runs once per wave at the end, then LDS across the four waves and one 64-bit integer atomic per non-zero sum per workgroup.  The
// counts are ballots and popcounts.  No float atomics.  flags bit 0 leaves the products and the reduction out: the A/B switch of
// tools/bench_register.py.
#include <cmath>
#include "tsl_interp.hpp"
#include "tsl_align_common.hpp"
#include "tsl_register_common.hpp"

namespace tsl {

#define RG_QUEUE TSL_BRK3              // entries of the LDS queue: every voxel of a brick can pass the gate

// At least 3 waves per SIMD: left alone the scheduler overlaps the 28 conversions and takes 194 VGPRs (2 waves); held to 168 it needs no scratch.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_register_linearize(MapDev S, int ss, MapDev D, int ds, RegisterDev A, long long* __restrict__ acc)
{
    __shared__ uint32_t queue[RG_QUEUE];
    __shared__ int q_total;                                       // entries queued so far by this workgroup, never reset: a brick's entries are those past `q_base`
    __shared__ long long sm[4][32];
    __shared__ int sc[4][8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int* __restrict__ Td = D.table + (size_t)ds * D.nb3;
    if (threadIdx.x == 0) q_total = 0;
    __syncthreads();
    int top = *S.pool_top;                                        // bricks handed out; the counter may stand past the pool when it filled up
    if (top > S.max_bricks) top = S.max_bricks;
    const int first = ss * S.nb3;
    const bool sums = !(A.flags & 1);
    long long v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = 0;
    int n_used = 0, n_gate = 0, n_unknown = 0, n_far = 0, n_grad = 0;      // per wave (uniform)
    int q_base = 0;
    const int li = threadIdx.x >> 4, lj = threadIdx.x & 15;       // the k-row this thread reads in pass 1

    for (int pb = blockIdx.x; pb < top; pb += gridDim.x) {
        const int b = S.owner[pb] - first;                        // uniform: the whole workgroup skips a brick of another submap
        if (b < 0 || b >= S.nb3) continue;
        const int bk = b % S.nbz, bj = (b / S.nbz) % S.nbx, bi = b / (S.nbz * S.nbx);
        const int i0 = bi * 16 - S.hN, j0 = bj * 16 - S.hN, k0 = bk * 16 - S.hNz;

        // ---- pass 1: compaction ----
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
            if ((k0 + r) & A.smask) continue;                     // uniform
            const bool seen = row && (int8_t)((obw[r >> 2] >> ((r & 3) * 8)) & 0xffu) > 0;
            const uint32_t tw = tww[r];
            const float w = h2f((h16)(tw >> 16)), t = h2f((h16)(tw & 0xffffu));
            const bool pass = seen && (w >= A.w_min) && !(fabsf(t) > A.band);
            n_gate += popc64(__ballot(seen && !pass));
            const unsigned long long m = __ballot(pass);
            if (m) {
                const int leader = (int)__builtin_ctzll(m);
                int base = 0;
                if (lane == leader) base = atomicAdd(&q_total, popc64(m));
                base = __shfl(base, leader);
                if (pass) queue[base + rank_below(m) - q_base] = ((uint32_t)(threadIdx.x * 16 + r) << 16) | (tw & 0xffffu);
            }
        }
        __syncthreads();
        const int n = q_total - q_base;                           // at most 4096: one entry per voxel of the brick
        q_base += n;

        // ---- pass 2: the queue, densely ----
        for (int e0 = wave * 64; e0 < n; e0 += 256) {
            const int e = e0 + lane;
            int bucket = -1;
            float sv = 0.0f, tv = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, p[3] = { 0.0f, 0.0f, 0.0f };
            if (e < n) {
                const uint32_t ent = queue[e];
                const int l = (int)(ent >> 16);
                tv = h2f((h16)(ent & 0xffffu));
                const float q0 = (float)(i0 + (l >> 8)) * A.vs, q1 = (float)(j0 + ((l >> 4) & 15)) * A.vs, q2 = (float)(k0 + (l & 15)) * A.vs;
                float u[3]; int c[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    p[a] = ((A.R[a * 3] * q0 + A.R[a * 3 + 1] * q1) + A.R[a * 3 + 2] * q2) + A.T[a];
                    u[a] = p[a] / A.vs; c[a] = cell_floor(u[a]);
                }
                bucket = AL_UNKNOWN;
                float V[8];
                if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && tsdf_read_cell(D, Td, c[0], c[1], c[2], V)) {
                    const float f0 = u[0] - (float)c[0], f1 = u[1] - (float)c[1], f2 = u[2] - (float)c[2];
                    sv = tri_value(V, f0, f1, f2);
                    tri_grad(V, f0, f1, f2, &g0, &g1, &g2);
                    g0 = g0 / A.vs; g1 = g1 / A.vs; g2 = g2 / A.vs;
                    const float gg = (g0 * g0 + g1 * g1) + g2 * g2;
                    bucket = fabsf(sv) > A.r_max ? AL_FAR : (gg == 0.0f || gg > A.gm2) ? AL_GRAD : AL_USED;
                }
            }
            const bool used = bucket == AL_USED;
            if (used && sums) {
                const float r = sv - tv;
                const float J[6] = { g0, g1, g2, p[1] * g2 - p[2] * g1, p[2] * g0 - p[0] * g2, p[0] * g1 - p[1] * g0 };
                const float ar = fabsf(r);
                const float wgt = (A.huber > 0.0f && ar > A.huber) ? A.huber / ar : 1.0f;
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
            n_used += popc64(__ballot(used)); n_unknown += popc64(__ballot(bucket == AL_UNKNOWN));
            n_far += popc64(__ballot(bucket == AL_FAR)); n_grad += popc64(__ballot(bucket == AL_GRAD));
        }
        __syncthreads();                                          // the queue is free for the next brick
    }

    // the wave's sums: after the five halving steps lane l holds sum number l >> 1 over its half of the wave, the last step adds the other half
    if (n_used && sums) {
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
        else { const int c = t - AL_NPROD; sum = ((long long)sc[0][c] + sc[1][c]) + ((long long)sc[2][c] + sc[3][c]); }
        if (sum != 0) __hip_atomic_fetch_add(acc + t, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// issues the queued frames of both handles, waits for the source's, and leaves dst's stream with the accumulator in dst's staging buffer
static int register_stage(tsl_tsdf* dst, tsl_tsdf* src, hipStream_t* q, long long** acc)
{
    TSL_HIP(hipSetDevice(dst->device));
    if (src != dst) { const int rc = tsl_tsdf_sync(src); if (rc) return rc; }      // as tsl_tsdf_fuse_submaps: the source is complete before dst's stream reads it
    *q = ms(dst);
    const int rc = grow(&dst->xbuf, &dst->xbuf_bytes, 512 + 64); if (rc) return rc;
    *acc = (long long*)dst->xbuf;
    return TSL_OK;
}

// one linearisation on q with the result on the host: zero the accumulator, launch, copy back through the pinned buffer, wait
static int register_run(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, hipStream_t q, const RegisterDev& A, long long* acc, tsl_align_sums* out)
{
    TSL_HIP(hipMemsetAsync(acc, 0, AL_SLOTS * sizeof(long long), q));
    int grid = src->M.max_bricks;                                  // never more workgroups than pool bricks
    if (grid > 4 * dst->ncu) grid = 4 * dst->ncu;
    if (grid < 1) grid = 1;
    prof_begin(dst, TSL_K_REGISTER, q);                           // tsl_tsdf_prof_query(dst, TSL_K_REGISTER): the kernel alone, what tools/bench_register.py reports
    hipLaunchKernelGGL(k_register_linearize, dim3((unsigned)grid), dim3(256), 0, q, src->M, rg_slot(src, src_sid), dst->M, rg_slot(dst, dst_sid), A, acc);
    prof_end(dst, q);
    TSL_HIP(hipGetLastError());
    TSL_HIP(hipMemcpyAsync(al_pinned(dst), acc, sizeof(tsl_align_sums), hipMemcpyDeviceToHost, q));
    TSL_HIP(hipStreamSynchronize(q));
    std::memcpy(out, al_pinned(dst), sizeof(tsl_align_sums));
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_register_linearize(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R[9], const double T[3], const tsl_register_cfg* c,
                                tsl_align_sums* out)
{
    RegisterDev A;
    int rc = register_check(dst, dst_sid, src, src_sid, R, T, c, out, c ? c->stride : 1, &A, "register_linearize"); if (rc) return rc;
    hipStream_t q; long long* acc;
    if ((rc = register_stage(dst, src, &q, &acc))) return rc;
    return register_run(dst, dst_sid, src, src_sid, q, A, acc, out);
}

int tsl_tsdf_register_submap(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R0[9], const double T0[3], const tsl_register_cfg* c,
                             const tsl_track_cfg* t, double R_out[9], double T_out[3], tsl_track_report* rep)
{
    const char* who = "register_submap";
    TSL_REQUIRE(dst && src, std::string(who) + ": null handle");
    TSL_REQUIRE(R_out && T_out, std::string(who) + ": null argument");
    int rc = track_check(t, who); if (rc) return rc;
    RegisterDev A;                                                 // every level is checked before anything runs
    for (int l = 0; l < t->n_levels; ++l) if ((rc = register_check(dst, dst_sid, src, src_sid, R0, T0, c, R_out, t->stride[l], &A, who))) return rc;
    hipStream_t q; long long* acc;
    if ((rc = register_stage(dst, src, &q, &acc))) return rc;
    return al_iterate(R0, T0, t, [&](int stride, const double* R, const double* T, tsl_align_sums* s) {
        const int rc2 = register_check(dst, dst_sid, src, src_sid, R, T, c, R_out, stride, &A, who); if (rc2) return rc2;
        return register_run(dst, dst_sid, src, src_sid, q, A, acc, s);
    }, R_out, T_out, rep);
}

}  // extern "C"

// tsl_register.hip -- map-to-map registration: a TSDF submap against another map, Gauss-Newton on the difference of the two signed distances.  The
// source's voxels near its surface are carried by X = (R, T) into the destination; there the destination's trilinear interpolant s (tsl_interp.hpp)
// should equal the value t the source stores: minimise the sum of (s(R q_i + T) - t_i)^2 over X.  The reference takes every submap pose from a pose
// graph outside and has no counterpart; this is the constraint such a graph consumes, and what re-anchors a tracked submap before it is fused.
//
// Definition (tests/register_ref.py restates it in numpy and every integer must equal it).  All f32, no contraction, in the
// written order.  Visited: the observed voxels (obs > 0) of the source submap whose indices (i, j, k) are each divisible by stride (1, 2, 4, 8 or 16).
// A visited voxel with the stored word tw falls into exactly one bucket:
//   gate     w = h2f(tw >> 16) fails w >= w_min, or not |t| <= band (a NaN is gated), t = h2f(tw & 0xffff); otherwise q = ((float)i vs, (float)j vs, (float)k vs),
//            p[a] = ((R[a][0] q0 + R[a][1] q1) + R[a][2] q2) + T[a]
//   unknown  the destination's sample at p is not KNOWN (section 4.7); otherwise s = tri_value, g = tri_grad / vs
//   far      not |s| <= r_max (a NaN s, from a stored value that is not finite, is far)
//   grad     gg = (g0 g0 + g1 g1) + g2 g2 is not in (0, g_max * g_max]
//   used     r = s - t, c = p x g, J = (g, c), wgt = huber > 0 && |r| > huber ? huber / |r| : 1, wJ = wgt J; the 28 products H_ab = wJ[a] J[b] (a <= b),
//            b_a = wJ[a] r, e = (wgt r) r, each added as rint(x * 2^20) into int64 sums (al_fix): the 33 integers of tsl_align_sums.
//
// The gate (pass 1 below) is tsl_register_common.hpp's, shared with tsl_register_search.hip; buckets unknown to used, the products and their reduction
// are tsl_align_common.hpp's (al_sample, al_products, al_flush), shared with tsl_align.hip.
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
#include "tsl_align_common.hpp"
#include "tsl_register_common.hpp"

namespace tsl {

#define RG_QUEUE TSL_BRK3              // entries of the LDS queue: every voxel of a brick can pass the gate

// At least 3 waves per SIMD: left alone the scheduler overlaps the 28 conversions and takes 194 VGPRs (2 waves); held to 168 it needs no scratch.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) k_register_linearize(MapDev S, int ss, MapDev D, int ds, RegisterDev A, long long* __restrict__ acc)
{
    __shared__ uint32_t queue[RG_QUEUE];
    __shared__ int q_total;                                       // entries queued so far by this workgroup, never reset: a brick's entries are those past `q_base`
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int* __restrict__ Td = D.table + (size_t)ds * D.nb3;
    if (threadIdx.x == 0) q_total = 0;
    __syncthreads();
    int top = *S.pool_top;                                        // bricks handed out; the counter may stand past the pool when it filled up
    if (top > S.max_bricks) top = S.max_bricks;
    const bool sums = !(A.flags & 1);
    long long v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = 0;
    int n_used = 0, n_gate = 0, n_unknown = 0, n_far = 0, n_grad = 0;      // per wave (uniform)
    int q_base = 0;

    for (int pb = blockIdx.x; pb < top; pb += gridDim.x) {
        int i0, j0, k0;
        if (!rg_brick_origin(S, pb, ss * S.nb3, &i0, &j0, &k0)) continue;      // uniform: the whole workgroup skips a brick of another submap

        // ---- pass 1: compaction ----
        rg_scan_row(S, A, pb, i0, j0, k0, [&](int r, bool seen, bool pass, uint32_t tw) {
            n_gate += popc64(__ballot(seen && !pass));
            rg_push(__ballot(pass), pass, r, tw, &q_total, queue, q_base);
        });
        __syncthreads();
        const int n = q_total - q_base;                           // at most 4096: one entry per voxel of the brick
        q_base += n;

        // ---- pass 2: the queue, densely ----
        for (int e0 = wave * 64; e0 < n; e0 += 256) {
            const int e = e0 + lane;
            int bucket = -1;
            float sv = 0.0f, tv = 0.0f, g[3] = { 0.0f, 0.0f, 0.0f }, p[3] = { 0.0f, 0.0f, 0.0f };
            if (e < n) {
                const uint32_t ent = queue[e];
                int i, j, k;
                rg_entry_voxel((int)(ent >> 16), i0, j0, k0, &i, &j, &k);
                tv = h2f((h16)(ent & 0xffffu));
                const float q0 = (float)i * A.vs, q1 = (float)j * A.vs, q2 = (float)k * A.vs;
#pragma unroll
                for (int a = 0; a < 3; ++a) p[a] = ((A.R[a * 3] * q0 + A.R[a * 3 + 1] * q1) + A.R[a * 3 + 2] * q2) + A.T[a];
                bucket = al_sample(p, D, Td, A.vs, A.r_max, A.gm2, &sv, g);
            }
            const bool used = bucket == AL_USED;
            if (used && sums) al_products(p, g, sv - tv, A.huber, v);
            n_used += popc64(__ballot(used)); n_unknown += popc64(__ballot(bucket == AL_UNKNOWN));
            n_far += popc64(__ballot(bucket == AL_FAR)); n_grad += popc64(__ballot(bucket == AL_GRAD));
        }
        __syncthreads();                                          // the queue is free for the next brick
    }
    al_flush(v, n_used, n_gate, n_unknown, n_far, n_grad, n_used && sums, acc);
}

// one linearisation on q with the result on the host: zero the accumulator, launch, copy back through the pinned buffer, wait
static int register_run(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, hipStream_t q, const RegisterDev& A, long long* acc, tsl_align_sums* out)
{
    TSL_HIP(hipMemsetAsync(acc, 0, AL_SLOTS * sizeof(long long), q));
    prof_begin(dst, TSL_K_REGISTER, q);                           // tsl_tsdf_prof_query(dst, TSL_K_REGISTER): the kernel alone, what tools/bench_register.py reports
    hipLaunchKernelGGL(k_register_linearize, dim3((unsigned)rg_grid(dst, src)), dim3(256), 0, q, src->M, rg_slot(src, src_sid), dst->M, rg_slot(dst, dst_sid), A, acc);
    prof_end(dst, q);
    TSL_HIP(hipGetLastError());
    return al_read_back(dst, q, acc, sizeof(tsl_align_sums), out);
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
    if ((rc = register_stage(dst, src, 512 + 64, &q, &acc))) return rc;
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
    if ((rc = register_stage(dst, src, 512 + 64, &q, &acc))) return rc;
    return al_iterate(R0, T0, t, [&](int stride, const double* R, const double* T, tsl_align_sums* s) {
        const int rc2 = register_check(dst, dst_sid, src, src_sid, R, T, c, R_out, stride, &A, who); if (rc2) return rc2;
        return register_run(dst, dst_sid, src, src_sid, q, A, acc, s);
    }, R_out, T_out, rep);
}

}  // extern "C"

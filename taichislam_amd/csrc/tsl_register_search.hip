// tsl_register_search.hip -- many poses scored in one call, and the search built on it: a lattice of candidate poses around a guess, each scored by
// brute force, the best one refined by tsl_tsdf_register_submap.  tsl_tsdf_register_submap is a local method; at a loop closure the guess from a
// drifted pose table can lie in the basin of another minimum (the quarter-turn alias of a room), and the registration then returns a confident wrong
// constraint.  The remedy is the one of correlative scan matching: score a window of poses, take the best, refine it locally.
//
// Definition (tests/register_search_ref.py restates it in numpy and every integer must equal it).  The score of pose k is
// e, n_used, n_unknown, n_far and n_grad of the tsl_align_sums that tsl_tsdf_register_linearize returns for that pose with the same handles, submap
// ids and configuration (section 4.9): the same lattice, gates, buckets, robust weight, f32 rounding of the pose and f32 order of evaluation.  The
// gradient is formed because n_grad depends on it (not for a far sample: al_sample returns before it); the 27 products of H and b are not.  The gather
// is pass 1 of tsl_register_common.hpp, the sample and the weight are al_sample and al_weight of tsl_align_common.hpp: the code of the linearisation.
//
// Kernels.  What does not depend on the pose is done once per call:
//   k_score_gather, counting   one workgroup per source brick, pass 1 of k_register_linearize (16-byte row loads, the lattice, weight and band tests,
//                              ballots): n_gate, n_pass and the integer sums of the passing voxels' indices -- tsl_register_gate and the size of the list
//   k_score_gather, filling    the same pass queues the survivors in LDS, reserves their places in the list with one atomic per brick and writes them
//                              as 8-byte entries { i | j << 16, k | t << 16 } (int16 indices, the f16 value), in any order: the sums are order-free
//   k_register_score           a 2-D grid, tiles of the list x chunks of 64 poses, one wave per workgroup.  The wave stages its tile in LDS; every
//                              lane owns one pose (12 floats in registers, loaded once) and walks the tile, so an entry read is an LDS broadcast and
//                              the 16 gathers of a sample are the lane's own.  e (int64) and the four counts stay in registers; at the end one
//                              integer atomic per non-zero value per pose per workgroup.  The tile is 256 entries, halved down to 64 while the grid
//                              would leave CUs idle (sc_tile; tsl_tsdf_register_score_tile tells which), so at most (entries / 64)
//                              workgroups add to one pose.  No float atomics.
// The other mapping -- lanes = entries, a wave reduction per pose -- was not built.
#include <cmath>
#include <memory>
#include <vector>
#include "tsl_align_common.hpp"
#include "tsl_register_common.hpp"

namespace tsl {

#define SC_TILE 256                    // entries of the largest tile
#define SC_POSES 64                    // poses of a chunk: one per lane
#define SC_MAX_POSES 65536
#define SC_CTR 8                       // int64 words at the start of the staging buffer: n_gate, n_pass, sum_i, sum_j, sum_k, the list's fill cursor
#define SC_POSE_OFF 1024               // bytes: the poses follow the counters (and the accumulator of tsl_register.hip, which a search uses afterwards)

static size_t sc_align(size_t b) { return (b + 255) & ~(size_t)255; }

// Pass 1 of k_register_linearize (rg_brick_origin, rg_scan_row, rg_push) over the bricks of submap `ss`.  list == nullptr: count (ctr[0..4]).
// Otherwise append the survivors to `list`, ctr[5] the cursor; `cap` = the n_pass a counting launch found on the same map, so no entry can land past it.
__global__ void __launch_bounds__(256) k_score_gather(MapDev S, int ss, RegisterDev A, long long* __restrict__ ctr, uint2* __restrict__ list, long long cap)
{
    __shared__ uint32_t queue[TSL_BRK3];
    __shared__ int q_n;
    __shared__ long long q_first;
    __shared__ long long sm[4][5];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool fill = list != nullptr;
    int top = *S.pool_top;
    if (top > S.max_bricks) top = S.max_bricks;
    long long n_gate = 0, n_pass = 0, si = 0, sj = 0, sk = 0;     // n_gate / n_pass per wave (uniform), the index sums per lane

    for (int pb = blockIdx.x; pb < top; pb += gridDim.x) {
        int i0, j0, k0;
        if (!rg_brick_origin(S, pb, ss * S.nb3, &i0, &j0, &k0)) continue;      // uniform: the whole workgroup skips a brick of another submap
        if (fill) {
            if (threadIdx.x == 0) q_n = 0;
            __syncthreads();
        }
        rg_scan_row(S, A, pb, i0, j0, k0, [&](int r, bool seen, bool pass, uint32_t tw) {
            const unsigned long long m = __ballot(pass);
            if (fill) rg_push(m, pass, r, tw, &q_n, queue, 0);
            else {
                n_gate += popc64(__ballot(seen && !pass));
                n_pass += popc64(m);
                if (pass) { si += i0 + (int)(threadIdx.x >> 4); sj += j0 + (int)(threadIdx.x & 15); sk += k0 + r; }
            }
        });
        if (fill) {
            __syncthreads();
            const int n = q_n;
            if (threadIdx.x == 0 && n) q_first = __hip_atomic_fetch_add(ctr + 5, (long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const long long at = q_first;
            for (int e = threadIdx.x; e < n; e += 256) {
                const uint32_t ent = queue[e];
                int i, j, k;
                rg_entry_voxel((int)(ent >> 16), i0, j0, k0, &i, &j, &k);
                if (at + e < cap) list[at + e] = make_uint2(((uint32_t)i & 0xffffu) | (((uint32_t)j & 0xffffu) << 16), ((uint32_t)k & 0xffffu) | ((ent & 0xffffu) << 16));
            }
        }
    }
    if (fill) return;
    si = wave_sum_ll(si); sj = wave_sum_ll(sj); sk = wave_sum_ll(sk);
    if (lane == 0) { sm[wave][0] = n_gate; sm[wave][1] = n_pass; sm[wave][2] = si; sm[wave][3] = sj; sm[wave][4] = sk; }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int t = threadIdx.x;
        const long long sum = (sm[0][t] + sm[1][t]) + (sm[2][t] + sm[3][t]);
        if (sum != 0) __hip_atomic_fetch_add(ctr + t, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// blockIdx.x: the tile of `tile` (<= SC_TILE) entries, blockIdx.y: the chunk of 64 poses; lane = pose.  A carries the gates; its pose is not read.
__global__ void __launch_bounds__(SC_POSES) k_register_score(MapDev D, int ds, RegisterDev A, const uint2* __restrict__ list, long long len, int tile,
                                                             const float* __restrict__ poses, int n, tsl_register_score* __restrict__ out)
{
    __shared__ uint2 ent[SC_TILE];
    const long long first = (long long)blockIdx.x * tile;
    const int cnt = (int)(len - first < (long long)tile ? len - first : (long long)tile);
    for (int e = threadIdx.x; e < cnt; e += SC_POSES) ent[e] = list[first + e];
    __syncthreads();
    const int k = blockIdx.y * SC_POSES + threadIdx.x;
    if (k >= n) return;
    const int* __restrict__ Td = D.table + (size_t)ds * D.nb3;
    const float4* pp = reinterpret_cast<const float4*>(poses + (size_t)k * 12);
    const float4 p0 = pp[0], p1 = pp[1], p2 = pp[2];
    const float R[9] = { p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x }, T[3] = { p2.y, p2.z, p2.w };
    const bool sums = !(A.flags & 1);
    long long e_sum = 0;
    int n_used = 0, n_unknown = 0, n_far = 0, n_grad = 0;
    for (int e = 0; e < cnt; ++e) {
        const uint2 en = ent[e];                                  // the same address in every lane: a broadcast
        const float tv = h2f((h16)(en.y >> 16));
        const float q0 = (float)(int)(short)(en.x & 0xffffu) * A.vs, q1 = (float)(int)(short)(en.x >> 16) * A.vs, q2 = (float)(int)(short)(en.y & 0xffffu) * A.vs;
        float p[3], sv, g[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = ((R[a * 3] * q0 + R[a * 3 + 1] * q1) + R[a * 3 + 2] * q2) + T[a];
        const int bucket = al_sample(p, D, Td, A.vs, A.r_max, A.gm2, &sv, g);
        if (bucket == AL_UNKNOWN) { ++n_unknown; continue; }
        if (bucket == AL_FAR) { ++n_far; continue; }
        if (bucket == AL_GRAD) { ++n_grad; continue; }
        ++n_used;
        if (sums) { const float r = sv - tv; e_sum += al_fix((al_weight(r, A.huber) * r) * r); }
    }
    tsl_register_score* o = out + k;
    if (e_sum != 0) __hip_atomic_fetch_add((long long*)&o->e, e_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_used) __hip_atomic_fetch_add(&o->n_used, n_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_unknown) __hip_atomic_fetch_add(&o->n_unknown, n_unknown, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_far) __hip_atomic_fetch_add(&o->n_far, n_far, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_grad) __hip_atomic_fetch_add(&o->n_grad, n_grad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The checks of a score call and the call itself; `who` names the entry point in a refusal.  m_min: see register_check.
static int score_check(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double* R, const double* T, int32_t n, const tsl_register_cfg* c, const void* out,
                       int stride, RegisterDev* A, const char* who, double m_min)
{
    const std::string w(who);
    TSL_REQUIRE(dst && src, w + ": null handle");
    TSL_REQUIRE(R && T && c && out, w + ": null argument");
    TSL_REQUIRE(n >= 1 && n <= SC_MAX_POSES, w + ": 1 .. 65536 poses");
    TSL_REQUIRE(al_finite(R, 9 * n) && al_finite(T, 3 * n), w + ": a pose is not finite");
    return register_check(dst, dst_sid, src, src_sid, R, T, c, out, stride, A, who, m_min);      // the pose is the only part of the checks that differs from pose to pose
}

// the tile of k_register_score for a list of `len` entries and `chunks` chunks of poses: 256, halved down to 64 while the grid would leave CUs idle
static int sc_tile(long long len, long long chunks, int ncu)
{
    int tile = SC_TILE;
    while (tile > 64 && ((len + tile - 1) / tile) * chunks < 8LL * ncu) tile >>= 1;
    return tile;
}

// The counting pass alone: what does not depend on the pose.  The stream is idle when it returns.
static int gate_run(tsl_tsdf* dst, tsl_tsdf* src, int src_sid, const RegisterDev& A, tsl_register_gate* gate)
{
    hipStream_t q; long long* ctr;
    const int rc = register_stage(dst, src, SC_POSE_OFF, &q, &ctr); if (rc) return rc;
    TSL_HIP(hipMemsetAsync(ctr, 0, SC_CTR * sizeof(long long), q));
    hipLaunchKernelGGL(k_score_gather, dim3((unsigned)rg_grid(dst, src)), dim3(256), 0, q, src->M, rg_slot(src, src_sid), A, ctr, (uint2*)nullptr, 0LL);
    TSL_HIP(hipGetLastError());
    return al_read_back(dst, q, ctr, sizeof(*gate), gate);
}

static int score_run(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double* R, const double* T, int32_t n, const RegisterDev& A,
                     tsl_register_score* out, tsl_register_gate* gate)
{
    tsl_register_gate g;
    int rc = gate_run(dst, src, src_sid, A, &g); if (rc) return rc;
    hipStream_t q = ms(dst);
    const int grid = rg_grid(dst, src);
    const int ss = rg_slot(src, src_sid), ds = rg_slot(dst, dst_sid);
    if (gate) *gate = g;
    std::memset(out, 0, sizeof(tsl_register_score) * (size_t)n);
    const long long len = g.n_pass;
    if (len == 0) return TSL_OK;                                   // nothing to register: every score is zero

    const size_t pose_bytes = sc_align(sizeof(float) * 12 * (size_t)n), out_bytes = sc_align(sizeof(tsl_register_score) * (size_t)n);
    rc = grow(&dst->xbuf, &dst->xbuf_bytes, SC_POSE_OFF + pose_bytes + out_bytes + sizeof(uint2) * (size_t)len); if (rc) return rc;      // the stream is idle: nothing reads the old buffer
    long long* ctr = (long long*)dst->xbuf;
    float* poses_dev = (float*)((char*)dst->xbuf + SC_POSE_OFF);
    tsl_register_score* out_dev = (tsl_register_score*)((char*)dst->xbuf + SC_POSE_OFF + pose_bytes);
    uint2* list = (uint2*)((char*)dst->xbuf + SC_POSE_OFF + pose_bytes + out_bytes);
    std::vector<float> poses((size_t)n * 12);                      // rounded to f32 once, as register_check rounds the pose of a linearisation
    for (int k = 0; k < n; ++k) {
        for (int i = 0; i < 9; ++i) poses[(size_t)k * 12 + i] = (float)R[(size_t)k * 9 + i];
        for (int i = 0; i < 3; ++i) poses[(size_t)k * 12 + 9 + i] = (float)T[(size_t)k * 3 + i];
    }
    TSL_HIP(hipMemsetAsync(ctr, 0, SC_CTR * sizeof(long long), q));
    TSL_HIP(hipMemsetAsync(out_dev, 0, sizeof(tsl_register_score) * (size_t)n, q));
    TSL_HIP(hipMemcpyAsync(poses_dev, poses.data(), sizeof(float) * poses.size(), hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(k_score_gather, dim3((unsigned)grid), dim3(256), 0, q, src->M, ss, A, ctr, list, len);
    TSL_HIP(hipGetLastError());
    const int chunks = (n + SC_POSES - 1) / SC_POSES;
    const int tile = sc_tile(len, chunks, dst->ncu);
    const long long tiles = (len + tile - 1) / tile;
    prof_begin(dst, TSL_K_REGISTER_SCORE, q);                      // tsl_tsdf_prof_query(dst, TSL_K_REGISTER_SCORE): the score kernel alone
    hipLaunchKernelGGL(k_register_score, dim3((unsigned)tiles, (unsigned)chunks), dim3(SC_POSES), 0, q, dst->M, ds, A, list, len, tile, poses_dev, (int)n, out_dev);
    prof_end(dst, q);
    TSL_HIP(hipGetLastError());
    TSL_HIP(hipMemcpyAsync(out, out_dev, sizeof(tsl_register_score) * (size_t)n, hipMemcpyDeviceToHost, q));
    TSL_HIP(hipStreamSynchronize(q));
    return TSL_OK;
}

// rint(x * 2^20) of an f32 value on the host: al_fix
static int64_t sc_fix(float x) { return (int64_t)std::rint((double)x * 1048576.0); }

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_register_score(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double* R, const double* T, int32_t n,
                            const tsl_register_cfg* c, tsl_register_score* out, tsl_register_gate* gate)
{
    RegisterDev A;
    const int rc = score_check(dst, dst_sid, src, src_sid, R, T, n, c, out, c ? c->stride : 1, &A, "register_score", 0.0); if (rc) return rc;
    return score_run(dst, dst_sid, src, src_sid, R, T, n, A, out, gate);
}

int tsl_tsdf_register_score_tile(tsl_tsdf* dst, int64_t entries, int32_t n)
{
    if (!dst || entries < 1 || n < 1 || n > SC_MAX_POSES) return 0;
    return sc_tile((long long)entries, (n + SC_POSES - 1) / SC_POSES, dst->ncu);
}

int tsl_tsdf_register_search(tsl_tsdf* dst, int dst_sid, tsl_tsdf* src, int src_sid, const double R0[9], const double T0[3],
                             const tsl_register_cfg* c, const tsl_search_cfg* s, const tsl_track_cfg* t,
                             double R_out[9], double T_out[3], tsl_search_report* rep, tsl_track_report* trk, tsl_register_score* scores)
{
    const char* who = "register_search";
    const std::string w(who);
    TSL_REQUIRE(dst && src, w + ": null handle");
    TSL_REQUIRE(R0 && T0 && c && s && R_out && T_out && rep, w + ": null argument");
    int rc = track_check(t, who); if (rc) return rc;
    // the lattice
    long long count = 1;
    for (int a = 0; a < 6; ++a) {
        const int32_t na = a < 3 ? s->n_r[a] : s->n_t[a - 3];
        const double step = a < 3 ? s->step_r[a] : s->step_t[a - 3];
        TSL_REQUIRE(na >= 0, w + ": a half-count is negative");
        TSL_REQUIRE(std::isfinite(step) && (na == 0 || step > 0.0), w + ": a step is not finite, or not positive on an axis with n > 0");
        TSL_REQUIRE(na <= SC_MAX_POSES, w + ": more than 65536 candidates");
        count *= 2 * (long long)na + 1;
        TSL_REQUIRE(count <= SC_MAX_POSES, w + ": more than 65536 candidates");
    }
    TSL_REQUIRE(!(s->flags & 1) || al_finite(s->pivot, 3), w + ": the pivot is not finite");
    TSL_REQUIRE(rg_finite(s->miss) && !(s->miss < 0.0f), w + ": miss must be finite and not negative");
    TSL_REQUIRE(s->min_used >= 0, w + ": min_used must not be negative");
    // every level of the refinement and the scoring stride are checked before anything runs; M >= miss: no cost can overflow
    RegisterDev A;
    const float miss = s->miss != 0.0f ? s->miss : rg_r_max(dst, c);
    if ((rc = register_check(dst, dst_sid, src, src_sid, R0, T0, c, R_out, s->stride, &A, who, (double)miss))) return rc;
    RegisterDev Al;
    for (int l = 0; l < t->n_levels; ++l) if ((rc = register_check(dst, dst_sid, src, src_sid, R0, T0, c, R_out, t->stride[l], &Al, who))) return rc;

    const int n = (int)count;
    // what a search that ends before the refinement returns: status 2 and the guess.  Written only once no refusal can follow.
    auto start = [&](const tsl_register_gate& g, const double* pivot) {
        std::memset(rep, 0, sizeof(*rep));
        rep->n_candidates = n; rep->best = -1; rep->status = 2; rep->gate = g;
        if (pivot) std::memcpy(rep->pivot, pivot, 3 * sizeof(double));
        std::memcpy(R_out, R0, 9 * sizeof(double)); std::memcpy(T_out, T0, 3 * sizeof(double));
        std::memcpy(rep->R_best, R0, 9 * sizeof(double)); std::memcpy(rep->T_best, T0, 3 * sizeof(double));
        if (trk) { trk->status = 2; trk->iterations = 0; }
        if (scores) std::memset(scores, 0, sizeof(tsl_register_score) * (size_t)n);
    };

    // the pivot: given, or the centroid of the gated source voxels carried by the guess -- the gate needs the counting pass only, not a score
    double pivot[3];
    tsl_register_gate g0;
    std::memset(&g0, 0, sizeof(g0));
    if (s->flags & 1) std::memcpy(pivot, s->pivot, sizeof(pivot));
    else {
        if ((rc = gate_run(dst, src, src_sid, A, &g0))) return rc;
        if (g0.n_pass == 0) { start(g0, nullptr); return TSL_OK; }      // status 2: nothing to register
        const double np = (double)g0.n_pass, vs = dst->cfg.voxel_scale;
        const double qb[3] = { ((double)g0.sum_i / np) * vs, ((double)g0.sum_j / np) * vs, ((double)g0.sum_k / np) * vs };
        for (int a = 0; a < 3; ++a) pivot[a] = ((R0[a * 3] * qb[0] + R0[a * 3 + 1] * qb[1]) + R0[a * 3 + 2] * qb[2]) + T0[a];
    }

    // the candidates: k runs over (r0, r1, r2, t0, t1, t2), the last fastest
    std::vector<double> Rc((size_t)n * 9), Tc((size_t)n * 3);
    {
        int idx[6] = { 0, 0, 0, 0, 0, 0 };
        const int32_t nn[6] = { s->n_r[0], s->n_r[1], s->n_r[2], s->n_t[0], s->n_t[1], s->n_t[2] };
        const double st[6] = { s->step_r[0], s->step_r[1], s->step_r[2], s->step_t[0], s->step_t[1], s->step_t[2] };
        for (int k = 0; k < n; ++k) {
            double off[6]; bool centre = true;
            for (int a = 0; a < 6; ++a) { off[a] = (double)(idx[a] - nn[a]) * st[a]; centre = centre && idx[a] == nn[a]; }
            double* Rk = &Rc[(size_t)k * 9]; double* Tk = &Tc[(size_t)k * 3];
            std::memcpy(Rk, R0, 9 * sizeof(double));
            if (centre) std::memcpy(Tk, T0, 3 * sizeof(double));   // the centre of the lattice is the guess itself, bit for bit
            else {
                const double xi[6] = { 0.0, 0.0, 0.0, off[0], off[1], off[2] };
                double Tp[3] = { T0[0] - pivot[0], T0[1] - pivot[1], T0[2] - pivot[2] };
                al_retract(xi, Rk, Tp);
                for (int a = 0; a < 3; ++a) Tk[a] = (Tp[a] + pivot[a]) + off[3 + a];
            }
            for (int a = 5; a >= 0; --a) { if (++idx[a] <= 2 * nn[a]) break; idx[a] = 0; }
        }
    }

    // a finite guess far enough out can give a candidate that is not: the last refusal, before any output is written
    TSL_REQUIRE(al_finite(Rc.data(), 9 * n) && al_finite(Tc.data(), 3 * n), w + ": a candidate pose is not finite");
    start(g0, pivot);

    // score and rank: J = e + F n_far + U (n_unknown + n_grad), exact integers; the least J among the valid candidates, ties to the least k
    std::vector<tsl_register_score> own;
    tsl_register_score* sc = scores;
    if (!sc) { own.resize((size_t)n); sc = own.data(); }
    if ((rc = score_run(dst, dst_sid, src, src_sid, Rc.data(), Tc.data(), n, A, sc, &rep->gate))) return rc;
    const int64_t F = sc_fix(A.r_max * A.r_max), U = sc_fix(miss * miss);
    const int32_t min_used = s->min_used > 0 ? s->min_used : 6;
    int best = -1; int64_t Jb = 0; int n_valid = 0;
    for (int k = 0; k < n; ++k) {
        if (sc[k].n_used < min_used) continue;
        ++n_valid;
        const int64_t J = sc[k].e + F * (int64_t)sc[k].n_far + U * ((int64_t)sc[k].n_unknown + (int64_t)sc[k].n_grad);
        if (best < 0 || J < Jb) { best = k; Jb = J; }
    }
    rep->n_valid = n_valid;
    if (best < 0) return TSL_OK;                                   // status 2: no valid candidate, the pose out is the guess
    rep->best = best; rep->J_best = Jb; rep->score_best = sc[best];
    std::memcpy(rep->R_best, &Rc[(size_t)best * 9], 9 * sizeof(double)); std::memcpy(rep->T_best, &Tc[(size_t)best * 3], 3 * sizeof(double));

    // refine: the iteration of tsl_tsdf_register_submap from the best candidate
    std::unique_ptr<tsl_track_report> mine;
    if (!trk) { mine.reset(new tsl_track_report); trk = mine.get(); }
    if ((rc = tsl_tsdf_register_submap(dst, dst_sid, src, src_sid, rep->R_best, rep->T_best, c, t, R_out, T_out, trk))) return rc;
    rep->status = trk->status;
    return TSL_OK;
}

}  // extern "C"

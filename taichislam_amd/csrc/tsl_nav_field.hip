// tsl_nav_field.hip -- cost-to-go fields and paths over 2-D cost planes: how expensive it is to get from every cell to the
// nearest goal, and along which cells.  The planes are the caller's (usually the `cost` output of tsl_tsdf_nav_grid); the handle supplies the device,
// the stream and scratch, and no map is read.  Everything is integer and the answer is the unique minimum of a sum of positive integers, so the
// result depends on no schedule and tests/nav_field_ref.py restates it bit for bit.
//
// Definition (include/taichislam_hip.h says the same).  cost u8 [B][H][W]; a cell is traversable when cost < lethal.  Direction codes 0 .. 7 are
//   (di, dj) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1); odd codes only with connectivity 8, and only when both cells the diagonal passes
//   between are traversable.  Step length s = 5 (axis) or 7 (diagonal).  field[x] = the minimum over move sequences from x to a seed cell of
//   value(seed) + sum of s * (neutral + cost[cell left]), clipped to 2^32 - 2; TSL_NAV_UNREACHED = 2^32 - 1 where no seed is reached.
//
// This file holds what is specific to 2-D: the two tuned kernels and the traits struct Nf2 that describes the solver.  The state, the control block, the
// clipped add, the seed, finish, seed-parent and paths kernels, the checks, the round loop (the host stops the rounds: every check_every rounds it reads
// the 4-byte count of marks the last round made) and the bodies of the entry points are in tsl_nav_field_common.hpp, shared with tsl_nav_field3.hip.  In
// the shared configuration NfCfg a stack of B planes is D = B with tz = B tiles of one plane each, and connectivity 4 / 8 is the move rank nz = 1 / 2.
//
//   k_nf_round    one round = one launch, one workgroup per 32 x 32 tile; a tile that is not marked active exits at once.  An active tile loads its
//                 field and cost with a one-cell halo into LDS (34 x 34 words + 34 x 34 halves, 6.8 KiB), turns the cost into a per-cell move mask and
//                 weight in registers, and relaxes in LDS -- every lane owns 4 cells, a half-wave reads 32 consecutive words: no bank conflict -- until a
//                 block of NF_BLOCK sweeps changes nothing or NF_SWEEPS is reached (then it marks itself).  Only the owner writes a tile's cells back; when a border cell
//                 changed it marks the neighbours that see it in the NEXT round's activity map (two maps, swapped every round) and counts the marks.
//                 Values only fall and each is the cost of a real move sequence, so a halo read that races a neighbour's write-back -- it sees the old
//                 or the new aligned word -- is harmless, and whoever changed a border cell marks the reader for the next round anyway.
//   k_nf_parent   one lane per cell: the lowest direction code whose neighbour explains the cell's value.
// No workgroup waits for another, there is no flag to spin on, and every loop has a bound known at launch (NF_SWEEPS, L).
#include "tsl_nav_field_common.hpp"

namespace tsl {

#define NF_T 32                    // tile edge in cells
#define NF_LD (NF_T + 2)           // a staged row: the tile and its halo
#define NF_SWEEPS 64               // sweeps of a tile per round at most ...
#define NF_BLOCK 8                 // ... in blocks of this many between two votes

__constant__ int c_nf_di[8] = { 1, 1, 0, -1, -1, -1, 0, 1 };
__constant__ int c_nf_dj[8] = { 0, 1, 1, 1, 0, -1, -1, -1 };

// ---- one round -------------------------------------------------------------------------------------------------------------------------------
// grid (tx, ty, B).  act_cur: this round's activity map (a tile clears its own word), act_next: the next round's.  parity = round & 1.
__global__ void __launch_bounds__(256) k_nf_round(NfCfg C, const uint8_t* __restrict__ cost, uint32_t* field, uint32_t* act_cur, uint32_t* act_next, NfCtl* ctl,
                                                  int round)
{
    __shared__ uint32_t sf[NF_LD * NF_LD];
    __shared__ uint16_t sw[NF_LD * NF_LD];                          // neutral + cost of a traversable cell, 0 for a wall and outside the plane
    __shared__ uint32_t s_edges;
    const int tid = threadIdx.x, parity = round & 1;
    const int tc = (int)blockIdx.x, tr = (int)blockIdx.y, p = (int)blockIdx.z;
    const size_t tile = ((size_t)p * C.ty + tr) * C.tx + tc;
    if (tile == 0 && tid == 0) ctl->marks[parity ^ 1] = 0u;         // the next round counts from 0; nobody else touches that word in this round
    if (act_cur[tile] == 0u) return;                                // (uniform)
    if (tid == 0) s_edges = 0u;
    __syncthreads();                                                // every lane has read the word
    if (tid == 0) act_cur[tile] = 0u;

    const int r0 = tr * NF_T, c0 = tc * NF_T;
    const size_t plane = (size_t)p * C.H * C.W;
    for (int e = tid; e < NF_LD * NF_LD; e += 256) {
        const int lr = e / NF_LD, lc = e - lr * NF_LD;
        const int r = r0 - 1 + lr, c = c0 - 1 + lc;
        uint32_t f = TSL_NAV_UNREACHED, w = 0u;
        if (r >= 0 && r < C.H && c >= 0 && c < C.W) {
            const size_t o = plane + (size_t)r * C.W + c;
            const int cs = cost[o];
            if (cs < C.lethal) { w = (uint32_t)(C.neutral + cs); f = field[o]; }
        }
        sf[e] = f; sw[e] = (uint16_t)w;
    }
    __syncthreads();

    // the lane's 4 cells: column tid & 31, rows (tid >> 5) + 8 k
    int idx[4]; uint32_t f0[4], f[4], wa[4], wd[4], mask[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lr = (tid >> 5) + 8 * k + 1, lc = (tid & 31) + 1;
        idx[k] = lr * NF_LD + lc;
        const uint32_t w = sw[idx[k]];
        f0[k] = f[k] = sf[idx[k]];
        wa[k] = 5u * w; wd[k] = 7u * w;
        uint32_t m = 0u;
        if (w) {
            const bool dn = sw[idx[k] + NF_LD] != 0, up = sw[idx[k] - NF_LD] != 0, rt = sw[idx[k] + 1] != 0, lf = sw[idx[k] - 1] != 0;
            m = (dn ? 1u : 0u) | (rt ? 4u : 0u) | (up ? 16u : 0u) | (lf ? 64u : 0u);
            if (C.nz > 1) {
                if (dn && rt && sw[idx[k] + NF_LD + 1]) m |= 2u;
                if (up && rt && sw[idx[k] - NF_LD + 1]) m |= 8u;
                if (up && lf && sw[idx[k] - NF_LD - 1]) m |= 32u;
                if (dn && lf && sw[idx[k] + NF_LD - 1]) m |= 128u;
            }
        }
        mask[k] = m;
    }

    // Sweeps in place, NF_BLOCK at a time without a barrier: a lane reads whatever its neighbours hold at that moment, each a valid upper bound.  The 32
    // reads of a sweep are issued together (one LDS latency per sweep, not one per read; a half-wave reads 32 consecutive words: no bank conflict) and
    // the lane's 4 cells, 8 rows apart, are 4 independent chains of arithmetic; the empty asm keeps the compiler from carrying LDS values from one
    // sweep into the next.  The vote comes once per block; a block in which no lane wrote saw constant values throughout, and every lane tested its
    // cells against them: the tile is at rest against this halo.  Walls and cells outside hold TSL_NAV_UNREACHED for ever, so the axis reads need no
    // mask; the diagonal ones do (the corner rule).
    int block = 0;
    for (; block < NF_SWEEPS / NF_BLOCK; ++block) {
        bool ch = false;
        for (int sweep = 0; sweep < NF_BLOCK; ++sweep) {
            uint32_t ma[4], md[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t m = mask[k];
                const int i = idx[k];
                const uint32_t a0 = sf[i + NF_LD], a1 = sf[i + 1], a2 = sf[i - NF_LD], a3 = sf[i - 1];
                const uint32_t d0 = sf[i + NF_LD + 1], d1 = sf[i - NF_LD + 1], d2 = sf[i - NF_LD - 1], d3 = sf[i + NF_LD - 1];
                ma[k] = min(min(a0, a1), min(a2, a3));
                md[k] = min(min((m & 2u) ? d0 : TSL_NAV_UNREACHED, (m & 8u) ? d1 : TSL_NAV_UNREACHED),
                            min((m & 32u) ? d2 : TSL_NAV_UNREACHED, (m & 128u) ? d3 : TSL_NAV_UNREACHED));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t cand = min(nf_add(ma[k], wa[k]), nf_add(md[k], wd[k]));
                if (mask[k] && cand < f[k]) { f[k] = cand; sf[idx[k]] = cand; ch = true; }
            }
            __asm__ volatile("" ::: "memory");
        }
        if (!__syncthreads_or(ch ? 1 : 0)) break;                   // (uniform)
    }
    const bool capped = block == NF_SWEEPS / NF_BLOCK;

    // write back what fell; bits 0 .. 3: a cell of the top / bottom / left / right border changed, 4 .. 7: the corner cell tl / tr / bl / br
    uint32_t edges = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (f[k] >= f0[k]) continue;
        const int lr = (tid >> 5) + 8 * k, lc = tid & 31;
        field[plane + (size_t)(r0 + lr) * C.W + c0 + lc] = f[k];      // (a cell outside the plane has mask 0 and never changes)
        const bool t = lr == 0, b = lr == NF_T - 1, l = lc == 0, r = lc == NF_T - 1;
        edges |= (t ? 1u : 0u) | (b ? 2u : 0u) | (l ? 4u : 0u) | (r ? 8u : 0u) | (t && l ? 16u : 0u) | (t && r ? 32u : 0u) | (b && l ? 64u : 0u) | (b && r ? 128u : 0u);
    }
    if (edges) atomicOr(&s_edges, edges);
    __syncthreads();
    if (tid != 0) return;
    const uint32_t e = s_edges;
    uint32_t n = 0u;
    const bool up = tr > 0, dn = tr + 1 < C.ty, lf = tc > 0, rt = tc + 1 < C.tx;
    const size_t row = (size_t)C.tx;
    if ((e & 1u) && up) { act_next[tile - row] = 1u; ++n; }
    if ((e & 2u) && dn) { act_next[tile + row] = 1u; ++n; }
    if ((e & 4u) && lf) { act_next[tile - 1] = 1u; ++n; }
    if ((e & 8u) && rt) { act_next[tile + 1] = 1u; ++n; }
    if (C.nz > 1) {
        if ((e & 16u) && up && lf) { act_next[tile - row - 1] = 1u; ++n; }
        if ((e & 32u) && up && rt) { act_next[tile - row + 1] = 1u; ++n; }
        if ((e & 64u) && dn && lf) { act_next[tile + row - 1] = 1u; ++n; }
        if ((e & 128u) && dn && rt) { act_next[tile + row + 1] = 1u; ++n; }
    }
    if (capped) { act_next[tile] = 1u; ++n; }
    if (n) atomicAdd(&ctl->marks[parity], n);
    atomicAdd(&ctl->visits, 1ull);
    atomicMax(&ctl->rounds, round + 1);
}

// ---- parents ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nf_parent(NfCfg C, const uint8_t* __restrict__ cost, const uint32_t* __restrict__ field, uint8_t* __restrict__ parent)
{
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t hw = (size_t)C.H * C.W;
    if (o >= hw * C.D) return;
    const size_t plane = o / hw * hw;
    const int r = (int)((o - plane) / C.W), c = (int)((o - plane) - (size_t)r * C.W);
    const uint32_t f = field[o];
    const int cs = cost[o];
    uint32_t par = 255u;
    if (f != TSL_NAV_UNREACHED && cs < C.lethal) {
        const uint32_t w = (uint32_t)(C.neutral + cs);
        bool open[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int nr = r + c_nf_di[d], nc = c + c_nf_dj[d];
            open[d] = nr >= 0 && nr < C.H && nc >= 0 && nc < C.W && (int)cost[plane + (size_t)nr * C.W + nc] < C.lethal;
        }
#pragma unroll
        for (int d = 7; d >= 0; --d) {                              // downwards: the lowest code that explains f is the one that stays
            bool ok = open[d];
            if (d & 1) ok = ok && C.nz > 1 && open[d - 1] && open[(d + 1) & 7];
            if (!ok) continue;
            const uint32_t fn = field[plane + (size_t)(r + c_nf_di[d]) * C.W + c + c_nf_dj[d]];
            if (fn != TSL_NAV_UNREACHED && nf_add(fn, (d & 1 ? 7u : 5u) * w) == f) par = (uint32_t)d;
        }
    }
    parent[o] = (uint8_t)par;
}

// ---- the solver, as tsl_nav_field_common.hpp sees it -----------------------------------------------------------------------------------------
struct Nf2 {
    static constexpr int TX = NF_T, TY = NF_T, TZ = 1, SEED = 8, NCOMP = 2;
    static constexpr bool LINKED = false;                           // the leading axis counts independent planes
    typedef tsl_nav_field_cfg cfg_t;
    typedef tsl_nav_field_stats stats_t;
    static constexpr const char* name = "nav_field";
    static constexpr const char* conn_text = ": connectivity must be 4 or 8";
    static constexpr int K_SEED = TSL_K_NAV_FIELD_SEED, K_ROUND = TSL_K_NAV_FIELD_ROUND, K_PARENT = TSL_K_NAV_FIELD_PARENT, K_PATHS = TSL_K_NAV_FIELD_PATHS;
    static NavFieldState*& state(tsl_tsdf* m) { return m->nav_field; }
    static int dims(const cfg_t* c, const std::string& w, NfCfg* C)
    {
        TSL_REQUIRE(c->B >= 1 && c->B <= 16, w + ": B must be 1 .. 16 planes");
        TSL_REQUIRE(c->H >= 1 && c->H <= 4096, w + ": H must be 1 .. 4096");
        TSL_REQUIRE(c->W >= 1 && c->W <= 4096, w + ": W must be 1 .. 4096");
        C->D = c->B; C->H = c->H; C->W = c->W;
        return TSL_OK;
    }
    static int rank(int conn) { return conn == 4 ? 1 : (conn == 8 ? 2 : 0); }
    static int default_rounds(const NfCfg& C) { return 4 * C.tx * C.ty + 64; }      // the tiles of one plane: the planes do not exchange anything
    __device__ static void step(int code, int&, int& r, int& c) { r += c_nf_di[code]; c += c_nf_dj[code]; }
    static void round(hipStream_t q, const NfCfg& C, const uint8_t* cost, uint32_t* field, uint32_t* act_cur, uint32_t* act_next, NfCtl* ctl, int r)
    {
        hipLaunchKernelGGL(k_nf_round, dim3((unsigned)C.tx, (unsigned)C.ty, (unsigned)C.tz), dim3(256), 0, q, C, cost, field, act_cur, act_next, ctl, r);
    }
    static void parent(hipStream_t q, const NfCfg& C, const uint8_t* cost, const uint32_t* field, uint8_t* par)
    {
        hipLaunchKernelGGL(k_nf_parent, dim3((unsigned)(((size_t)C.D * C.H * C.W + 255) / 256)), dim3(256), 0, q, C, cost, field, par);
    }
};

void nav_field_release(tsl_tsdf* m) { nf_release(&m->nav_field); }

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_nav_field(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const uint8_t* cost, const int32_t* seeds, int32_t n_seeds, uint32_t* field, uint8_t* parent,
                       tsl_nav_field_stats* stats)
{
    return nf_field_host<Nf2>(m, cfg, cost, seeds, n_seeds, field, parent, stats);
}

int tsl_tsdf_nav_field_dev(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const void* cost_dev, const void* seeds_dev, int32_t n_seeds, void* field_dev, void* parent_dev,
                           void* stats_dev, void* user_stream)
{
    return nf_field_dev<Nf2>(m, cfg, cost_dev, seeds_dev, n_seeds, field_dev, parent_dev, stats_dev, user_stream);
}

int tsl_tsdf_nav_field_paths(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const uint32_t* field, const uint8_t* parent, const int32_t* starts, int32_t n_starts,
                             int32_t max_len, int16_t* cells, int32_t* length, uint8_t* status, uint32_t* cost)
{
    return nf_paths_host<Nf2>(m, cfg, field, parent, starts, n_starts, max_len, cells, length, status, cost);
}

int tsl_tsdf_nav_field_paths_dev(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const void* field_dev, const void* parent_dev, const void* starts_dev, int32_t n_starts,
                                 int32_t max_len, void* cells_dev, void* length_dev, void* status_dev, void* cost_dev, void* user_stream)
{
    return nf_paths_dev<Nf2>(m, cfg, field_dev, parent_dev, starts_dev, n_starts, max_len, cells_dev, length_dev, status_dev, cost_dev, user_stream);
}

}  // extern "C"

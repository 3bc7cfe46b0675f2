// tsl_nav_field3.hip -- cost-to-go fields and paths over 3-D cost volumes: how expensive it is to fly from every cell to the
// nearest goal, and along which cells.  The volume is the caller's (usually DenseTSDF.flight_volume: the ESDF sampled at a stride); the handle supplies
// the device, the stream and scratch, and no map is read.  It is the scheme of tsl_nav_field.hip carried into 3-D: everything is integer and the answer
// is the unique minimum of a sum of positive integers, so the result depends on no schedule and tests/nav_field3d_ref.py restates it bit for bit.
//
// Definition (include/taichislam_hip.h says the same).  cost u8 [D][H][W], layer k, row i, column j; a cell is traversable when cost < lethal.  Direction
//   codes 0 .. 25 are (dk, di, dj): 0 .. 7 = (0, the (di, dj) of nav_field's codes 0 .. 7), 8 = (1,0,0), 9 .. 16 = (1, the same eight), 17 = (-1,0,0),
//   18 .. 25 = (-1, the same eight).  Connectivity 6 / 18 / 26 = the codes with at most 1 / 2 / 3 non-zero components; step length s = 5 / 7 / 9 for 1 / 2 /
//   3 of them.  A move by (dk, di, dj) is allowed only when every cell x + (a dk, b di, c dj), a, b, c in {0, 1}, is inside and traversable.
//   field[x] = the minimum over move sequences from x to a seed cell of value(seed) + sum of s * (neutral + cost[cell left]), clipped to 2^32 - 2;
//   TSL_NAV_UNREACHED = 2^32 - 1 where no seed is reached.
//
// This file holds what is specific to 3-D: the two tuned kernels, the compile-time direction helpers they need and the traits struct Nf3 that describes
// the solver.  The state, the control block, the clipped add, the seed, finish, seed-parent and paths kernels, the checks, the round loop with the host's
// check and the bodies of the entry points are in tsl_nav_field_common.hpp, shared with tsl_nav_field.hip.
//
//   k_nf3_round   one round = one launch, one workgroup per tile; a tile that is not marked active exits at once.  An active tile loads its field and
//                 cost with a one-cell halo on all six faces, edges and corners included, into LDS, turns the cost into per-cell registers (5 w, 7 w, 9 w
//                 and a 26-bit mask of allowed moves, which keeps the corner rule out of the loop) and relaxes in LDS until a block of NF3_BLOCK sweeps
//                 changes nothing or NF3_SWEEPS is reached (then it marks itself).  Only the owner writes a tile's cells back; a changed cell on a face,
//                 edge or corner marks EVERY neighbour tile whose halo holds it (up to 7) in the NEXT round's activity map.  Values only fall and each is
//                 the cost of a real move sequence, so a halo read that races a neighbour's write-back is harmless, as in 2-D.
//   k_nf3_parent  one lane per cell: the lowest direction code whose neighbour explains the cell's value (codes tried from 25 down).
// No workgroup waits for another, there is no flag to spin on, and every loop has a bound known at launch (NF3_SWEEPS, L).
//
// Tile shape and LDS pitch.  A tile is 16 (j) x 8 (i) x 8 (k) = 1024 cells, 4 per lane of a 256-lane workgroup; with the halo 18 x 10 x 10 cells.  A thin
// tile (32 x 4 x 8 has the same volume and any pitch is conflict-free) was not taken: a round moves information across at most one tile, so the number of
// rounds follows the shortest edge, and the halo of 16 x 8 x 8 is 76 % of its cells against 99 % for 32 x 4 x 8.  ds_read_b32 serves a wave in two groups of
// 32 lanes, bank = word address mod 32.  Lane t owns column j = t & 15, layer parity (t >> 4) & 1 and row i = t >> 5; its four cells are the layers
// parity + 2 c.  A group of 32 lanes therefore reads, at every one of the 26 offsets (the same offset for all lanes), two runs of 16 consecutive words that
// lie one PLANE pitch apart: they meet no conflict exactly when the plane pitch is 16 mod 32.  The row pitch is free; 18 (no padding) makes a plane 180
// words, and the least pitch >= 180 that is 16 mod 32 is 208.  (Had the two runs been two rows, the row pitch itself would have to be 16 mod 32, that is
// 48: 2.7 times the LDS.  With 18 as the row pitch and rows as the second run the banks 18 .. 31 of the second run fall on 2 .. 15 of the first: 14 of 32
// lanes two-way.)  Measured on a 128^3 serpentine, with a vote every 8 sweeps: pitch 208 34.2 us per round, 192 (every read two-way) 35.1, 180 (no padding)
// 35.3; on a uniform volume with every tile at work 43.1 / 48.1 / 48.3.  LDS: 10 x 208 words + as many halves = 12.4 KiB; the kernel takes 213 VGPRs, so
// two workgroups share a CU.  The lane's four cells are four independent chains; the move mask is applied with arithmetic (v | all-ones), not with compare
// and select, which spilled 119 SGPRs and cost 41.3 us per round.
#include "tsl_nav_field_common.hpp"

namespace tsl {

#define NF3_TJ 16                  // tile edges in cells
#define NF3_TI 8
#define NF3_TK 8
#define NF3_LDJ (NF3_TJ + 2)       // a staged row: the tile and its halo (no padding: the row pitch does not enter the bank rule, see above)
#define NF3_LDI (NF3_TI + 2)
#define NF3_LDK (NF3_TK + 2)
#define NF3_PP 208                 // plane pitch in words: >= 18 * 10 and 16 mod 32
#define NF3_LDS (NF3_LDK * NF3_PP)
#define NF3_SWEEPS 48              // sweeps of a tile per round at most ...
#define NF3_BLOCK 2                // ... in blocks of this many between two votes (a sweep is 104 reads per lane: the vote is cheap beside it, a quiet block is not)
#define NF3_MAX_DIM 1024
#define NF3_MAX_CELLS (1ll << 27)

static_assert(NF3_PP >= NF3_LDJ * NF3_LDI && NF3_PP % 32 == 16, "the plane pitch must hold a plane and be 16 mod 32 (bank rule of ds_read_b32)");
static_assert(NF3_TJ * NF3_TI * NF3_TK == 4 * 256, "four cells per lane");

// direction code -> (dk, di, dj); constant-folded where the code is a constant of an unrolled loop
__host__ __device__ constexpr int nf3_e(int d) { return d < 8 ? d : (d < 17 ? d - 9 : d - 18); }            // the 2-D code, -1 for the two vertical moves
__host__ __device__ constexpr int nf3_dk(int d) { return d < 8 ? 0 : (d < 17 ? 1 : -1); }
__host__ __device__ constexpr int nf3_di(int d) { return nf3_e(d) < 0 ? 0 : (nf3_e(d) <= 1 || nf3_e(d) == 7 ? 1 : (nf3_e(d) >= 3 && nf3_e(d) <= 5 ? -1 : 0)); }
__host__ __device__ constexpr int nf3_dj(int d) { return nf3_e(d) < 0 ? 0 : (nf3_e(d) >= 1 && nf3_e(d) <= 3 ? 1 : (nf3_e(d) >= 5 ? -1 : 0)); }
__host__ __device__ constexpr int nf3_nz(int d) { return (nf3_dk(d) != 0) + (nf3_di(d) != 0) + (nf3_dj(d) != 0); }
__host__ __device__ constexpr int nf3_off(int d) { return nf3_dk(d) * NF3_PP + nf3_di(d) * NF3_LDJ + nf3_dj(d); }
// bit (a + 1) * 9 + (b + 1) * 3 + (c + 1) of a 27-bit neighbourhood word; the cells a move by code d passes: every x + (a dk, b di, c dj) but x itself
__host__ __device__ constexpr uint32_t nf3_bit(int a, int b, int c) { return 1u << ((a + 1) * 9 + (b + 1) * 3 + (c + 1)); }
__host__ __device__ constexpr uint32_t nf3_need(int d)
{
    return (nf3_bit(nf3_dk(d), 0, 0) | nf3_bit(0, nf3_di(d), 0) | nf3_bit(0, 0, nf3_dj(d)) | nf3_bit(nf3_dk(d), nf3_di(d), 0) | nf3_bit(nf3_dk(d), 0, nf3_dj(d)) |
            nf3_bit(0, nf3_di(d), nf3_dj(d)) | nf3_bit(nf3_dk(d), nf3_di(d), nf3_dj(d))) & ~nf3_bit(0, 0, 0);
}
static_assert(nf3_dk(8) == 1 && nf3_di(8) == 0 && nf3_dj(8) == 0 && nf3_dk(17) == -1 && nf3_nz(17) == 1, "codes 8 and 17 are the vertical moves");
static_assert(nf3_di(1) == 1 && nf3_dj(1) == 1 && nf3_di(3) == -1 && nf3_dj(3) == 1 && nf3_di(5) == -1 && nf3_dj(5) == -1 && nf3_di(7) == 1 && nf3_dj(7) == -1, "nav_field's diagonals");
static_assert(nf3_dk(25) == -1 && nf3_di(25) == 1 && nf3_dj(25) == -1 && nf3_nz(25) == 3 && nf3_nz(9) == 2 && nf3_nz(10) == 3, "codes 9 .. 16 and 18 .. 25");

__constant__ int c_nf3_dk[26] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1 };
__constant__ int c_nf3_di[26] = { 1, 1, 0, -1, -1, -1, 0, 1, 0, 1, 1, 0, -1, -1, -1, 0, 1, 0, 1, 1, 0, -1, -1, -1, 0, 1 };
__constant__ int c_nf3_dj[26] = { 0, 1, 1, 1, 0, -1, -1, -1, 0, 0, 1, 1, 1, 0, -1, -1, -1, 0, 0, 1, 1, 1, 0, -1, -1, -1 };

// ---- one round -------------------------------------------------------------------------------------------------------------------------------
// grid (tx, ty, tz).  act_cur: this round's activity map (a tile clears its own word), act_next: the next round's.  parity = round & 1.
__global__ void __launch_bounds__(256) k_nf3_round(NfCfg C, const uint8_t* __restrict__ cost, uint32_t* field, uint32_t* act_cur, uint32_t* act_next, NfCtl* ctl,
                                                   int round)
{
    __shared__ uint32_t sf[NF3_LDS];
    __shared__ uint16_t sw[NF3_LDS];                                // neutral + cost of a traversable cell, 0 for a wall and outside the volume
    __shared__ uint32_t s_edges;
    const int tid = threadIdx.x, parity = round & 1;
    const int tc = (int)blockIdx.x, tr = (int)blockIdx.y, tk = (int)blockIdx.z;
    const size_t tile = ((size_t)tk * C.ty + tr) * C.tx + tc;
    if (tile == 0 && tid == 0) ctl->marks[parity ^ 1] = 0u;         // the next round counts from 0; nobody else touches that word in this round
    if (act_cur[tile] == 0u) return;                                // (uniform)
    if (tid == 0) s_edges = 0u;
    __syncthreads();                                                // every lane has read the word
    if (tid == 0) act_cur[tile] = 0u;

    const int k0 = tk * NF3_TK, r0 = tr * NF3_TI, c0 = tc * NF3_TJ;
    const size_t hw = (size_t)C.H * C.W;
    for (int e = tid; e < NF3_LDK * NF3_LDI * NF3_LDJ; e += 256) {
        const int lk = e / (NF3_LDI * NF3_LDJ), rem = e - lk * (NF3_LDI * NF3_LDJ), lr = rem / NF3_LDJ, lc = rem - lr * NF3_LDJ;
        const int k = k0 - 1 + lk, r = r0 - 1 + lr, c = c0 - 1 + lc;
        uint32_t f = TSL_NAV_UNREACHED, w = 0u;
        if (k >= 0 && k < C.D && r >= 0 && r < C.H && c >= 0 && c < C.W) {
            const size_t o = (size_t)k * hw + (size_t)r * C.W + c;
            const int cs = cost[o];
            if (cs < C.lethal) { w = (uint32_t)(C.neutral + cs); f = field[o]; }
        }
        const int l = lk * NF3_PP + lr * NF3_LDJ + lc;
        sf[l] = f; sw[l] = (uint16_t)w;
    }
    __syncthreads();

    // the lane's 4 cells: column tid & 15, row tid >> 5, layers ((tid >> 4) & 1) + 2 c
    const int lj = tid & 15, li = tid >> 5, lk0 = (tid >> 4) & 1;
    int idx[4]; uint32_t f0[4], f[4], w5[4], w7[4], w9[4], mask[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        idx[c] = (lk0 + 2 * c + 1) * NF3_PP + (li + 1) * NF3_LDJ + lj + 1;
        const uint32_t w = sw[idx[c]];
        f0[c] = f[c] = sf[idx[c]];
        w5[c] = 5u * w; w7[c] = 7u * w; w9[c] = 9u * w;
        uint32_t open = 0u, m = 0u;
        if (w) {
#pragma unroll
            for (int a = -1; a <= 1; ++a)
#pragma unroll
                for (int b = -1; b <= 1; ++b)
#pragma unroll
                    for (int e = -1; e <= 1; ++e)
                        if (sw[idx[c] + a * NF3_PP + b * NF3_LDJ + e]) open |= nf3_bit(a, b, e);
#pragma unroll
            for (int d = 0; d < 26; ++d)
                if (nf3_nz(d) <= C.nz && (open & nf3_need(d)) == nf3_need(d)) m |= 1u << d;
        }
        mask[c] = m;
    }

    // Sweeps in place, NF3_BLOCK at a time without a barrier, as in tsl_nav_field.hip: a lane reads whatever its neighbours hold at that moment, each a
    // valid upper bound; the 26 reads of a cell are issued together and the lane's 4 cells are 4 independent chains; the empty asm keeps the compiler
    // from carrying LDS values from one sweep into the next.  A block in which no lane wrote saw constant values throughout: the tile is at rest against
    // this halo.  Walls and cells outside hold TSL_NAV_UNREACHED for ever, so the six axis reads need no mask; the twenty diagonal ones do (the corner
    // rule, and the connectivity).
    int block = 0;
    for (; block < NF3_SWEEPS / NF3_BLOCK; ++block) {
        bool ch = false;
        for (int sweep = 0; sweep < NF3_BLOCK; ++sweep) {
            uint32_t m5[4], m7[4], m9[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t shut = ~mask[c];
                const int i = idx[c];
                uint32_t a5 = TSL_NAV_UNREACHED, a7 = TSL_NAV_UNREACHED, a9 = TSL_NAV_UNREACHED;
#pragma unroll
                for (int d = 0; d < 26; ++d) {
                    const uint32_t v = sf[i + nf3_off(d)];
                    const uint32_t no = (uint32_t)((int32_t)(shut << (31 - d)) >> 31);      // all ones when the move is not allowed: v | no is TSL_NAV_UNREACHED
                    if (nf3_nz(d) == 1) a5 = min(a5, v);
                    else if (nf3_nz(d) == 2) a7 = min(a7, v | no);
                    else a9 = min(a9, v | no);
                }
                m5[c] = a5; m7[c] = a7; m9[c] = a9;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t cand = min(nf_add(m5[c], w5[c]), min(nf_add(m7[c], w7[c]), nf_add(m9[c], w9[c])));
                if (mask[c] && cand < f[c]) { f[c] = cand; sf[idx[c]] = cand; ch = true; }
            }
            __asm__ volatile("" ::: "memory");
        }
        if (!__syncthreads_or(ch ? 1 : 0)) break;                   // (uniform)
    }
    const bool capped = block == NF3_SWEEPS / NF3_BLOCK;

    // write back what fell; s_edges: bit (a + 1) * 9 + (b + 1) * 3 + (c + 1) = the halo of the neighbour tile at (a, b, c) holds a cell that changed
    uint32_t edges = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (f[c] >= f0[c]) continue;
        const int lk = lk0 + 2 * c;
        field[(size_t)(k0 + lk) * hw + (size_t)(r0 + li) * C.W + c0 + lj] = f[c];      // (a cell outside the volume has mask 0 and never changes)
        // per axis the set of tile offsets that see the cell: bit 0 = -1, bit 1 = 0, bit 2 = +1; the neighbours are the product of the three sets
        const uint32_t mj = 2u | (lj == 0 ? 1u : 0u) | (lj == NF3_TJ - 1 ? 4u : 0u);
        const uint32_t mi = 2u | (li == 0 ? 1u : 0u) | (li == NF3_TI - 1 ? 4u : 0u);
        const uint32_t mk = 2u | (lk == 0 ? 1u : 0u) | (lk == NF3_TK - 1 ? 4u : 0u);
        const uint32_t pl = ((mi & 1u) ? mj : 0u) | ((mi & 2u) ? mj << 3 : 0u) | ((mi & 4u) ? mj << 6 : 0u);
        edges |= ((mk & 1u) ? pl : 0u) | ((mk & 2u) ? pl << 9 : 0u) | ((mk & 4u) ? pl << 18 : 0u);
    }
    edges &= ~nf3_bit(0, 0, 0);
    if (edges) atomicOr(&s_edges, edges);
    __syncthreads();
    if (tid != 0) return;
    const uint32_t e = s_edges;
    uint32_t n = 0u;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b)
            for (int c = -1; c <= 1; ++c) {
                if (!(e & nf3_bit(a, b, c))) continue;
                if ((a != 0) + (b != 0) + (c != 0) > C.nz) continue;    // a tile across an edge or a corner reads the cell only through a diagonal move
                const int nk = tk + a, nr = tr + b, nc = tc + c;
                if (nk < 0 || nk >= C.tz || nr < 0 || nr >= C.ty || nc < 0 || nc >= C.tx) continue;
                act_next[((size_t)nk * C.ty + nr) * C.tx + nc] = 1u; ++n;
            }
    if (capped) { act_next[tile] = 1u; ++n; }
    if (n) atomicAdd(&ctl->marks[parity], n);
    atomicAdd(&ctl->visits, 1ull);
    atomicMax(&ctl->rounds, round + 1);
}

// ---- parents ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nf3_parent(NfCfg C, const uint8_t* __restrict__ cost, const uint32_t* __restrict__ field, uint8_t* __restrict__ parent)
{
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t hw = (size_t)C.H * C.W;
    if (o >= hw * C.D) return;
    const int k = (int)(o / hw), r = (int)((o - (size_t)k * hw) / C.W), c = (int)(o - (size_t)k * hw - (size_t)r * C.W);
    const uint32_t f = field[o];
    const int cs = cost[o];
    uint32_t par = 255u;
    if (f != TSL_NAV_UNREACHED && cs < C.lethal) {
        const uint32_t w = (uint32_t)(C.neutral + cs);
        uint32_t open = 0u;
#pragma unroll
        for (int a = -1; a <= 1; ++a)
#pragma unroll
            for (int b = -1; b <= 1; ++b)
#pragma unroll
                for (int e = -1; e <= 1; ++e) {
                    const int nk = k + a, nr = r + b, nc = c + e;
                    if (nk >= 0 && nk < C.D && nr >= 0 && nr < C.H && nc >= 0 && nc < C.W && (int)cost[(size_t)nk * hw + (size_t)nr * C.W + nc] < C.lethal)
                        open |= nf3_bit(a, b, e);
                }
#pragma unroll
        for (int d = 25; d >= 0; --d) {                             // downwards: the lowest code that explains f is the one that stays
            if (nf3_nz(d) > C.nz || (open & nf3_need(d)) != nf3_need(d)) continue;
            const uint32_t fn = field[(size_t)(k + nf3_dk(d)) * hw + (size_t)(r + nf3_di(d)) * C.W + c + nf3_dj(d)];
            if (fn != TSL_NAV_UNREACHED && nf_add(fn, (nf3_nz(d) == 1 ? 5u : (nf3_nz(d) == 2 ? 7u : 9u)) * w) == f) par = (uint32_t)d;
        }
    }
    parent[o] = (uint8_t)par;
}

// ---- the solver, as tsl_nav_field_common.hpp sees it -----------------------------------------------------------------------------------------
struct Nf3 {
    static constexpr int TX = NF3_TJ, TY = NF3_TI, TZ = NF3_TK, SEED = TSL_NAV3_SEED, NCOMP = 3;
    static constexpr bool LINKED = true;                            // the leading axis is the layers of one volume
    typedef tsl_nav_field3_cfg cfg_t;
    typedef tsl_nav_field3_stats stats_t;
    static constexpr const char* name = "nav_field3";
    static constexpr const char* conn_text = ": connectivity must be 6, 18 or 26";
    static constexpr int K_SEED = -1, K_ROUND = -1, K_PARENT = -1, K_PATHS = -1;      // no profiling id: time the _dev call with events
    static NavFieldState*& state(tsl_tsdf* m) { return m->nav_field3; }
    static int dims(const cfg_t* c, const std::string& w, NfCfg* C)
    {
        TSL_REQUIRE(c->D >= 1 && c->D <= NF3_MAX_DIM, w + ": D must be 1 .. 1024");
        TSL_REQUIRE(c->H >= 1 && c->H <= NF3_MAX_DIM, w + ": H must be 1 .. 1024");
        TSL_REQUIRE(c->W >= 1 && c->W <= NF3_MAX_DIM, w + ": W must be 1 .. 1024");
        TSL_REQUIRE((long long)c->D * c->H * c->W <= NF3_MAX_CELLS, w + ": D * H * W is above 2^27 cells");
        C->D = c->D; C->H = c->H; C->W = c->W;
        return TSL_OK;
    }
    static int rank(int conn) { return conn == 6 ? 1 : (conn == 18 ? 2 : (conn == 26 ? 3 : 0)); }
    static int default_rounds(const NfCfg& C)
    {
        const long long cap = 4ll * C.tx * C.ty * C.tz + 64;
        return (int)(cap < 65536 ? cap : 65536);
    }
    __device__ static void step(int code, int& k, int& r, int& c) { k += c_nf3_dk[code]; r += c_nf3_di[code]; c += c_nf3_dj[code]; }
    static void round(hipStream_t q, const NfCfg& C, const uint8_t* cost, uint32_t* field, uint32_t* act_cur, uint32_t* act_next, NfCtl* ctl, int r)
    {
        hipLaunchKernelGGL(k_nf3_round, dim3((unsigned)C.tx, (unsigned)C.ty, (unsigned)C.tz), dim3(256), 0, q, C, cost, field, act_cur, act_next, ctl, r);
    }
    static void parent(hipStream_t q, const NfCfg& C, const uint8_t* cost, const uint32_t* field, uint8_t* par)
    {
        hipLaunchKernelGGL(k_nf3_parent, dim3((unsigned)(((size_t)C.D * C.H * C.W + 255) / 256)), dim3(256), 0, q, C, cost, field, par);
    }
};

void nav_field3_release(tsl_tsdf* m) { nf_release(&m->nav_field3); }

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_nav_field3(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const uint8_t* cost, const int32_t* seeds, int32_t n_seeds, uint32_t* field, uint8_t* parent,
                        tsl_nav_field3_stats* stats)
{
    return nf_field_host<Nf3>(m, cfg, cost, seeds, n_seeds, field, parent, stats);
}

int tsl_tsdf_nav_field3_dev(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const void* cost_dev, const void* seeds_dev, int32_t n_seeds, void* field_dev, void* parent_dev,
                            void* stats_dev, void* user_stream)
{
    return nf_field_dev<Nf3>(m, cfg, cost_dev, seeds_dev, n_seeds, field_dev, parent_dev, stats_dev, user_stream);
}

int tsl_tsdf_nav_field3_paths(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const uint32_t* field, const uint8_t* parent, const int32_t* starts, int32_t n_starts,
                              int32_t max_len, int16_t* cells, int32_t* length, uint8_t* status, uint32_t* cost)
{
    return nf_paths_host<Nf3>(m, cfg, field, parent, starts, n_starts, max_len, cells, length, status, cost);
}

int tsl_tsdf_nav_field3_paths_dev(tsl_tsdf* m, const tsl_nav_field3_cfg* cfg, const void* field_dev, const void* parent_dev, const void* starts_dev, int32_t n_starts,
                                  int32_t max_len, void* cells_dev, void* length_dev, void* status_dev, void* cost_dev, void* user_stream)
{
    return nf_paths_dev<Nf3>(m, cfg, field_dev, parent_dev, starts_dev, n_starts, max_len, cells_dev, length_dev, status_dev, cost_dev, user_stream);
}

}  // extern "C"

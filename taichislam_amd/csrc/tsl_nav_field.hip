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
//   k_nf_seed     one lane per seed: a seed outside or on a wall counts in n_bad; the others atomicMin into the field and mark their tile and its eight
//                 neighbours active (a seed on a tile's border is a border value the neighbours have not seen).
//   k_nf_round    one round = one launch, one workgroup per 32 x 32 tile; a tile that is not marked active exits at once.  An active tile loads its
//                 field and cost with a one-cell halo into LDS (34 x 34 words + 34 x 34 halves, 6.8 KiB), turns the cost into a per-cell move mask and
//                 weight in registers, and relaxes in LDS -- every lane owns 4 cells, a half-wave reads 32 consecutive words: no bank conflict -- until a
//                 block of NF_BLOCK sweeps changes nothing or NF_SWEEPS is reached (then it marks itself).  Only the owner writes a tile's cells back; when a border cell
//                 changed it marks the neighbours that see it in the NEXT round's activity map (two maps, swapped every round) and counts the marks.
//                 Values only fall and each is the cost of a real move sequence, so a halo read that races a neighbour's write-back -- it sees the old
//                 or the new aligned word -- is harmless, and whoever changed a border cell marks the reader for the next round anyway.
//   k_nf_finish   one lane: the statistics, from the control block.
//   k_nf_parent   one lane per cell: the lowest direction code whose neighbour explains the cell's value.
//   k_nf_seed_parent   one lane per seed: parent 8 where the field equals a seed value placed there.
//   k_nf_paths    one lane per start: follows parents for at most L cells.
// No workgroup waits for another, there is no flag to spin on, and every loop has a bound known at launch (NF_SWEEPS, L).  The host stops the rounds:
// every check_every rounds it reads the 4-byte count of marks the last round made; a round that marked nothing leaves nothing active.
#include "tsl_tsdf.hpp"

namespace tsl {

#define NF_T 32                    // tile edge in cells
#define NF_LD (NF_T + 2)           // a staged row: the tile and its halo
#define NF_SWEEPS 64               // sweeps of a tile per round at most ...
#define NF_BLOCK 8                 // ... in blocks of this many between two votes
#define NF_MAXV 0xfffffffeu        // the clip of every sum
#define NF_MAX_SEEDS 65536
#define NF_MAX_STARTS (1 << 20)
#define NF_CHECK_DEFAULT 8

struct NfCfg { int B, H, W, neutral, lethal, conn8, tx, ty, max_rounds, rounds_fixed, check_every; };

// device control block: marks made by the rounds of either parity, the last round that visited a tile + 1, bad seeds, tile visits
struct NfCtl { uint32_t marks[2]; int32_t rounds, n_bad; unsigned long long visits; };

struct NavFieldState {
    void *cost, *seeds, *field, *parent, *act, *ctl, *stats, *starts, *cells, *plen, *pstatus, *pcost;
    size_t b_cost, b_seeds, b_field, b_parent, b_act, b_ctl, b_stats, b_starts, b_cells, b_plen, b_pstatus, b_pcost;
    uint32_t* pin;                 // pinned: the count the host reads between rounds, and the statistics on their way back
};

__device__ __forceinline__ uint32_t nf_add(uint32_t a, uint32_t c)      // a + c clipped to NF_MAXV; unreached stays unreached
{
    return a == TSL_NAV_UNREACHED ? a : (a > NF_MAXV - c ? NF_MAXV : a + c);
}

__constant__ int c_nf_di[8] = { 1, 1, 0, -1, -1, -1, 0, 1 };
__constant__ int c_nf_dj[8] = { 0, 1, 1, 1, 0, -1, -1, -1 };

// ---- seeds -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nf_seed(NfCfg C, const uint8_t* __restrict__ cost, const int32_t* __restrict__ seeds, int S, uint32_t* field, uint32_t* act,
                                                 NfCtl* ctl)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    const int p = seeds[s * 4], r = seeds[s * 4 + 1], c = seeds[s * 4 + 2];
    const uint32_t v = (uint32_t)seeds[s * 4 + 3];
    bool ok = p >= 0 && p < C.B && r >= 0 && r < C.H && c >= 0 && c < C.W;
    size_t o = 0;
    if (ok) { o = ((size_t)p * C.H + r) * C.W + c; ok = (int)cost[o] < C.lethal; }
    if (!ok) { atomicAdd(&ctl->n_bad, 1); return; }
    atomicMin(&field[o], v > NF_MAXV ? NF_MAXV : v);
    const int tr = r / NF_T, tc = c / NF_T;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b) {
            const int nr = tr + a, nc = tc + b;
            if (nr >= 0 && nr < C.ty && nc >= 0 && nc < C.tx) act[((size_t)p * C.ty + nr) * C.tx + nc] = 1u;
        }
}

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
            if (C.conn8) {
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
    if (C.conn8) {
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

__global__ void k_nf_finish(const NfCtl* __restrict__ ctl, int last_round, tsl_nav_field_stats* st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->converged = ctl->marks[last_round & 1] == 0u ? 1 : 0;
    st->rounds = ctl->rounds;
    st->tile_visits = (int64_t)ctl->visits;
    st->n_bad_seeds = ctl->n_bad;
    st->reserved_ = 0;
}

// ---- parents ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nf_parent(NfCfg C, const uint8_t* __restrict__ cost, const uint32_t* __restrict__ field, uint8_t* __restrict__ parent)
{
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t hw = (size_t)C.H * C.W;
    if (o >= hw * C.B) return;
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
            if (d & 1) ok = ok && C.conn8 && open[d - 1] && open[(d + 1) & 7];
            if (!ok) continue;
            const uint32_t fn = field[plane + (size_t)(r + c_nf_di[d]) * C.W + c + c_nf_dj[d]];
            if (fn != TSL_NAV_UNREACHED && nf_add(fn, (d & 1 ? 7u : 5u) * w) == f) par = (uint32_t)d;
        }
    }
    parent[o] = (uint8_t)par;
}

__global__ void __launch_bounds__(256) k_nf_seed_parent(NfCfg C, const uint8_t* __restrict__ cost, const int32_t* __restrict__ seeds, int S,
                                                        const uint32_t* __restrict__ field, uint8_t* parent)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    const int p = seeds[s * 4], r = seeds[s * 4 + 1], c = seeds[s * 4 + 2];
    const uint32_t v = (uint32_t)seeds[s * 4 + 3];
    if (!(p >= 0 && p < C.B && r >= 0 && r < C.H && c >= 0 && c < C.W)) return;
    const size_t o = ((size_t)p * C.H + r) * C.W + c;
    if ((int)cost[o] >= C.lethal) return;
    if (field[o] == (v > NF_MAXV ? NF_MAXV : v)) parent[o] = 8;     // (several seeds of one value on a cell store the same byte)
}

// ---- paths -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_nf_paths(int B, int H, int W, const uint32_t* __restrict__ field, const uint8_t* __restrict__ parent,
                                                 const int32_t* __restrict__ starts, int P, int L, int16_t* __restrict__ cells, int32_t* __restrict__ length,
                                                 uint8_t* __restrict__ status, uint32_t* __restrict__ cost)
{
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q >= P) return;
    const int p = starts[q * 3];
    int r = starts[q * 3 + 1], c = starts[q * 3 + 2];
    int st = 1, len = 0;                                            // truncated unless the walk ends
    uint32_t f = TSL_NAV_UNREACHED;
    bool go = true;
    size_t plane = 0;
    if (!(p >= 0 && p < B && r >= 0 && r < H && c >= 0 && c < W)) { st = 3; go = false; }
    else {
        plane = (size_t)p * H * W;
        f = field[plane + (size_t)r * W + c];
        if (f == TSL_NAV_UNREACHED || parent[plane + (size_t)r * W + c] > 8) { st = 2; go = false; }
    }
    int16_t* out = cells ? cells + (size_t)q * L * 2 : nullptr;
    for (int t = 0; t < L; ++t) {
        int16_t a = -1, b = -1;
        if (go) {
            a = (int16_t)r; b = (int16_t)c; len = t + 1;
            const int par = parent[plane + (size_t)r * W + c];
            if (par == 8) { st = 0; go = false; }
            else if (par > 8) { st = 2; go = false; }               // a parent plane that is not of this field
            else {
                r += c_nf_di[par]; c += c_nf_dj[par];
                if (!(r >= 0 && r < H && c >= 0 && c < W)) { st = 2; go = false; }
            }
        }
        if (out) { out[t * 2] = a; out[t * 2 + 1] = b; }
    }
    if (length) length[q] = len;
    if (status) status[q] = (uint8_t)st;
    if (cost) cost[q] = f;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
void nav_field_release(tsl_tsdf* m)
{
    NavFieldState* S = m->nav_field;
    if (!S) return;
    void* ptrs[] = { S->cost, S->seeds, S->field, S->parent, S->act, S->ctl, S->stats, S->starts, S->cells, S->plen, S->pstatus, S->pcost };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (S->pin) (void)hipHostFree(S->pin);
    delete S;
    m->nav_field = nullptr;
}

static int nf_dims(const tsl_nav_field_cfg* c, const std::string& w)
{
    TSL_REQUIRE(c->B >= 1 && c->B <= 16, w + ": B must be 1 .. 16 planes");
    TSL_REQUIRE(c->H >= 1 && c->H <= 4096, w + ": H must be 1 .. 4096");
    TSL_REQUIRE(c->W >= 1 && c->W <= 4096, w + ": W must be 1 .. 4096");
    return TSL_OK;
}

static int nf_check(tsl_tsdf* m, const tsl_nav_field_cfg* c, const void* cost, const void* seeds, int S, const void* field, NfCfg* C, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(cost, w + ": null cost");
    TSL_REQUIRE(field, w + ": null field");
    int rc = nf_dims(c, w); if (rc) return rc;
    TSL_REQUIRE(S >= 0 && S <= NF_MAX_SEEDS, w + ": S must be 0 .. 65536 seeds");
    TSL_REQUIRE(seeds || S == 0, w + ": null seeds while S > 0");
    TSL_REQUIRE(c->neutral >= 1 && c->neutral <= 255, w + ": neutral must be 1 .. 255");
    TSL_REQUIRE(c->lethal >= 1 && c->lethal <= 255, w + ": lethal must be 1 .. 255");
    TSL_REQUIRE(c->connectivity == 4 || c->connectivity == 8, w + ": connectivity must be 4 or 8");
    TSL_REQUIRE(c->max_rounds >= 0, w + ": max_rounds is negative");
    TSL_REQUIRE(c->rounds_fixed >= 0, w + ": rounds_fixed is negative");
    TSL_REQUIRE(c->check_every >= 0, w + ": check_every is negative");
    C->B = c->B; C->H = c->H; C->W = c->W; C->neutral = c->neutral; C->lethal = c->lethal; C->conn8 = c->connectivity == 8;
    C->tx = (c->W + NF_T - 1) / NF_T; C->ty = (c->H + NF_T - 1) / NF_T;
    C->max_rounds = c->max_rounds ? c->max_rounds : 4 * C->tx * C->ty + 64;
    C->rounds_fixed = c->rounds_fixed;
    C->check_every = c->check_every ? c->check_every : NF_CHECK_DEFAULT;
    return TSL_OK;
}

#define NF_GROW(field, bytes_field, bytes) do { if ((rc = grow(&S->field, &S->bytes_field, (bytes)))) return rc; } while (0)

static int nf_state(tsl_tsdf* m)
{
    if (m->nav_field) return TSL_OK;
    NavFieldState* S = new NavFieldState();                         // value-initialised: every pointer null, every size 0
    if (hipHostMalloc((void**)&S->pin, 64) != hipSuccess) { delete S; (void)hipGetLastError(); set_error("nav_field: no pinned memory"); return TSL_ERR_HIP; }
    m->nav_field = S;
    return TSL_OK;
}

// everything on q, every pointer a device pointer.  With rounds_fixed = 0 it waits for q at each check.
static int nf_launch(tsl_tsdf* m, hipStream_t q, const NfCfg& C, const uint8_t* cost, const int32_t* seeds, int S_n, uint32_t* field, uint8_t* parent,
                     tsl_nav_field_stats* stats)
{
    int rc;
    NavFieldState* S = m->nav_field;
    const size_t tiles = (size_t)C.B * C.tx * C.ty, cells = (size_t)C.B * C.H * C.W;
    NF_GROW(act, b_act, tiles * 2 * sizeof(uint32_t));
    NF_GROW(ctl, b_ctl, sizeof(NfCtl));
    NF_GROW(stats, b_stats, sizeof(tsl_nav_field_stats));
    if (!stats) stats = (tsl_nav_field_stats*)S->stats;
    uint32_t* act = (uint32_t*)S->act;
    NfCtl* ctl = (NfCtl*)S->ctl;
    TSL_HIP(hipMemsetAsync(field, 0xff, cells * sizeof(uint32_t), q));
    TSL_HIP(hipMemsetAsync(act, 0, tiles * 2 * sizeof(uint32_t), q));
    TSL_HIP(hipMemsetAsync(ctl, 0, sizeof(NfCtl), q));
    if (S_n > 0) {
        prof_begin(m, TSL_K_NAV_FIELD_SEED, q);
        hipLaunchKernelGGL(k_nf_seed, dim3((unsigned)((S_n + 255) / 256)), dim3(256), 0, q, C, cost, seeds, S_n, field, act, ctl);
        prof_end(m, q);
        TSL_HIP(hipGetLastError());
    }
    const dim3 grid((unsigned)C.tx, (unsigned)C.ty, (unsigned)C.B);
    int r = 0;
    const int total = C.rounds_fixed > 0 ? C.rounds_fixed : C.max_rounds;
    while (r < total) {
        const int n = C.rounds_fixed > 0 ? total : (C.check_every < total - r ? C.check_every : total - r);
        for (int e = r + n; r < e; ++r) {
            prof_begin(m, TSL_K_NAV_FIELD_ROUND, q);
            hipLaunchKernelGGL(k_nf_round, grid, dim3(256), 0, q, C, cost, field, act + (size_t)(r & 1) * tiles, act + (size_t)((r & 1) ^ 1) * tiles, ctl, r);
            prof_end(m, q);
        }
        TSL_HIP(hipGetLastError());
        if (C.rounds_fixed > 0) break;
        TSL_HIP(hipMemcpyAsync(S->pin, &ctl->marks[(r - 1) & 1], sizeof(uint32_t), hipMemcpyDeviceToHost, q));
        TSL_HIP(hipStreamSynchronize(q));
        if (S->pin[0] == 0u) break;                                 // the last round marked nothing: nothing is active
    }
    hipLaunchKernelGGL(k_nf_finish, dim3(1), dim3(64), 0, q, ctl, r - 1, stats);
    if (parent) {
        prof_begin(m, TSL_K_NAV_FIELD_PARENT, q);
        hipLaunchKernelGGL(k_nf_parent, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, q, C, cost, field, parent);
        if (S_n > 0) hipLaunchKernelGGL(k_nf_seed_parent, dim3((unsigned)((S_n + 255) / 256)), dim3(256), 0, q, C, cost, seeds, S_n, field, parent);
        prof_end(m, q);
    }
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

static int nf_paths_check(tsl_tsdf* m, const tsl_nav_field_cfg* c, const void* field, const void* parent, const void* starts, int P, int L, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(field, w + ": null field");
    TSL_REQUIRE(parent, w + ": null parent");
    int rc = nf_dims(c, w); if (rc) return rc;
    TSL_REQUIRE(P >= 0 && P <= NF_MAX_STARTS, w + ": P must be 0 .. 2^20 starts");
    TSL_REQUIRE(starts || P == 0, w + ": null starts while P > 0");
    TSL_REQUIRE(L >= 1, w + ": L must be at least 1");
    TSL_REQUIRE((long long)P * L <= (1ll << 28), w + ": P * L is above 2^28 cells");
    return TSL_OK;
}

static int nf_paths_launch(tsl_tsdf* m, hipStream_t q, const tsl_nav_field_cfg* c, const uint32_t* field, const uint8_t* parent, const int32_t* starts, int P, int L,
                           int16_t* cells, int32_t* length, uint8_t* status, uint32_t* cost)
{
    if (P == 0) return TSL_OK;
    prof_begin(m, TSL_K_NAV_FIELD_PATHS, q);
    hipLaunchKernelGGL(k_nf_paths, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, q, c->B, c->H, c->W, field, parent, starts, P, L, cells, length, status, cost);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_nav_field(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const uint8_t* cost, const int32_t* seeds, int32_t n_seeds, uint32_t* field, uint8_t* parent,
                       tsl_nav_field_stats* stats)
{
    NfCfg C;
    int rc = nf_check(m, cfg, cost, seeds, n_seeds, field, &C, "nav_field"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nf_state(m))) return rc;
    NavFieldState* S = m->nav_field;
    const size_t cells = (size_t)C.B * C.H * C.W;
    NF_GROW(cost, b_cost, cells);
    NF_GROW(field, b_field, cells * sizeof(uint32_t));
    if (parent) NF_GROW(parent, b_parent, cells);
    if (n_seeds > 0) NF_GROW(seeds, b_seeds, (size_t)n_seeds * 4 * sizeof(int32_t));
    NF_GROW(stats, b_stats, sizeof(tsl_nav_field_stats));
    TSL_HIP(hipMemcpyAsync(S->cost, cost, cells, hipMemcpyHostToDevice, q));
    if (n_seeds > 0) TSL_HIP(hipMemcpyAsync(S->seeds, seeds, (size_t)n_seeds * 4 * sizeof(int32_t), hipMemcpyHostToDevice, q));
    if ((rc = nf_launch(m, q, C, (const uint8_t*)S->cost, (const int32_t*)S->seeds, n_seeds, (uint32_t*)S->field, parent ? (uint8_t*)S->parent : nullptr,
                        (tsl_nav_field_stats*)S->stats))) return rc;
    TSL_HIP(hipMemcpyAsync(S->pin + 4, S->stats, sizeof(tsl_nav_field_stats), hipMemcpyDeviceToHost, q));
    TSL_HIP(hipStreamSynchronize(q));
    TSL_HIP(hipMemcpy(field, S->field, cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (parent) TSL_HIP(hipMemcpy(parent, S->parent, cells, hipMemcpyDeviceToHost));
    if (stats) memcpy(stats, S->pin + 4, sizeof(tsl_nav_field_stats));
    return TSL_OK;
}

int tsl_tsdf_nav_field_dev(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const void* cost_dev, const void* seeds_dev, int32_t n_seeds, void* field_dev, void* parent_dev,
                           void* stats_dev, void* user_stream)
{
    NfCfg C;
    int rc = nf_check(m, cfg, cost_dev, seeds_dev, n_seeds, field_dev, &C, "nav_field_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nf_state(m))) return rc;
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nf_launch(m, q, C, (const uint8_t*)cost_dev, (const int32_t*)seeds_dev, n_seeds, (uint32_t*)field_dev, (uint8_t*)parent_dev,
                        (tsl_nav_field_stats*)stats_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_tsdf_nav_field_paths(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const uint32_t* field, const uint8_t* parent, const int32_t* starts, int32_t n_starts,
                             int32_t max_len, int16_t* cells, int32_t* length, uint8_t* status, uint32_t* cost)
{
    int rc = nf_paths_check(m, cfg, field, parent, starts, n_starts, max_len, "nav_field_paths"); if (rc) return rc;
    if (n_starts == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nf_state(m))) return rc;
    NavFieldState* S = m->nav_field;
    const size_t ncells = (size_t)cfg->B * cfg->H * cfg->W, P = (size_t)n_starts, L = (size_t)max_len;
    NF_GROW(field, b_field, ncells * sizeof(uint32_t));
    NF_GROW(parent, b_parent, ncells);
    NF_GROW(starts, b_starts, P * 3 * sizeof(int32_t));
    NF_GROW(cells, b_cells, P * L * 2 * sizeof(int16_t));
    NF_GROW(plen, b_plen, P * sizeof(int32_t));
    NF_GROW(pstatus, b_pstatus, P);
    NF_GROW(pcost, b_pcost, P * sizeof(uint32_t));
    TSL_HIP(hipMemcpyAsync(S->field, field, ncells * sizeof(uint32_t), hipMemcpyHostToDevice, q));
    TSL_HIP(hipMemcpyAsync(S->parent, parent, ncells, hipMemcpyHostToDevice, q));
    TSL_HIP(hipMemcpyAsync(S->starts, starts, P * 3 * sizeof(int32_t), hipMemcpyHostToDevice, q));
    if ((rc = nf_paths_launch(m, q, cfg, (const uint32_t*)S->field, (const uint8_t*)S->parent, (const int32_t*)S->starts, n_starts, max_len, (int16_t*)S->cells,
                              (int32_t*)S->plen, (uint8_t*)S->pstatus, (uint32_t*)S->pcost))) return rc;
    TSL_HIP(hipStreamSynchronize(q));
    if (cells) TSL_HIP(hipMemcpy(cells, S->cells, P * L * 2 * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (length) TSL_HIP(hipMemcpy(length, S->plen, P * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (status) TSL_HIP(hipMemcpy(status, S->pstatus, P, hipMemcpyDeviceToHost));
    if (cost) TSL_HIP(hipMemcpy(cost, S->pcost, P * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TSL_OK;
}

int tsl_tsdf_nav_field_paths_dev(tsl_tsdf* m, const tsl_nav_field_cfg* cfg, const void* field_dev, const void* parent_dev, const void* starts_dev, int32_t n_starts,
                                 int32_t max_len, void* cells_dev, void* length_dev, void* status_dev, void* cost_dev, void* user_stream)
{
    int rc = nf_paths_check(m, cfg, field_dev, parent_dev, starts_dev, n_starts, max_len, "nav_field_paths_dev"); if (rc) return rc;
    if (n_starts == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nf_paths_launch(m, q, cfg, (const uint32_t*)field_dev, (const uint8_t*)parent_dev, (const int32_t*)starts_dev, n_starts, max_len, (int16_t*)cells_dev,
                              (int32_t*)length_dev, (uint8_t*)status_dev, (uint32_t*)cost_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

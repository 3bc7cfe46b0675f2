// tsl_nav_field_common.hpp -- the one copy of what the cost-to-go family shares: the fields over 2-D cost planes (tsl_nav_field.hip, DESIGN.md section
// 4.16) and over 3-D cost volumes (tsl_nav_field3.hip, section 4.18).  Shared: the scratch of a handle (NavFieldState, one instance per solver), the
// control block, the clipped add, the seed, finish, seed-parent and paths kernels, the argument checks, the round loop with its host check and the
// bodies of the four entry points (host form, device form, paths host form, paths device form).  Not shared: the tile relaxation and the parent pass
// of each solver, which are tuned to their dimension and stay in their own file.
//
// One configuration struct serves both.  A field has three extents D, H, W; `nz` is the move rank, the largest number of non-zero components a move
// may have: connectivity 4 / 8 is nz 1 / 2, connectivity 6 / 18 / 26 is nz 1 / 2 / 3.  2-D is the case in which the leading extent counts independent
// planes (D = B) and a tile is one plane thick, so tz = B: no move and no activity mark crosses the leading axis.
//
// Each solver describes itself in a traits struct T, defined in its own .hip behind its kernels:
//   TX, TY, TZ       tile edges in cells along W, H and the leading axis
//   LINKED           whether the leading axis links cells (false: independent planes)
//   SEED, NCOMP      the parent code of a seed cell (the number of direction codes), the components of a path cell (the last NCOMP of leading, row, col)
//   cfg_t, stats_t   the public types; name: the prefix of the entry points' names in error texts ("nav_field": nav_field_dev, nav_field_paths, ...)
//   K_SEED, K_ROUND, K_PARENT, K_PATHS   profiling ids, -1 for none
//   state(m)         the handle's instance of NavFieldState
//   dims(c, w, C)    the refusals about the extents, with their texts; fills C->D, C->H, C->W
//   rank(conn)       the move rank of a connectivity, 0 for one that is not accepted; conn_text: the refusal
//   default_rounds(C)   max_rounds where the caller gives 0
//   step(code, k, r, c) __device__: one move by a direction code (the direction tables)
//   round(...), parent(...)   the launches of its round kernel and of its parent kernel
#pragma once
#include <cstring>
#include <string>
#include "tsl_stage.hpp"

namespace tsl {

#define NF_MAXV 0xfffffffeu        // the clip of every sum
#define NF_MAX_SEEDS 65536
#define NF_MAX_STARTS (1 << 20)
#define NF_CHECK_DEFAULT 8

struct NfCfg { int D, H, W, neutral, lethal, nz, tx, ty, tz, max_rounds, rounds_fixed, check_every; };

// device control block: marks made by the rounds of either parity, the last round that visited a tile + 1, bad seeds, tile visits
struct NfCtl { uint32_t marks[2]; int32_t rounds, n_bad; unsigned long long visits; };

struct NavFieldState {
    void *act, *ctl, *stats;       // the activity maps, the control block, the statistics of a call that asks for none
    size_t b_act, b_ctl, b_stats;
    uint32_t* pin;                 // pinned: the count the host reads between rounds
};

__device__ __forceinline__ uint32_t nf_add(uint32_t a, uint32_t c)      // a + c clipped to NF_MAXV; unreached stays unreached
{
    return a == TSL_NAV_UNREACHED ? a : (a > NF_MAXV - c ? NF_MAXV : a + c);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------------
// one lane per seed: a seed outside or on a wall counts in n_bad; the others atomicMin into the field and mark their tile and its neighbours active (a
// seed on a tile's border is a border value the neighbours have not seen) -- across the leading axis only where that axis links cells
template <class T>
__global__ void __launch_bounds__(256) k_nf_seed(NfCfg C, const uint8_t* __restrict__ cost, const int32_t* __restrict__ seeds, int S, uint32_t* field, uint32_t* act,
                                                 NfCtl* ctl)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    const int k = seeds[s * 4], r = seeds[s * 4 + 1], c = seeds[s * 4 + 2];
    const uint32_t v = (uint32_t)seeds[s * 4 + 3];
    bool ok = k >= 0 && k < C.D && r >= 0 && r < C.H && c >= 0 && c < C.W;
    size_t o = 0;
    if (ok) { o = ((size_t)k * C.H + r) * C.W + c; ok = (int)cost[o] < C.lethal; }
    if (!ok) { atomicAdd(&ctl->n_bad, 1); return; }
    atomicMin(&field[o], v > NF_MAXV ? NF_MAXV : v);
    const int tk = k / T::TZ, tr = r / T::TY, tc = c / T::TX, reach = T::LINKED ? 1 : 0;
    for (int a = -reach; a <= reach; ++a)
        for (int b = -1; b <= 1; ++b)
            for (int e = -1; e <= 1; ++e) {
                const int nk = tk + a, nr = tr + b, nc = tc + e;
                if (nk >= 0 && nk < C.tz && nr >= 0 && nr < C.ty && nc >= 0 && nc < C.tx) act[((size_t)nk * C.ty + nr) * C.tx + nc] = 1u;
            }
}

// one lane: the statistics, from the control block
template <class T>
__global__ void k_nf_finish(const NfCtl* __restrict__ ctl, int last_round, typename T::stats_t* st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->converged = ctl->marks[last_round & 1] == 0u ? 1 : 0;
    st->rounds = ctl->rounds;
    st->tile_visits = (int64_t)ctl->visits;
    st->n_bad_seeds = ctl->n_bad;
    st->reserved_ = 0;
}

// one lane per seed: parent T::SEED where the field equals a seed value placed there
template <class T>
__global__ void __launch_bounds__(256) k_nf_seed_parent(NfCfg C, const uint8_t* __restrict__ cost, const int32_t* __restrict__ seeds, int S,
                                                        const uint32_t* __restrict__ field, uint8_t* parent)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= S) return;
    const int k = seeds[s * 4], r = seeds[s * 4 + 1], c = seeds[s * 4 + 2];
    const uint32_t v = (uint32_t)seeds[s * 4 + 3];
    if (!(k >= 0 && k < C.D && r >= 0 && r < C.H && c >= 0 && c < C.W)) return;
    const size_t o = ((size_t)k * C.H + r) * C.W + c;
    if ((int)cost[o] >= C.lethal) return;
    if (field[o] == (v > NF_MAXV ? NF_MAXV : v)) parent[o] = T::SEED;      // (several seeds of one value on a cell store the same byte)
}

// one lane per start: follows parents for at most L cells
template <class T>
__global__ void __launch_bounds__(64) k_nf_paths(int D, int H, int W, const uint32_t* __restrict__ field, const uint8_t* __restrict__ parent,
                                                 const int32_t* __restrict__ starts, int P, int L, int16_t* __restrict__ cells, int32_t* __restrict__ length,
                                                 uint8_t* __restrict__ status, uint32_t* __restrict__ cost)
{
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q >= P) return;
    int k = starts[q * 3], r = starts[q * 3 + 1], c = starts[q * 3 + 2];
    int st = 1, len = 0;                                            // truncated unless the walk ends
    uint32_t f = TSL_NAV_UNREACHED;
    bool go = true;
    const size_t hw = (size_t)H * W;
    if (!(k >= 0 && k < D && r >= 0 && r < H && c >= 0 && c < W)) { st = 3; go = false; }
    else {
        const size_t o = (size_t)k * hw + (size_t)r * W + c;
        f = field[o];
        if (f == TSL_NAV_UNREACHED || parent[o] > T::SEED) { st = 2; go = false; }
    }
    int16_t* out = cells ? cells + (size_t)q * L * T::NCOMP : nullptr;
    for (int t = 0; t < L; ++t) {
        int16_t v[3] = { -1, -1, -1 };
        if (go) {
            v[0] = (int16_t)k; v[1] = (int16_t)r; v[2] = (int16_t)c; len = t + 1;
            const int par = parent[(size_t)k * hw + (size_t)r * W + c];
            if (par == T::SEED) { st = 0; go = false; }
            else if (par > T::SEED) { st = 2; go = false; }         // a parent array that is not of this field
            else {
                T::step(par, k, r, c);
                if (!(k >= 0 && k < D && r >= 0 && r < H && c >= 0 && c < W)) { st = 2; go = false; }
            }
        }
        if (out) {
#pragma unroll
            for (int a = 0; a < T::NCOMP; ++a) out[t * T::NCOMP + a] = v[3 - T::NCOMP + a];
        }
    }
    if (length) length[q] = len;
    if (status) status[q] = (uint8_t)st;
    if (cost) cost[q] = f;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
inline void nf_release(NavFieldState** slot)
{
    NavFieldState* S = *slot;
    if (!S) return;
    void* ptrs[] = { S->act, S->ctl, S->stats };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (S->pin) (void)hipHostFree(S->pin);
    delete S;
    *slot = nullptr;
}

inline int nf_state(NavFieldState** slot, const char* name)
{
    if (*slot) return TSL_OK;
    NavFieldState* S = new NavFieldState();                         // value-initialised: every pointer null, every size 0
    if (hipHostMalloc((void**)&S->pin, 64) != hipSuccess) { delete S; (void)hipGetLastError(); set_error(std::string(name) + ": no pinned memory"); return TSL_ERR_HIP; }
    *slot = S;
    return TSL_OK;
}

#define NF_GROW(field, bytes_field, bytes) do { if ((rc = grow(&S->field, &S->bytes_field, (bytes)))) return rc; } while (0)

// a profiling bracket for a solver that has ids; kid < 0: none
inline void nf_prof_begin(tsl_tsdf* m, int kid, hipStream_t q) { if (kid >= 0) prof_begin(m, kid, q); }
inline void nf_prof_end(tsl_tsdf* m, int kid, hipStream_t q) { if (kid >= 0) prof_end(m, q); }

template <class T>
int nf_check(tsl_tsdf* m, const typename T::cfg_t* c, const void* cost, const void* seeds, int S, const void* field, NfCfg* C, const std::string& w)
{
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(cost, w + ": null cost");
    TSL_REQUIRE(field, w + ": null field");
    int rc = T::dims(c, w, C); if (rc) return rc;
    TSL_REQUIRE(S >= 0 && S <= NF_MAX_SEEDS, w + ": S must be 0 .. 65536 seeds");
    TSL_REQUIRE(seeds || S == 0, w + ": null seeds while S > 0");
    TSL_REQUIRE(c->neutral >= 1 && c->neutral <= 255, w + ": neutral must be 1 .. 255");
    TSL_REQUIRE(c->lethal >= 1 && c->lethal <= 255, w + ": lethal must be 1 .. 255");
    TSL_REQUIRE(T::rank(c->connectivity) != 0, w + T::conn_text);
    TSL_REQUIRE(c->max_rounds >= 0, w + ": max_rounds is negative");
    TSL_REQUIRE(c->rounds_fixed >= 0, w + ": rounds_fixed is negative");
    TSL_REQUIRE(c->check_every >= 0, w + ": check_every is negative");
    C->neutral = c->neutral; C->lethal = c->lethal; C->nz = T::rank(c->connectivity);
    C->tx = (C->W + T::TX - 1) / T::TX; C->ty = (C->H + T::TY - 1) / T::TY; C->tz = (C->D + T::TZ - 1) / T::TZ;
    C->max_rounds = c->max_rounds ? c->max_rounds : T::default_rounds(*C);
    C->rounds_fixed = c->rounds_fixed;
    C->check_every = c->check_every ? c->check_every : NF_CHECK_DEFAULT;
    return TSL_OK;
}

// everything on q, every pointer a device pointer.  With rounds_fixed = 0 it waits for q at each check: every check_every rounds the host reads the
// 4-byte count of marks the last round made; a round that marked nothing leaves nothing active.
template <class T>
int nf_launch(tsl_tsdf* m, hipStream_t q, const NfCfg& C, const uint8_t* cost, const int32_t* seeds, int S_n, uint32_t* field, uint8_t* parent,
              typename T::stats_t* stats)
{
    int rc;
    NavFieldState* S = T::state(m);
    const size_t tiles = (size_t)C.tx * C.ty * C.tz, cells = (size_t)C.D * C.H * C.W;
    NF_GROW(act, b_act, tiles * 2 * sizeof(uint32_t));
    NF_GROW(ctl, b_ctl, sizeof(NfCtl));
    NF_GROW(stats, b_stats, sizeof(typename T::stats_t));
    if (!stats) stats = (typename T::stats_t*)S->stats;
    uint32_t* act = (uint32_t*)S->act;
    NfCtl* ctl = (NfCtl*)S->ctl;
    TSL_HIP(hipMemsetAsync(field, 0xff, cells * sizeof(uint32_t), q));
    TSL_HIP(hipMemsetAsync(act, 0, tiles * 2 * sizeof(uint32_t), q));
    TSL_HIP(hipMemsetAsync(ctl, 0, sizeof(NfCtl), q));
    if (S_n > 0) {
        nf_prof_begin(m, T::K_SEED, q);
        hipLaunchKernelGGL(k_nf_seed<T>, dim3((unsigned)((S_n + 255) / 256)), dim3(256), 0, q, C, cost, seeds, S_n, field, act, ctl);
        nf_prof_end(m, T::K_SEED, q);
        TSL_HIP(hipGetLastError());
    }
    int r = 0;
    const int total = C.rounds_fixed > 0 ? C.rounds_fixed : C.max_rounds;
    while (r < total) {
        const int n = C.rounds_fixed > 0 ? total : (C.check_every < total - r ? C.check_every : total - r);
        for (int e = r + n; r < e; ++r) {                           // the activity maps swap every round: this round's, then the next round's
            nf_prof_begin(m, T::K_ROUND, q);
            T::round(q, C, cost, field, act + (size_t)(r & 1) * tiles, act + (size_t)((r & 1) ^ 1) * tiles, ctl, r);
            nf_prof_end(m, T::K_ROUND, q);
        }
        TSL_HIP(hipGetLastError());
        if (C.rounds_fixed > 0) break;
        TSL_HIP(hipMemcpyAsync(S->pin, &ctl->marks[(r - 1) & 1], sizeof(uint32_t), hipMemcpyDeviceToHost, q));
        TSL_HIP(hipStreamSynchronize(q));
        if (S->pin[0] == 0u) break;                                 // the last round marked nothing: nothing is active
    }
    hipLaunchKernelGGL(k_nf_finish<T>, dim3(1), dim3(64), 0, q, ctl, r - 1, stats);
    if (parent) {
        nf_prof_begin(m, T::K_PARENT, q);
        T::parent(q, C, cost, field, parent);
        if (S_n > 0) hipLaunchKernelGGL(k_nf_seed_parent<T>, dim3((unsigned)((S_n + 255) / 256)), dim3(256), 0, q, C, cost, seeds, S_n, field, parent);
        nf_prof_end(m, T::K_PARENT, q);
    }
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

template <class T>
int nf_paths_check(tsl_tsdf* m, const typename T::cfg_t* c, const void* field, const void* parent, const void* starts, int P, int L, NfCfg* C, const std::string& w)
{
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(field, w + ": null field");
    TSL_REQUIRE(parent, w + ": null parent");
    int rc = T::dims(c, w, C); if (rc) return rc;
    TSL_REQUIRE(P >= 0 && P <= NF_MAX_STARTS, w + ": P must be 0 .. 2^20 starts");
    TSL_REQUIRE(starts || P == 0, w + ": null starts while P > 0");
    TSL_REQUIRE(L >= 1, w + ": L must be at least 1");
    TSL_REQUIRE((long long)P * L <= (1ll << 28), w + ": P * L is above 2^28 cells");
    return TSL_OK;
}

template <class T>
int nf_paths_launch(tsl_tsdf* m, hipStream_t q, const NfCfg& C, const uint32_t* field, const uint8_t* parent, const int32_t* starts, int P, int L, int16_t* cells,
                    int32_t* length, uint8_t* status, uint32_t* cost)
{
    nf_prof_begin(m, T::K_PATHS, q);
    hipLaunchKernelGGL(k_nf_paths<T>, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, q, C.D, C.H, C.W, field, parent, starts, P, L, cells, length, status, cost);
    nf_prof_end(m, T::K_PATHS, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// ---- the bodies of the entry points --------------------------------------------------------------------------------------------------------------
// host pointers: runs on the handle's stream, waits and copies back
template <class T>
int nf_field_host(tsl_tsdf* m, const typename T::cfg_t* cfg, const uint8_t* cost, const int32_t* seeds, int n_seeds, uint32_t* field, uint8_t* parent,
                  typename T::stats_t* stats)
{
    typedef typename T::stats_t stats_t;
    NfCfg C;
    int rc = nf_check<T>(m, cfg, cost, seeds, n_seeds, field, &C, T::name); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nf_state(&T::state(m), T::name))) return rc;
    const size_t cells = (size_t)C.D * C.H * C.W;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_cost = st.in(cost, cells), i_seeds = st.in(seeds, (size_t)(n_seeds > 0 ? n_seeds : 0) * 4 * sizeof(int32_t)),
              i_field = st.out(field, cells * sizeof(uint32_t)), i_parent = st.out(parent, cells), i_stats = st.out(stats, sizeof(stats_t));
    if ((rc = st.upload())) return rc;
    if ((rc = nf_launch<T>(m, q, C, st.ptr<const uint8_t>(i_cost), st.ptr<const int32_t>(i_seeds), n_seeds, st.ptr<uint32_t>(i_field), st.ptr<uint8_t>(i_parent),
                           st.ptr<stats_t>(i_stats)))) return rc;
    return st.download();
}

// device pointers: ordered with the caller's stream
template <class T>
int nf_field_dev(tsl_tsdf* m, const typename T::cfg_t* cfg, const void* cost_dev, const void* seeds_dev, int n_seeds, void* field_dev, void* parent_dev, void* stats_dev,
                 void* user_stream)
{
    NfCfg C;
    int rc = nf_check<T>(m, cfg, cost_dev, seeds_dev, n_seeds, field_dev, &C, std::string(T::name) + "_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nf_state(&T::state(m), T::name))) return rc;
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nf_launch<T>(m, q, C, (const uint8_t*)cost_dev, (const int32_t*)seeds_dev, n_seeds, (uint32_t*)field_dev, (uint8_t*)parent_dev,
                           (typename T::stats_t*)stats_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

template <class T>
int nf_paths_host(tsl_tsdf* m, const typename T::cfg_t* cfg, const uint32_t* field, const uint8_t* parent, const int32_t* starts, int n_starts, int max_len,
                  int16_t* cells, int32_t* length, uint8_t* status, uint32_t* cost)
{
    NfCfg C;                                                        // of which the paths use the extents only
    int rc = nf_paths_check<T>(m, cfg, field, parent, starts, n_starts, max_len, &C, std::string(T::name) + "_paths"); if (rc) return rc;
    if (n_starts == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    const size_t ncells = (size_t)C.D * C.H * C.W, P = (size_t)n_starts, L = (size_t)max_len;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_field = st.in(field, ncells * sizeof(uint32_t)), i_parent = st.in(parent, ncells), i_starts = st.in(starts, P * 3 * sizeof(int32_t)),
              i_cells = st.out(cells, P * L * T::NCOMP * sizeof(int16_t)), i_len = st.out(length, P * sizeof(int32_t)), i_status = st.out(status, P),
              i_cost = st.out(cost, P * sizeof(uint32_t));
    if ((rc = st.upload())) return rc;
    if ((rc = nf_paths_launch<T>(m, q, C, st.ptr<const uint32_t>(i_field), st.ptr<const uint8_t>(i_parent), st.ptr<const int32_t>(i_starts), n_starts, max_len,
                                 st.ptr<int16_t>(i_cells), st.ptr<int32_t>(i_len), st.ptr<uint8_t>(i_status), st.ptr<uint32_t>(i_cost)))) return rc;
    return st.download();
}

template <class T>
int nf_paths_dev(tsl_tsdf* m, const typename T::cfg_t* cfg, const void* field_dev, const void* parent_dev, const void* starts_dev, int n_starts, int max_len,
                 void* cells_dev, void* length_dev, void* status_dev, void* cost_dev, void* user_stream)
{
    NfCfg C;
    int rc = nf_paths_check<T>(m, cfg, field_dev, parent_dev, starts_dev, n_starts, max_len, &C, std::string(T::name) + "_paths_dev"); if (rc) return rc;
    if (n_starts == 0) return TSL_OK;                               // (and no state is allocated)
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nf_paths_launch<T>(m, q, C, (const uint32_t*)field_dev, (const uint8_t*)parent_dev, (const int32_t*)starts_dev, n_starts, max_len, (int16_t*)cells_dev,
                                 (int32_t*)length_dev, (uint8_t*)status_dev, (uint32_t*)cost_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // namespace tsl

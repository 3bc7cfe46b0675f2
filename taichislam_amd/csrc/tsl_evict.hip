// tsl_evict.hip -- brick-granular evict / snapshot / restore of a DenseTSDF (include/taichislam_hip.h, "evict and restore bricks"; DESIGN.md
// "Evict and restore bricks").  The reference has no counterpart: its map is a dense field that cannot give memory back.
//
// A call selects pool bricks by one of three integer rules, packs the selected bricks' planes in ASCENDING KEY order into the caller's buffers and, when
// asked to release them, fills the holes they leave with the bricks at the top of the pool, so that the pool stays dense (mesh, frontier, ESDF, register
// and fusion walk pool indices 0 .. pool_top - 1 and take every one for live).  No atomic decides a payload row or a pool index: rows are a radix sort
// of the selected bricks by key (rocPRIM), holes and movers an inclusive scan of two flags per pool brick.  The only atomics are three counters.
//   k_ev_select_box / k_ev_mark    sel[p] of every pool brick from the box rule / from the sorted key list through the table
//   k_ev_keys                      sort key (the brick's key when selected, 2^32 - 1 otherwise) and pool index; counts the selection
//   radix sort                     the first `selected` pairs are the payload rows
//   k_ev_pack                      one workgroup per row, grid-stride: the planes in 16-byte words, no LDS
//   k_ev_flags, scan, k_ev_holes   holes = selected p < new_top ascending, movers = kept p >= new_top ascending
//   k_ev_release                   one workgroup per pool slot in [new_top, top): mover k goes to hole k (planes, owner, touch, table), the slot is zeroed
//                                  (pool_claim hands slots out as zero), evicted keys leave the table, pool_top = new_top
// Restore classifies the payload rows through the table (absent: new, present: conflict), refuses the whole call when the new bricks do not fit, then
// claims through pool_claim and copies, one workgroup per row.
#include "tsl_stage.hpp"
#include <rocprim/rocprim.hpp>

namespace tsl {

struct EvDev {
    int* sel;                          // [max_bricks] 1: the pool brick is selected
    uint32_t *key, *key_s;             // [max_bricks] sort key, unsorted / sorted
    int *ord, *ord_s;                  // [max_bricks] pool index, unsorted / sorted by key
    unsigned long long *fl, *sc;       // [max_bricks] { hole | mover << 32 } and its inclusive scan
    int* holes;                        // [max_bricks] the holes, ascending
    int* ctr;                          // [0] selected [1] missing [2] keys out of range [3] new rows [4] conflicts [5] rows out of order
};
struct EvictState {
    EvDev D; bool ready;
    void* temp; size_t b_temp;         // rocPRIM
    void* kin; size_t b_kin;           // the key list of a call: as given | sorted
    void* rows; size_t b_rows;         // restore: per payload row its key in this map | its pool brick (-1: absent)
};

#define EV_KEEP_BOX 0
#define EV_CLEAR_BOX 1
#define EV_KEYS 2
struct EvBox { int lo[3], hi[3]; };

__device__ __forceinline__ void ev_count(int* ctr, bool pred)
{
    const unsigned long long m = __ballot(pred);
    if (m && lane_id() == (int)__builtin_ctzll(m)) __hip_atomic_fetch_add(ctr, popc64(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// keep_box: the brick's 16^3 voxel range does not intersect [lo, hi]; clear_box: it lies wholly inside.  Integer, brick_of's geometry
__global__ void __launch_bounds__(256) k_ev_select_box(MapDev M, EvDev E, int top, int rule, int slot, EvBox B)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= top) return;
    const int key = M.owner[p], s = key / M.nb3, b = key - s * M.nb3;
    const int a0[3] = { 16 * (b / (M.nbz * M.nbx)) - M.hN, 16 * ((b / M.nbz) % M.nbx) - M.hN, 16 * (b % M.nbz) - M.hNz };
    bool meets = true, inside = true;
    for (int a = 0; a < 3; ++a) {
        meets = meets && a0[a] <= B.hi[a] && a0[a] + 15 >= B.lo[a];
        inside = inside && a0[a] >= B.lo[a] && a0[a] + 15 <= B.hi[a];
    }
    E.sel[p] = ((slot < 0 || s == slot) && (rule == EV_KEEP_BOX ? !meets : inside)) ? 1 : 0;
}

// keys rule: the list is sorted, so a duplicate follows its first copy and counts once
__global__ void __launch_bounds__(256) k_ev_mark(MapDev M, EvDev E, const int* __restrict__ ks, int nkeys, int top, long long all)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool bad = false, miss = false;
    if (i < nkeys) {
        const int k = ks[i];
        if (k < 0 || (long long)k >= all) bad = true;
        else if (i == 0 || ks[i - 1] != k) {
            const int p = M.table[k];
            if (p < 0 || p >= top) miss = true; else E.sel[p] = 1;
        }
    }
    ev_count(&E.ctr[2], bad); ev_count(&E.ctr[1], miss);
}

__global__ void __launch_bounds__(256) k_ev_keys(MapDev M, EvDev E, int top)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    bool s = false;
    if (p < top) { s = E.sel[p] != 0; E.key[p] = s ? (uint32_t)M.owner[p] : 0xffffffffu; E.ord[p] = p; }
    ev_count(&E.ctr[0], s);
}

// n16 16-byte words from src to dst by the 256 threads of the workgroup; ZERO: the source is cleared behind the read (the same thread does both)
template <bool ZERO>
__device__ __forceinline__ void ev_copy(uint4* __restrict__ dst, uint4* __restrict__ src, int n16)
{
    for (int w = threadIdx.x; w < n16; w += 256) { dst[w] = src[w]; if (ZERO) src[w] = make_uint4(0u, 0u, 0u, 0u); }
}
__device__ __forceinline__ void ev_zero(uint4* dst, int n16) { for (int w = threadIdx.x; w < n16; w += 256) dst[w] = make_uint4(0u, 0u, 0u, 0u); }
#define EV_TW16 (TSL_BRK3 * 4 / 16)
#define EV_B16 (TSL_BRK3 / 16)
#define EV_COL16 (TSL_BRK3 * 8 / 16)
__device__ __forceinline__ uint4* ev_tw(const MapDev& M, int p) { return reinterpret_cast<uint4*>(M.tw + (size_t)p * TSL_BRK3); }
__device__ __forceinline__ uint4* ev_obs(const MapDev& M, int p) { return reinterpret_cast<uint4*>(M.obs + (size_t)p * TSL_BRK3); }
__device__ __forceinline__ uint4* ev_occ(const MapDev& M, int p) { return reinterpret_cast<uint4*>(M.occ + (size_t)p * TSL_BRK3); }
__device__ __forceinline__ uint4* ev_col(const MapDev& M, int p) { return reinterpret_cast<uint4*>(M.col + (size_t)p * TSL_BRK3 * 4); }

// the payload: row r = the selected brick with the r-th smallest key
__global__ void __launch_bounds__(256) k_ev_pack(MapDev M, EvDev E, int nrows, int* keys, uint4* tw, uint4* obs, uint4* occ, uint4* col)
{
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int p = E.ord_s[r];
        if (keys && threadIdx.x == 0) keys[r] = (int)E.key_s[r];
        if (tw) ev_copy<false>(tw + (size_t)r * EV_TW16, ev_tw(M, p), EV_TW16);
        if (obs) ev_copy<false>(obs + (size_t)r * EV_B16, ev_obs(M, p), EV_B16);
        if (occ) ev_copy<false>(occ + (size_t)r * EV_B16, ev_occ(M, p), EV_B16);
        if (col && M.col) ev_copy<false>(col + (size_t)r * EV_COL16, ev_col(M, p), EV_COL16);
    }
}

__global__ void __launch_bounds__(256) k_ev_flags(EvDev E, int top, int new_top)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= top) return;
    const bool s = E.sel[p] != 0;
    E.fl[p] = (unsigned long long)(s && p < new_top) | ((unsigned long long)(!s && p >= new_top) << 32);
}
__global__ void __launch_bounds__(256) k_ev_holes(EvDev E, int top)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < top && (E.fl[p] & 1ull)) E.holes[(uint32_t)E.sc[p] - 1u] = p;
}

// one workgroup per pool slot p in [new_top, top): a selected one is cleared; a kept one is mover k and goes to hole k.  Sources (>= new_top) and
// destinations (< new_top) are disjoint, every slot and every table entry has one writer.
__global__ void __launch_bounds__(256) k_ev_release(MapDev M, EvDev E, int top, int new_top)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) M.pool_top[0] = new_top;
    for (int p = new_top + blockIdx.x; p < top; p += gridDim.x) {
        if (E.sel[p]) {
            if (threadIdx.x == 0) { M.table[M.owner[p]] = TSL_EMPTY; M.touch[p] = 0; }
            ev_zero(ev_tw(M, p), EV_TW16); ev_zero(ev_obs(M, p), EV_B16); ev_zero(ev_occ(M, p), EV_B16);
            if (M.col) ev_zero(ev_col(M, p), EV_COL16);
        } else {
            const int h = E.holes[(uint32_t)(E.sc[p] >> 32) - 1u];
            if (threadIdx.x == 0) {
                const int o = M.owner[p];
                M.table[M.owner[h]] = TSL_EMPTY;                  // the evicted brick that lived in the hole
                M.owner[h] = o; M.table[o] = h;
                M.touch[h] = M.touch[p]; M.touch[p] = 0;
            }
            ev_copy<true>(ev_tw(M, h), ev_tw(M, p), EV_TW16); ev_copy<true>(ev_obs(M, h), ev_obs(M, p), EV_B16); ev_copy<true>(ev_occ(M, h), ev_occ(M, p), EV_B16);
            if (M.col) ev_copy<true>(ev_col(M, h), ev_col(M, p), EV_COL16);
        }
    }
}

// restore: the key of every payload row in this map (slot >= 0: its brick in that slot), whether the brick exists, and the order of the rows
__device__ __forceinline__ long long rs_key(int k, int slot, int nb3) { return k < 0 ? -1ll : (slot >= 0 ? (long long)slot * nb3 + k % nb3 : (long long)k); }
__global__ void __launch_bounds__(256) k_rs_classify(MapDev M, EvDev E, const int* __restrict__ keys, int n, int slot, int top, long long all, int* rows)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool bad = false, order = false, fresh = false, conflict = false;
    if (r < n) {
        const long long k = rs_key(keys[r], slot, M.nb3);
        if (k < 0 || k >= all) { bad = true; rows[r] = -1; rows[n + r] = -1; }
        else {
            order = r > 0 && rs_key(keys[r - 1], slot, M.nb3) >= k;
            const int p = M.table[k];
            conflict = p >= 0 && p < top; fresh = !conflict;
            rows[r] = (int)k; rows[n + r] = conflict ? p : -1;
        }
    }
    ev_count(&E.ctr[2], bad); ev_count(&E.ctr[5], order); ev_count(&E.ctr[3], fresh); ev_count(&E.ctr[4], conflict);
}
__global__ void __launch_bounds__(256) k_rs_write(MapDev M, const int* __restrict__ rows, int n, int overwrite, uint4* tw, uint4* obs, uint4* occ, uint4* col)
{
    __shared__ int s_p;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        int p = rows[n + r];
        if (p >= 0 && !overwrite) continue;                       // (uniform: every thread reads the same word)
        if (p < 0) {
            if (threadIdx.x == 0) { const int k = rows[r]; s_p = pool_claim<false>(M, k / M.nb3, k % M.nb3); }
            __syncthreads();
            p = s_p;
            __syncthreads();
            if (p < 0) continue;                                  // (cannot happen: the host checked the room; pool_claim has raised the error bit)
        }
        if (threadIdx.x == 0) M.touch[p] = 1;
        ev_copy<false>(ev_tw(M, p), tw + (size_t)r * EV_TW16, EV_TW16);
        ev_copy<false>(ev_obs(M, p), obs + (size_t)r * EV_B16, EV_B16);
        ev_copy<false>(ev_occ(M, p), occ + (size_t)r * EV_B16, EV_B16);
        if (col && M.col) ev_copy<false>(ev_col(M, p), col + (size_t)r * EV_COL16, EV_COL16);
    }
}

void evict_release(tsl_tsdf* m)
{
    EvictState* S = m->evict;
    if (!S) return;
    void* ptrs[] = { S->D.sel, S->D.key, S->D.key_s, S->D.ord, S->D.ord_s, S->D.fl, S->D.sc, S->D.holes, S->D.ctr, S->temp, S->kin, S->rows };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete S;
    m->evict = nullptr;
}

#define EV_ALLOC(field, type, count) TSL_HIP(hipMalloc((void**)&S->D.field, sizeof(type) * (size_t)(count)))
static int ev_prepare(tsl_tsdf* m)
{
    if (!m->evict) m->evict = new EvictState();      // value-initialised: every pointer null, every size 0
    EvictState* S = m->evict;
    if (S->ready) return TSL_OK;
    const size_t nb = (size_t)m->M.max_bricks;
    EV_ALLOC(sel, int, nb); EV_ALLOC(key, uint32_t, nb); EV_ALLOC(key_s, uint32_t, nb); EV_ALLOC(ord, int, nb); EV_ALLOC(ord_s, int, nb);
    EV_ALLOC(fl, unsigned long long, nb); EV_ALLOC(sc, unsigned long long, nb); EV_ALLOC(holes, int, nb); EV_ALLOC(ctr, int, 8);
    S->ready = true;
    return TSL_OK;
}

// What every call does first: refuse between merge_begin and merge_finish, flush the queued frames, finish a running ESDF update, read the brick count.
// A capacity error of the frames behind the call comes back in *pending and is returned when the call has done its work, as tsl_tsdf_reset does.
static int ev_enter(tsl_tsdf* m, const char* who, int* top, int* pending)
{
    // (between merge_begin and merge_pack the per-brick sums of the splat wait in fuse_acc under their POOL index -- fuse_dirty; from merge_union on the union list does)
    TSL_REQUIRE(m->mrg_nunion < 0 && !m->fuse_dirty, std::string(who) + ": a merge has begun on this map (tsl_tsdf_merge_begin) and is not finished; finish it first");
    TSL_HIP(hipSetDevice(m->device));
    *pending = tsl_tsdf_sync(m);
    if (*pending && *pending != TSL_ERR_CAPACITY) return *pending;
    int rc = esdf_finish(m); if (rc) return rc;
    if ((rc = tsl_tsdf_bricks_in_use(m, top))) return rc;
    return ev_prepare(m);
}
static int ev_read_ctr(tsl_tsdf* m, hipStream_t q, int* out)
{
    TSL_HIP(hipGetLastError());
    TSL_HIP(hipMemcpyAsync(&m->h_ints[48], m->evict->D.ctr, sizeof(int) * 8, hipMemcpyDeviceToHost, q));
    TSL_HIP(hipStreamSynchronize(q));
    for (int i = 0; i < 8; ++i) out[i] = m->h_ints[48 + i];
    return TSL_OK;
}
static void ev_invalidate_esdf(tsl_tsdf* m, hipStream_t q)
{
    m->esdf_valid = false; m->esdf_query_ok = false;
    if (m->esdf_ok) (void)hipMemsetAsync(m->esdf_ok, 0, (size_t)m->M.max_bricks, q);
}
static unsigned blocks(int n) { return (unsigned)((n + 255) / 256); }

struct EvPlanes { int* keys; uint4 *tw, *obs, *occ, *col; };

// Selection: sel[] of the pool bricks and the counts.  keys_dev: the key list in device memory (keys rule)
static int ev_select(tsl_tsdf* m, hipStream_t q, const tsl_evict_cfg* cfg, const int* keys_dev, int64_t nkeys, int top, tsl_evict_stats* st)
{
    EvictState* S = m->evict;
    const long long all = (long long)m->nsub * m->nb3;
    TSL_HIP(hipMemsetAsync(S->D.ctr, 0, sizeof(int) * 8, q));
    if (cfg->rule == EV_KEYS) {
        if (top > 0) TSL_HIP(hipMemsetAsync(S->D.sel, 0, sizeof(int) * (size_t)top, q));
        if (nkeys > 0) {
            int rc = grow(&S->kin, &S->b_kin, sizeof(int) * 2 * (size_t)nkeys); if (rc) return rc;
            uint32_t* in = (uint32_t*)S->kin; uint32_t* sorted = in + nkeys;
            if ((const void*)keys_dev != (const void*)in) TSL_HIP(hipMemcpyAsync(in, keys_dev, sizeof(int) * (size_t)nkeys, hipMemcpyDeviceToDevice, q));
            size_t tb = 0;
            TSL_HIP(rocprim::radix_sort_keys(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)nkeys, 0u, 32u, q));
            if ((!S->temp || tb > S->b_temp) && (rc = grow(&S->temp, &S->b_temp, tb + 256))) return rc;
            tb = S->b_temp;
            TSL_HIP(rocprim::radix_sort_keys(S->temp, tb, in, sorted, (size_t)nkeys, 0u, 32u, q));
            hipLaunchKernelGGL(k_ev_mark, dim3(blocks((int)nkeys)), dim3(256), 0, q, m->M, S->D, (const int*)sorted, (int)nkeys, top, all);
        }
    } else if (top > 0) {
        EvBox B; for (int a = 0; a < 3; ++a) { B.lo[a] = cfg->lo[a]; B.hi[a] = cfg->hi[a]; }
        const int slot = cfg->sid < 0 ? -1 : (m->cfg.is_global_map ? 0 : cfg->sid);
        hipLaunchKernelGGL(k_ev_select_box, dim3(blocks(top)), dim3(256), 0, q, m->M, S->D, top, cfg->rule, slot, B);
    }
    if (top > 0) hipLaunchKernelGGL(k_ev_keys, dim3(blocks(top)), dim3(256), 0, q, m->M, S->D, top);
    int c[8]; int rc = ev_read_ctr(m, q, c); if (rc) return rc;
    st->selected = c[0]; st->missing = c[1];
    TSL_REQUIRE(c[2] == 0, "evict: a key lies outside [0, max_submap_num * bricks per submap)");
    return TSL_OK;
}

// Pack the selection (when P names a buffer) and release it (cfg->release).  The selection is that of ev_select, E = st->selected > 0.
static int ev_apply(tsl_tsdf* m, hipStream_t q, const tsl_evict_cfg* cfg, const EvPlanes& P, int top, tsl_evict_stats* st)
{
    EvictState* S = m->evict;
    const int E = st->selected, new_top = top - E;
    int rc;
    if (P.keys || P.tw || P.obs || P.occ || P.col) {
        size_t tb = 0;
        TSL_HIP(rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)top, 0u, 32u, q));
        if ((!S->temp || tb > S->b_temp) && (rc = grow(&S->temp, &S->b_temp, tb + 256))) return rc;
        tb = S->b_temp;
        TSL_HIP(rocprim::radix_sort_pairs(S->temp, tb, S->D.key, S->D.key_s, S->D.ord, S->D.ord_s, (size_t)top, 0u, 32u, q));
        prof_begin(m, TSL_K_EVICT, q);
        hipLaunchKernelGGL(k_ev_pack, dim3(E < 4096 ? E : 4096), dim3(256), 0, q, m->M, S->D, E, P.keys, P.tw, P.obs, P.occ, P.col);
        prof_end(m, q);
    }
    if (cfg->release) {
        size_t tb = 0;
        TSL_HIP(rocprim::inclusive_scan(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)top, rocprim::plus<unsigned long long>(), q));
        if ((!S->temp || tb > S->b_temp) && (rc = grow(&S->temp, &S->b_temp, tb + 256))) return rc;
        prof_begin(m, TSL_K_EVICT, q);
        hipLaunchKernelGGL(k_ev_flags, dim3(blocks(top)), dim3(256), 0, q, S->D, top, new_top);
        tb = S->b_temp;
        const hipError_t es = rocprim::inclusive_scan(S->temp, tb, S->D.fl, S->D.sc, (size_t)top, rocprim::plus<unsigned long long>(), q);
        if (es == hipSuccess) {
            hipLaunchKernelGGL(k_ev_holes, dim3(blocks(top)), dim3(256), 0, q, S->D, top);
            hipLaunchKernelGGL(k_ev_release, dim3(E < 4096 ? E : 4096), dim3(256), 0, q, m->M, S->D, top, new_top);
        }
        prof_end(m, q);                                         // (the bracket is closed before any status is looked at)
        TSL_HIP(es);
        unsigned long long* tot = reinterpret_cast<unsigned long long*>(&m->h_ints[56]);
        TSL_HIP(hipGetLastError());
        TSL_HIP(hipMemcpyAsync(tot, S->D.sc + (top - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
        ev_invalidate_esdf(m, q);
        TSL_HIP(hipStreamSynchronize(q));
        st->moved = (int)(*tot >> 32);
        st->bricks_after = new_top;
    }
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

static int ev_check_cfg(tsl_tsdf* m, const tsl_evict_cfg* cfg, const void* keys_in, int64_t nkeys, int64_t cap, tsl_evict_stats* stats)
{
    TSL_REQUIRE(m && cfg && stats, "evict: null argument");
    TSL_REQUIRE(cfg->rule >= EV_KEEP_BOX && cfg->rule <= EV_KEYS, "evict: rule must be TSL_EVICT_KEEP_BOX, TSL_EVICT_CLEAR_BOX or TSL_EVICT_KEYS");
    TSL_REQUIRE(cap >= 0 && cap <= 0x7fffffffll, "evict: bad capacity");
    if (cfg->rule == EV_KEYS) TSL_REQUIRE(nkeys >= 0 && nkeys <= 0x7fffffffll && (nkeys == 0 || keys_in), "evict: the keys rule needs a key list");
    else {
        for (int a = 0; a < 3; ++a) TSL_REQUIRE(cfg->lo[a] <= cfg->hi[a], "evict: the box is empty (lo > hi)");
        TSL_REQUIRE(cfg->sid >= -1 && (cfg->sid <= 0 || (!m->cfg.is_global_map && cfg->sid < m->nsub)), "evict: submap id out of range");
    }
    return TSL_OK;
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_evict_dev(tsl_tsdf* m, const tsl_evict_cfg* cfg, const void* keys_in_dev, int64_t nkeys, void* keys_dev, void* tw_dev, void* obs_dev, void* occ_dev,
                       void* col_dev, int64_t cap, tsl_evict_stats* stats, void* user_stream)
{
    int rc = ev_check_cfg(m, cfg, keys_in_dev, nkeys, cap, stats); if (rc) return rc;
    TSL_REQUIRE(aligned16(keys_dev) && aligned16(tw_dev) && aligned16(obs_dev) && aligned16(occ_dev) && aligned16(col_dev), "evict_dev: payload buffers must be 16-byte aligned");
    std::memset(stats, 0, sizeof(*stats));
    int top = 0, pending = 0;
    if ((rc = ev_enter(m, "evict", &top, &pending))) return rc;
    stats->bricks_before = stats->bricks_after = top;
    hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = ev_select(m, q, cfg, (const int*)keys_in_dev, cfg->rule == EV_KEYS ? nkeys : 0, top, stats))) return rc;
    const EvPlanes P = { (int*)keys_dev, (uint4*)tw_dev, (uint4*)obs_dev, (uint4*)occ_dev, (uint4*)col_dev };
    const bool pack = P.keys || P.tw || P.obs || P.occ || P.col;
    if (pack && stats->selected > cap) { set_error("evict: the payload buffers are too small for the selection (stats.selected rows); nothing was changed"); return TSL_ERR_CAPACITY; }
    if (stats->selected > 0 && (pack || cfg->release) && (rc = ev_apply(m, q, cfg, P, top, stats))) return rc;
    if ((rc = order_after(m, (hipStream_t)user_stream, q))) return rc;
    return pending;
}

int tsl_tsdf_evict(tsl_tsdf* m, const tsl_evict_cfg* cfg, const int32_t* keys_in, int64_t nkeys, int32_t* keys, uint32_t* tw, int8_t* obs, int8_t* occ, uint16_t* col,
                   int64_t cap, tsl_evict_stats* stats)
{
    int rc = ev_check_cfg(m, cfg, keys_in, nkeys, cap, stats); if (rc) return rc;
    std::memset(stats, 0, sizeof(*stats));
    int top = 0, pending = 0;
    if ((rc = ev_enter(m, "evict", &top, &pending))) return rc;
    stats->bricks_before = stats->bricks_after = top;
    hipStream_t q = ms(m);
    EvictState* S = m->evict;
    const int64_t nk = cfg->rule == EV_KEYS ? nkeys : 0;
    if (nk > 0) {
        if ((rc = grow(&S->kin, &S->b_kin, sizeof(int) * 2 * (size_t)nk))) return rc;
        TSL_HIP(hipMemcpyAsync(S->kin, keys_in, sizeof(int) * (size_t)nk, hipMemcpyHostToDevice, q));
    }
    if ((rc = ev_select(m, q, cfg, (const int*)S->kin, nk, top, stats))) return rc;
    const bool pack = keys || tw || obs || occ || col;
    if (pack && stats->selected > cap) { set_error("evict: the payload buffers are too small for the selection (stats.selected rows); nothing was changed"); return TSL_ERR_CAPACITY; }
    const size_t n = (size_t)stats->selected;
    if (n > 0 && (pack || cfg->release)) {
        // the planes of the selection are staged in the handle's staging buffer (tsl_stage.hpp: every call that uses it waits for the stream before it returns)
        const bool hc = col && m->M.col;
        const size_t o_keys = 0, o_tw = (n * 4 + 15) & ~(size_t)15, o_obs = o_tw + (tw ? n * TSL_BRK3 * 4 : 0), o_occ = o_obs + (obs ? n * TSL_BRK3 : 0),
                     o_col = o_occ + (occ ? n * TSL_BRK3 : 0), total = o_col + (hc ? n * TSL_BRK3 * 8 : 0);
        if (pack && (rc = grow(&m->xbuf, &m->xbuf_bytes, total + 64))) return rc;
        char* base = (char*)m->xbuf;
        const EvPlanes P = { pack && keys ? (int*)(base + o_keys) : nullptr, pack && tw ? (uint4*)(base + o_tw) : nullptr, pack && obs ? (uint4*)(base + o_obs) : nullptr,
                             pack && occ ? (uint4*)(base + o_occ) : nullptr, pack && hc ? (uint4*)(base + o_col) : nullptr };
        if ((rc = ev_apply(m, q, cfg, P, top, stats))) return rc;
        TSL_HIP(hipStreamSynchronize(q));
        if (keys) TSL_HIP(hipMemcpy(keys, base + o_keys, n * 4, hipMemcpyDeviceToHost));
        if (tw) TSL_HIP(hipMemcpy(tw, base + o_tw, n * TSL_BRK3 * 4, hipMemcpyDeviceToHost));
        if (obs) TSL_HIP(hipMemcpy(obs, base + o_obs, n * TSL_BRK3, hipMemcpyDeviceToHost));
        if (occ) TSL_HIP(hipMemcpy(occ, base + o_occ, n * TSL_BRK3, hipMemcpyDeviceToHost));
        if (hc) TSL_HIP(hipMemcpy(col, base + o_col, n * TSL_BRK3 * 8, hipMemcpyDeviceToHost));
    }
    return pending;
}

static int restore_impl(tsl_tsdf* m, hipStream_t q, const int* keys_dev, const EvPlanes& P, int64_t n, int sid, int on_conflict, int top, tsl_evict_stats* stats)
{
    EvictState* S = m->evict;
    int rc = grow(&S->rows, &S->b_rows, sizeof(int) * 2 * (size_t)n); if (rc) return rc;
    const int slot = sid < 0 ? -1 : (m->cfg.is_global_map ? 0 : sid);
    TSL_HIP(hipMemsetAsync(S->D.ctr, 0, sizeof(int) * 8, q));
    hipLaunchKernelGGL(k_rs_classify, dim3(blocks((int)n)), dim3(256), 0, q, m->M, S->D, keys_dev, (int)n, slot, top, (long long)m->nsub * m->nb3, (int*)S->rows);
    int c[8]; if ((rc = ev_read_ctr(m, q, c))) return rc;
    TSL_REQUIRE(c[2] == 0, "restore_bricks: a key lies outside [0, max_submap_num * bricks per submap)");
    TSL_REQUIRE(c[5] == 0, "restore_bricks: the keys (of the slot they go to) must ascend strictly");
    if ((int64_t)top + c[3] > m->M.max_bricks) { set_error("restore_bricks: the payload's new bricks do not fit the pool (max_bricks); nothing was changed"); return TSL_ERR_CAPACITY; }
    stats->restored = c[3] + (on_conflict ? c[4] : 0); stats->skipped = on_conflict ? 0 : c[4];
    stats->bricks_after = top + c[3];
    if (stats->restored == 0) return TSL_OK;
    ev_invalidate_esdf(m, q);
    hipLaunchKernelGGL(k_rs_write, dim3(n < 4096 ? (unsigned)n : 4096u), dim3(256), 0, q, m->M, (const int*)S->rows, (int)n, on_conflict, P.tw, P.obs, P.occ, P.col);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}
static int restore_check(tsl_tsdf* m, const void* keys, const void* tw, const void* obs, const void* occ, int64_t n, int sid, int on_conflict, tsl_evict_stats* stats)
{
    TSL_REQUIRE(m && stats, "restore_bricks: null argument");
    TSL_REQUIRE(n >= 0 && n <= 0x7fffffffll && (n == 0 || (keys && tw && obs && occ)), "restore_bricks: null planes or a bad row count");
    TSL_REQUIRE(on_conflict == 0 || on_conflict == 1, "restore_bricks: on_conflict must be TSL_RESTORE_SKIP or TSL_RESTORE_OVERWRITE");
    TSL_REQUIRE(sid >= -1 && (sid <= 0 || (!m->cfg.is_global_map && sid < m->nsub)), "restore_bricks: submap id out of range");
    return TSL_OK;
}

int tsl_tsdf_restore_bricks_dev(tsl_tsdf* m, const void* keys_dev, const void* tw_dev, const void* obs_dev, const void* occ_dev, const void* col_dev, int64_t n, int sid,
                                int on_conflict, tsl_evict_stats* stats, void* user_stream)
{
    int rc = restore_check(m, keys_dev, tw_dev, obs_dev, occ_dev, n, sid, on_conflict, stats); if (rc) return rc;
    TSL_REQUIRE(aligned16(tw_dev) && aligned16(obs_dev) && aligned16(occ_dev) && aligned16(col_dev), "restore_bricks_dev: payload buffers must be 16-byte aligned");
    std::memset(stats, 0, sizeof(*stats));
    int top = 0, pending = 0;
    if ((rc = ev_enter(m, "restore_bricks", &top, &pending))) return rc;
    stats->bricks_before = stats->bricks_after = top;
    if (n == 0) return pending;
    hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    const EvPlanes P = { nullptr, (uint4*)tw_dev, (uint4*)obs_dev, (uint4*)occ_dev, (uint4*)col_dev };
    if ((rc = restore_impl(m, q, (const int*)keys_dev, P, n, sid, on_conflict, top, stats))) return rc;
    if ((rc = order_after(m, (hipStream_t)user_stream, q))) return rc;
    return pending;
}

int tsl_tsdf_restore_bricks(tsl_tsdf* m, const int32_t* keys, const uint32_t* tw, const int8_t* obs, const int8_t* occ, const uint16_t* col, int64_t n, int sid,
                            int on_conflict, tsl_evict_stats* stats)
{
    int rc = restore_check(m, keys, tw, obs, occ, n, sid, on_conflict, stats); if (rc) return rc;
    std::memset(stats, 0, sizeof(*stats));
    int top = 0, pending = 0;
    if ((rc = ev_enter(m, "restore_bricks", &top, &pending))) return rc;
    stats->bricks_before = stats->bricks_after = top;
    if (n == 0) return pending;
    hipStream_t q = ms(m);
    const size_t c = (size_t)n;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_k = st.in(keys, c * 4), i_tw = st.in(tw, c * TSL_BRK3 * 4), i_obs = st.in(obs, c * TSL_BRK3), i_occ = st.in(occ, c * TSL_BRK3),
              i_col = st.in(m->M.col ? col : nullptr, c * TSL_BRK3 * 8);
    if ((rc = st.upload())) return rc;
    const EvPlanes P = { nullptr, st.ptr<uint4>(i_tw), st.ptr<uint4>(i_obs), st.ptr<uint4>(i_occ), st.ptr<uint4>(i_col) };
    if ((rc = restore_impl(m, q, st.ptr<const int>(i_k), P, n, sid, on_conflict, top, stats))) return rc;
    TSL_HIP(hipStreamSynchronize(q));
    return pending;
}

int tsl_tsdf_brick_keys_dev(tsl_tsdf* m, void* keys_dev, int64_t cap, int32_t* n, void* user_stream)
{
    TSL_REQUIRE(m && n && cap >= 0, "brick_keys: bad argument");
    TSL_HIP(hipSetDevice(m->device));
    int top = 0; int rc = tsl_tsdf_bricks_in_use(m, &top); if (rc) return rc;
    *n = top;
    if (!keys_dev || top == 0) return TSL_OK;
    if (top > cap) { set_error("brick_keys: the buffer is too small (*n keys)"); return TSL_ERR_CAPACITY; }
    hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    TSL_HIP(hipMemcpyAsync(keys_dev, m->M.owner, sizeof(int) * (size_t)top, hipMemcpyDeviceToDevice, q));
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_tsdf_brick_keys(tsl_tsdf* m, int32_t* keys, int64_t cap, int32_t* n)
{
    TSL_REQUIRE(m && n && cap >= 0, "brick_keys: bad argument");
    TSL_HIP(hipSetDevice(m->device));
    int top = 0; int rc = tsl_tsdf_bricks_in_use(m, &top); if (rc) return rc;      // (issues the queued frames and waits for them)
    *n = top;
    if (!keys || top == 0) return TSL_OK;
    if (top > cap) { set_error("brick_keys: the buffer is too small (*n keys)"); return TSL_ERR_CAPACITY; }
    TSL_HIP(hipMemcpy(keys, m->M.owner, sizeof(int) * (size_t)top, hipMemcpyDeviceToHost));
    return TSL_OK;
}

}  // extern "C"

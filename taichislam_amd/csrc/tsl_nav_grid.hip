// tsl_nav_grid.hip -- height bands of the TSDF projected into 2-D navigation grids: per band and (x, y) column a class (free / occupied / unknown), the
// squared planar distance to the nearest obstacle column and, through a caller's table, a cost.  This is what a 2-D planner
// or a costmap layer consumes; the reference has no such pass.  Everything is integer except the one f32 comparison of the voxel classes, so the
// result depends on no schedule and tests/nav_grid_ref.py restates it bit for bit.
//
// Definition.  The pass reads the submap slot of tsl_tsdf_query_points and writes nothing to the map.
//   Voxel classes: those of tsl_tsdf_frontier_extract -- UNKNOWN: brick absent or observed count <= 0; OCCUPIED: observed and the f16 TSDF widened to
//     f32 < thres; FREE: every other observed voxel (thres = free_thres, 0 = the map's surface threshold) -- with ONE difference: an observed voxel
//     whose TSDF is a NaN (it can only come in through tsl_tsdf_import_sparse) is UNKNOWN here.  The frontier pass calls it FREE; a navigation grid
//     must not.
//   Band b: the voxel layers k_min[b] <= k <= k_max[b] (signed indices, both ends inclusive).  Per band and column: n_occ, n_free, n_unknown over the
//     band's layers, and lo / hi, the lowest / highest OCCUPIED layer (32767 / -32768 when there is none).
//   Cell class, tested in this order: TSL_NAV_OCCUPIED when n_occ >= min_occ; TSL_NAV_FREE when n_free >= min_free and (max_unknown < 0 or n_unknown <=
//     max_unknown); TSL_NAV_UNKNOWN otherwise.
//   d2: the exact squared Euclidean distance, in voxels, from the cell to the nearest obstacle cell of its band when that is <= R * R, else R * R + 1.
//     Obstacles: the OCCUPIED cells; with flags bit 0 the UNKNOWN cells too; with flags bit 1 every position just outside the grid.
//   cost: cost_unknown for an UNKNOWN cell, else lut[d2].
//
//   k_nav_project  one workgroup per brick column (bx, by), one lane per voxel column.  A lane's 16 layers of a brick are 64 contiguous bytes of tw and
//                  16 of obs: five 16-byte loads give a 16-bit occupied and a 16-bit free mask (nav_column_load, tsl_nav_common.hpp, which
//                  k_terrain_columns calls too: the one copy of the classes and of the NaN rule); every band that meets the brick takes its layers out
//                  of them with an AND, two popcounts and a find-first / find-last.  The map is read once however many bands there are; an absent
//                  brick and a brick no band meets cost no memory access.
//   k_nav_rows     along j: g = the distance to the nearest obstacle of the row, capped at R + 1.  A wave per row: the row's obstacles become a bit
//                  string in LDS (one ballot per 64 cells), a cell finds its nearest set bit on either side with a count-leading / trailing-zeros
//                  over at most R / 64 + 2 words.
//   k_nav_cols     along i: d2 = min over di of di * di + g[ui + di][uj]^2, clipped to R * R + 1.  A workgroup takes 16 rows x 64 columns and stages
//                  the (16 + 2 R) x 64 bytes of g it needs in LDS (at most 33.5 KiB, whatever N is); a lane owns one column and 4 rows, reads each
//                  staged value once and feeds it to its 4 running minima.  The cost lookup rides along.  (16 rows per lane, a 64 x 64 tile, read a
//                  quarter of the LDS but left a 256^2 grid with 16 workgroups whose lanes each walk a chain of 16 + 2 R steps: at R = 254 the
//                  pass took 101 us, latency of that one chain, on a device that was otherwise empty -- profiles/nav_grid.txt.)
// The wall (flags bit 1) is the initial value of both passes.  No atomics, no iteration, no workgroup waits for another.
#include "tsl_nav_common.hpp"
#include "tsl_stage.hpp"

namespace tsl {

#define NAV_TILE 64            // k_nav_cols: columns of a workgroup's tile, one per lane
#define NAV_RB 4               // ... rows per lane
#define NAV_ROWS (4 * NAV_RB)  // ... rows of the tile (four waves)
#define NAV_G_FAR 255          // staged g of a row outside the grid: 255^2 > R * R + 1 for every R <= 254

struct NavCfg : NavBands { int R, flags, min_occ, min_free, max_unknown, cost_unknown; };

struct NavState { void *cls, *g; size_t b_cls, b_g; };      // scratch of the distance passes: the classes when the caller wants none, g

// ---- projection -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nav_project(MapDev M, NavCfg C, uint8_t* __restrict__ cls, uint16_t* __restrict__ counts, int16_t* __restrict__ span)
{
    const int bx = (int)blockIdx.x / M.nbx, by = (int)blockIdx.x - bx * M.nbx;
    const int tid = threadIdx.x;                                   // li * 16 + lj: the lane's 16 layers are voxels tid * 16 .. tid * 16 + 15 of a brick
    const int* __restrict__ T = M.table + (size_t)C.s * M.nb3 + (size_t)(bx * M.nbx + by) * M.nbz;
    int nocc[NAV_MAX_BANDS], nfree[NAV_MAX_BANDS], lo[NAV_MAX_BANDS], hi[NAV_MAX_BANDS];
#pragma unroll
    for (int b = 0; b < NAV_MAX_BANDS; ++b) { nocc[b] = 0; nfree[b] = 0; lo[b] = 0x7fffffff; hi[b] = -1; }
    int umin = 0x7fffffff, umax = -1;                              // (uniform) the hull of the bands
    for (int b = 0; b < C.B; ++b) { umin = min(umin, C.uk0[b]); umax = max(umax, C.uk1[b]); }

    for (int bz = umin >> 4; bz <= (umax >> 4); ++bz) {
        const int z0 = bz * 16;
        bool met = false;                                          // (uniform) does any band hold a layer of this brick
        for (int b = 0; b < C.B; ++b) met = met || (C.uk0[b] <= z0 + 15 && C.uk1[b] >= z0);
        if (!met) continue;
        const int P = T[bz];
        if (P < 0) continue;                                       // absent: 16 unknown layers, which the counts below get as the remainder
        uint32_t mo, mf, tw[16];
        nav_column_load(M, P, tid, C.thres, mo, mf, tw);
#pragma unroll
        for (int b = 0; b < NAV_MAX_BANDS; ++b) {
            const int l0 = max(C.uk0[b], z0) - z0, l1 = min(C.uk1[b], z0 + 15) - z0;      // (a band beyond n_bands is empty: uk0 = 0, uk1 = -1)
            if (l0 <= l1) {                                        // (uniform)
                const uint32_t lm = ((2u << l1) - 1u) & ~((1u << l0) - 1u);
                const uint32_t o = mo & lm;
                nocc[b] += __popc(o);
                nfree[b] += __popc(mf & lm);
                if (o) { lo[b] = min(lo[b], z0 + (int)__builtin_ctz(o)); hi[b] = max(hi[b], z0 + 31 - (int)__builtin_clz(o)); }
            }
        }
    }

    const int ui = bx * 16 + (tid >> 4), uj = by * 16 + (tid & 15);
    const int mocc = C.min_occ ? C.min_occ : 1, mfree = C.min_free ? C.min_free : 1;
#pragma unroll
    for (int b = 0; b < NAV_MAX_BANDS; ++b) {
        if (b >= C.B) continue;                                    // (uniform)
        const size_t o = ((size_t)b * M.N + ui) * M.N + uj;
        const int nunk = (C.uk1[b] - C.uk0[b] + 1) - nocc[b] - nfree[b];
        if (cls) {
            int c = TSL_NAV_UNKNOWN;
            if (nocc[b] >= mocc) c = TSL_NAV_OCCUPIED;
            else if (nfree[b] >= mfree && (C.max_unknown < 0 || nunk <= C.max_unknown)) c = TSL_NAV_FREE;
            cls[o] = (uint8_t)c;
        }
        if (counts) { counts[o * 3] = (uint16_t)nocc[b]; counts[o * 3 + 1] = (uint16_t)nfree[b]; counts[o * 3 + 2] = (uint16_t)nunk; }
        if (span) { span[o * 2] = (int16_t)(hi[b] < 0 ? 32767 : lo[b] - M.hNz); span[o * 2 + 1] = (int16_t)(hi[b] < 0 ? -32768 : hi[b] - M.hNz); }
    }
}

// ---- distance transform, along j ---------------------------------------------------------------------------------------------------------
// One wave per row of one band.  words = ceil(N / 64); dynamic LDS: 4 * words * 8 bytes.
__global__ void __launch_bounds__(256) k_nav_rows(int N, int rows, int R, int flags, int words, const uint8_t* __restrict__ cls, uint8_t* __restrict__ g)
{
    extern __shared__ unsigned long long s_nav_bits[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + wave;                     // b * N + ui
    const bool live = row < rows;
    unsigned long long* bits = s_nav_bits + (size_t)wave * words;
    const size_t base = (size_t)(live ? row : 0) * N;
    for (int w = 0; w < words; ++w) {
        const int uj = w * 64 + lane;
        bool ob = false;
        if (live && uj < N) { const int c = cls[base + uj]; ob = c == TSL_NAV_OCCUPIED || ((flags & 1) && c == TSL_NAV_UNKNOWN); }
        const unsigned long long bal = __ballot(ob);
        if (lane == 0) bits[w] = bal;
    }
    __syncthreads();                                                // (every wave of the workgroup makes the same number of trips)
    if (!live) return;
    const int cap = R + 1, far = R / 64 + 1;                        // a set bit more than `far` words away is farther than R + 1 cells
    for (int w = 0; w < words; ++w) {
        const int uj = w * 64 + lane;
        if (uj >= N) break;
        int d = cap;
        if (flags & 2) d = min(d, min(uj + 1, N - uj));            // the wall: obstacles at uj = -1 and uj = N
        // nearest obstacle at or below uj
        unsigned long long m = bits[w] & (~0ull >> (63 - lane));
        for (int v = w; ; ) {
            if (m) { d = min(d, uj - (v * 64 + 63 - (int)__builtin_clzll(m))); break; }
            if (--v < 0 || w - v > far) break;
            m = bits[v];
        }
        // nearest obstacle above uj
        m = lane == 63 ? 0ull : bits[w] & (~0ull << (lane + 1));
        for (int v = w; ; ) {
            if (m) { d = min(d, v * 64 + (int)__builtin_ctzll(m) - uj); break; }
            if (++v >= words || v - w > far) break;
            m = bits[v];
        }
        g[base + uj] = (uint8_t)d;
    }
}

// ---- distance transform, along i, and the cost -------------------------------------------------------------------------------------------
// grid (column strips, row tiles, bands); dynamic LDS: (NAV_ROWS + 2 R) * NAV_TILE bytes
__global__ void __launch_bounds__(256) k_nav_cols(int N, int R, int flags, int cost_unknown, const uint8_t* __restrict__ g, const uint8_t* __restrict__ cls,
                                                  const uint8_t* __restrict__ lut, uint16_t* __restrict__ d2, uint8_t* __restrict__ cost)
{
    extern __shared__ uint32_t s_nav_g[];                           // [NAV_ROWS + 2 R][16] words = [..][64] bytes
    const int uj0 = (int)blockIdx.x * NAV_TILE, ui0 = (int)blockIdx.y * NAV_ROWS, b = (int)blockIdx.z;
    const int nrow = NAV_ROWS + 2 * R;
    const size_t plane = (size_t)b * N * N;
    for (int e = threadIdx.x; e < nrow * 16; e += 256) {
        const int r = e >> 4, c = e & 15;
        const int ui = ui0 - R + r, uj = uj0 + c * 4;
        uint32_t v = 0xffffffffu;                                   // NAV_G_FAR in every byte
        if (ui >= 0 && ui < N && uj < N) v = *reinterpret_cast<const uint32_t*>(g + plane + (size_t)ui * N + uj);      // (N is a multiple of 16: a word is inside the row or outside)
        s_nav_g[e] = v;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int uj = uj0 + lane, r0 = wave * NAV_RB;                  // the lane's rows: ui0 + r0 .. + NAV_RB - 1
    if (uj >= N) return;
    const uint8_t* sg = reinterpret_cast<const uint8_t*>(s_nav_g);
    const uint32_t farv = (uint32_t)(R * R + 1);
    uint32_t acc[NAV_RB];
#pragma unroll
    for (int r = 0; r < NAV_RB; ++r) {
        const int ui = ui0 + r0 + r;
        const uint32_t wd = (uint32_t)min(ui + 1, N - ui);          // the wall: obstacle rows at ui = -1 and ui = N
        acc[r] = (flags & 2) && ui < N ? min(farv, wd * wd) : farv;
    }
    // staged row s holds grid row ui0 - R + s; the lane's row r sees it at di = s - R - r0 - r.  Rows beyond |di| <= R only offer values above R * R
    for (int s = r0; s < r0 + NAV_RB + 2 * R; ++s) {
        const uint32_t gv = sg[s * NAV_TILE + lane];
        const uint32_t g2 = gv * gv;
        const int d0 = s - R - r0;
#pragma unroll
        for (int r = 0; r < NAV_RB; ++r) { const int di = d0 - r; acc[r] = min(acc[r], (uint32_t)(di * di) + g2); }
    }
#pragma unroll
    for (int r = 0; r < NAV_RB; ++r) {
        const int ui = ui0 + r0 + r;
        if (ui >= N) break;
        const size_t o = plane + (size_t)ui * N + uj;
        const uint32_t v = min(acc[r], farv);
        if (d2) d2[o] = (uint16_t)v;
        if (cost) cost[o] = cls[o] == TSL_NAV_UNKNOWN ? (uint8_t)cost_unknown : lut[v];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
void nav_release(tsl_tsdf* m)
{
    NavState* S = m->nav;
    if (!S) return;
    void* ptrs[] = { S->cls, S->g };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete S;
    m->nav = nullptr;
}

static int nav_check(tsl_tsdf* m, const tsl_nav_cfg* c, const void* lut, const void* cls, const void* d2, const void* cost, const void* counts, const void* span,
                     NavCfg* C, const char* who)
{
    const std::string w(who);
    const int rc = nav_bands_check(m, c, lut, cls || d2 || cost || counts || span, cost, w, [&]() -> int {
        TSL_REQUIRE(c->min_occ >= 0, w + ": min_occ is negative");
        TSL_REQUIRE(c->min_free >= 0, w + ": min_free is negative");
        return TSL_OK;
    }, []() -> int { return TSL_OK; }, C);
    if (rc) return rc;
    C->R = c->radius; C->flags = c->flags;
    C->min_occ = c->min_occ; C->min_free = c->min_free; C->max_unknown = c->max_unknown; C->cost_unknown = c->cost_unknown;
    return TSL_OK;
}

// the two distance passes on q over a class plane [B][N][N] (g: B * N * N bytes of scratch); tsl_nav_terrain.hip runs them over its own classes
int nav_edt_launch(tsl_tsdf* m, hipStream_t q, int N, int B, int R, int flags, int cost_unknown, const uint8_t* cls, uint8_t* g, const uint8_t* lut, uint16_t* d2,
                   uint8_t* cost)
{
    const int words = (N + 63) / 64, rows = N * B;
    prof_begin(m, TSL_K_NAV_EDT_ROWS, q);
    hipLaunchKernelGGL(k_nav_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), sizeof(unsigned long long) * 4 * (size_t)words, q, N, rows, R, flags, words, cls, g);
    prof_end(m, q);
    prof_begin(m, TSL_K_NAV_EDT, q);
    hipLaunchKernelGGL(k_nav_cols, dim3((unsigned)((N + NAV_TILE - 1) / NAV_TILE), (unsigned)((N + NAV_ROWS - 1) / NAV_ROWS), (unsigned)B), dim3(256),
                       (size_t)(NAV_ROWS + 2 * R) * NAV_TILE, q, N, R, flags, cost_unknown, (const uint8_t*)g, cls, lut, d2, cost);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// the three launches on q; every pointer a device pointer, null planes skipped
static int nav_launch(tsl_tsdf* m, hipStream_t q, const NavCfg& C, const uint8_t* lut, uint8_t* cls, uint16_t* d2, uint8_t* cost, uint16_t* counts, int16_t* span)
{
    int rc;
    if (!m->nav) m->nav = new NavState();                          // value-initialised: every pointer null, every size 0
    NavState* S = m->nav;
    const int N = m->N;
    const size_t cells = (size_t)N * N * C.B;
    const bool edt = d2 || cost;
    if (edt) {
        if ((rc = grow(&S->g, &S->b_g, cells))) return rc;
        if (!cls) { if ((rc = grow(&S->cls, &S->b_cls, cells))) return rc; cls = (uint8_t*)S->cls; }      // the distance pass reads the classes: they go to scratch
    }
    if (cls || counts || span) {
        prof_begin(m, TSL_K_NAV_PROJECT, q);
        hipLaunchKernelGGL(k_nav_project, dim3((unsigned)(m->nbx * m->nbx)), dim3(256), 0, q, m->M, C, cls, counts, span);
        prof_end(m, q);
        TSL_HIP(hipGetLastError());
    }
    if (edt) return nav_edt_launch(m, q, N, C.B, C.R, C.flags, C.cost_unknown, cls, (uint8_t*)S->g, lut, d2, cost);
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_nav_grid(tsl_tsdf* m, const tsl_nav_cfg* cfg, const uint8_t* lut, uint8_t* cls, uint16_t* d2, uint8_t* cost, uint16_t* counts, int16_t* span)
{
    NavCfg C;
    int rc = nav_check(m, cfg, lut, cls, d2, cost, counts, span, &C, "nav_grid"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames: the pass runs behind them
    const size_t cells = (size_t)m->N * m->N * C.B;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_lut = st.in(lut, (size_t)C.R * C.R + 2), i_cls = st.out(cls, cells), i_cost = st.out(cost, cells), i_d2 = st.out(d2, cells * 2),
              i_span = st.out(span, cells * 4), i_cnt = st.out(counts, cells * 6);
    if ((rc = st.upload())) return rc;
    if ((rc = nav_launch(m, q, C, st.ptr<const uint8_t>(i_lut), st.ptr<uint8_t>(i_cls), st.ptr<uint16_t>(i_d2), st.ptr<uint8_t>(i_cost), st.ptr<uint16_t>(i_cnt),
                         st.ptr<int16_t>(i_span)))) return rc;
    return st.download();
}

int tsl_tsdf_nav_grid_dev(tsl_tsdf* m, const tsl_nav_cfg* cfg, const void* lut_dev, void* cls_dev, void* d2_dev, void* cost_dev, void* counts_dev, void* span_dev,
                          void* user_stream)
{
    NavCfg C;
    int rc = nav_check(m, cfg, lut_dev, cls_dev, d2_dev, cost_dev, counts_dev, span_dev, &C, "nav_grid_dev"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nav_launch(m, q, C, (const uint8_t*)lut_dev, (uint8_t*)cls_dev, (uint16_t*)d2_dev, (uint8_t*)cost_dev, (uint16_t*)counts_dev, (int16_t*)span_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

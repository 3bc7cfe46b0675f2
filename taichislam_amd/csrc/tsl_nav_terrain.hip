// tsl_nav_terrain.hip -- terrain layers for ground robots: per height band and (x, y) column the height of the surface a robot can
// stand on, over the robot's footprint the step and the slope of that surface, and a class, a distance and a cost in the vocabulary of the navigation
// grids (tsl_nav_grid.hip), so that the cost-to-go fields take them unchanged.  The reference has no such pass.  Everything is integer except the one f32
// comparison of the voxel classes and one f64 expression per column, so the result depends on no schedule and tests/nav_terrain_ref.py restates it bit
// for bit.
//
// Definition (all k are signed voxel layers).  The submap slot, the voxel classes and thres are those of tsl_tsdf_nav_grid: thres = free_thres, 0 = the
// map's surface threshold; an observed NaN is UNKNOWN; a layer outside the volume is UNKNOWN.
//   Bands: n_bands in 1 .. 16, k_min[b] <= k_max[b] inside the volume: the range in which the support layer is looked for.
//   Standable: layer k of a column is standable when voxel k is OCCUPIED, none of the `clearance` layers k + 1 .. k + clearance is OCCUPIED and all of the
//     `free_run` layers k + 1 .. k + free_run are FREE; 0 <= free_run <= clearance <= Nz.  The layers tested above k may leave the band; where they leave
//     the volume they are UNKNOWN -- not occupied and not free.
//   Support: the lowest (pick = 0) or the highest (pick = 1) standable layer k of the column with k_min <= k <= k_max.
//   col (u8): 0 = the column has a support; 1 = obstructed: the band holds an OCCUPIED voxel but no standable layer (a wall, a top without headroom);
//     2 = empty: no OCCUPIED voxel in the band.
//   height (int16): 16 * k + q for the support layer k, 32767 where col != 0.  q in 0 .. 15 places the level set thres between the centres of layers k
//     and k + 1.  When voxel k + 1 is FREE: r = 16.0 * ((double)thres - (double)t_k) / ((double)t_k1 - (double)t_k), the f16 values widened exactly --
//     three correctly rounded IEEE f64 operations in this order (the product with 16 is exact) -- and q = r >= 15.0 ? 15 : (r >= 0.0 ? (int)r : 0): a NaN
//     r (infinite voxels) gives 0.  When voxel k + 1 is not FREE, q = 0.  The height is that of the iso-level thres, which lies about thres above the zero
//     crossing.  A volume with Nz > 4094 is refused: height would not fit.
//   Window statistics, for the cells with col == 0, over the (2 w + 1)^2 cells within Chebyshev distance w = window (0 .. 16), clipped to the grid:
//     nsup (uint16) = how many of them have a support, step (uint16) = the maximum minus the minimum height over those; both 65535 where col != 0.
//   slope2 (uint32): a Sobel gradient of height at stride s = slope_base (1 .. 16).  With h(di, dj) = height[i + di][j + dj]:
//     gx = h(s,-s) + 2 h(s,0) + h(s,s) - h(-s,-s) - 2 h(-s,0) - h(-s,s), gy the same with the roles of i and j exchanged,
//     slope2 = min(gx^2 + gy^2, 2^32 - 2) in 64 bits; valid only when the cell and all eight cells at stride s are inside the grid and have a support,
//     2^32 - 1 otherwise.  tan(slope) = sqrt(slope2) / (128 s).
//   cls (u8, the codes of nav_grid), tested in this order: col == 1 -> OCCUPIED; col == 2 -> UNKNOWN; step > max_step -> OCCUPIED; slope2 valid and
//     > max_slope2 -> OCCUPIED; nsup < min_support -> UNKNOWN; otherwise FREE.  max_step in 0 .. 65534 sixteenths of a voxel; max_slope2 = 2^32 - 1
//     switches the slope test off.
//   d2, cost: nav_grid's own passes (k_nav_rows, k_nav_cols) over this cls plane, with its radius, flags, lut and cost_unknown.
//
//   k_terrain_columns  one workgroup per brick column, one lane per voxel column, the loads and the masks of k_nav_project (nav_column_load).  A lane walks its bricks from
//                      the top down, from the brick that holds layer min(max k_max + clearance, top), and carries two counters: the run of layers that
//                      are not occupied and the run of FREE layers directly above.  They start at "unbounded" and 0 (above the volume nothing is occupied
//                      and nothing is free; below the top the first brick's own layers settle them before a band's layer can ask).  An absent brick adds
//                      16 to the first and zeroes the second at no memory access.  The 16 layers of a brick give a 16-bit mask of standable layers; every
//                      band that meets the brick takes its support out of it with an AND and a find-first / find-last, and the two f16 values of q out of
//                      the lane's own 36 bytes of LDS (the brick's 16 values and the lowest one of the brick above: a dynamic index into registers would
//                      be a chain of selects).  The map is read once however many bands there are.
//   k_terrain_window   32 x 32 tiles of one band with a halo of max(window, slope_base) cells: at most 64 x 64 int16 heights in LDS, 32767 outside the
//                      grid.  Maximum, minimum and count are separable: one pass along j into three [32 + 2 w][32] arrays, one along i out of them; then the
//                      nine Sobel reads and the class.  No atomics, no iteration, no workgroup waits for another.
#include "tsl_nav_common.hpp"
#include "tsl_stage.hpp"

namespace tsl {

#define TER_TILE 32            // k_terrain_window: cells of a tile along each axis
#define TER_DIM 64             // ... row stride of the staged heights: the tile and a halo of at most 16 cells on each side
#define TER_NONE 32767         // height of a column without a support
#define TER_UNBOUNDED (1 << 20)

struct TerCfg : NavBands {
    int pick, clearance, free_run, window, slope_base, max_step, min_support, R, flags, cost_unknown;
    uint32_t max_slope2;
};

struct NavTerrainState { void *height, *col, *cls, *g; size_t b_height, b_col, b_cls, b_g; };      // the planes a later stage reads when the caller wants none, g

// ---- columns ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_terrain_columns(MapDev M, TerCfg C, int16_t* __restrict__ height, uint8_t* __restrict__ col)
{
    __shared__ uint32_t s_ter_t[256 * 9];                          // per lane: 16 f16 values of the brick at hand in 8 words, the lowest of the brick above in the ninth
    const int bx = (int)blockIdx.x / M.nbx, by = (int)blockIdx.x - bx * M.nbx;
    const int tid = threadIdx.x;                                   // li * 16 + lj: the lane's 16 layers are voxels tid * 16 .. tid * 16 + 15 of a brick
    const int* __restrict__ T = M.table + (size_t)C.s * M.nb3 + (size_t)(bx * M.nbx + by) * M.nbz;
    uint32_t* st = s_ter_t + tid * 9;
    int sup[NAV_MAX_BANDS];                                        // the support as an unsigned layer, -1 = none so far
    uint32_t pair[NAV_MAX_BANDS];                                  // t_k | t_k1 << 16 of it
#pragma unroll
    for (int b = 0; b < NAV_MAX_BANDS; ++b) { sup[b] = -1; pair[b] = 0u; }
    uint32_t anyocc = 0u, k1free = 0u;                             // bit b: band b holds an occupied voxel / the voxel above its support is FREE
    int umin = 0x7fffffff, umax = -1;                              // (uniform) the hull of the bands
    for (int b = 0; b < C.B; ++b) { umin = min(umin, C.uk0[b]); umax = max(umax, C.uk1[b]); }
    const int utop = min(umax + C.clearance, M.Nz - 1);            // no layer above it is asked about by a layer of a band
    int nrun = TER_UNBOUNDED, frun = 0;                            // layers directly above that are not occupied / that are FREE
    uint32_t tabove = 0u, above_free = 0u;                         // the lowest voxel of the brick above: its f16 bits, whether it is FREE

    for (int bz = utop >> 4; bz >= (umin >> 4); --bz) {
        const int z0 = bz * 16;
        const int P = T[bz];
        if (P < 0) { nrun += 16; frun = 0; above_free = 0u; continue; }      // absent: 16 unknown layers
        uint32_t mo, mf, tw[16];
        nav_column_load(M, P, tid, C.thres, mo, mf, tw);
        uint32_t ms = 0u;                                          // the standable layers of the brick
#pragma unroll
        for (int lk = 15; lk >= 0; --lk) {
            const bool occ = (mo >> lk) & 1u, fre = (mf >> lk) & 1u;
            ms |= (occ && nrun >= C.clearance && frun >= C.free_run) ? (1u << lk) : 0u;
            nrun = occ ? 0 : nrun + 1;
            frun = fre ? frun + 1 : 0;
        }
        bool met = false;                                          // (uniform) does any band hold a layer of this brick
        for (int b = 0; b < C.B; ++b) met = met || (C.uk0[b] <= z0 + 15 && C.uk1[b] >= z0);
        if (met) {
#pragma unroll
            for (int w = 0; w < 8; ++w) st[w] = (tw[2 * w] & 0xffffu) | (tw[2 * w + 1] << 16);
            st[8] = tabove;
            const uint32_t mf17 = mf | (above_free << 16);
#pragma unroll
            for (int b = 0; b < NAV_MAX_BANDS; ++b) {
                const int l0 = max(C.uk0[b], z0) - z0, l1 = min(C.uk1[b], z0 + 15) - z0;      // (a band beyond n_bands is empty: uk0 = 0, uk1 = -1)
                if (l0 <= l1) {                                    // (uniform)
                    const uint32_t lm = ((2u << l1) - 1u) & ~((1u << l0) - 1u);
                    if (mo & lm) anyocc |= 1u << b;
                    const uint32_t s = ms & lm;
                    if (s && (C.pick == 0 || sup[b] < 0)) {        // top down: the lowest is the last one found, the highest the first
                        const int lk = C.pick == 0 ? (int)__builtin_ctz(s) : 31 - (int)__builtin_clz(s);
                        const uint32_t tk = (st[lk >> 1] >> ((lk & 1) * 16)) & 0xffffu, tk1 = (st[(lk + 1) >> 1] >> (((lk + 1) & 1) * 16)) & 0xffffu;
                        sup[b] = z0 + lk;
                        pair[b] = tk | (tk1 << 16);
                        k1free = (k1free & ~(1u << b)) | (((mf17 >> (lk + 1)) & 1u) << b);
                    }
                }
            }
        }
        tabove = tw[0] & 0xffffu;
        above_free = mf & 1u;
    }

    const int ui = bx * 16 + (tid >> 4), uj = by * 16 + (tid & 15);
#pragma unroll
    for (int b = 0; b < NAV_MAX_BANDS; ++b) {
        if (b >= C.B) continue;                                    // (uniform)
        const size_t o = ((size_t)b * M.N + ui) * M.N + uj;
        int h = TER_NONE, c = ((anyocc >> b) & 1u) ? 1 : 2;
        if (sup[b] >= 0) {
            int q = 0;
            if ((k1free >> b) & 1u) {
                const double tk = (double)h2f((h16)(pair[b] & 0xffffu)), tk1 = (double)h2f((h16)(pair[b] >> 16));
                const double r = 16.0 * ((double)C.thres - tk) / (tk1 - tk);
                q = r >= 15.0 ? 15 : (r >= 0.0 ? (int)r : 0);
            }
            h = 16 * (sup[b] - M.hNz) + q;
            c = 0;
        }
        if (height) height[o] = (int16_t)h;
        if (col) col[o] = (uint8_t)c;
    }
}

// ---- window statistics, slope and class -----------------------------------------------------------------------------------------------------
// grid (tiles along j, tiles along i, bands)
__global__ void __launch_bounds__(256) k_terrain_window(int N, int window, int slope_base, int max_step, int min_support, uint32_t max_slope2,
                                                        const int16_t* __restrict__ height, const uint8_t* __restrict__ col, uint16_t* __restrict__ step,
                                                        uint16_t* __restrict__ nsup, uint32_t* __restrict__ slope2, uint8_t* __restrict__ cls)
{
    __shared__ int16_t s_ter_h[TER_DIM * TER_DIM];
    __shared__ int16_t s_ter_max[TER_DIM * TER_TILE], s_ter_min[TER_DIM * TER_TILE];
    __shared__ uint16_t s_ter_cnt[TER_DIM * TER_TILE];
    const int uj0 = (int)blockIdx.x * TER_TILE, ui0 = (int)blockIdx.y * TER_TILE, b = (int)blockIdx.z;
    const int tid = threadIdx.x;
    const int w = window, s = slope_base, H = max(w, s), D = TER_TILE + 2 * H;      // H <= 16: D <= TER_DIM
    const size_t plane = (size_t)b * N * N;
    for (int e = tid; e < D * D; e += 256) {
        const int r = e / D, c = e - r * D;
        const int gi = ui0 - H + r, gj = uj0 - H + c;
        int v = TER_NONE;
        if (gi >= 0 && gi < N && gj >= 0 && gj < N) v = height[plane + (size_t)gi * N + gj];
        s_ter_h[r * TER_DIM + c] = (int16_t)v;
    }
    __syncthreads();
    // along j: the rows ui0 - w .. ui0 + 31 + w, the tile's 32 columns
    for (int e = tid; e < (TER_TILE + 2 * w) * TER_TILE; e += 256) {
        const int rr = e >> 5, c = e & 31;
        const int16_t* row = s_ter_h + (H - w + rr) * TER_DIM + (H - w + c);
        int mx = -32768, mn = TER_NONE, n = 0;
        for (int d = 0; d <= 2 * w; ++d) {
            const int v = row[d];
            const bool has = v != TER_NONE;
            mx = max(mx, has ? v : -32768);
            mn = min(mn, v);
            n += has ? 1 : 0;
        }
        s_ter_max[e] = (int16_t)mx; s_ter_min[e] = (int16_t)mn; s_ter_cnt[e] = (uint16_t)n;
    }
    __syncthreads();
    const int c = tid & 31;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = (tid >> 5) + 8 * k;
        const int ui = ui0 + r, uj = uj0 + c;
        if (ui >= N || uj >= N) continue;
        const size_t o = plane + (size_t)ui * N + uj;
        const int16_t* hc = s_ter_h + (H + r) * TER_DIM + (H + c);
        uint32_t vstep = 65535u, vsup = 65535u, vslope = 0xffffffffu;
        int vcls;
        if (hc[0] != TER_NONE) {
            int mx = -32768, mn = TER_NONE, n = 0;
            for (int d = 0; d <= 2 * w; ++d) {
                const int a = (r + d) * TER_TILE + c;
                mx = max(mx, (int)s_ter_max[a]); mn = min(mn, (int)s_ter_min[a]); n += s_ter_cnt[a];
            }
            vstep = (uint32_t)(mx - mn); vsup = (uint32_t)n;
            const int so = s * TER_DIM;
            const int mm = hc[-so - s], m0 = hc[-so], mp = hc[-so + s], zm = hc[-s], zp = hc[s], pm = hc[so - s], p0 = hc[so], pp = hc[so + s];
            const bool valid = mm != TER_NONE && m0 != TER_NONE && mp != TER_NONE && zm != TER_NONE && zp != TER_NONE && pm != TER_NONE && p0 != TER_NONE && pp != TER_NONE;
            if (valid) {
                const long long gx = (long long)(pm + 2 * p0 + pp - mm - 2 * m0 - mp), gy = (long long)(mp + 2 * zp + pp - mm - 2 * zm - pm);
                const long long g2 = gx * gx + gy * gy;
                vslope = g2 > 0xfffffffell ? 0xfffffffeu : (uint32_t)g2;
            }
            vcls = (int)vstep > max_step ? TSL_NAV_OCCUPIED : (valid && vslope > max_slope2) ? TSL_NAV_OCCUPIED : (int)vsup < min_support ? TSL_NAV_UNKNOWN : TSL_NAV_FREE;
        } else vcls = (cls && col[o] == 1) ? TSL_NAV_OCCUPIED : TSL_NAV_UNKNOWN;
        if (step) step[o] = (uint16_t)vstep;
        if (nsup) nsup[o] = (uint16_t)vsup;
        if (slope2) slope2[o] = vslope;
        if (cls) cls[o] = (uint8_t)vcls;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
void nav_terrain_release(tsl_tsdf* m)
{
    NavTerrainState* S = m->nav_terrain;
    if (!S) return;
    void* ptrs[] = { S->height, S->col, S->cls, S->g };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete S;
    m->nav_terrain = nullptr;
}

static int ter_check(tsl_tsdf* m, const tsl_nav_terrain_cfg* c, const void* lut, bool any_out, const void* cost, TerCfg* C, const char* who)
{
    const std::string w(who);
    const int rc = nav_bands_check(m, c, lut, any_out, cost, w, [&]() -> int {
        TSL_REQUIRE(c->clearance >= 0 && c->clearance <= m->Nz, w + ": clearance must be 0 .. Nz layers");
        TSL_REQUIRE(c->free_run >= 0 && c->free_run <= c->clearance, w + ": free_run must be 0 .. clearance");
        TSL_REQUIRE(c->pick == 0 || c->pick == 1, w + ": pick must be 0 (lowest) or 1 (highest)");
        TSL_REQUIRE(c->window >= 0 && c->window <= 16, w + ": window must be 0 .. 16 cells");
        TSL_REQUIRE(c->slope_base >= 1 && c->slope_base <= 16, w + ": slope_base must be 1 .. 16 cells");
        TSL_REQUIRE(c->max_step >= 0 && c->max_step <= 65534, w + ": max_step must be 0 .. 65534 sixteenths of a voxel");
        TSL_REQUIRE(c->min_support >= 0, w + ": min_support is negative");
        return TSL_OK;
    }, [&]() -> int {
        TSL_REQUIRE(m->Nz <= 4094, w + ": the volume is too high (Nz > 4094: height would not fit int16)");
        return TSL_OK;
    }, C);
    if (rc) return rc;
    C->pick = c->pick; C->clearance = c->clearance; C->free_run = c->free_run; C->window = c->window; C->slope_base = c->slope_base;
    C->max_step = c->max_step; C->min_support = c->min_support; C->max_slope2 = c->max_slope2;
    C->R = c->radius; C->flags = c->flags; C->cost_unknown = c->cost_unknown;
    return TSL_OK;
}

#define TER_GROW(field, bytes_field, bytes) do { if ((rc = grow(&S->field, &S->bytes_field, (bytes)))) return rc; } while (0)

// the launches on q; every pointer a device pointer, null planes skipped (a plane a later stage reads goes to scratch)
static int ter_launch(tsl_tsdf* m, hipStream_t q, const TerCfg& C, const uint8_t* lut, int16_t* height, uint8_t* col, uint16_t* step, uint16_t* nsup, uint32_t* slope2,
                      uint8_t* cls, uint16_t* d2, uint8_t* cost)
{
    int rc;
    if (!m->nav_terrain) m->nav_terrain = new NavTerrainState();   // value-initialised: every pointer null, every size 0
    NavTerrainState* S = m->nav_terrain;
    const int N = m->N;
    const size_t cells = (size_t)N * N * C.B;
    const bool edt = d2 || cost;
    const bool win = step || nsup || slope2 || cls || edt;
    if (edt) {
        TER_GROW(g, b_g, cells);
        if (!cls) { TER_GROW(cls, b_cls, cells); cls = (uint8_t*)S->cls; }      // the distance pass reads the classes: they go to scratch
    }
    if (win) {
        if (!height) { TER_GROW(height, b_height, cells * 2); height = (int16_t*)S->height; }
        if (cls && !col) { TER_GROW(col, b_col, cells); col = (uint8_t*)S->col; }
    }
    prof_begin(m, TSL_K_NAV_TERRAIN_COLUMNS, q);
    hipLaunchKernelGGL(k_terrain_columns, dim3((unsigned)(m->nbx * m->nbx)), dim3(256), 0, q, m->M, C, height, col);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    if (win) {
        const unsigned tiles = (unsigned)((N + TER_TILE - 1) / TER_TILE);
        prof_begin(m, TSL_K_NAV_TERRAIN_WINDOW, q);
        hipLaunchKernelGGL(k_terrain_window, dim3(tiles, tiles, (unsigned)C.B), dim3(256), 0, q, N, C.window, C.slope_base, C.max_step, C.min_support, C.max_slope2,
                           (const int16_t*)height, (const uint8_t*)col, step, nsup, slope2, cls);
        prof_end(m, q);
        TSL_HIP(hipGetLastError());
    }
    if (edt) return nav_edt_launch(m, q, N, C.B, C.R, C.flags, C.cost_unknown, cls, (uint8_t*)S->g, lut, d2, cost);
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_nav_terrain(tsl_tsdf* m, const tsl_nav_terrain_cfg* cfg, const uint8_t* lut, int16_t* height, uint8_t* col, uint16_t* step, uint16_t* nsup,
                         uint32_t* slope2, uint8_t* cls, uint16_t* d2, uint8_t* cost)
{
    TerCfg C;
    int rc = ter_check(m, cfg, lut, height || col || step || nsup || slope2 || cls || d2 || cost, cost, &C, "nav_terrain"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames: the pass runs behind them
    const size_t cells = (size_t)m->N * m->N * C.B;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_lut = st.in(lut, (size_t)C.R * C.R + 2), i_slope = st.out(slope2, cells * 4), i_height = st.out(height, cells * 2), i_step = st.out(step, cells * 2),
              i_nsup = st.out(nsup, cells * 2), i_d2 = st.out(d2, cells * 2), i_col = st.out(col, cells), i_cls = st.out(cls, cells), i_cost = st.out(cost, cells);
    if ((rc = st.upload())) return rc;
    if ((rc = ter_launch(m, q, C, st.ptr<const uint8_t>(i_lut), st.ptr<int16_t>(i_height), st.ptr<uint8_t>(i_col), st.ptr<uint16_t>(i_step), st.ptr<uint16_t>(i_nsup),
                         st.ptr<uint32_t>(i_slope), st.ptr<uint8_t>(i_cls), st.ptr<uint16_t>(i_d2), st.ptr<uint8_t>(i_cost)))) return rc;
    return st.download();
}

int tsl_tsdf_nav_terrain_dev(tsl_tsdf* m, const tsl_nav_terrain_cfg* cfg, const void* lut_dev, void* height_dev, void* col_dev, void* step_dev, void* nsup_dev,
                             void* slope2_dev, void* cls_dev, void* d2_dev, void* cost_dev, void* user_stream)
{
    TerCfg C;
    int rc = ter_check(m, cfg, lut_dev, height_dev || col_dev || step_dev || nsup_dev || slope2_dev || cls_dev || d2_dev || cost_dev, cost_dev, &C, "nav_terrain_dev");
    if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = ter_launch(m, q, C, (const uint8_t*)lut_dev, (int16_t*)height_dev, (uint8_t*)col_dev, (uint16_t*)step_dev, (uint16_t*)nsup_dev, (uint32_t*)slope2_dev,
                         (uint8_t*)cls_dev, (uint16_t*)d2_dev, (uint8_t*)cost_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

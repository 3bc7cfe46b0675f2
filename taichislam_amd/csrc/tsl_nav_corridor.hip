// tsl_nav_corridor.hip -- safe corridors: the free axis-aligned box around a cell of a cost plane or volume, and the chain of such
// boxes along a path of nav_paths / nav_paths3d -- the overlapping convex free regions a corridor-based trajectory optimiser takes.  The volume is the
// caller's (a cost plane of nav_grid / nav_terrain, the volume of flight_volume, any u8 array); the handle supplies the device, the stream and scratch, and
// no map is read.  Everything is integer and the face order makes the box unique, so the result depends on no schedule and tests/nav_corridor_ref.py
// restates it byte for byte.
//
// Definition (include/taichislam_hip.h says the same).  cost u8 [D][H][W], layer k, row i, column j; a cell is free when it is inside and cost <
//   free_below.  The box of a seed c starts as lo = hi = c with six open faces and grows in rounds; in a round the open faces are tried in the order -j,
//   +j, -i, +i, -k, +k; a try moves the face out by one cell and succeeds when the new coordinate is within ext of c on that axis, inside the volume, and
//   every cell of the new slab -- one cell thick, spanning the box as it stands at that moment on the other two axes -- is free; a try that fails closes
//   the face for good.  A seed outside gives six times -1 and TSL_BOX_OUTSIDE, a seed that is not free lo = hi = c and TSL_BOX_BLOCKED.
//   The corridor of a path: s_0 = 0; box q is the box of cell s_q; t_q is the last cell such that s_q .. t_q all lie in it (s_q for a blocked or outside
//   seed); t_q = len - 1 ends the walk (status 0); otherwise s_q+1 = t_q when t_q > s_q, else s_q + 1; max_boxes boxes without an end give status 1.
//
//   k_nc_pack        the u8 volume -> one free bit per cell, row pitch ceil(W / 64) words: a wave reads 64 consecutive cells of a row, one 64-bit ballot
//                    of cost < free_below is the word, lane 0 stores it.  Bits past W are 0.  The volume is read once; the bit volume, D * H *
//                    ceil(W / 64) * 8 bytes, is what the inflation reads, many times over, from cache: an eighth of the volume where W is a multiple of
//                    64 (32 MB at the 2^28 cap), up to twice that for a W just above one (66 MB for W = 65 at the cap), and at worst 8 bytes per cell
//                    for W = 1 (128 MB for 4096 x 4096 x 1).
//   k_nc_boxes /     one wave per seed; the box and the six open bits are wave-uniform.  A +-k or +-i slab is a set of rows, each the bit run j0 .. j1 (at
//   k_nc_path_boxes  most 5 words): one lane per (row, word), looped in steps of the wave; a +-j slab is one bit per (k, i) of the box, one lane each,
//                    looped.  A try is decided by __all.  Bounds come from the coordinates, never from padding.  (path_boxes: the seeds are the cells of
//                    the paths, int16, and the cells past a path's length start no work.)
//   k_nc_chain       one wave per path over the per-cell boxes: 64 cells per ballot of "outside the box", the lowest set bit is the first cell outside.
// No atomics, no LDS, no workgroup waits for another, and every loop has a bound known at launch (ext, L, max_boxes).
#include <string>
#include "tsl_stage.hpp"

namespace tsl {

#define NC_MAX_DIM 4096
#define NC_MAX_CELLS (1ll << 28)
#define NC_MAX_EXT 127
#define NC_MAX_SEEDS (1 << 20)
#define NC_MAX_PATHS (1 << 16)
#define NC_MAX_LEN 4096
#define NC_MAX_PATH_CELLS (1ll << 22)

typedef unsigned long long nc_word;

struct NcCfg { int D, H, W, pitch, free_below, ek, ei, ej, Q; };

// the scratch of a handle: the bit volume and the per-cell boxes and flags of the corridor form
enum { NC_BITS, NC_CBOX, NC_CFLAG, NC_NBUF };
struct NavCorridorState { void* p[NC_NBUF]; size_t b[NC_NBUF]; };

// ---- pack ------------------------------------------------------------------------------------------------------------------------------------
// one wave per word of the bit volume
__global__ void __launch_bounds__(256) k_nc_pack(NcCfg C, const uint8_t* __restrict__ cost, nc_word* __restrict__ bits, size_t n_words)
{
    const size_t word = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= n_words) return;                                    // (uniform over the wave)
    const int lane = (int)(threadIdx.x & 63);
    const size_t row = word / (size_t)C.pitch;
    const int j = (int)(word - row * (size_t)C.pitch) * 64 + lane;
    const bool is_free = j < C.W && (int)cost[row * (size_t)C.W + j] < C.free_below;
    const nc_word b = __ballot(is_free ? 1 : 0);
    if (lane == 0) bits[word] = b;
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------------------
// the bits j0 .. j1 of a row that fall into word w (which holds at least one of them)
__device__ __forceinline__ nc_word nc_run(int j0, int j1, int w)
{
    const int lo = max(j0 - w * 64, 0), hi = min(j1 - w * 64, 63);
    return (~0ull >> (63 - hi)) & (~0ull << lo);
}

// a slab of nr rows (row0, row0 + stride, ..: indices k * H + i), each the run j0 .. j1: one lane per (row, word)
__device__ __forceinline__ bool nc_rows_free(const NcCfg& C, const nc_word* __restrict__ bits, int lane, size_t row0, size_t stride, int nr, int j0, int j1)
{
    const int w0 = j0 >> 6, nw = (j1 >> 6) - w0 + 1, n = nr * nw;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        bool ok = true;
        if (t < n) {
            const int r = t / nw, w = w0 + (t - r * nw);
            const nc_word m = nc_run(j0, j1, w);
            ok = (bits[(row0 + (size_t)r * stride) * (size_t)C.pitch + w] & m) == m;
        }
        if (!__all(ok ? 1 : 0)) return false;
    }
    return true;
}

// the slab at column nj: one bit per (k, i) of the box, one lane each
__device__ __forceinline__ bool nc_col_free(const NcCfg& C, const nc_word* __restrict__ bits, int lane, int k0, int k1, int i0, int i1, int nj)
{
    const int ni = i1 - i0 + 1, n = (k1 - k0 + 1) * ni, w = nj >> 6, sh = nj & 63;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        bool ok = true;
        if (t < n) {
            const int a = t / ni, k = k0 + a, i = i0 + (t - a * ni);
            ok = ((bits[((size_t)k * C.H + i) * (size_t)C.pitch + w] >> sh) & 1ull) != 0ull;
        }
        if (!__all(ok ? 1 : 0)) return false;
    }
    return true;
}

// the box of the seed (ck, ci, cj), which every lane of the wave passes alike: b = { k0, i0, j0, k1, i1, j1 }; returns the flag
__device__ __forceinline__ int nc_inflate(const NcCfg& C, const nc_word* __restrict__ bits, int lane, int ck, int ci, int cj, int b[6])
{
    if (!(ck >= 0 && ck < C.D && ci >= 0 && ci < C.H && cj >= 0 && cj < C.W)) {
        for (int a = 0; a < 6; ++a) b[a] = -1;
        return TSL_BOX_OUTSIDE;
    }
    int k0 = ck, k1 = ck, i0 = ci, i1 = ci, j0 = cj, j1 = cj;
    b[0] = b[3] = ck; b[1] = b[4] = ci; b[2] = b[5] = cj;
    if (((bits[((size_t)ck * C.H + ci) * (size_t)C.pitch + (cj >> 6)] >> (cj & 63)) & 1ull) == 0ull) return TSL_BOX_BLOCKED;
    // a face that is open at the start of a round moves or closes in it, and moves at most ext times: no face is open after max ext + 1 rounds
    const int rounds = max(C.ek, max(C.ei, C.ej)) + 1;
    unsigned open = 63u;
    for (int r = 0; r < rounds && open; ++r) {
        if (open & 1u) {
            const int nj = j0 - 1;
            if (cj - nj <= C.ej && nj >= 0 && nc_col_free(C, bits, lane, k0, k1, i0, i1, nj)) j0 = nj; else open &= ~1u;
        }
        if (open & 2u) {
            const int nj = j1 + 1;
            if (nj - cj <= C.ej && nj < C.W && nc_col_free(C, bits, lane, k0, k1, i0, i1, nj)) j1 = nj; else open &= ~2u;
        }
        if (open & 4u) {
            const int ni = i0 - 1;
            if (ci - ni <= C.ei && ni >= 0 && nc_rows_free(C, bits, lane, (size_t)k0 * C.H + ni, (size_t)C.H, k1 - k0 + 1, j0, j1)) i0 = ni; else open &= ~4u;
        }
        if (open & 8u) {
            const int ni = i1 + 1;
            if (ni - ci <= C.ei && ni < C.H && nc_rows_free(C, bits, lane, (size_t)k0 * C.H + ni, (size_t)C.H, k1 - k0 + 1, j0, j1)) i1 = ni; else open &= ~8u;
        }
        if (open & 16u) {
            const int nk = k0 - 1;
            if (ck - nk <= C.ek && nk >= 0 && nc_rows_free(C, bits, lane, (size_t)nk * C.H + i0, 1, i1 - i0 + 1, j0, j1)) k0 = nk; else open &= ~16u;
        }
        if (open & 32u) {
            const int nk = k1 + 1;
            if (nk - ck <= C.ek && nk < C.D && nc_rows_free(C, bits, lane, (size_t)nk * C.H + i0, 1, i1 - i0 + 1, j0, j1)) k1 = nk; else open &= ~32u;
        }
    }
    b[0] = k0; b[1] = i0; b[2] = j0; b[3] = k1; b[4] = i1; b[5] = j1;
    return 0;
}

// component `lane` of a box, without a dynamic index into registers
__device__ __forceinline__ int nc_pick(const int b[6], int lane)
{
    return lane == 0 ? b[0] : (lane == 1 ? b[1] : (lane == 2 ? b[2] : (lane == 3 ? b[3] : (lane == 4 ? b[4] : b[5]))));
}

// one wave per seed of an int32 [S][3] list
__global__ void __launch_bounds__(256) k_nc_boxes(NcCfg C, const nc_word* __restrict__ bits, const int32_t* __restrict__ cells, int n, int16_t* __restrict__ boxes,
                                                  uint8_t* __restrict__ flags)
{
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (s >= n) return;
    const int lane = (int)(threadIdx.x & 63);
    const int ck = __builtin_amdgcn_readfirstlane(cells[(size_t)s * 3]), ci = __builtin_amdgcn_readfirstlane(cells[(size_t)s * 3 + 1]),
              cj = __builtin_amdgcn_readfirstlane(cells[(size_t)s * 3 + 2]);
    int b[6];
    const int flag = nc_inflate(C, bits, lane, ck, ci, cj, b);
    if (boxes && lane < 6) boxes[(size_t)s * 6 + lane] = (int16_t)nc_pick(b, lane);
    if (flags && lane == 0) flags[s] = (uint8_t)flag;
}

// one wave per cell of the paths, int16 [P][L][3]; the cells past a path's length start no work and leave their scratch rows as they are
__global__ void __launch_bounds__(256) k_nc_path_boxes(NcCfg C, const nc_word* __restrict__ bits, const int16_t* __restrict__ cells, const int32_t* __restrict__ length,
                                                       int n, int L, int16_t* __restrict__ boxes, uint8_t* __restrict__ flags)
{
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (s >= n) return;
    const int p = s / L;
    if (s - p * L >= length[p]) return;                             // (uniform)
    const int lane = (int)(threadIdx.x & 63);
    const int ck = __builtin_amdgcn_readfirstlane((int)cells[(size_t)s * 3]), ci = __builtin_amdgcn_readfirstlane((int)cells[(size_t)s * 3 + 1]),
              cj = __builtin_amdgcn_readfirstlane((int)cells[(size_t)s * 3 + 2]);
    int b[6];
    const int flag = nc_inflate(C, bits, lane, ck, ci, cj, b);
    if (lane < 6) boxes[(size_t)s * 6 + lane] = (int16_t)nc_pick(b, lane);
    if (lane == 0) flags[s] = (uint8_t)flag;
}

// ---- chain -----------------------------------------------------------------------------------------------------------------------------------
// one wave per path.  Rows past `count`: boxes and seed -1, link 255.
__global__ void __launch_bounds__(256) k_nc_chain(NcCfg C, const int16_t* __restrict__ cells, const int32_t* __restrict__ length, int P, int L,
                                                  const int16_t* __restrict__ cbox, const uint8_t* __restrict__ cflag, int16_t* __restrict__ boxes,
                                                  int32_t* __restrict__ seed, uint8_t* __restrict__ link, int32_t* __restrict__ count, uint8_t* __restrict__ status)
{
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (p >= P) return;
    const int lane = (int)(threadIdx.x & 63), Q = C.Q;
    int len = length[p];
    if (len > L) len = L;
    const int16_t* pc = cells + (size_t)p * L * 3;
    const int16_t* pb = cbox + (size_t)p * L * 6;
    const uint8_t* pf = cflag + (size_t)p * L;
    int q = 0, st = 2;
    if (len > 0) {
        st = 1;
        int s = 0, prev[6] = { 0, 0, 0, 0, 0, 0 }, pflag = 0;
        while (q < Q) {
            int b[6];
            for (int a = 0; a < 6; ++a) b[a] = pb[(size_t)s * 6 + a];
            const int f = pf[s];
            int lk = 0;
            if (q > 0) {                                            // a box of a seed outside the volume has no cells
                const bool meet = f != TSL_BOX_OUTSIDE && pflag != TSL_BOX_OUTSIDE && max(b[0], prev[0]) <= min(b[3], prev[3]) &&
                                  max(b[1], prev[1]) <= min(b[4], prev[4]) && max(b[2], prev[2]) <= min(b[5], prev[5]);
                lk = meet ? 1 : 2;
            }
            if (f) lk += 4;
            const size_t row = (size_t)p * Q + q;
            if (boxes && lane < 6) boxes[row * 6 + lane] = (int16_t)nc_pick(b, lane);
            if (lane == 0) {
                if (seed) seed[row] = s;
                if (link) link[row] = (uint8_t)lk;
            }
            ++q;
            int t = s;
            if (f == 0) {
                t = len - 1;
                for (int base = s + 1; base < len; base += 64) {    // the first cell after s that is outside the box
                    const int x = base + lane;
                    bool out = false;
                    if (x < len) {
                        const int k = pc[(size_t)x * 3], i = pc[(size_t)x * 3 + 1], j = pc[(size_t)x * 3 + 2];
                        out = !(k >= b[0] && k <= b[3] && i >= b[1] && i <= b[4] && j >= b[2] && j <= b[5]);
                    }
                    const nc_word m = __ballot(out ? 1 : 0);
                    if (m) { t = base + (__ffsll((long long)m) - 1) - 1; break; }
                }
            }
            if (t == len - 1) { st = 0; break; }
            s = t > s ? t : s + 1;
            for (int a = 0; a < 6; ++a) prev[a] = b[a];
            pflag = f;
        }
    }
    if (boxes) for (int x = q * 6 + lane; x < Q * 6; x += 64) boxes[(size_t)p * Q * 6 + x] = (int16_t)-1;
    for (int x = q + lane; x < Q; x += 64) {
        if (seed) seed[(size_t)p * Q + x] = -1;
        if (link) link[(size_t)p * Q + x] = (uint8_t)255;
    }
    if (lane == 0) {
        if (count) count[p] = q;
        if (status) status[p] = (uint8_t)st;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
void nav_corridor_release(tsl_tsdf* m)
{
    NavCorridorState* S = m->nav_corridor;
    if (!S) return;
    for (void* p : S->p) if (p) (void)hipFree(p);
    delete S;
    m->nav_corridor = nullptr;
}

static int nc_state(tsl_tsdf* m)
{
    if (!m->nav_corridor) m->nav_corridor = new NavCorridorState();     // value-initialised: every pointer null, every size 0
    return TSL_OK;
}

#define NC_GROW(which, bytes) do { if ((rc = grow(&S->p[which], &S->b[which], (bytes)))) return rc; } while (0)

// the refusals every entry point shares (max_boxes is read by the corridor forms only, against L)
static int nc_check(tsl_tsdf* m, const tsl_nav_corridor_cfg* c, const void* cost, NcCfg* C, const std::string& w)
{
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(cost, w + ": null cost");
    TSL_REQUIRE(c->D >= 1 && c->D <= NC_MAX_DIM, w + ": D must be 1 .. 4096");
    TSL_REQUIRE(c->H >= 1 && c->H <= NC_MAX_DIM, w + ": H must be 1 .. 4096");
    TSL_REQUIRE(c->W >= 1 && c->W <= NC_MAX_DIM, w + ": W must be 1 .. 4096");
    TSL_REQUIRE((long long)c->D * c->H * c->W <= NC_MAX_CELLS, w + ": D * H * W is above 2^28 cells");
    TSL_REQUIRE(c->free_below >= 1 && c->free_below <= 255, w + ": free_below must be 1 .. 255");
    TSL_REQUIRE(c->ext_k >= 0 && c->ext_k <= NC_MAX_EXT, w + ": ext_k must be 0 .. 127");
    TSL_REQUIRE(c->ext_i >= 0 && c->ext_i <= NC_MAX_EXT, w + ": ext_i must be 0 .. 127");
    TSL_REQUIRE(c->ext_j >= 0 && c->ext_j <= NC_MAX_EXT, w + ": ext_j must be 0 .. 127");
    C->D = c->D; C->H = c->H; C->W = c->W; C->pitch = (c->W + 63) / 64; C->free_below = c->free_below;
    C->ek = c->ext_k; C->ei = c->ext_i; C->ej = c->ext_j; C->Q = c->max_boxes;
    return TSL_OK;
}

static int nc_check_boxes(tsl_tsdf* m, const tsl_nav_corridor_cfg* c, const void* cost, const void* cells, int n, NcCfg* C, const std::string& w)
{
    int rc = nc_check(m, c, cost, C, w); if (rc) return rc;
    TSL_REQUIRE(n >= 0 && n <= NC_MAX_SEEDS, w + ": S must be 0 .. 2^20 cells");
    TSL_REQUIRE(cells || n == 0, w + ": null cells while S > 0");
    return TSL_OK;
}

static int nc_check_corridor(tsl_tsdf* m, const tsl_nav_corridor_cfg* c, const void* cost, const void* cells, const void* length, int P, int L, NcCfg* C,
                             const std::string& w)
{
    int rc = nc_check(m, c, cost, C, w); if (rc) return rc;
    TSL_REQUIRE(P >= 0 && P <= NC_MAX_PATHS, w + ": P must be 0 .. 2^16 paths");
    TSL_REQUIRE(L >= 1 && L <= NC_MAX_LEN, w + ": L must be 1 .. 4096");
    TSL_REQUIRE((long long)P * L <= NC_MAX_PATH_CELLS, w + ": P * L is above 2^22 cells");
    TSL_REQUIRE(c->max_boxes >= 1 && c->max_boxes <= L, w + ": max_boxes must be 1 .. L");
    TSL_REQUIRE(cells || P == 0, w + ": null cells while P > 0");
    TSL_REQUIRE(length || P == 0, w + ": null length while P > 0");
    return TSL_OK;
}

static size_t nc_words(const NcCfg& C) { return (size_t)C.D * C.H * C.pitch; }

// the bit volume of `cost`, into the handle's scratch
static int nc_pack(tsl_tsdf* m, hipStream_t q, const NcCfg& C, const uint8_t* cost)
{
    int rc;
    NavCorridorState* S = m->nav_corridor;
    const size_t words = nc_words(C);
    NC_GROW(NC_BITS, words * sizeof(nc_word));
    hipLaunchKernelGGL(k_nc_pack, dim3((unsigned)((words + 3) / 4)), dim3(256), 0, q, C, cost, (nc_word*)S->p[NC_BITS], words);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// everything on q, every pointer a device pointer.  (A call that has to grow the scratch frees and allocates device memory, which waits for the device:
// the first call and any call larger than those before it, in the _dev forms too, as in tsl_nav_field3.hip.)
static int nc_boxes_launch(tsl_tsdf* m, hipStream_t q, const NcCfg& C, const uint8_t* cost, const int32_t* cells, int n, int16_t* boxes, uint8_t* flags)
{
    int rc = nc_pack(m, q, C, cost); if (rc) return rc;
    hipLaunchKernelGGL(k_nc_boxes, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, q, C, (const nc_word*)m->nav_corridor->p[NC_BITS], cells, n, boxes, flags);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

static int nc_corridor_launch(tsl_tsdf* m, hipStream_t q, const NcCfg& C, const uint8_t* cost, const int16_t* cells, const int32_t* length, int P, int L,
                              int16_t* boxes, int32_t* seed, uint8_t* link, int32_t* count, uint8_t* status)
{
    int rc;
    NavCorridorState* S = m->nav_corridor;
    const size_t n = (size_t)P * L;
    NC_GROW(NC_CBOX, n * 6 * sizeof(int16_t));
    NC_GROW(NC_CFLAG, n);
    if ((rc = nc_pack(m, q, C, cost))) return rc;
    hipLaunchKernelGGL(k_nc_path_boxes, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, q, C, (const nc_word*)S->p[NC_BITS], cells, length, (int)n, L,
                       (int16_t*)S->p[NC_CBOX], (uint8_t*)S->p[NC_CFLAG]);
    TSL_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nc_chain, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, q, C, cells, length, P, L, (const int16_t*)S->p[NC_CBOX],
                       (const uint8_t*)S->p[NC_CFLAG], boxes, seed, link, count, status);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_nav_boxes(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const uint8_t* cost, const int32_t* cells, int32_t n, int16_t* boxes, uint8_t* flags)
{
    NcCfg C;
    int rc = nc_check_boxes(m, cfg, cost, cells, n, &C, "nav_boxes"); if (rc) return rc;
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nc_state(m))) return rc;
    const size_t N = (size_t)n;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_cost = st.in(cost, (size_t)C.D * C.H * C.W), i_cells = st.in(cells, N * 3 * sizeof(int32_t)), i_boxes = st.out(boxes, N * 6 * sizeof(int16_t)),
              i_flags = st.out(flags, N);
    if ((rc = st.upload())) return rc;
    if ((rc = nc_boxes_launch(m, q, C, st.ptr<const uint8_t>(i_cost), st.ptr<const int32_t>(i_cells), n, st.ptr<int16_t>(i_boxes), st.ptr<uint8_t>(i_flags)))) return rc;
    return st.download();
}

int tsl_tsdf_nav_boxes_dev(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const void* cost_dev, const void* cells_dev, int32_t n, void* boxes_dev, void* flags_dev,
                           void* user_stream)
{
    NcCfg C;
    int rc = nc_check_boxes(m, cfg, cost_dev, cells_dev, n, &C, "nav_boxes_dev"); if (rc) return rc;
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nc_state(m))) return rc;
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nc_boxes_launch(m, q, C, (const uint8_t*)cost_dev, (const int32_t*)cells_dev, n, (int16_t*)boxes_dev, (uint8_t*)flags_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_tsdf_nav_corridor(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const uint8_t* cost, const int16_t* cells, const int32_t* length, int32_t P, int32_t L,
                          int16_t* boxes, int32_t* seed, uint8_t* link, int32_t* count, uint8_t* status)
{
    NcCfg C;
    int rc = nc_check_corridor(m, cfg, cost, cells, length, P, L, &C, "nav_corridor"); if (rc) return rc;
    if (P == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nc_state(m))) return rc;
    const size_t np = (size_t)P, nq = np * C.Q;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_cost = st.in(cost, (size_t)C.D * C.H * C.W), i_cells = st.in(cells, np * L * 3 * sizeof(int16_t)), i_len = st.in(length, np * sizeof(int32_t)),
              i_boxes = st.out(boxes, nq * 6 * sizeof(int16_t)), i_seed = st.out(seed, nq * sizeof(int32_t)), i_link = st.out(link, nq),
              i_count = st.out(count, np * sizeof(int32_t)), i_status = st.out(status, np);
    if ((rc = st.upload())) return rc;
    if ((rc = nc_corridor_launch(m, q, C, st.ptr<const uint8_t>(i_cost), st.ptr<const int16_t>(i_cells), st.ptr<const int32_t>(i_len), P, L, st.ptr<int16_t>(i_boxes),
                                 st.ptr<int32_t>(i_seed), st.ptr<uint8_t>(i_link), st.ptr<int32_t>(i_count), st.ptr<uint8_t>(i_status)))) return rc;
    return st.download();
}

int tsl_tsdf_nav_corridor_dev(tsl_tsdf* m, const tsl_nav_corridor_cfg* cfg, const void* cost_dev, const void* cells_dev, const void* length_dev, int32_t P, int32_t L,
                              void* boxes_dev, void* seed_dev, void* link_dev, void* count_dev, void* status_dev, void* user_stream)
{
    NcCfg C;
    int rc = nc_check_corridor(m, cfg, cost_dev, cells_dev, length_dev, P, L, &C, "nav_corridor_dev"); if (rc) return rc;
    if (P == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = nc_state(m))) return rc;
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = nc_corridor_launch(m, q, C, (const uint8_t*)cost_dev, (const int16_t*)cells_dev, (const int32_t*)length_dev, P, L, (int16_t*)boxes_dev,
                                 (int32_t*)seed_dev, (uint8_t*)link_dev, (int32_t*)count_dev, (uint8_t*)status_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

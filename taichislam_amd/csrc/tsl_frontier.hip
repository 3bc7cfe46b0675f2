// tsl_frontier.hip -- exploration frontiers of the TSDF: the free voxels that border unobserved space, grouped into connected clusters
// (DESIGN.md section 4.11).  The reference answers "where does the known map end" per facelet inside its topology graph (topo_graph.py, out of
// scope: serial and scipy-bound); this is the read-only map pass behind it, defined by the project.  Everything is integer except the one f32
// comparison of q_occupied (tsl_query.hip), so the result depends on no schedule and tests/frontier_ref.py restates it bit for bit.
//
//   mark       one workgroup per allocated brick of the slot: 18^3 class codes (brick + halo, through the 26 neighbour bricks) in LDS, the 4096
//              voxels evaluated, bitmap + masks written for the bricks that hold a frontier voxel (the others drop out here)
//   label      per frontier brick: union-find over its voxels in LDS (roots are the smaller index), every voxel left pointing at its local root
//   join       unions across brick faces, edges and corners: compare-and-swap on the root words, every read an agent-scope atomic load
//   flatten    every voxel pointed at its global root
//   summarise  roots numbered; per-cluster integer sums, bounding box and least key, reduced in the wave before any global atomic
//   emit       min_cluster filter, clusters and voxels sorted by key (rocPRIM), records and rows written
// No workgroup waits for another inside a launch; every loop is capped and a cap that is reached comes back as an error.
#include "tsl_tsdf.hpp"
#include <rocprim/rocprim.hpp>
#include <cmath>

namespace tsl {

#define FR_T 18
#define FR_T3 (FR_T * FR_T * FR_T)
enum { FR_OUT = 0, FR_UNKNOWN = 1, FR_FREE = 2, FR_OCC = 3 };          // class codes; FR_OUT: outside the volume (no class)
enum { FRC_BRICKS = 0, FRC_VOXELS = 1, FRC_ROOTS = 2, FRC_KEPT = 3, FRC_KEPT_VOXELS = 4, FRC_ERR = 5, FRC_CURSOR = 6, FRC_N = 8 };      // counter words
enum { FRE_LABEL = 1, FRE_JOIN = 2, FRE_FLATTEN = 4, FRE_HASH = 8 };                                                                     // error bits
// Caps.  A parent chain holds every node at most once, so a find takes at most as many steps as there are nodes: 4096 in a brick, frontier
// bricks * 4096 across bricks; a retry of a union follows another thread's successful union, of which there are fewer than nodes.  The caps are
// those true bounds (+ 1): they cannot be reached by any map, only by a corrupted parent array, and then the launch ends instead of spinning.

struct FrCfg { int s; float thres; int min_unknown, conn, min_cluster, flags, k_min, k_max; };
struct FrAcc { int key, count; long long sum[3]; int nsum[3], lo[3], hi[3], pad_; };      // per-root accumulator
struct FrDev {
    int* ctr;                    // [FRC_N]
    int cap_fb;                  // frontier bricks the arrays below hold
    int *fb_brick;               // [cap_fb] brick id inside the submap
    int *hkey, *hval; int hmask; // brick id -> frontier brick (open addressing, >= 2 slots per frontier brick)
    uint32_t* bits;              // [cap_fb][128] frontier bitmap of the brick
    uint8_t* mask;               // [cap_fb][4096] unknown-face masks
    int* lab;                    // [cap_fb][4096] parent (node = frontier brick * 4096 + voxel), -1 no frontier voxel; roots end as -2 - slot
    FrAcc* acc;                  // [frontier voxels] one per root
    uint32_t *ckey, *ckey_s; int *cval, *cval_s, *row;      // cluster sort (key or ~0 when dropped, slot) and slot -> row
    uint32_t *vkey, *vkey_s; unsigned long long *vval, *vval_s;      // voxel sort (key, row << 8 | mask)
    int16_t* o_idx; uint8_t* o_mask; int* o_cluster; tsl_frontier_cluster* o_clusters;      // the result
};

struct FrontierState {
    FrDev D; size_t b_ctr, b_brick, b_hkey, b_hval, b_bits, b_mask, b_lab, b_acc, b_ckey, b_ckey_s, b_cval, b_cval_s, b_row, b_vkey, b_vkey_s, b_vval, b_vval_s,
          b_idx, b_omask, b_ocl, b_ocls, b_temp;
    void* temp; int n_voxels, n_clusters; bool valid;
};

// the 13 neighbour offsets that are lexicographically positive: every unordered pair of neighbours is looked at once, from its smaller voxel
__device__ __forceinline__ void fr_dir(int d, int* dx, int* dy, int* dz)
{
    if (d < 9) { *dx = 1; *dy = d / 3 - 1; *dz = d % 3 - 1; }
    else if (d < 12) { *dx = 0; *dy = 1; *dz = d - 10; }
    else { *dx = 0; *dy = 0; *dz = 1; }
}
__device__ __forceinline__ bool fr_dir_ok(int conn, int dx, int dy, int dz) { return abs(dx) + abs(dy) + abs(dz) <= (conn == 6 ? 1 : conn == 18 ? 2 : 3); }
__device__ __forceinline__ int fr_tile(int x, int y, int z) { return (x * FR_T + y) * FR_T + z; }      // tile coords = brick coords + 1
__device__ __forceinline__ uint32_t fr_hash(int b, int mask) { return ((uint32_t)b * 0x9E3779B1u >> 7) & (uint32_t)mask; }

__device__ __forceinline__ int fr_lookup(const FrDev& D, int b)
{
    uint32_t h = fr_hash(b, D.hmask);
    for (int it = 0; it <= D.hmask; ++it) {
        const int k = D.hkey[h];                      // (written by the mark launch, read by later launches)
        if (k == b) return D.hval[h];
        if (k == -1) return -1;
        h = (h + 1) & (uint32_t)D.hmask;
    }
    return -1;
}

// ---- mark ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fr_mark(MapDev M, FrCfg C, FrDev D)
{
    __shared__ uint8_t s_c[FR_T3];
    __shared__ uint32_t s_bits[128];
    __shared__ int s_nb[27], s_wc[4], s_fb;
    const int nused = min(M.pool_top[0], M.max_bricks);      // the bricks in use, read here: the host does not wait for the count
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    for (int p = blockIdx.x; p < nused; p += gridDim.x) {
        const int owner = M.owner[p];
        const int s = owner / M.nb3, b = owner - s * M.nb3;
        if (s != C.s) continue;                                                  // (uniform) a brick of another submap
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        __syncthreads();                                                         // the previous brick's tile is no longer read
        if (threadIdx.x < 27) {
            const int i = bi + (int)threadIdx.x / 9 - 1, j = bj + ((int)threadIdx.x / 3) % 3 - 1, k = bk + (int)threadIdx.x % 3 - 1;
            s_nb[threadIdx.x] = (i < 0 || i >= M.nbx || j < 0 || j >= M.nbx || k < 0 || k >= M.nbz) ? -2 : pool_lookup_ro(M, s, (i * M.nbx + j) * M.nbz + k);
        }
        __syncthreads();
        for (int t = threadIdx.x; t < FR_T3; t += 256) {
            const int tz = t % FR_T, ty = (t / FR_T) % FR_T, tx = t / (FR_T * FR_T);
            const int np = s_nb[(((tx + 15) >> 4) * 3 + ((ty + 15) >> 4)) * 3 + ((tz + 15) >> 4)];
            int code = FR_UNKNOWN;                                               // an absent brick inside the volume
            if (np == -2 || !in_volume(M, bi * 16 + tx - 1 - M.hN, bj * 16 + ty - 1 - M.hN, bk * 16 + tz - 1 - M.hNz)) code = FR_OUT;
            else if (np >= 0) {
                const size_t v = (size_t)np * TSL_BRK3 + ((((tx + 15) & 15) << 8) | (((ty + 15) & 15) << 4) | ((tz + 15) & 15));
                if (M.obs[v] > 0) code = h2f((h16)(M.tw[v] & 0xffffu)) < C.thres ? FR_OCC : FR_FREE;      // the test of q_occupied
            }
            s_c[t] = (uint8_t)code;
        }
        __syncthreads();
        uint8_t mk[16];
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int lx = q, ly = (int)threadIdx.x >> 4, lz = (int)threadIdx.x & 15;
            const int t0 = fr_tile(lx + 1, ly + 1, lz + 1);
            int m6 = 0; bool fr = false;
            if (s_c[t0] == FR_FREE) {
                m6 = (s_c[t0 - FR_T * FR_T] == FR_UNKNOWN ? 1 : 0) | (s_c[t0 + FR_T * FR_T] == FR_UNKNOWN ? 2 : 0) | (s_c[t0 - FR_T] == FR_UNKNOWN ? 4 : 0) |
                     (s_c[t0 + FR_T] == FR_UNKNOWN ? 8 : 0) | (s_c[t0 - 1] == FR_UNKNOWN ? 16 : 0) | (s_c[t0 + 1] == FR_UNKNOWN ? 32 : 0);
                fr = __popc(m6) >= C.min_unknown;
                if (fr && (C.flags & 1)) {
                    for (int a = -1; a <= 1; ++a) for (int e = -1; e <= 1; ++e) for (int c = -1; c <= 1; ++c)
                        if (s_c[t0 + (a * FR_T + e) * FR_T + c] == FR_OCC) fr = false;
                }
                const int k = bk * 16 + lz - M.hNz;
                if (C.k_min <= C.k_max && (k < C.k_min || k > C.k_max)) fr = false;
            }
            mk[q] = fr ? (uint8_t)m6 : (uint8_t)0;
            const unsigned long long bal = __ballot(fr);
            if (lane == 0) { s_bits[q * 8 + wid * 2] = (uint32_t)bal; s_bits[q * 8 + wid * 2 + 1] = (uint32_t)(bal >> 32); }
            cnt += popc64(bal);
        }
        if (lane == 0) s_wc[wid] = cnt;
        __syncthreads();
        const int total = s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
        if (total == 0) continue;                                                // (uniform) most bricks: nothing after this step sees them
        if (threadIdx.x == 0) {
            const int fb = __hip_atomic_fetch_add(&D.ctr[FRC_BRICKS], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&D.ctr[FRC_VOXELS], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_fb = fb;
            if (fb < D.cap_fb) {                                                 // (beyond: only counted -- the host grows the arrays and marks again)
                D.fb_brick[fb] = b;
                uint32_t h = fr_hash(b, D.hmask); bool done = false;
                for (int it = 0; it <= D.hmask && !done; ++it) {
                    if (atomicCAS(&D.hkey[h], -1, b) == -1) { D.hval[h] = fb; done = true; }
                    h = (h + 1) & (uint32_t)D.hmask;
                }
                if (!done) atomicOr(&D.ctr[FRC_ERR], FRE_HASH);
            }
        }
        __syncthreads();
        const int fb = s_fb;
        if (fb >= D.cap_fb) continue;
        if (threadIdx.x < 128) D.bits[(size_t)fb * 128 + threadIdx.x] = s_bits[threadIdx.x];
#pragma unroll
        for (int q = 0; q < 16; ++q) D.mask[(size_t)fb * TSL_BRK3 + q * 256 + threadIdx.x] = mk[q];
    }
}

// ---- label: union-find in LDS ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fr_ld_s(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// root of x with path halving: a non-root only ever moves to an ancestor, roots change by compare-and-swap alone
__device__ __forceinline__ int fr_find_s(int* par, int x, bool* fail)
{
    for (int it = 0; it < TSL_BRK3 + 1; ++it) {
        const int p = fr_ld_s(par + x);
        if (p == x) return x;
        const int g = fr_ld_s(par + p);
        if (g != p) __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        x = g;
    }
    *fail = true;
    return x;
}
__device__ __forceinline__ void fr_union_s(int* par, int a, int b, bool* fail)
{
    for (int it = 0; it < TSL_BRK3 + 1; ++it) {
        a = fr_find_s(par, a, fail); b = fr_find_s(par, b, fail);
        if (a == b || *fail) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(par + hi, hi, lo);
        if (old == hi) return;
        a = old; b = lo;                                                          // hi was joined elsewhere in the meantime: go on from there
    }
    *fail = true;
}

__global__ void __launch_bounds__(256) k_fr_label(FrCfg C, FrDev D)
{
    __shared__ int s_par[TSL_BRK3];
    __shared__ uint32_t s_bits[128];
    const int nfb = min(D.ctr[FRC_BRICKS], D.cap_fb);
    bool fail = false;
    for (int fb = blockIdx.x; fb < nfb; fb += gridDim.x) {
        __syncthreads();
        if (threadIdx.x < 128) s_bits[threadIdx.x] = D.bits[(size_t)fb * 128 + threadIdx.x];
        __syncthreads();
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) s_par[l] = ((s_bits[l >> 5] >> (l & 31)) & 1u) ? l : -1;
        __syncthreads();
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            if (!((s_bits[l >> 5] >> (l & 31)) & 1u)) continue;
            const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
            for (int d = 0; d < 13; ++d) {
                int dx, dy, dz; fr_dir(d, &dx, &dy, &dz);
                if (!fr_dir_ok(C.conn, dx, dy, dz)) continue;
                const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
                if (nx > 15 || ny < 0 || ny > 15 || nz < 0 || nz > 15) continue;                  // across the brick's boundary: k_fr_join
                const int n = (nx << 8) | (ny << 4) | nz;
                if ((s_bits[n >> 5] >> (n & 31)) & 1u) fr_union_s(s_par, l, n, &fail);
            }
        }
        __syncthreads();
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            const bool f = (s_bits[l >> 5] >> (l & 31)) & 1u;
            D.lab[(size_t)fb * TSL_BRK3 + l] = f ? fb * TSL_BRK3 + fr_find_s(s_par, l, &fail) : -1;
        }
    }
    if (fail) atomicOr(&D.ctr[FRC_ERR], FRE_LABEL);
}

// ---- join: lock-free union-find over the local roots, across bricks --------------------------------------------------------------------
__device__ __forceinline__ int fr_ld_g(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// root of x with path halving, for the join launch alone: while unions are going on any ancestor is as good a parent as another
__device__ __forceinline__ int fr_find_g(int* lab, int x, int cap, bool* fail)
{
    for (int it = 0; it < cap; ++it) {
        const int p = fr_ld_g(lab + x);
        if (p == x) return x;
        const int g = fr_ld_g(lab + p);
        if (g != p) __hip_atomic_store(lab + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    *fail = true;
    return x;
}
// root of x, nothing written: for the flatten launch, whose only stores are each voxel's own final root (a halving store of another thread could
// land behind that store and leave the voxel pointing at a mere ancestor)
__device__ __forceinline__ int fr_root_g(int* lab, int x, int cap, bool* fail)
{
    for (int it = 0; it < cap; ++it) {
        const int p = fr_ld_g(lab + x);
        if (p == x) return x;
        x = p;
    }
    *fail = true;
    return x;
}
__device__ __forceinline__ void fr_union_g(int* lab, int a, int b, int cap, bool* fail)
{
    for (int it = 0; it < cap; ++it) {
        a = fr_find_g(lab, a, cap, fail); b = fr_find_g(lab, b, cap, fail);
        if (a == b || *fail) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(lab + hi, hi, lo);
        if (old == hi) return;
        a = old; b = lo;
    }
    *fail = true;
}

__global__ void __launch_bounds__(256) k_fr_join(MapDev M, FrCfg C, FrDev D)
{
    __shared__ int s_nfb[27];
    const int nfb = min(D.ctr[FRC_BRICKS], D.cap_fb), cap = nfb * TSL_BRK3 + 1;      // (fewer than 2^19 bricks in a volume of fewer than 2^31 voxels)
    bool fail = false;
    for (int fb = blockIdx.x; fb < nfb; fb += gridDim.x) {
        const int b = D.fb_brick[fb];
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        __syncthreads();
        if (threadIdx.x < 27) {
            const int i = bi + (int)threadIdx.x / 9 - 1, j = bj + ((int)threadIdx.x / 3) % 3 - 1, k = bk + (int)threadIdx.x % 3 - 1;
            s_nfb[threadIdx.x] = (i < 0 || i >= M.nbx || j < 0 || j >= M.nbx || k < 0 || k >= M.nbz) ? -1 : fr_lookup(D, (i * M.nbx + j) * M.nbz + k);
        }
        __syncthreads();
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
            if (lx != 15 && ly != 0 && ly != 15 && lz != 0 && lz != 15) continue;                  // (lx == 0 reaches no brick in a positive direction)
            if (!((D.bits[(size_t)fb * 128 + (l >> 5)] >> (l & 31)) & 1u)) continue;
            for (int d = 0; d < 13; ++d) {
                int dx, dy, dz; fr_dir(d, &dx, &dy, &dz);
                if (!fr_dir_ok(C.conn, dx, dy, dz)) continue;
                const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
                const int ox = nx >> 4, oy = ny >> 4, oz = nz >> 4;                                 // -1, 0, 1: the brick the neighbour lies in
                if (ox == 0 && oy == 0 && oz == 0) continue;                                        // inside: k_fr_label
                const int fb2 = s_nfb[((ox + 1) * 3 + (oy + 1)) * 3 + (oz + 1)];
                if (fb2 < 0) continue;
                const int n = ((nx & 15) << 8) | ((ny & 15) << 4) | (nz & 15);
                if ((D.bits[(size_t)fb2 * 128 + (n >> 5)] >> (n & 31)) & 1u) fr_union_g(D.lab, fb * TSL_BRK3 + l, fb2 * TSL_BRK3 + n, cap, &fail);
            }
        }
    }
    if (fail) atomicOr(&D.ctr[FRC_ERR], FRE_JOIN);
}

__global__ void __launch_bounds__(256) k_fr_flatten(FrDev D)
{
    const int nfb = min(D.ctr[FRC_BRICKS], D.cap_fb), cap = nfb * TSL_BRK3 + 1;
    bool fail = false;
    for (int fb = blockIdx.x; fb < nfb; fb += gridDim.x)
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            if (!((D.bits[(size_t)fb * 128 + (l >> 5)] >> (l & 31)) & 1u)) continue;
            const int x = fb * TSL_BRK3 + l;
            const int r = fr_root_g(D.lab, x, cap, &fail);      // roots do not change in this launch; a voxel another thread has already flattened reads as one step
            if (r != x) __hip_atomic_store(D.lab + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    if (fail) atomicOr(&D.ctr[FRC_ERR], FRE_FLATTEN);
}

// ---- summarise -------------------------------------------------------------------------------------------------------------------------
// every root takes a slot of the accumulator table and leaves -2 - slot in its own word
__global__ void __launch_bounds__(256) k_fr_roots(FrDev D)
{
    const int nfb = min(D.ctr[FRC_BRICKS], D.cap_fb);
    for (int fb = blockIdx.x; fb < nfb; fb += gridDim.x)
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            const int x = fb * TSL_BRK3 + l;
            const bool root = ((D.bits[(size_t)fb * 128 + (l >> 5)] >> (l & 31)) & 1u) && D.lab[x] == x;
            const int slot = wave_reserve(&D.ctr[FRC_ROOTS], root);
            if (root) {
                FrAcc a; a.key = 0x7fffffff; a.count = 0; a.pad_ = 0;
                for (int c = 0; c < 3; ++c) { a.sum[c] = 0; a.nsum[c] = 0; a.lo[c] = 0x7fffffff; a.hi[c] = -0x7fffffff - 1; }
                D.acc[slot] = a;
                D.lab[x] = -2 - slot;
            }
        }
}

// accumulator slot of frontier voxel x behind k_fr_flatten / k_fr_roots: x is a root (-2 - slot) or points at one.  Anything else (-1: never for a
// frontier voxel) is reported and the voxel left out, so that no index derived from it is used
__device__ __forceinline__ int fr_slot(const FrDev& D, int x)
{
    int r = D.lab[x];
    if (r >= 0) r = D.lab[r];
    if (r > -2) { atomicOr(&D.ctr[FRC_ERR], FRE_FLATTEN); return -1; }
    return -2 - r;
}
__device__ __forceinline__ int wave_sum_i(int v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d); return v; }
__device__ __forceinline__ int wave_min_i(int v) { for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d)); return v; }
__device__ __forceinline__ int wave_max_i(int v) { for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d)); return v; }

__global__ void __launch_bounds__(256) k_fr_sum(MapDev M, FrDev D)
{
    const int nfb = min(D.ctr[FRC_BRICKS], D.cap_fb);
    const int lane = lane_id();
    for (int fb = blockIdx.x; fb < nfb; fb += gridDim.x) {
        const int b = D.fb_brick[fb];
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            bool f = (D.bits[(size_t)fb * 128 + (l >> 5)] >> (l & 31)) & 1u;
            if (!__ballot(f)) continue;                                                             // (wave-uniform)
            const int ui = bi * 16 + (l >> 8), uj = bj * 16 + ((l >> 4) & 15), uk = bk * 16 + (l & 15);
            const int c3[3] = { ui - M.hN, uj - M.hN, uk - M.hNz };
            const int key = (ui * M.N + uj) * M.Nz + uk;
            const int slot = f ? fr_slot(D, fb * TSL_BRK3 + l) : -1;
            f = f && slot >= 0;
            unsigned long long todo = __ballot(f);
            const int m6 = f ? D.mask[(size_t)fb * TSL_BRK3 + l] : 0;
            // the lanes of one cluster are reduced together, one set of atomics per cluster and wave (a wave of 64 neighbouring voxels meets few clusters)
            while (todo) {
                const int leader = (int)__builtin_ctzll(todo);
                const int ls = __shfl(slot, leader);
                const bool mine = f && slot == ls;
                todo &= ~__ballot(mine);
                const int n = wave_sum_i(mine ? 1 : 0), kmin = wave_min_i(mine ? key : 0x7fffffff);
                int sm[3], ns[3], lo[3], hi[3];
                for (int c = 0; c < 3; ++c) {
                    sm[c] = wave_sum_i(mine ? c3[c] : 0);                                           // |index| < 2^15, 64 lanes: no overflow
                    ns[c] = wave_sum_i(mine ? ((m6 >> (2 * c + 1)) & 1) - ((m6 >> (2 * c)) & 1) : 0);
                    lo[c] = wave_min_i(mine ? c3[c] : 0x7fffffff); hi[c] = wave_max_i(mine ? c3[c] : -0x7fffffff - 1);
                }
                if (lane == leader) {
                    FrAcc* a = D.acc + ls;
                    atomicMin(&a->key, kmin); atomicAdd(&a->count, n);
                    for (int c = 0; c < 3; ++c) {
                        atomic_add_i64((int64_t*)&a->sum[c], (long long)sm[c]);
                        if (ns[c]) atomicAdd(&a->nsum[c], ns[c]);
                        atomicMin(&a->lo[c], lo[c]); atomicMax(&a->hi[c], hi[c]);
                    }
                }
            }
        }
    }
}

// min_cluster: the sort key of a dropped cluster is ~0 (every real key is below 2^31), kept clusters and their voxels are counted
__global__ void __launch_bounds__(256) k_fr_filter(FrCfg C, FrDev D)
{
    const int ncl = D.ctr[FRC_ROOTS];
    for (int sl0 = blockIdx.x * 256; sl0 < ncl; sl0 += gridDim.x * 256) {
        const int sl = sl0 + threadIdx.x;
        const bool in = sl < ncl;
        const int cnt = in ? D.acc[sl].count : 0;
        const bool kept = in && cnt >= C.min_cluster;
        if (in) { D.ckey[sl] = kept ? (uint32_t)D.acc[sl].key : 0xffffffffu; D.cval[sl] = sl; }
        const unsigned long long bal = __ballot(kept);
        const int tot = wave_sum_i(kept ? cnt : 0);
        if (bal && lane_id() == 0) {
            __hip_atomic_fetch_add(&D.ctr[FRC_KEPT], popc64(bal), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&D.ctr[FRC_KEPT_VOXELS], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fr_clusters(FrDev D, int ncl, int nkept)
{
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= ncl) return;
    const int sl = D.cval_s[pos];
    D.row[sl] = pos < nkept ? pos : -1;
    if (pos >= nkept) return;
    const FrAcc a = D.acc[sl];
    tsl_frontier_cluster r;
    r.key = a.key; r.count = a.count; r.reserved_[0] = r.reserved_[1] = 0;
    for (int c = 0; c < 3; ++c) { r.sum[c] = a.sum[c]; r.nsum[c] = a.nsum[c]; r.lo[c] = (int16_t)a.lo[c]; r.hi[c] = (int16_t)a.hi[c]; }
    D.o_clusters[pos] = r;
}

__global__ void __launch_bounds__(256) k_fr_emit(MapDev M, FrDev D)
{
    const int nfb = min(D.ctr[FRC_BRICKS], D.cap_fb);
    for (int fb = blockIdx.x; fb < nfb; fb += gridDim.x) {
        const int b = D.fb_brick[fb];
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        for (int l = threadIdx.x; l < TSL_BRK3; l += 256) {
            const bool f = (D.bits[(size_t)fb * 128 + (l >> 5)] >> (l & 31)) & 1u;
            const int slot = f ? fr_slot(D, fb * TSL_BRK3 + l) : -1;
            const int row = slot >= 0 ? D.row[slot] : -1;
            const int pos = wave_reserve(&D.ctr[FRC_CURSOR], row >= 0);
            if (row >= 0) {
                const int ui = bi * 16 + (l >> 8), uj = bj * 16 + ((l >> 4) & 15), uk = bk * 16 + (l & 15);
                D.vkey[pos] = (uint32_t)((ui * M.N + uj) * M.Nz + uk);
                D.vval[pos] = ((unsigned long long)(uint32_t)row << 8) | D.mask[(size_t)fb * TSL_BRK3 + l];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_fr_unpack(MapDev M, FrDev D, int n)
{
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= n) return;
    const int key = (int)D.vkey_s[pos];
    const unsigned long long v = D.vval_s[pos];
    const int uk = key % M.Nz, uj = (key / M.Nz) % M.N, ui = key / (M.Nz * M.N);
    D.o_idx[(size_t)pos * 3] = (int16_t)(ui - M.hN); D.o_idx[(size_t)pos * 3 + 1] = (int16_t)(uj - M.hN); D.o_idx[(size_t)pos * 3 + 2] = (int16_t)(uk - M.hNz);
    D.o_mask[pos] = (uint8_t)(v & 0xffu);
    D.o_cluster[pos] = (int)(v >> 8);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
void frontier_release(tsl_tsdf* m)
{
    FrontierState* S = m->frontier;
    if (!S) return;
    void* ptrs[] = { S->D.ctr, S->D.fb_brick, S->D.hkey, S->D.hval, S->D.bits, S->D.mask, S->D.lab, S->D.acc, S->D.ckey, S->D.ckey_s, S->D.cval, S->D.cval_s, S->D.row,
                     S->D.vkey, S->D.vkey_s, S->D.vval, S->D.vval_s, S->D.o_idx, S->D.o_mask, S->D.o_cluster, S->D.o_clusters, S->temp };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete S;
    m->frontier = nullptr;
}

static int fr_check(tsl_tsdf* m, const tsl_frontier_cfg* c, FrCfg* C, const char* who)
{
    const std::string w(who);
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(c, w + ": null cfg");
    TSL_REQUIRE(std::isfinite(c->free_thres), w + ": free_thres is not finite");
    TSL_REQUIRE(c->connectivity == 0 || c->connectivity == 6 || c->connectivity == 18 || c->connectivity == 26, w + ": connectivity must be 6, 18 or 26 (0 = 26)");
    TSL_REQUIRE(c->min_unknown >= 0 && c->min_unknown <= 6, w + ": min_unknown must be 0 .. 6");
    TSL_REQUIRE(c->min_cluster >= 0, w + ": min_cluster is negative");
    TSL_REQUIRE((long long)m->N * m->N * m->Nz < (1ll << 31), w + ": the volume is too large for 31-bit voxel keys (N * N * Nz >= 2^31)");
    C->s = m->cfg.is_global_map ? 0 : m->active;
    C->thres = c->free_thres != 0.0f ? c->free_thres : m->surf_thres;
    C->min_unknown = c->min_unknown ? c->min_unknown : 1;
    C->conn = c->connectivity ? c->connectivity : 26;
    C->min_cluster = c->min_cluster ? c->min_cluster : 1;
    C->flags = c->flags; C->k_min = c->k_min; C->k_max = c->k_max;
    return TSL_OK;
}

#define FR_GROW(field, bytes_field, type, count) do { void* p_ = S->D.field; if ((rc = grow(&p_, &S->bytes_field, sizeof(type) * (size_t)(count)))) { S->D.field = nullptr; return rc; } S->D.field = (type*)p_; } while (0)

// sizes the per-brick arrays for `cap` frontier bricks
static int fr_reserve_bricks(FrontierState* S, int cap)
{
    int rc;
    int hs = 64; while (hs < 2 * cap) hs <<= 1;
    FR_GROW(fb_brick, b_brick, int, cap);
    FR_GROW(hkey, b_hkey, int, hs); FR_GROW(hval, b_hval, int, hs);
    FR_GROW(bits, b_bits, uint32_t, (size_t)cap * 128);
    FR_GROW(mask, b_mask, uint8_t, (size_t)cap * TSL_BRK3);
    FR_GROW(lab, b_lab, int, (size_t)cap * TSL_BRK3);
    S->D.cap_fb = cap; S->D.hmask = hs - 1;
    return TSL_OK;
}

static int fr_extract(tsl_tsdf* m, const FrCfg& C, hipStream_t q, int32_t* n_voxels, int32_t* n_clusters)
{
    int rc;
    if (!m->frontier) { m->frontier = new FrontierState(); }      // value-initialised: every pointer null, every size 0
    FrontierState* S = m->frontier;
    S->valid = false;
    FR_GROW(ctr, b_ctr, int, FRC_N);
    if (S->D.cap_fb == 0 && (rc = fr_reserve_bricks(S, 256))) return rc;
    const int nb_grid = m->M.max_bricks < 4096 ? m->M.max_bricks : 4096;
    int* h = m->h_ints;
    // ---- mark; twice when the map holds more frontier bricks than the arrays did (the map does not change in between: the stream is ours)
    for (int pass = 0; ; ++pass) {
        TSL_HIP(hipMemsetAsync(S->D.ctr, 0, sizeof(int) * FRC_N, q));
        TSL_HIP(hipMemsetAsync(S->D.hkey, 0xff, sizeof(int) * ((size_t)S->D.hmask + 1), q));
        prof_begin(m, TSL_K_FRONTIER_MARK, q);
        hipLaunchKernelGGL(k_fr_mark, dim3(nb_grid), dim3(256), 0, q, m->M, C, S->D);
        prof_end(m, q);
        TSL_HIP(hipGetLastError());
        TSL_HIP(hipMemcpyAsync(h, S->D.ctr, sizeof(int) * FRC_N, hipMemcpyDeviceToHost, q));
        TSL_HIP(hipStreamSynchronize(q));
        if (h[FRC_BRICKS] <= S->D.cap_fb) break;
        TSL_REQUIRE(pass == 0, "frontier_extract: the frontier brick count changed between two passes over an unchanged map");
        if ((rc = fr_reserve_bricks(S, h[FRC_BRICKS] + h[FRC_BRICKS] / 4))) return rc;
    }
    const int nfb = h[FRC_BRICKS], nvox = h[FRC_VOXELS];
    if (h[FRC_ERR]) { set_error("frontier_extract: the brick hash table overflowed"); return TSL_ERR_CAPACITY; }
    int ncl = 0, nkept = 0, nkv = 0;
    if (nvox > 0) {
        FR_GROW(acc, b_acc, FrAcc, nvox);
        FR_GROW(ckey, b_ckey, uint32_t, nvox); FR_GROW(ckey_s, b_ckey_s, uint32_t, nvox); FR_GROW(cval, b_cval, int, nvox); FR_GROW(cval_s, b_cval_s, int, nvox);
        FR_GROW(row, b_row, int, nvox);
        const int g = nfb < 4096 ? nfb : 4096;
        prof_begin(m, TSL_K_FRONTIER_LABEL, q);
        hipLaunchKernelGGL(k_fr_label, dim3(g), dim3(256), 0, q, C, S->D);
        prof_end(m, q);
        prof_begin(m, TSL_K_FRONTIER_JOIN, q);
        hipLaunchKernelGGL(k_fr_join, dim3(g), dim3(256), 0, q, m->M, C, S->D);
        hipLaunchKernelGGL(k_fr_flatten, dim3(g), dim3(256), 0, q, S->D);
        prof_end(m, q);
        prof_begin(m, TSL_K_FRONTIER_SUM, q);
        hipLaunchKernelGGL(k_fr_roots, dim3(g), dim3(256), 0, q, S->D);
        hipLaunchKernelGGL(k_fr_sum, dim3(g), dim3(256), 0, q, m->M, S->D);
        hipLaunchKernelGGL(k_fr_filter, dim3((unsigned)((nvox + 255) / 256 < 1024 ? (nvox + 255) / 256 : 1024)), dim3(256), 0, q, C, S->D);
        prof_end(m, q);
        TSL_HIP(hipGetLastError());
        TSL_HIP(hipMemcpyAsync(h, S->D.ctr, sizeof(int) * FRC_N, hipMemcpyDeviceToHost, q));
        TSL_HIP(hipStreamSynchronize(q));
        if (h[FRC_ERR]) { set_error("frontier_extract: an iteration cap was reached (error bits " + std::to_string(h[FRC_ERR]) + ": 1 label, 2 join, 4 flatten): the parent array is corrupt"); return TSL_ERR_CAPACITY; }
        ncl = h[FRC_ROOTS]; nkept = h[FRC_KEPT]; nkv = h[FRC_KEPT_VOXELS];
    }
    if (nkept > 0) {
        FR_GROW(vkey, b_vkey, uint32_t, nkv); FR_GROW(vkey_s, b_vkey_s, uint32_t, nkv); FR_GROW(vval, b_vval, unsigned long long, nkv); FR_GROW(vval_s, b_vval_s, unsigned long long, nkv);
        FR_GROW(o_idx, b_idx, int16_t, (size_t)nkv * 3); FR_GROW(o_mask, b_omask, uint8_t, nkv); FR_GROW(o_cluster, b_ocl, int, nkv);
        FR_GROW(o_clusters, b_ocls, tsl_frontier_cluster, nkept);
    }
    if (ncl > 0) {
        size_t ta = 0, tb = 0;
        TSL_HIP(rocprim::radix_sort_pairs(nullptr, ta, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)ncl, 0u, 32u, q));
        if (nkv > 0) TSL_HIP(rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)nkv, 0u, 32u, q));
        if ((rc = grow(&S->temp, &S->b_temp, (ta > tb ? ta : tb) + 256))) return rc;
        size_t tbytes = S->b_temp;
        prof_begin(m, TSL_K_FRONTIER_EMIT, q);
        hipError_t e1 = rocprim::radix_sort_pairs(S->temp, tbytes, S->D.ckey, S->D.ckey_s, S->D.cval, S->D.cval_s, (size_t)ncl, 0u, 32u, q), e2 = hipSuccess;
        if (e1 == hipSuccess) hipLaunchKernelGGL(k_fr_clusters, dim3((unsigned)((ncl + 255) / 256)), dim3(256), 0, q, S->D, ncl, nkept);
        if (e1 == hipSuccess && nkv > 0) {
            hipLaunchKernelGGL(k_fr_emit, dim3(nfb < 4096 ? nfb : 4096), dim3(256), 0, q, m->M, S->D);
            tbytes = S->b_temp;
            e2 = rocprim::radix_sort_pairs(S->temp, tbytes, S->D.vkey, S->D.vkey_s, S->D.vval, S->D.vval_s, (size_t)nkv, 0u, 32u, q);
            if (e2 == hipSuccess) hipLaunchKernelGGL(k_fr_unpack, dim3((unsigned)((nkv + 255) / 256)), dim3(256), 0, q, m->M, S->D, nkv);
        }
        prof_end(m, q);                                      // (the bracket is closed before any status is looked at)
        TSL_HIP(e1); TSL_HIP(e2);
        TSL_HIP(hipGetLastError());
    }
    S->n_voxels = nkv; S->n_clusters = nkept; S->valid = true;
    if (n_voxels) *n_voxels = nkv;
    if (n_clusters) *n_clusters = nkept;
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_frontier_extract(tsl_tsdf* m, const tsl_frontier_cfg* cfg, int32_t* n_voxels, int32_t* n_clusters)
{
    FrCfg C;
    int rc = fr_check(m, cfg, &C, "frontier_extract"); if (rc) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames: the pass runs behind them
    if ((rc = fr_extract(m, C, q, n_voxels, n_clusters))) return rc;
    TSL_HIP(hipStreamSynchronize(q));
    return TSL_OK;
}

int tsl_tsdf_frontier_read(tsl_tsdf* m, int16_t* idx, uint8_t* mask, int32_t* cluster, tsl_frontier_cluster* clusters, int64_t n_voxels, int64_t n_clusters)
{
    TSL_REQUIRE(m, "frontier_read: null handle");
    TSL_REQUIRE(m->frontier && m->frontier->valid, "frontier_read: call tsl_tsdf_frontier_extract first");
    const FrontierState* S = m->frontier;
    TSL_REQUIRE(n_voxels >= 0 && n_clusters >= 0, "frontier_read: a negative size");
    TSL_REQUIRE(n_voxels <= S->n_voxels && n_clusters <= S->n_clusters, "frontier_read: more rows than the last extraction produced");
    TSL_HIP(hipSetDevice(m->device));
    TSL_HIP(hipStreamSynchronize(m->stream_));
    if (n_voxels > 0) {
        if (idx) TSL_HIP(hipMemcpy(idx, S->D.o_idx, sizeof(int16_t) * 3 * (size_t)n_voxels, hipMemcpyDeviceToHost));
        if (mask) TSL_HIP(hipMemcpy(mask, S->D.o_mask, (size_t)n_voxels, hipMemcpyDeviceToHost));
        if (cluster) TSL_HIP(hipMemcpy(cluster, S->D.o_cluster, sizeof(int32_t) * (size_t)n_voxels, hipMemcpyDeviceToHost));
    }
    if (n_clusters > 0 && clusters) TSL_HIP(hipMemcpy(clusters, S->D.o_clusters, sizeof(tsl_frontier_cluster) * (size_t)n_clusters, hipMemcpyDeviceToHost));
    return TSL_OK;
}

int tsl_tsdf_frontier_dev(tsl_tsdf* m, const tsl_frontier_cfg* cfg, void** idx_dev, void** mask_dev, void** cluster_dev, void** clusters_dev,
                          int32_t* n_voxels, int32_t* n_clusters, void* user_stream)
{
    FrCfg C;
    int rc = fr_check(m, cfg, &C, "frontier_dev"); if (rc) return rc;
    TSL_REQUIRE(n_voxels && n_clusters, "frontier_dev: null count pointer");
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = fr_extract(m, C, q, n_voxels, n_clusters))) return rc;
    const FrontierState* S = m->frontier;
    if (idx_dev) *idx_dev = *n_voxels ? S->D.o_idx : nullptr;
    if (mask_dev) *mask_dev = *n_voxels ? S->D.o_mask : nullptr;
    if (cluster_dev) *cluster_dev = *n_voxels ? S->D.o_cluster : nullptr;
    if (clusters_dev) *clusters_dev = *n_clusters ? S->D.o_clusters : nullptr;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

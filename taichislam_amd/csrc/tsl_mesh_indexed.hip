// tsl_mesh_indexed.hip -- the marching-cubes mesh of generate_mesh(1) as an INDEXED mesh: one vertex per grid edge that a valid cell's case names,
// in ascending edge-key order, and int32 triangles over those rows in ascending cell-key order (include/taichislam_hip.h, "indexed mesh"; DESIGN.md
// "Indexed marching-cubes mesh").  The cell, tile and vertex rules are those of tsl_mc.hpp, shared with the soup of tsl_mesh.hip.
//
// No atomic decides an output position.  A vertex row is  base_v[brick] + (used edges of the brick below this one)  and a triangle row is
// base_t[brick] + (triangles of the brick's cells below this one); the bases are an exclusive scan of the per-brick totals in ascending brick-key
// order (the pool's allocation order plays no part):
//   k_mi_summary   per brick in use: its key for the sort, and its sign flags
//   radix sort     the bricks in use by key (rocPRIM); their number is read first -- it sizes the sort and the scan, which otherwise run over the whole pool
//   k_mi_count     per brick, 19^3 tile in LDS: which of its 3 x 4096 edges are used (a bitmap in key order, with a running count per word),
//                  and the totals { used edges, triangles }
//   k_mi_gather, inclusive scan (rocPRIM), k_mi_scatter      totals in key order -> base per pool brick
//   k_mi_emit      per brick: one lane per used edge writes the vertex row; every triangle corner finds the row of its edge through the bitmap
//                  of the brick that owns the edge (this brick or one of its seven +1 neighbours)
#include "tsl_mc.hpp"
#include <rocprim/rocprim.hpp>

namespace tsl {

#define MI_C 17                                                              // cells -1 .. 15 per axis name the edges a brick owns
#define MI_C3 (MI_C * MI_C * MI_C)
#define MI_WORDS 384                                                         // 3 x 4096 edge bits per brick; bit l * 3 + axis = the brick's part of the edge key

struct MiDev {
    uint32_t* flags;                   // [max_bricks] bit 0: a stored value < 0, bit 1: one that is not
    uint32_t *key, *key_s; int *ord, *ord_s;      // [max_bricks] brick key (owner) and pool index of the bricks in use, unsorted / sorted by key
    uint32_t* bits;                    // [max_bricks][384] used edges
    uint16_t* pref;                    // [max_bricks][384] used edges of the brick in the words below
    unsigned long long *cnt, *g, *gi;  // [max_bricks] { used edges | triangles << 32 } per pool brick; the same in key order; its inclusive scan
    unsigned long long* base;          // [max_bricks] { first vertex row | first triangle row << 32 } per pool brick
    float *v, *n, *c; int16_t* e; int* idx;       // the mesh: [cap_v][3] x 3, [cap_v][4], [cap_t][3]
};

struct MeshIdxState {
    MiDev D;
    void* temp; size_t b_temp;
    int64_t cap_v, cap_t;              // rows allocated (the buffers only grow)
    int64_t max_v, max_t;              // capacities of the last call
    int64_t n_v, n_t;                  // true counts of the last call
    bool valid, ready;
};

__device__ __forceinline__ int mi_cell(int x, int y, int z) { return (x * MI_C + y) * MI_C + z; }      // cell coords = brick coords + 1
// table edge e -> the offset of its LOWER corner and its axis: the grid edge it is, whichever way the table walks it
__device__ __forceinline__ int mi_edge(int e, int* d)
{
    int a, b; mc_edge_corners(e, &a, &b);
    int da[3], db[3]; mc_corner(a, da); mc_corner(b, db);
    int axis = 0;
    for (int c = 0; c < 3; ++c) { d[c] = da[c] < db[c] ? da[c] : db[c]; if (da[c] != db[c]) axis = c; }
    return axis;
}

__global__ void __launch_bounds__(256) k_mi_summary(MapDev M, MiDev D, int nused)
{
    for (int p = blockIdx.x; p < nused; p += gridDim.x) {
        const uint32_t f = mc_brick_flags(M, p);
        if (threadIdx.x == 0) { D.flags[p] = f; D.key[p] = (uint32_t)M.owner[p]; D.ord[p] = p; D.cnt[p] = 0ull; }
    }
}

// Thread t owns the 16 voxels l = 16 t .. 16 t + 15 of the brick (one z-run): consecutive threads, consecutive keys.
__global__ void __launch_bounds__(256) k_mi_count(MapDev M, MiDev D, float thres, int nused)
{
    __shared__ unsigned long long s_tri[256];
    __shared__ uint16_t s_t[MC_T3];
    __shared__ uint32_t s_o[MC_OWORDS];
    __shared__ uint32_t s_cv[(MI_C3 + 31) / 32];          // valid cells, cell coordinates -1 .. 15
    __shared__ uint32_t s_bits[MI_WORDS];
    __shared__ int s_nb[27], s_w[4], s_skip;
    s_tri[threadIdx.x] = MC_TRI_PACKED[threadIdx.x];
    for (int p = blockIdx.x; p < nused; p += gridDim.x) {
        const int owner = M.owner[p];
        const int s = owner / M.nb3, b = owner - s * M.nb3;
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        mc_gather(M, D.flags, nused, p, s, bi, bj, bk, 0, MC_T3, s_nb, s_t, s_o, &s_skip);
        if (s_skip) continue;                                            // (uniform) cnt[p] stays 0: no edge of this brick is used, no cell of it has a triangle
        for (int i = threadIdx.x; i < (MI_C3 + 31) / 32; i += 256) s_cv[i] = 0u;
        for (int i = threadIdx.x; i < MI_WORDS; i += 256) s_bits[i] = 0u;
        __syncthreads();
        for (int c = threadIdx.x; c < MI_C3; c += 256) {
            const int z = c % MI_C, y = (c / MI_C) % MI_C, x = c / (MI_C * MI_C);
            if (mc_valid(s_t, s_o, x - 1, y - 1, z - 1, thres)) atomicOr(&s_cv[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
        // an edge is used when a valid cell among the four around it names it; a case names exactly the edges whose corners differ in sign
        const int lx = (int)threadIdx.x >> 4, ly = (int)threadIdx.x & 15;
        unsigned long long mybits = 0ull;                                // 48 bits: 16 voxels x 3 axes
        int mytri = 0;
        for (int lz = 0; lz < 16; ++lz) {
            const bool n0 = h2f(s_t[mc_tile(lx + 1, ly + 1, lz + 1)]) < 0.0f;
            const int cx = lx + 1, cy = ly + 1, cz = lz + 1;             // cell coordinates of the voxel's own cell
            const bool v000 = mc_bit(s_cv, mi_cell(cx, cy, cz)), v100 = mc_bit(s_cv, mi_cell(cx - 1, cy, cz)), v010 = mc_bit(s_cv, mi_cell(cx, cy - 1, cz)),
                       v001 = mc_bit(s_cv, mi_cell(cx, cy, cz - 1)), v110 = mc_bit(s_cv, mi_cell(cx - 1, cy - 1, cz)), v101 = mc_bit(s_cv, mi_cell(cx - 1, cy, cz - 1)),
                       v011 = mc_bit(s_cv, mi_cell(cx, cy - 1, cz - 1));
            const bool nx = h2f(s_t[mc_tile(lx + 2, ly + 1, lz + 1)]) < 0.0f, ny = h2f(s_t[mc_tile(lx + 1, ly + 2, lz + 1)]) < 0.0f,
                       nz = h2f(s_t[mc_tile(lx + 1, ly + 1, lz + 2)]) < 0.0f;
            if (n0 != nx && (v000 || v010 || v001 || v011)) mybits |= 1ull << (3 * lz);
            if (n0 != ny && (v000 || v100 || v001 || v101)) mybits |= 1ull << (3 * lz + 1);
            if (n0 != nz && (v000 || v100 || v010 || v110)) mybits |= 1ull << (3 * lz + 2);
            if (v000) mytri += mc_ntri(s_tri[mc_case(s_t, lx, ly, lz)]);
        }
        {   // bit 48 t of the brick's bitmap onwards: word 3 t / 2, at bit 0 (t even) or 16 (t odd)
            const int w = ((int)threadIdx.x * 48) >> 5, sh = ((int)threadIdx.x * 48) & 31;
            const uint32_t a = (uint32_t)(mybits << sh), c2 = (uint32_t)(mybits >> (32 - sh));
            if (a) atomicOr(&s_bits[w], a);
            if (c2) atomicOr(&s_bits[w + 1], c2);                        // (w + 1 <= 383: t even ends in word w + 1 = 3 t / 2 + 1, t odd in word w + 1 = (3 t + 1) / 2)
        }
        __syncthreads();
        // running count per word: thread t < 192 takes words 2 t, 2 t + 1
        const uint32_t w0 = threadIdx.x < MI_WORDS / 2 ? s_bits[2 * threadIdx.x] : 0u, w1 = threadIdx.x < MI_WORDS / 2 ? s_bits[2 * threadIdx.x + 1] : 0u;
        int nv = 0, nt = 0;
        const int first = mc_block_scan(__popc(w0) + __popc(w1), s_w, &nv);
        if (threadIdx.x < MI_WORDS / 2) {
            const size_t o = (size_t)p * MI_WORDS + 2 * threadIdx.x;
            D.bits[o] = w0; D.bits[o + 1] = w1;
            D.pref[o] = (uint16_t)first; D.pref[o + 1] = (uint16_t)(first + __popc(w0));
        }
        (void)mc_block_scan(mytri, s_w, &nt);
        if (threadIdx.x == 0) D.cnt[p] = (unsigned long long)(uint32_t)nv | (unsigned long long)(uint32_t)nt << 32;
    }
}

__global__ void __launch_bounds__(256) k_mi_gather(MiDev D, int n)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) D.g[r] = D.cnt[D.ord_s[r]];
}
__global__ void __launch_bounds__(256) k_mi_scatter(MiDev D, int n)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) D.base[D.ord_s[r]] = D.gi[r] - D.g[r];                    // (both halves of the packed word: neither difference borrows)
}

__global__ void __launch_bounds__(256) k_mi_emit(MapDev M, MiDev D, float thres, float vs, long long max_v, long long max_t, int nused)
{
    __shared__ unsigned long long s_tri[256];
    __shared__ uint16_t s_t[MC_T3];
    __shared__ uint32_t s_o[MC_OWORDS];
    __shared__ uint32_t s_bits[MI_WORDS];
    __shared__ uint16_t s_list[3 * TSL_BRK3];             // the brick's used edges (bit numbers) in key order
    __shared__ int s_nb[27], s_w[4], s_skip;
    __shared__ uint32_t s_basev[8];
    s_tri[threadIdx.x] = MC_TRI_PACKED[threadIdx.x];
    for (int p = blockIdx.x; p < nused; p += gridDim.x) {
        const unsigned long long cnt = D.cnt[p];
        if (cnt == 0ull) continue;                                       // (uniform)
        const int owner = M.owner[p];
        const int s = owner / M.nb3, b = owner - s * M.nb3;
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        mc_gather(M, D.flags, nused, p, s, bi, bj, bk, 0, MC_T3, s_nb, s_t, s_o, &s_skip);
        if (s_skip) continue;                                            // (never with a count: the same test as in k_mi_count)
        const int nv = (int)(uint32_t)cnt, nt = (int)(cnt >> 32);
        const unsigned long long base = D.base[p];
        if (threadIdx.x < 8) {                                           // first vertex row of the eight bricks that own the edges of this brick's cells
            const int np = s_nb[((((int)threadIdx.x >> 2) + 1) * 3 + ((((int)threadIdx.x >> 1) & 1) + 1)) * 3 + (((int)threadIdx.x & 1) + 1)];
            s_basev[threadIdx.x] = np >= 0 ? (uint32_t)D.base[np] : 0u;
        }
        // ---- vertices: the used edges as a list, then one lane per vertex ----
        if (threadIdx.x < MI_WORDS / 2) {
            const size_t o = (size_t)p * MI_WORDS + 2 * threadIdx.x;
            int at = D.pref[o];
            for (int h = 0; h < 2; ++h) {
                uint32_t w = D.bits[o + h];
                s_bits[2 * threadIdx.x + h] = w;
                while (w) { const int bit = __builtin_ctz(w); w &= w - 1u; if (at < 3 * TSL_BRK3) s_list[at] = (uint16_t)((2 * threadIdx.x + h) * 32 + bit); ++at; }
            }
        }
        __syncthreads();
        for (int r = threadIdx.x; r < nv; r += 256) {
            const long long row = (long long)(uint32_t)base + r;
            if (row >= max_v) break;                                     // rows ascend with r: nothing of this thread's is stored from here on
            const int bit = s_list[r], l = bit / 3, a = bit - 3 * l;
            const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
            const int i = bi * 16 + lx - M.hN, j = bj * 16 + ly - M.hN, k = bk * 16 + lz - M.hNz;
            const int ux = lx + (a == 0), uy = ly + (a == 1), uz = lz + (a == 2);            // the upper corner, brick coordinates 0 .. 16
            const float p0[3] = { (float)i, (float)j, (float)k };
            const float p1[3] = { (float)(i + (a == 0)), (float)(j + (a == 1)), (float)(k + (a == 2)) };
            float pv[3], mu, nn[3];
            mc_vertex(h2f(s_t[mc_tile(lx + 1, ly + 1, lz + 1)]), h2f(s_t[mc_tile(ux + 1, uy + 1, uz + 1)]), p0, p1, pv, &mu);      // from the lower corner to the upper one
            const size_t o = (size_t)row * 3;
            if (D.c) {                                                   // the same corners and mu
                const int npu = s_nb[(((ux >> 4) + 1) * 3 + ((uy >> 4) + 1)) * 3 + ((uz >> 4) + 1)];
                const uint2* col = reinterpret_cast<const uint2*>(M.col);
                float vc[3];
                mc_colour(col[(size_t)p * TSL_BRK3 + l], npu >= 0 ? col[(size_t)npu * TSL_BRK3 + (((ux & 15) << 8) | ((uy & 15) << 4) | (uz & 15))] : make_uint2(0u, 0u), mu, vc);
                for (int c = 0; c < 3; ++c) D.c[o + c] = vc[c];
            }
            mc_tile_normal(s_t, (int)rnd_f(pv[0]) - i + lx + 1, (int)rnd_f(pv[1]) - j + ly + 1, (int)rnd_f(pv[2]) - k + lz + 1, nn);
            D.v[o] = pv[0] * vs; D.v[o + 1] = pv[1] * vs; D.v[o + 2] = pv[2] * vs;
            D.n[o] = nn[0]; D.n[o + 1] = nn[1]; D.n[o + 2] = nn[2];
            reinterpret_cast<short4*>(D.e)[row] = make_short4((short)i, (short)j, (short)k, (short)a);
        }
        // ---- triangles: thread t walks the cells of its z-run in key order ----
        if (nt == 0) continue;                                           // (uniform) a brick that only owns edges of its neighbours' cells
        const int lx = (int)threadIdx.x >> 4, ly = (int)threadIdx.x & 15;
        int mytri = 0;
        uint32_t vmask = 0u;
        for (int lz = 0; lz < 16; ++lz)
            if (mc_valid(s_t, s_o, lx, ly, lz, thres)) { vmask |= 1u << lz; mytri += mc_ntri(s_tri[mc_case(s_t, lx, ly, lz)]); }
        int total = 0;
        long long at = (long long)(base >> 32) + mc_block_scan(mytri, s_w, &total);
        for (int lz = 0; lz < 16 && mytri; ++lz) {
            if (!((vmask >> lz) & 1u)) continue;
            const unsigned long long tri = s_tri[mc_case(s_t, lx, ly, lz)];
            for (int u = 0; u < 5; ++u) {
                if (((tri >> (12 * u)) & 0xfull) == 0xfull) continue;
                if (at < max_t) {
                    int rows[3];
                    for (int q = 0; q < 3; ++q) {
                        int d[3];
                        const int a = mi_edge((int)((tri >> (4 * (3 * u + q))) & 0xfull), d);
                        const int ox = lx + d[0], oy = ly + d[1], oz = lz + d[2];      // the voxel that owns the edge, brick coordinates 0 .. 16
                        const int np = s_nb[(((ox >> 4) + 1) * 3 + ((oy >> 4) + 1)) * 3 + ((oz >> 4) + 1)];
                        const int bit = ((((ox & 15) << 8) | ((oy & 15) << 4) | (oz & 15))) * 3 + a;
                        int row = -1;
                        if (np >= 0) {                                   // (always: both corners of a used edge are observed, so their bricks exist)
                            const size_t o = (size_t)np * MI_WORDS + (bit >> 5);
                            row = (int)(s_basev[(ox >> 4) * 4 + (oy >> 4) * 2 + (oz >> 4)] + D.pref[o] + __popc(D.bits[o] & ((1u << (bit & 31)) - 1u)));
                        }
                        rows[q] = row;
                    }
                    int* o = D.idx + (size_t)at * 3;
                    o[0] = rows[0]; o[1] = rows[1]; o[2] = rows[2];
                }
                ++at;
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
void mesh_indexed_release(tsl_tsdf* m)
{
    MeshIdxState* S = m->mesh_idx;
    if (!S) return;
    void* ptrs[] = { S->D.flags, S->D.key, S->D.key_s, S->D.ord, S->D.ord_s, S->D.bits, S->D.pref, S->D.cnt, S->D.g, S->D.gi, S->D.base,
                     S->D.v, S->D.n, S->D.c, S->D.e, S->D.idx, S->temp };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete S;
    m->mesh_idx = nullptr;
}

#define MI_ALLOC(field, type, count) do { if (S->D.field) { (void)hipFree(S->D.field); S->D.field = nullptr; } TSL_HIP(hipMalloc((void**)&S->D.field, sizeof(type) * (size_t)(count))); } while (0)

static int mi_prepare(tsl_tsdf* m, int64_t max_v, int64_t max_t)
{
    if (!m->mesh_idx) m->mesh_idx = new MeshIdxState();      // value-initialised: every pointer null, every size 0
    MeshIdxState* S = m->mesh_idx;
    const size_t nb = (size_t)m->M.max_bricks;
    if (!S->ready) {
        MI_ALLOC(flags, uint32_t, nb); MI_ALLOC(key, uint32_t, nb); MI_ALLOC(key_s, uint32_t, nb); MI_ALLOC(ord, int, nb); MI_ALLOC(ord_s, int, nb);
        MI_ALLOC(bits, uint32_t, nb * MI_WORDS); MI_ALLOC(pref, uint16_t, nb * MI_WORDS);
        MI_ALLOC(cnt, unsigned long long, nb); MI_ALLOC(g, unsigned long long, nb); MI_ALLOC(gi, unsigned long long, nb); MI_ALLOC(base, unsigned long long, nb);
        S->ready = true;
    }
    if (S->cap_v < max_v) {
        void* old[] = { S->D.v, S->D.n, S->D.c, S->D.e };
        for (void* p : old) if (p) (void)hipFree(p);
        S->D.v = S->D.n = S->D.c = nullptr; S->D.e = nullptr; S->cap_v = 0;
        MI_ALLOC(v, float, 3 * (size_t)max_v); MI_ALLOC(n, float, 3 * (size_t)max_v); MI_ALLOC(e, int16_t, 4 * (size_t)max_v);
        if (m->M.col) MI_ALLOC(c, float, 3 * (size_t)max_v);
        S->cap_v = max_v;
    }
    if (S->cap_t < max_t) {
        if (S->D.idx) (void)hipFree(S->D.idx);
        S->D.idx = nullptr; S->cap_t = 0;
        MI_ALLOC(idx, int, 3 * (size_t)max_t);
        S->cap_t = max_t;
    }
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_mesh_generate_indexed(tsl_tsdf* m, float surface_thres, int64_t max_vertices, int64_t max_triangles, int64_t* n_vertices, int64_t* n_triangles)
{
    TSL_REQUIRE(m, "mesh_generate_indexed: null handle");
    TSL_REQUIRE(n_vertices && n_triangles, "mesh_generate_indexed: null argument");
    TSL_REQUIRE(max_vertices > 0 && max_triangles > 0, "mesh_generate_indexed: max_vertices and max_triangles must be positive");
    TSL_REQUIRE(max_vertices <= 0x7fffffffll && max_triangles <= 0x7fffffffll, "mesh_generate_indexed: rows are 32-bit indices (capacity > 2^31 - 1)");
    TSL_REQUIRE((int64_t)m->M.max_bricks * 3 * TSL_BRK3 <= 0x7fffffffll, "mesh_generate_indexed: the brick pool is too large for 32-bit vertex rows");
    TSL_HIP(hipSetDevice(m->device));
    if (m->mesh_idx) m->mesh_idx->valid = false;
    int rc; if ((rc = mi_prepare(m, max_vertices, max_triangles))) return rc;
    MeshIdxState* S = m->mesh_idx;
    int n = 0; if ((rc = tsl_tsdf_bricks_in_use(m, &n))) return rc;      // (issues the queued frames and waits for them: the mesh is of the map behind them)
    hipStream_t q = ms(m);
    unsigned long long* tot = reinterpret_cast<unsigned long long*>(m->h_ints);
    *tot = 0ull;
    if (n > 0) {
        size_t ta = 0, tb = 0;
        TSL_HIP(rocprim::radix_sort_pairs(nullptr, ta, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)n, 0u, 32u, q));
        TSL_HIP(rocprim::inclusive_scan(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)n, rocprim::plus<unsigned long long>(), q));
        if ((!S->temp || (ta > tb ? ta : tb) > S->b_temp) && (rc = grow(&S->temp, &S->b_temp, (ta > tb ? ta : tb) + 256))) return rc;      // (never null: rocPRIM takes a null pointer for a size query)
        prof_begin(m, TSL_K_MESH, q);
        const int g = n < 2048 ? n : 2048;
        hipLaunchKernelGGL(k_mi_summary, dim3(g), dim3(256), 0, q, m->M, S->D, n);
        size_t tbytes = S->b_temp;
        hipError_t e1 = rocprim::radix_sort_pairs(S->temp, tbytes, S->D.key, S->D.key_s, S->D.ord, S->D.ord_s, (size_t)n, 0u, 32u, q), e2 = hipSuccess;
        if (e1 == hipSuccess) {
            hipLaunchKernelGGL(k_mi_count, dim3(g), dim3(256), 0, q, m->M, S->D, surface_thres, n);
            hipLaunchKernelGGL(k_mi_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, S->D, n);
            tbytes = S->b_temp;
            e2 = rocprim::inclusive_scan(S->temp, tbytes, S->D.g, S->D.gi, (size_t)n, rocprim::plus<unsigned long long>(), q);
        }
        if (e1 == hipSuccess && e2 == hipSuccess) {
            hipLaunchKernelGGL(k_mi_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, S->D, n);
            hipLaunchKernelGGL(k_mi_emit, dim3(g), dim3(256), 0, q, m->M, S->D, surface_thres, m->P.vs, (long long)max_vertices, (long long)max_triangles, n);
        }
        prof_end(m, q);                                          // (the bracket is closed before any status is looked at)
        TSL_HIP(e1); TSL_HIP(e2);
        TSL_HIP(hipGetLastError());
        TSL_HIP(hipMemcpyAsync(tot, S->D.gi + (n - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
        TSL_HIP(hipStreamSynchronize(q));
    }
    S->n_v = (int64_t)(uint32_t)*tot; S->n_t = (int64_t)(*tot >> 32);
    S->max_v = max_vertices; S->max_t = max_triangles; S->valid = true;
    *n_vertices = S->n_v; *n_triangles = S->n_t;
    return TSL_OK;
}

int tsl_mesh_read_indexed(tsl_tsdf* m, float* verts, float* normals, float* colors, int16_t* edges, int32_t* indices, int64_t n_vertices, int64_t n_triangles)
{
    TSL_REQUIRE(m, "mesh_read_indexed: null handle");
    const MeshIdxState* S = m->mesh_idx;
    TSL_REQUIRE(S && S->valid, "mesh_read_indexed: call tsl_mesh_generate_indexed first");
    TSL_REQUIRE(n_vertices >= 0 && n_triangles >= 0, "mesh_read_indexed: negative row count");
    TSL_REQUIRE(n_vertices <= (S->n_v < S->max_v ? S->n_v : S->max_v) && n_triangles <= (S->n_t < S->max_t ? S->n_t : S->max_t),
                "mesh_read_indexed: more rows than the last tsl_mesh_generate_indexed stored");
    TSL_HIP(hipSetDevice(m->device));
    TSL_HIP(hipStreamSynchronize(ms(m)));
    const size_t nv = (size_t)n_vertices, nt = (size_t)n_triangles;
    if (verts && nv) TSL_HIP(hipMemcpy(verts, S->D.v, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost));
    if (normals && nv) TSL_HIP(hipMemcpy(normals, S->D.n, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost));
    if (colors && S->D.c && nv) TSL_HIP(hipMemcpy(colors, S->D.c, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost));
    if (edges && nv) TSL_HIP(hipMemcpy(edges, S->D.e, sizeof(int16_t) * 4 * nv, hipMemcpyDeviceToHost));
    if (indices && nt) TSL_HIP(hipMemcpy(indices, S->D.idx, sizeof(int32_t) * 3 * nt, hipMemcpyDeviceToHost));
    return TSL_OK;
}

int tsl_mesh_indexed_dev(tsl_tsdf* m, void** verts_dev, void** normals_dev, void** colors_dev, void** edges_dev, void** indices_dev, int64_t* n_vertices, int64_t* n_triangles)
{
    TSL_REQUIRE(m, "mesh_indexed_dev: null handle");
    const MeshIdxState* S = m->mesh_idx;
    TSL_REQUIRE(S && S->valid, "mesh_indexed_dev: call tsl_mesh_generate_indexed first");
    if (verts_dev) *verts_dev = S->D.v; if (normals_dev) *normals_dev = S->D.n; if (colors_dev) *colors_dev = S->D.c;
    if (edges_dev) *edges_dev = S->D.e; if (indices_dev) *indices_dev = S->D.idx;
    if (n_vertices) *n_vertices = S->n_v; if (n_triangles) *n_triangles = S->n_t;
    return TSL_OK;
}

}  // extern "C"

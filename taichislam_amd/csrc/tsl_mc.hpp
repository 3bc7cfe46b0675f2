// tsl_mc.hpp -- the marching-cubes rules of MarchingCubeMesher (taichi_slam/mapping/marching_cube_mesher.py:44-221, reference root) that the triangle
// soup (tsl_mesh.hip) and the indexed mesh (tsl_mesh_indexed.hip) share: the 19^3 brick tile and how it is gathered, the cell rule on it, the brick
// sign flags, the vertex, its colour and its f16 normal, the block scan.  One definition each: the two meshes are held to the reference and to each
// other bit for bit, and a rule stated twice is a rule that can be mended once.
#pragma once
#include "tsl_tsdf.hpp"
#include "mc_tables_data.h"

namespace tsl {

#define MC_EPS 1e-6f                                                         // marching_cube_mesher.py:6
// Everything a brick's cells read lies in [-1, 17]^3 around the brick: a cell needs its 8 corners (voxel .. voxel + 1) and, per vertex, the central
// differences around the voxel nearest to it (corner .. corner + 1, each +- 1).  The tile holds f16 TSDF bits (0 where nothing is stored: reading an
// inactive cell yields 0, A7) and one observed bit per entry.
#define MC_T 19
#define MC_T3 (MC_T * MC_T * MC_T)
#define MC_OWORDS ((MC_T3 + 31) / 32)
__device__ __forceinline__ int mc_tile(int x, int y, int z) { return (x * MC_T + y) * MC_T + z; }      // tile coords = brick coords + 1
__device__ __forceinline__ bool mc_bit(const uint32_t* b, int i) { return (b[i >> 5] >> (i & 31)) & 1u; }
// cube corner q -> offset (grid_xyz :196-206) and table edge e -> its two corners, in the order the table walks it (edges_grid_id :208-221)
__device__ __forceinline__ void mc_corner(int q, int* d) { d[0] = ((q + 1) >> 1) & 1; d[1] = (q >> 1) & 1; d[2] = (q >> 2) & 1; }
__device__ __forceinline__ void mc_edge_corners(int e, int* a, int* b)
{
    if (e < 4) { *a = e; *b = (e + 1) & 3; }
    else if (e < 8) { *a = e; *b = 4 + ((e - 3) & 3); }
    else { *a = e - 8; *b = e - 4; }
}

// ---- the cell at brick coordinates (x, y, z), each -1 .. 15, on the tile ----
// valid: its own voxel observed and below the threshold (:184), all eight corners observed (:133-138)
__device__ __forceinline__ bool mc_valid(const uint16_t* s_t, const uint32_t* s_o, int x, int y, int z, float thres)
{
    const int t0 = mc_tile(x + 1, y + 1, z + 1);
    if (!(mc_bit(s_o, t0) && h2f(s_t[t0]) < thres)) return false;
    for (int q = 1; q < 8; ++q) {
        int d[3]; mc_corner(q, d);
        if (!mc_bit(s_o, mc_tile(x + 1 + d[0], y + 1 + d[1], z + 1 + d[2]))) return false;
    }
    return true;
}
// its case (:141-144)
__device__ __forceinline__ int mc_case(const uint16_t* s_t, int x, int y, int z)
{
    int c = 0;
    for (int q = 0; q < 8; ++q) {
        int d[3]; mc_corner(q, d);
        if (h2f(s_t[mc_tile(x + 1 + d[0], y + 1 + d[1], z + 1 + d[2])]) < 0.0f) c |= 1 << q;
    }
    return c;
}
// the triangles of a packed case word (MC_TRI_PACKED)
__device__ __forceinline__ int mc_ntri(unsigned long long tri)
{
    int n = 0;
    for (int t = 0; t < 5; ++t) if (((tri >> (12 * t)) & 0xfull) != 0xfull) ++n;                      // :173-177 (triTable[cube][3t] != -1)
    return n;
}

// ---- which bricks can hold a triangle at all: a cell emits one only if its eight corners are not all on one side of zero (the case table is empty
//      for 0 and 255, :141-177).  The flags of pool brick p, from one coalesced pass over its stored values: bit 0 it holds a value < 0, bit 1 one
//      that is not (a voxel nobody wrote reads 0, as in the reference).  Every thread of the block calls it (two barriers) and gets the same word. ----
__device__ __forceinline__ uint32_t mc_brick_flags(const MapDev& M, int p)
{
    const uint4* tw = reinterpret_cast<const uint4*>(M.tw + (size_t)p * TSL_BRK3);
    uint32_t f = 0u;
#pragma unroll
    for (int q = 0; q < TSL_BRK3 / 4 / 256; ++q) {
        const uint4 v = tw[q * 256 + threadIdx.x];
        const uint32_t w4[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int u = 0; u < 4; ++u) f |= h2f((h16)(w4[u] & 0xffffu)) < 0.0f ? 1u : 2u;
    }
    const int neg = __syncthreads_or((int)(f & 1u)), nn = __syncthreads_or((int)(f & 2u));
    return (neg ? 1u : 0u) | (nn ? 2u : 0u);
}

// ---- the neighbourhood of pool brick p (brick (bi, bj, bk) of submap s): the pool indices of the 27 bricks around it in s_nb, and -- unless the brick
//      and the seven +1 bricks its cells' corners reach into are all on one side of zero by their flags (then *s_skip; in a map of a closed surface
//      most bricks are) -- entries [t_begin, t_end) of the tile, gathered once through those 27.  Ends with the tile visible to every thread. ----
__device__ __forceinline__ void mc_gather(const MapDev& M, const uint32_t* __restrict__ flags, int nused, int p, int s, int bi, int bj, int bk,
                                          int t_begin, int t_end, int* s_nb, uint16_t* s_t, uint32_t* s_o, int* s_skip)
{
    __syncthreads();                                                     // the previous tile is no longer read
    if (threadIdx.x < 64) {                                              // (the first wave)
        int np = -1; bool corner = false;
        if (threadIdx.x < 27) {
            const int di = (int)threadIdx.x / 9 - 1, dj = ((int)threadIdx.x / 3) % 3 - 1, dk = (int)threadIdx.x % 3 - 1;
            const int i = bi + di, j = bj + dj, k = bk + dk;
            np = (i < 0 || i >= M.nbx || j < 0 || j >= M.nbx || k < 0 || k >= M.nbz) ? -1 : pool_lookup_ro(M, s, (i * M.nbx + j) * M.nbz + k);
            if (np >= nused) np = -1;                                       // (never: the table only names bricks in use; it bounds an index read from memory)
            s_nb[threadIdx.x] = np;
            corner = di >= 0 && dj >= 0 && dk >= 0;                         // the eight bricks the corners of this brick's cells lie in
        }
        const uint32_t f = corner ? (np >= 0 ? flags[np] : 2u) : 0u;        // (no brick: the corners read 0)
        const bool neg = __ballot((f & 1u) != 0u) != 0ull, nn = __ballot((f & 2u) != 0u) != 0ull;
        if (threadIdx.x == 0) *s_skip = (neg && nn) ? 0 : 1;
    }
    for (int i = threadIdx.x; i < MC_OWORDS; i += 256) s_o[i] = 0u;
    __syncthreads();
    if (*s_skip) return;                                                 // (uniform) every corner of every cell on one side of zero: no triangle
    // four independent loads per thread and round, from a valid address unconditionally so that nothing separates the requests: a loop of
    // dependent gathers costs a memory latency per entry
    for (int c = t_begin; c < t_end; c += 4 * 256) {
        uint32_t tw[4]; int8_t ob[4]; bool ok[4]; int tt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = c + u * 256 + (int)threadIdx.x;
            tt[u] = t;
            const int tc = t < t_end ? t : 0;
            const int tz = tc % MC_T, ty = (tc / MC_T) % MC_T, tx = tc / (MC_T * MC_T);
            const int np = s_nb[(((tx + 15) >> 4) * 3 + ((ty + 15) >> 4)) * 3 + ((tz + 15) >> 4)];
            ok[u] = t < t_end && np >= 0 && in_volume(M, bi * 16 + tx - 1 - M.hN, bj * 16 + ty - 1 - M.hN, bk * 16 + tz - 1 - M.hNz);
            const size_t v = (size_t)(ok[u] ? np : p) * TSL_BRK3 + ((((tx + 15) & 15) << 8) | (((ty + 15) & 15) << 4) | ((tz + 15) & 15));
            tw[u] = M.tw[v]; ob[u] = M.obs[v];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tt[u];
            if (t >= t_end) continue;
            s_t[t] = ok[u] ? (uint16_t)(tw[u] & 0xffffu) : (uint16_t)0;
            if (ok[u] && ob[u] > 0) atomicOr(&s_o[t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();
}

// ---- the vertex on the edge from corner p0 (value v0) to corner p1 (value v1), vertexInterp :44-60.  mu = -v0 / f16(v1 - v0) (valp2 - valp1 of two
//      f16 values is an f16 operation) depends on the direction by the rounding of that difference: the soup walks an edge the way the table does,
//      the indexed mesh from the lower corner to the upper one ("Indexed marching-cubes mesh"). ----
__device__ __forceinline__ void mc_vertex(float v0, float v1, const float* p0, const float* p1, float* pv, float* mu)
{
    *mu = 0.0f;
    if (fabsf(0.0f - v0) < MC_EPS) { pv[0] = p0[0]; pv[1] = p0[1]; pv[2] = p0[2]; }
    else if (fabsf(0.0f - v1) < MC_EPS) { pv[0] = p1[0]; pv[1] = p1[1]; pv[2] = p1[2]; }
    else { *mu = (0.0f - v0) / h2f(hsub(f2h(v1), f2h(v0))); for (int a = 0; a < 3; ++a) pv[a] = p0[a] + *mu * (p1[a] - p0[a]); }
}
// its colour from the two corners' stored colour words (three f16 channels in a uint2), vertexInterp_color :62-82 (Q13: only channel 0 is tested;
// p_color is an f16 variable, first assigned c1)
__device__ __forceinline__ void mc_colour(uint2 c0bits, uint2 c1bits, float mu, float* vc)
{
    const h16 c0[3] = { (h16)(c0bits.x & 0xffffu), (h16)(c0bits.x >> 16), (h16)(c0bits.y & 0xffffu) };
    const h16 c1[3] = { (h16)(c1bits.x & 0xffffu), (h16)(c1bits.x >> 16), (h16)(c1bits.y & 0xffffu) };
    for (int a = 0; a < 3; ++a) vc[a] = h2f(c0[a]);
    if (h2f(c0[0]) == 0.0f) { for (int a = 0; a < 3; ++a) vc[a] = h2f(c1[a]); }
    else if (!(h2f(c1[0]) == 0.0f)) { for (int a = 0; a < 3; ++a) vc[a] = h2f(f2h(h2f(c0[a]) + mu * h2f(hsub(c1[a], c0[a])))); }
}
// generate_normal :84-93 from the three f16 central differences: f16 normalisation (invlen = 1 / norm; invlen * v)
__device__ __forceinline__ void mc_normal(h16 n0, h16 n1, h16 n2, float* n)
{
    const h16 nrm = hsqrt(hadd(hadd(hmul(n0, n0), hmul(n1, n1)), hmul(n2, n2)));
    const h16 inv = f2h(1.0f / h2f(nrm));
    n[0] = h2f(hmul(inv, n0)); n[1] = h2f(hmul(inv, n1)); n[2] = h2f(hmul(inv, n2));
}
// ... around the tile entry (q0, q1, q2), the voxel nearest to the vertex: one of the edge's two corners, tile coordinates 1 .. 17.  Clamped to that
// range: a NaN map value makes a NaN vertex, whose nearest voxel is anything, and the differences must stay inside the tile.
__device__ __forceinline__ void mc_tile_normal(const uint16_t* s_t, int q0, int q1, int q2, float* n)
{
    q0 = min(max(q0, 1), MC_T - 2); q1 = min(max(q1, 1), MC_T - 2); q2 = min(max(q2, 1), MC_T - 2);
    mc_normal(hsub(s_t[mc_tile(q0 + 1, q1, q2)], s_t[mc_tile(q0 - 1, q1, q2)]), hsub(s_t[mc_tile(q0, q1 + 1, q2)], s_t[mc_tile(q0, q1 - 1, q2)]),
              hsub(s_t[mc_tile(q0, q1, q2 + 1)], s_t[mc_tile(q0, q1, q2 - 1)]), n);
}

// ---- scans ----
// inclusive scan over the wave's 64 lanes
__device__ __forceinline__ int mc_wave_scan(int v)
{
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane_id() >= d) v += o; }
    return v;
}
// exclusive scan of one value per thread over the block's 256 threads (s_w: 4 ints, free to reuse at the next barrier); *total = the block's sum
__device__ __forceinline__ int mc_block_scan(int mine, int* s_w, int* total)
{
    const int incl = mc_wave_scan(mine);
    __syncthreads();
    if (lane_id() == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    int first = incl - mine;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) first += s_w[w];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return first;
}

}  // namespace tsl

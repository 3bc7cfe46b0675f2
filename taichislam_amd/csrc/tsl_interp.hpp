// tsl_interp.hpp -- the trilinear cell read shared by the ESDF point queries (tsl_esdf_query.hip), the view renderer (tsl_render.hip) and the frame-to-model
// alignments (tsl_align.hip; tsl_align_rgbd.hip reads the colours of the same corners with tsdf_read_cell_lum): the cell of a
// coordinate, the pool bricks of its 8 corners, and the interpolant with its gradient in ONE fixed f32 order of evaluation, which is the contract
// tests/esdf_query_ref.py and tests/render_view_ref.py restate in numpy bit for bit (DESIGN.md sections 4.6 and 4.7).
#pragma once
#include "tsl_tsdf.hpp"

namespace tsl {

__device__ __forceinline__ float lerp_f(float a, float b, float t) { return a + t * (b - a); }

// the cell index of a coordinate: floor, clamped far outside any volume (the +1 corner cannot overflow; NaN lands on the clamp)
__device__ __forceinline__ int cell_floor(float u) { return (int)fmaxf(fminf(floorf(u), 16777216.0f), -16777216.0f); }

// Pool bricks of the 8 corners of the cell whose base voxel has brick id `bb` and local index (li, lj, lk); corner c = p << 2 | q << 1 | r is the voxel
// base + (p, q, r).  The +1 neighbour leaves the brick only from local index 15: only the distinct bricks are looked up (one lookup for 82 % of the
// cells).  `T` is the submap's table; the cell must lie in the volume with its +1 corner.
__device__ __forceinline__ void cell_bricks(const MapDev& M, const int* __restrict__ T, int bb, int li, int lj, int lk, int P[8])
{
    const bool cx = li == 15, cy = lj == 15, cz = lk == 15;
    const int dX = M.nbx * M.nbz, dY = M.nbz;
    int P0 = T[bb], P1 = 0, P2 = 0, P3 = 0, P4 = 0, P5 = 0, P6 = 0, P7 = 0;
    if (cz) P1 = T[bb + 1];
    if (cy) P2 = T[bb + dY];
    if (cy && cz) P3 = T[bb + dY + 1];
    if (cx) P4 = T[bb + dX];
    if (cx && cz) P5 = T[bb + dX + 1];
    if (cx && cy) P6 = T[bb + dX + dY];
    if (cx && cy && cz) P7 = T[bb + dX + dY + 1];
    if (!cz) { P1 = P0; P3 = P2; P5 = P4; P7 = P6; }
    if (!cy) { P2 = P0; P3 = P1; P6 = P4; P7 = P5; }
    if (!cx) { P4 = P0; P5 = P1; P6 = P2; P7 = P3; }
    P[0] = P0; P[1] = P1; P[2] = P2; P[3] = P3; P[4] = P4; P[5] = P5; P[6] = P6; P[7] = P7;
}
// data index of corner c (an absent brick reads brick 0, which exists: an in-bounds dummy read)
__device__ __forceinline__ size_t corner_voxel(const int P[8], int c, int li, int lj, int lk)
{
    const int l = ((((li + (c >> 2)) & 15)) << 8) | (((lj + ((c >> 1) & 1)) & 15) << 4) | ((lk + (c & 1)) & 15);
    return (size_t)(P[c] < 0 ? 0 : P[c]) * TSL_BRK3 + l;
}

// V[p << 2 | q << 1 | r] = c_pqr, f = the cell fractions; the order of evaluation is the contract
__device__ __forceinline__ float tri_value(const float V[8], float f0, float f1, float f2)
{
    const float c000 = V[0], c001 = V[1], c010 = V[2], c011 = V[3], c100 = V[4], c101 = V[5], c110 = V[6], c111 = V[7];
    return lerp_f(lerp_f(lerp_f(c000, c100, f0), lerp_f(c010, c110, f0), f1), lerp_f(lerp_f(c001, c101, f0), lerp_f(c011, c111, f0), f1), f2);
}
// the gradient of that interpolant per CELL (divide by the voxel size for a gradient per metre)
__device__ __forceinline__ void tri_grad(const float V[8], float f0, float f1, float f2, float* g0, float* g1, float* g2)
{
    const float c000 = V[0], c001 = V[1], c010 = V[2], c011 = V[3], c100 = V[4], c101 = V[5], c110 = V[6], c111 = V[7];
    *g0 = lerp_f(lerp_f(c100 - c000, c110 - c010, f1), lerp_f(c101 - c001, c111 - c011, f1), f2);
    *g1 = lerp_f(lerp_f(c010 - c000, c110 - c100, f0), lerp_f(c011 - c001, c111 - c101, f0), f2);
    *g2 = lerp_f(lerp_f(c001 - c000, c101 - c100, f0), lerp_f(c011 - c010, c111 - c110, f0), f1);
}

// the 8 corner values of the cell with base voxel (b0, b1, b2); false when a corner is outside the volume, in an unallocated brick or not observed
__device__ __forceinline__ bool tsdf_read_cell(const MapDev& M, const int* __restrict__ T, int b0, int b1, int b2, float V[8])
{
    if (!(in_volume(M, b0, b1, b2) && in_volume(M, b0 + 1, b1 + 1, b2 + 1))) return false;
    int l000; const int bb = brick_of(M, b0, b1, b2, &l000);
    const int li = l000 >> 8, lj = (l000 >> 4) & 15, lk = l000 & 15;
    int P[8]; cell_bricks(M, T, bb, li, lj, lk, P);
    // all 16 gathers are issued before any is used: two dependent latencies per sample (table, then data)
    uint32_t tw[8]; int ob[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { const size_t v = corner_voxel(P, c, li, lj, lk); tw[c] = M.tw[v]; ob[c] = M.obs[v]; }
    bool known = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) { known = known && P[c] >= 0 && ob[c] > 0; V[c] = h2f((h16)(tw[c] & 0xffffu)); }
    return known;
}

// the luminance of a stored colour {r | g << 16, b}: ((77 r + 150 g) + 29 b) / 256 of the three f16 channels converted to f32
__device__ __forceinline__ float voxel_luminance(uint2 c)
{
    const float r = h2f((h16)(c.x & 0xffffu)), g = h2f((h16)(c.x >> 16)), b = h2f((h16)(c.y & 0xffffu));
    return ((77.0f * r + 150.0f * g) + 29.0f * b) / 256.0f;
}

// tsdf_read_cell of a textured map (M.col is not null) that also returns the luminances Y of the 8 corners: all 24 gathers -- tw, obs and one 8-byte
// load of col per corner -- are issued before any is used.  The values of an unknown cell mean nothing.
__device__ __forceinline__ bool tsdf_read_cell_lum(const MapDev& M, const int* __restrict__ T, int b0, int b1, int b2, float V[8], float Y[8])
{
    if (!(in_volume(M, b0, b1, b2) && in_volume(M, b0 + 1, b1 + 1, b2 + 1))) return false;
    int l000; const int bb = brick_of(M, b0, b1, b2, &l000);
    const int li = l000 >> 8, lj = (l000 >> 4) & 15, lk = l000 & 15;
    int P[8]; cell_bricks(M, T, bb, li, lj, lk, P);
    const uint2* __restrict__ col = reinterpret_cast<const uint2*>(M.col);
    uint32_t tw[8]; int ob[8]; uint2 cc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { const size_t v = corner_voxel(P, c, li, lj, lk); tw[c] = M.tw[v]; ob[c] = M.obs[v]; cc[c] = col[v]; }
    bool known = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) { known = known && P[c] >= 0 && ob[c] > 0; V[c] = h2f((h16)(tw[c] & 0xffffu)); Y[c] = voxel_luminance(cc[c]); }
    return known;
}

}  // namespace tsl

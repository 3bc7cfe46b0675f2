// tsl_mesh.hip -- marching cubes over every active TSDF voxel.  Replaces MarchingCubeMesher.generate_mesh_kernel and
// helpers (taichi_slam/mapping/marching_cube_mesher.py:44-187, reference root).
//
// The triangle soup of generate_mesh: three rows per triangle, placed by an atomic on the facet counter.  The cell, tile and vertex rules are those
// of tsl_mc.hpp; what is here is how the two kernels read the map, split the work and reserve their rows.
#include "tsl_mc.hpp"

namespace tsl {

__device__ __forceinline__ float rd_tsdf(const MapDev& M, int s, int i, int j, int k, int* obs)
{
    if (!in_volume(M, i, j, k)) { *obs = 0; return 0.0f; }                   // reading outside / an inactive cell yields 0 (A7)
    int l; const int b = brick_of(M, i, j, k, &l);
    const int p = pool_lookup_ro(M, s, b);
    if (p < 0) { *obs = 0; return 0.0f; }
    const size_t v = (size_t)p * TSL_BRK3 + l;
    *obs = M.obs[v];
    return h2f((h16)(M.tw[v] & 0xffffu));
}
__device__ __forceinline__ h16 rd_tsdf_h(const MapDev& M, int s, int i, int j, int k)
{
    if (!in_volume(M, i, j, k)) return 0;
    int l; const int b = brick_of(M, i, j, k, &l);
    const int p = pool_lookup_ro(M, s, b);
    return p < 0 ? (h16)0 : (h16)(M.tw[(size_t)p * TSL_BRK3 + l] & 0xffffu);
}
// generate_normal :84-93 with the central differences read through the brick table
__device__ __forceinline__ void gen_normal(const MapDev& M, int s, const float* p, float* out)
{
    const int q0 = (int)rnd_f(p[0]), q1 = (int)rnd_f(p[1]), q2 = (int)rnd_f(p[2]);
    mc_normal(hsub(rd_tsdf_h(M, s, q0 + 1, q1, q2), rd_tsdf_h(M, s, q0 - 1, q1, q2)), hsub(rd_tsdf_h(M, s, q0, q1 + 1, q2), rd_tsdf_h(M, s, q0, q1 - 1, q2)),
              hsub(rd_tsdf_h(M, s, q0, q1, q2 + 1), rd_tsdf_h(M, s, q0, q1, q2 - 1)), out);
}

__device__ __forceinline__ uint2 rd_col(const MapDev& M, int s, int i, int j, int k)
{
    if (!in_volume(M, i, j, k)) return make_uint2(0u, 0u);
    int l; const int b = brick_of(M, i, j, k, &l);
    const int p = pool_lookup_ro(M, s, b);
    return p < 0 ? make_uint2(0u, 0u) : reinterpret_cast<const uint2*>(M.col)[(size_t)p * TSL_BRK3 + l];
}

// ---- any step, every value through the brick table (step > 1 reaches beyond the brick's halo; at step 1 the mesh_gather option selects it) ----
// One thread per voxel of every allocated brick.  The 8 corner values of the cell are kept per thread in LDS (dynamic edge -> corner indexing would
// otherwise spill to scratch), and triangles are emitted with a wave-level scan of the per-voxel triangle counts and ONE atomic per wave on the
// facet counter (the reference does one atomic per triangle, :114).
__global__ void __launch_bounds__(256) k_marching_cubes(MapDev M, int nused, int step, float thres, float vs, long long max_tri,
                                                        float* __restrict__ verts, float* __restrict__ normals, float* __restrict__ colors, int* counter)
{
    __shared__ unsigned long long s_tri[256];
    __shared__ float s_val[8][256];
    s_tri[threadIdx.x] = MC_TRI_PACKED[threadIdx.x];
    __syncthreads();
    for (int p = blockIdx.x; p < nused; p += gridDim.x) {
        const int owner = M.owner[p];
        const int s = owner / M.nb3, b = owner - s * M.nb3;
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        for (int l0 = 0; l0 < TSL_BRK3; l0 += 256) {
            const int l = l0 + threadIdx.x;
            const size_t v = (size_t)p * TSL_BRK3 + l;
            const int i = bi * 16 + (l >> 8) - M.hN, j = bj * 16 + ((l >> 4) & 15) - M.hN, k = bk * 16 + (l & 15) - M.hNz;
            int ntri = 0, cube = 0;
            unsigned long long tri = ~0ull;
            if (M.obs[v] > 0 && h2f((h16)(M.tw[v] & 0xffffu)) < thres) {                         // :184
                bool bad = false;
                for (int q = 0; q < 8; ++q) {                                                     // :133-138
                    int d[3]; mc_corner(q, d);
                    int o; const float val = rd_tsdf(M, s, i + d[0] * step, j + d[1] * step, k + d[2] * step, &o);
                    s_val[q][threadIdx.x] = val;
                    if (o == 0) bad = true;
                    if (val < 0.0f) cube |= 1 << q;                                               // :141-144
                }
                if (!bad) { tri = s_tri[cube]; ntri = mc_ntri(tri); }
            }
            // wave-level emission: inclusive scan of ntri, one atomic per wave
            const int inc = mc_wave_scan(ntri);
            const int wave_total = __shfl(inc, 63);
            int base = 0;
            if (wave_total) {
                if (lane_id() == 63) base = __hip_atomic_fetch_add(counter, wave_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                base = __shfl(base, 63);
            }
            long long idx = (long long)base + inc - ntri;
            for (int t = 0; t < 5 && ntri; ++t) {
                if (((tri >> (12 * t)) & 0xfull) == 0xfull) continue;
                if (idx < max_tri) {                                                              // Q10: clamp by the returned index
                    for (int q = 0; q < 3; ++q) {
                        const int e = (int)((tri >> (4 * (3 * t + q))) & 0xfull);
                        int ca, cb; mc_edge_corners(e, &ca, &cb);
                        int da[3], db[3]; mc_corner(ca, da); mc_corner(cb, db);
                        const float p0[3] = { (float)(i + da[0] * step), (float)(j + da[1] * step), (float)(k + da[2] * step) };
                        const float p1[3] = { (float)(i + db[0] * step), (float)(j + db[1] * step), (float)(k + db[2] * step) };
                        float pv[3], mu;
                        mc_vertex(s_val[ca][threadIdx.x], s_val[cb][threadIdx.x], p0, p1, pv, &mu);
                        const size_t o = ((size_t)idx * 3 + q) * 3;
                        if (colors) {
                            float vc[3];
                            mc_colour(rd_col(M, s, i + da[0] * step, j + da[1] * step, k + da[2] * step), rd_col(M, s, i + db[0] * step, j + db[1] * step, k + db[2] * step), mu, vc);
                            for (int a = 0; a < 3; ++a) colors[o + a] = vc[a];
                        }
                        float nn[3]; gen_normal(M, s, pv, nn);                                   // :100-102
                        for (int a = 0; a < 3; ++a) { verts[o + a] = pv[a] * vs; normals[o + a] = nn[a]; }   // :41-42,:97-99
                    }
                }
                ++idx;
            }
        }
    }
}


// ---- step 1 (every caller of the reference: scripts/taichislam_node.py:338, tests/marching_cube_test.py:21): brick + halo staged in LDS ----
// The 19^3 tile of tsl_mc.hpp (14.3 KiB) is gathered ONCE per brick through the 27 surrounding brick-table entries; the corner reads (8 per voxel)
// and the normal reads (6 per vertex, up to 90 per voxel) then come from LDS instead of one table lookup + one scattered 4-byte load each.
// Emission: the brick's triangles are counted first (pass 1), reserved with ONE atomic, then written (pass 2).
#define MC_SLAB 2         // x-layers of a brick per work item of k_marching_cubes_lds
#define MC_LIST 4096             // triangles listed in LDS at a time

// the brick sign flags by which k_marching_cubes_lds skips a brick before it gathers the tile from 27 bricks
__global__ void __launch_bounds__(256) k_mc_summary(MapDev M, int nused, uint32_t* __restrict__ flags, int* counter)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0;                  // :182 (the triangle counter of the mesh that follows)
    if (nused < 0) nused = min(M.pool_top[0], M.max_bricks);                // (the bricks in use, read here: the host does not wait for the count)
    for (int p = blockIdx.x; p < nused; p += gridDim.x) {
        const uint32_t f = mc_brick_flags(M, p);
        if (threadIdx.x == 0) flags[p] = f;
    }
}

__global__ void __launch_bounds__(256) k_marching_cubes_lds(MapDev M, int nused, float thres, float vs, long long max_tri,
                                                            float* __restrict__ verts, float* __restrict__ normals, float* __restrict__ colors, int* counter,
                                                            const uint32_t* __restrict__ flags)
{
    __shared__ int s_skip;
    if (nused < 0) nused = min(M.pool_top[0], M.max_bricks);
    __shared__ unsigned long long s_tri[256];
    __shared__ uint32_t s_list[MC_LIST];
    __shared__ uint16_t s_t[MC_T3];
    __shared__ uint32_t s_o[MC_OWORDS];
    __shared__ int s_nb[27];
    __shared__ int s_wtot[5], s_base;
    s_tri[threadIdx.x] = MC_TRI_PACKED[threadIdx.x];
    // a work item is a SLAB of a brick, MC_SLAB of its 16 x-layers: the surface crosses few bricks -- 56 of the 442 of a 128^3 sphere -- and a brick
    // per workgroup left three quarters of the CUs idle while those few walked their cells and emitted their vertices (one wave per SIMD: every
    // dependent instruction at its full latency)
    for (int item = blockIdx.x; item < nused * (16 / MC_SLAB); item += gridDim.x) {
        const int p = item / (16 / MC_SLAB), x0 = (item % (16 / MC_SLAB)) * MC_SLAB;
        const int owner = M.owner[p];
        const int s = owner / M.nb3, b = owner - s * M.nb3;
        const int bk = b % M.nbz, bj = (b / M.nbz) % M.nbx, bi = b / (M.nbz * M.nbx);
        // the tile entries of the slab's cells, their corners and the normals' neighbours: x-layers x0 .. x0 + MC_SLAB + 2 of the 19^3 tile
        mc_gather(M, flags, nused, p, s, bi, bj, bk, x0 * MC_T * MC_T, (x0 + MC_SLAB + 3) * MC_T * MC_T, s_nb, s_t, s_o, &s_skip);
        if (s_skip) continue;                                                // (uniform)
        // ---- pass 1: the brick's triangle count.  ONE reservation per brick (a reservation per wave and 256 cells -- the first form of
        //      this kernel -- put ~2 000 returning atomics on one address per mesh, ~12 ns each in the L2).  Thread t has the cells
        //      (x0 .. x0 + MC_SLAB - 1, t >> 4, t & 15).  The scan is this kernel's own: thread 0 sums the waves and reserves between the same two barriers,
        //      where mc_block_scan would need a third ----
        const int cy = (int)threadIdx.x >> 4, cz = (int)threadIdx.x & 15;
        int mine = 0;
        for (int lx = x0; lx < x0 + MC_SLAB; ++lx) if (mc_valid(s_t, s_o, lx, cy, cz, thres)) mine += mc_ntri(s_tri[mc_case(s_t, lx, cy, cz)]);
        const int incl = mc_wave_scan(mine);
        if (lane_id() == 63) s_wtot[threadIdx.x >> 6] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tot = s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
            s_wtot[4] = tot;
            s_base = tot ? __hip_atomic_fetch_add(counter, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        }
        __syncthreads();
        const int total = s_wtot[4];
        if (total == 0) continue;                                         // (uniform) nothing to emit from this brick
        int first = incl - mine;                                          // this thread's first triangle among the brick's
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) first += s_wtot[w];
        // ---- pass 2: the triangles as a LIST in LDS (cell | triangle of the case << 12 | case << 16, in the order of the reservation), then
        //      one VERTEX per thread and step.  Walking the cells again and letting each thread emit its own cells' triangles (the first
        //      form) keeps 5 - 10 % of the lanes busy -- the surface crosses few of a wave's 64 cells -- through 15 serial vertex slots of
        //      ~600 instructions (the f16 normal arithmetic is emulated bit for bit): 148 us per mesh of a 128^3 sphere, this way 1/4. ----
        for (int w0 = 0; w0 < total; w0 += MC_LIST) {                     // (one window unless the brick is noise: MC_LIST triangles at a time)
            if (w0) __syncthreads();
            int at = first;
            for (int lx = x0; lx < x0 + MC_SLAB && mine; ++lx) {
                if (!mc_valid(s_t, s_o, lx, cy, cz, thres)) continue;
                const int cube = mc_case(s_t, lx, cy, cz), n = mc_ntri(s_tri[cube]);
                for (int t = 0; t < n; ++t, ++at)
                    if (at >= w0 && at < w0 + MC_LIST) s_list[at - w0] = (uint32_t)(lx << 8 | (int)threadIdx.x) | (uint32_t)t << 12 | (uint32_t)cube << 16;
            }
            __syncthreads();
            const int nv = 3 * min(total - w0, MC_LIST);
            for (int v = threadIdx.x; v < nv; v += 256) {
                const uint32_t en = s_list[v / 3];
                const int q = v % 3, l = (int)(en & 0xfffu), t = (int)((en >> 12) & 7u);
                const long long idx = (long long)s_base + w0 + v / 3;
                if (idx >= max_tri) continue;                                                     // Q10: clamp by the returned index
                const unsigned long long tri = s_tri[en >> 16];
                // the triangles of a case are its non-empty slots in order: slot of the t-th one
                int slot = 0;
                for (int u = 0, seen = 0; u < 5; ++u) if (((tri >> (12 * u)) & 0xfull) != 0xfull) { if (seen == t) slot = u; ++seen; }
                const int lx = l >> 8, ly = (l >> 4) & 15, lz = l & 15;
                const int i = bi * 16 + lx - M.hN, j = bj * 16 + ly - M.hN, k = bk * 16 + lz - M.hNz;
                const int e = (int)((tri >> (4 * (3 * slot + q))) & 0xfull);
                int ca, cb; mc_edge_corners(e, &ca, &cb);                                          // the corners in the table's order
                int da[3], db[3]; mc_corner(ca, da); mc_corner(cb, db);
                const float p0[3] = { (float)(i + da[0]), (float)(j + da[1]), (float)(k + da[2]) };
                const float p1[3] = { (float)(i + db[0]), (float)(j + db[1]), (float)(k + db[2]) };
                float pv[3], mu, nn[3];
                mc_vertex(h2f(s_t[mc_tile(lx + 1 + da[0], ly + 1 + da[1], lz + 1 + da[2])]), h2f(s_t[mc_tile(lx + 1 + db[0], ly + 1 + db[1], lz + 1 + db[2])]), p0, p1, pv, &mu);
                const size_t o = ((size_t)idx * 3 + q) * 3;
                if (colors) {                                                            // (colours stay in HBM)
                    float vc[3];
                    mc_colour(rd_col(M, s, i + da[0], j + da[1], k + da[2]), rd_col(M, s, i + db[0], j + db[1], k + db[2]), mu, vc);
                    for (int a = 0; a < 3; ++a) colors[o + a] = vc[a];
                }
                mc_tile_normal(s_t, (int)rnd_f(pv[0]) - i + lx + 1, (int)rnd_f(pv[1]) - j + ly + 1, (int)rnd_f(pv[2]) - k + lz + 1, nn);
                verts[o] = pv[0] * vs; verts[o + 1] = pv[1] * vs; verts[o + 2] = pv[2] * vs;                  // :41-42,:97-99
                normals[o] = nn[0]; normals[o + 1] = nn[1]; normals[o + 2] = nn[2];                           // :100-102
            }
        }
    }
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_mesh_generate(tsl_tsdf* m, int step, float surface_thres, int64_t max_tri, int32_t* n_tri)
{
    TSL_REQUIRE(m && n_tri, "mesh_generate: null argument"); TSL_REQUIRE(step >= 1 && max_tri > 0, "mesh_generate: bad step / max_triangles");
    TSL_HIP(hipSetDevice(m->device));
    int rc;
    if (m->mesh_cap < max_tri) {
        if (m->mesh_v) { (void)hipFree(m->mesh_v); (void)hipFree(m->mesh_n); if (m->mesh_c) (void)hipFree(m->mesh_c); m->mesh_v = m->mesh_n = m->mesh_c = nullptr; }
        if ((rc = dev_alloc(m, (void**)&m->mesh_v, sizeof(float) * 9 * (size_t)max_tri, 0))) return rc;
        if ((rc = dev_alloc(m, (void**)&m->mesh_n, sizeof(float) * 9 * (size_t)max_tri, 0))) return rc;
        if (m->M.col) { if ((rc = dev_alloc(m, (void**)&m->mesh_c, sizeof(float) * 9 * (size_t)max_tri, 0))) return rc; }
        m->mesh_cap = max_tri;
    }
    if (!m->mesh_count) { if ((rc = dev_alloc(m, (void**)&m->mesh_count, sizeof(int) * 4, 0))) return rc; }
    const bool tiles = step == 1 && !m->mesh_gather;     // the LDS-tile kernel: it reads the number of bricks in use on the device (one host round trip per mesh less)
    int nused = 0; if (!tiles && (rc = tsl_tsdf_bricks_in_use(m, &nused))) return rc;
    if (!m->mesh_flags) { if ((rc = dev_alloc(m, (void**)&m->mesh_flags, sizeof(uint32_t) * (size_t)m->M.max_bricks, 0))) return rc; }
    (void)ms(m);                                         // the queued frames are issued first: the mesh is of the map behind them
    prof_begin(m, TSL_K_MESH);
    if (!tiles) TSL_HIP(hipMemsetAsync(m->mesh_count, 0, sizeof(int), ms(m)));                          // :182
    if (tiles) {
        const int g1 = m->M.max_bricks < 2048 ? m->M.max_bricks : 2048, g2 = m->M.max_bricks < 1024 ? m->M.max_bricks * (16 / MC_SLAB) : 8192;
        hipLaunchKernelGGL(k_mc_summary, dim3(g1), dim3(256), 0, ms(m), m->M, -1, m->mesh_flags, m->mesh_count);
        hipLaunchKernelGGL(k_marching_cubes_lds, dim3(g2), dim3(256), 0, ms(m), m->M, -1,
                           surface_thres, m->P.vs, (long long)max_tri, m->mesh_v, m->mesh_n, m->M.col ? m->mesh_c : (float*)nullptr, m->mesh_count,
                           (const uint32_t*)m->mesh_flags);
    }
    else if (nused > 0)             // coarser meshes (step > 1) reach beyond the brick's halo: every value through the brick table
        hipLaunchKernelGGL(k_marching_cubes, dim3(nused < 16384 ? nused : 16384), dim3(256), 0, ms(m), m->M, nused, step,
                           surface_thres, m->P.vs, (long long)max_tri, m->mesh_v, m->mesh_n, m->M.col ? m->mesh_c : (float*)nullptr, m->mesh_count);
    prof_end(m);
    TSL_HIP(hipGetLastError());
    TSL_HIP(hipMemcpyAsync(m->h_ints, m->mesh_count, sizeof(int), hipMemcpyDeviceToHost, ms(m)));
    TSL_HIP(hipStreamSynchronize(ms(m)));
    *n_tri = m->h_ints[0];
    return TSL_OK;
}

int tsl_mesh_read(tsl_tsdf* m, float* verts, float* normals, float* colors, int64_t n_vertices)
{
    TSL_REQUIRE(m, "mesh_read: null handle"); TSL_REQUIRE(n_vertices >= 0 && n_vertices <= 3 * m->mesh_cap, "mesh_read: more vertices than the mesh buffers hold");
    TSL_HIP(hipSetDevice(m->device));
    TSL_HIP(hipStreamSynchronize(ms(m)));
    if (n_vertices == 0) return TSL_OK;
    if (verts) TSL_HIP(hipMemcpy(verts, m->mesh_v, sizeof(float) * 3 * (size_t)n_vertices, hipMemcpyDeviceToHost));
    if (normals) TSL_HIP(hipMemcpy(normals, m->mesh_n, sizeof(float) * 3 * (size_t)n_vertices, hipMemcpyDeviceToHost));
    if (colors && m->mesh_c) TSL_HIP(hipMemcpy(colors, m->mesh_c, sizeof(float) * 3 * (size_t)n_vertices, hipMemcpyDeviceToHost));
    return TSL_OK;
}

/* mesh_vertices / mesh_normals / mesh_colors as DEVICE pointers (f32 [3 * max_triangles][3]; colours NULL for untextured maps) and the
 * triangle count of the last tsl_mesh_generate -- taichislam_node.py:342 hands the mesh to the renderer without a host copy.  The
 * pointers change when a later tsl_mesh_generate asks for a larger max_triangles. */
int tsl_mesh_buffers_dev(tsl_tsdf* m, void** verts_dev, void** normals_dev, void** colors_dev, int32_t* n_tri)
{
    TSL_REQUIRE(m, "mesh_buffers_dev: null handle"); TSL_REQUIRE(m->mesh_v && m->mesh_count, "mesh_buffers_dev: call tsl_mesh_generate first");
    TSL_HIP(hipSetDevice(m->device));
    if (verts_dev) *verts_dev = m->mesh_v; if (normals_dev) *normals_dev = m->mesh_n; if (colors_dev) *colors_dev = m->mesh_c;
    TSL_HIP(hipMemcpyAsync(m->h_ints, m->mesh_count, sizeof(int), hipMemcpyDeviceToHost, ms(m)));
    TSL_HIP(hipStreamSynchronize(ms(m)));
    if (n_tri) *n_tri = m->h_ints[0];
    return TSL_OK;
}

}  // extern "C"

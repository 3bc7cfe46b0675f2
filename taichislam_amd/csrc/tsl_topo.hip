// tsl_topo.hip -- the ray and facelet work of TopoGraphGen (taichi_slam/mapping/topo_graph.py, reference root): the skeleton graph of free space as convex
// polyhedra around sample points.  Read-only on the map.  The definition is the SEQUENTIAL reading of the reference (include/taichislam_hip.h, "free-space
// topology graph"): every loop in ascending index order, f32 arithmetic in the order the source writes it, no contraction.
//   k_topo_rays      a batch of combined rays (topo_graph.py:472-507): one wave per ray.  The node loop and the sphere test are wave-uniform, the lanes stride
//                    over a node's facelets, one wave reduction picks the least (t, facelet index) -- which is what the sequential strict `<` keeps -- and the
//                    map walk puts one step on each lane, 64 steps at a time in ascending order, one ballot per chunk: the steps are independent of each
//                    other, so the first set bit of the first chunk that has one is the step at which the serial walk of tsl_query.hip stops.
//   k_topo_facelets  the facelets of one hull (Facelet.init :36-50, detect_facelet_frontier :324-342): one wave per facelet writes it into the store, asks the
//                    two point queries and casts the frontier ray through the same code.  The rays see the nodes made BEFORE this one only (the reference
//                    raises num_nodes after the loop, :442), so a launch never reads what it writes.
// As in tsl_nav_corridor.hip: no atomic decides an output, every loop has a bound known at launch, every refusal comes before any launch.
#include "tsl_query.hpp"
#include "tsl_stage.hpp"
#include <cfloat>
#include <mutex>

#define TOPO_MAX_NODES 4096               // max_map_node, topo_graph.py:159
#define TOPO_MAX_RAYS (1 << 20)
#define TOPO_MAX_POLY 4096                // facelets one call may add (a hull of 512 points has at most 1020)
#define TOPO_MAX_STEPS 1048576.0f         // steps of one map walk

struct tsl_topo {
    tsl_tsdf* map;                         // null once the map was destroyed: every call but destroy is refused from then on
    int device, coll_det_num; float max_raycast_dist; int64_t max_facelets;
    int64_t nf, cap_f; int nn, cap_n;
    float *tri, *v0, *e1, *e2, *nrm, *ctr; int* poly;      // facelet store, structure of arrays: [cap_f][9] the three vertices, [cap_f][3] each, [cap_f]
    float* nctr; int* nrange;                              // node store: [cap_n][3] centre, [cap_n][2] first facelet, one past the last
    void* sbuf; size_t sbuf_bytes;                         // staging of the host-pointer forms
};

namespace tsl {

struct TopoDev { float *v0, *e1, *e2, *nrm, *ctr; int* poly; float* tri; const float* nctr; const int* nrange; int nn; float max_raycast_dist; };
struct MapQ { int s; float vs_f, vs_len, thres; };          // the active slot, the voxel size as the map divides by it / as raycast multiplies by it, the surface threshold

static std::mutex g_topo_mu;
static std::vector<tsl_topo*> g_topos;

__device__ __forceinline__ void cross3(const float* a, const float* b, float* c)
{ c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; }
__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// v.normalized(): v / sqrt(x * x + y * y + z * z), the sum left to right, the division per component
__device__ __forceinline__ void normalize3(float* v)
{ const float n = sqrt_rn((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n; }
__device__ __forceinline__ float canon(float x) { return x != x ? __uint_as_float(0x7fc00000u) : x; }

// rayTriangleIntersect  topo_graph.py:52-70
__device__ __forceinline__ bool tri_hit(const TopoDev& T, size_t i, const float* P, const float* w, float* t)
{
    const float e1[3] = { T.e1[i * 3], T.e1[i * 3 + 1], T.e1[i * 3 + 2] }, e2[3] = { T.e2[i * 3], T.e2[i * 3 + 1], T.e2[i * 3 + 2] };
    float q[3]; cross3(w, e2, q);
    const float a = dot3(e1, q);
    *t = 0.0f;
    if (!(fabsf(a) > 0.00001f)) return false;
    const float s[3] = { (P[0] - T.v0[i * 3]) / a, (P[1] - T.v0[i * 3 + 1]) / a, (P[2] - T.v0[i * 3 + 2]) / a };
    float r[3]; cross3(s, e1, r);
    const float b0 = dot3(s, q), b1 = dot3(r, w), b2 = (1.0f - b0) - b1;
    *t = dot3(e2, r);
    return !(b0 < 0.0f || b1 < 0.0f || b2 < 0.0f);
}

// detect_collision_facelets  :472-488, by one wave: the least t in (backward, max_dist) over the nodes k != skip inside the reach; the lowest facelet among equals
__device__ __forceinline__ bool wave_facelets(const TopoDev& T, const float* P, const float* w, float max_dist, float backward, int skip, float* best_t, int* best_poly)
{
    const int lane = lane_id();
    float bt = max_dist; int bi = 0x7fffffff;
    const float reach = max_dist + T.max_raycast_dist;
    for (int k = 0; k < T.nn; ++k) {
        if (k == skip) continue;
        const float dx = P[0] - T.nctr[k * 3], dy = P[1] - T.nctr[k * 3 + 1], dz = P[2] - T.nctr[k * 3 + 2];
        if (!(sqrt_rn((dx * dx + dy * dy) + dz * dz) < reach)) continue;
        const int e = T.nrange[k * 2 + 1];
        for (int i = T.nrange[k * 2] + lane; i < e; i += 64) {
            float t;
            if (tri_hit(T, (size_t)i, P, w, &t) && backward < t && t < bt) { bt = t; bi = i; }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const float ot = __shfl_xor(bt, d); const int oi = __shfl_xor(bi, d);
        if (ot < bt || (ot == bt && oi < bi)) { bt = ot; bi = oi; }
    }
    *best_t = bt;
    *best_poly = bi != 0x7fffffff ? T.poly[bi] : -1;
    return bi != 0x7fffffff;
}

// BaseMap.raycast (mapping_common.py:165-178) as tsl_tsdf_query_raycast walks it, by one wave; a length below one voxel (a negative one too) makes no step
__device__ __forceinline__ bool wave_walk(const MapDev& M, const MapQ& Q, float maxd, const float* pos, const float* dir, float* x, float* len)
{
    const int lane = lane_id();
    const int steps = (int)(maxd / Q.vs_f);
    x[0] = x[1] = x[2] = 0.0f; *len = 0.0f;
    for (int base = 0; base < steps; base += 64) {
        const int jj = base + lane;
        const float l = (float)jj * Q.vs_len;
        float y[3];
        for (int a = 0; a < 3; ++a) y[a] = dir[a] * l + pos[a];
        bool occ = false;
        if (jj < steps) {
            const float q0 = y[0] / Q.vs_f, q1 = y[1] / Q.vs_f, q2 = y[2] / Q.vs_f;
            occ = (cell_fits(q0) && cell_fits(q1) && cell_fits(q2)) ? q_occupied(M, Q.s, rnd_i(q0), rnd_i(q1), rnd_i(q2), Q.thres) : 0.0f < Q.thres;
        }
        const unsigned long long m = __ballot(occ);
        if (m) {
            const int src = (int)__builtin_ctzll(m);
            for (int a = 0; a < 3; ++a) x[a] = __shfl(y[a], src);
            *len = __shfl(l, src);
            return true;
        }
    }
    if (steps > 0) { const float l = (float)(steps - 1) * Q.vs_len; *len = l; for (int a = 0; a < 3; ++a) x[a] = dir[a] * l + pos[a]; }
    return false;
}

// raycast  :490-507 (facelets_only: detect_collision_facelets alone, type 1)
__device__ __forceinline__ void topo_ray(const MapDev& M, const MapQ& Q, const TopoDev& T, const float* pos, const float* dir, float max_dist, float backward, int skip,
                                         bool facelets_only, bool* hit, int* type, float* x, float* len, int* poly)
{
    float lc; const bool sp = wave_facelets(T, pos, dir, max_dist, backward, skip, &lc, poly);
    for (int a = 0; a < 3; ++a) x[a] = pos[a] + dir[a] * lc;
    *hit = sp; *type = 1; *len = lc;
    if (facelets_only) return;
    float xm[3], lm;
    const bool sm = wave_walk(M, Q, sp ? lc : max_dist, pos, dir, xm, &lm);
    if (!sp || (sm && lm < lc)) { for (int a = 0; a < 3; ++a) x[a] = xm[a]; *len = lm; *type = 0; *hit = sm; }
}

__global__ void __launch_bounds__(256) k_topo_rays(MapDev M, MapQ Q, TopoDev T, const float* __restrict__ pos, const float* __restrict__ dir, const int* __restrict__ skip,
                                                   int n, float max_dist, float backward, int flags, uint8_t* hit, uint8_t* type, float* end_xyz, float* len, int* poly)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n) return;                                                        // whole waves leave
    const float P[3] = { pos[(size_t)q * 3], pos[(size_t)q * 3 + 1], pos[(size_t)q * 3 + 2] }, w[3] = { dir[(size_t)q * 3], dir[(size_t)q * 3 + 1], dir[(size_t)q * 3 + 2] };
    bool h; int ty, pl; float x[3], l;
    topo_ray(M, Q, T, P, w, max_dist, backward, skip ? skip[q] : -1, (flags & 1) != 0, &h, &ty, x, &l, &pl);
    if (lane_id() == 0) {
        hit[q] = h ? 1 : 0; type[q] = (uint8_t)ty; len[q] = l; poly[q] = pl;
        for (int a = 0; a < 3; ++a) end_xyz[(size_t)q * 3 + a] = canon(x[a]);
    }
}

// is_pos_occupy (mode 0) / is_pos_unobserved (mode 1) with the rule of k_query_points for positions that are not finite or have no int cell
__device__ __forceinline__ bool point_query(const MapDev& M, const MapQ& Q, int mode, const float* p)
{
    const float q0 = p[0] / Q.vs_f, q1 = p[1] / Q.vs_f, q2 = p[2] / Q.vs_f;
    if (!(cell_fits(q0) && cell_fits(q1) && cell_fits(q2))) return mode == 1 ? true : 0.0f < Q.thres;
    float t; int o; q_read(M, Q.s, rnd_i(q0), rnd_i(q1), rnd_i(q2), &t, &o);
    return mode == 1 ? o == 0 : t < Q.thres;
}

// why a facelet is no frontier: 1 its centre is unobserved, 2 the voxel in front of it is occupied, 3 the frontier ray hit something
__global__ void __launch_bounds__(256) k_topo_facelets(MapDev M, MapQ Q, TopoDev T, const float* __restrict__ tris, int nf, int first, int node, float sx, float sy, float sz,
                                                       float max_dist, uint8_t* is_frontier, uint8_t* reason, int* neigh)
{
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= nf) return;
    const bool lead = lane_id() == 0;
    const float* tv = tris + (size_t)f * 9;
    float v0[3], v1[3], v2[3], e1[3], e2[3], c[3], nv[3], nn[3];
    for (int a = 0; a < 3; ++a) { v0[a] = tv[a]; v1[a] = tv[3 + a]; v2[a] = tv[6 + a]; }
    const float st[3] = { sx, sy, sz };
    for (int a = 0; a < 3; ++a) {                                              // Facelet.init  :36-50, naive_norm :396
        e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a];
        const float sum = (v0[a] + v1[a]) + v2[a];
        c[a] = sum / 3.0f;
        nv[a] = sum - 3.0f * st[a];
    }
    normalize3(nv);
    cross3(e1, e2, nn); normalize3(nn);
    if (dot3(nn, nv) < 0.0f) for (int a = 0; a < 3; ++a) nn[a] = -nn[a];
    const size_t g = (size_t)first + f;
    if (lead) {
        for (int a = 0; a < 9; ++a) T.tri[g * 9 + a] = tv[a];
        for (int a = 0; a < 3; ++a) { T.v0[g * 3 + a] = v0[a]; T.e1[g * 3 + a] = e1[a]; T.e2[g * 3 + a] = e2[a]; T.nrm[g * 3 + a] = nn[a]; T.ctr[g * 3 + a] = c[a]; }
        T.poly[g] = node;
    }
    // detect_facelet_frontier  :324-342; is_near_pos_occupy(center, 0) loops over range(-0, 0), which is empty: false
    int why = 0, nb = -1;
    if (point_query(M, Q, 1, c)) why = 1;
    else {
        float p[3];
        for (int a = 0; a < 3; ++a) p[a] = c[a] + nn[a] * Q.vs_len;
        if (point_query(M, Q, 0, p)) why = 2;
        else {
            bool h; int ty, pl; float x[3], l;
            topo_ray(M, Q, T, p, nn, max_dist, -0.01f, -1, false, &h, &ty, x, &l, &pl);
            if (h) { why = 3; if (ty == 1) nb = pl; }
        }
    }
    if (lead) { is_frontier[f] = why == 0 ? 1 : 0; if (reason) reason[f] = (uint8_t)why; neigh[f] = nb; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
void topo_map_gone(tsl_tsdf* m)
{
    std::lock_guard<std::mutex> lk(g_topo_mu);
    for (tsl_topo* t : g_topos) if (t->map == m) t->map = nullptr;
}

static int topo_check(tsl_topo* t, const std::string& w)
{
    TSL_REQUIRE(t, w + ": null handle");
    TSL_REQUIRE(t->map, w + ": the map of this graph was destroyed");
    return TSL_OK;
}
static int topo_check_ray(tsl_topo* t, float max_dist, float backward, const std::string& w)
{
    TSL_REQUIRE(max_dist >= 0.0f && max_dist <= FLT_MAX, w + ": max_dist is negative or not finite");
    TSL_REQUIRE(max_dist / t->map->P.vs < TOPO_MAX_STEPS, w + ": max_dist is above 2^20 voxels");
    TSL_REQUIRE(backward == backward, w + ": backward is not a number");
    return TSL_OK;
}

static MapQ map_q(const tsl_tsdf* m) { MapQ Q; Q.s = m->cfg.is_global_map ? 0 : m->active; Q.vs_f = m->P.vs; Q.vs_len = (float)m->cfg.voxel_scale; Q.thres = m->surf_thres; return Q; }
static TopoDev topo_dev(const tsl_topo* t)
{ TopoDev T; T.v0 = t->v0; T.e1 = t->e1; T.e2 = t->e2; T.nrm = t->nrm; T.ctr = t->ctr; T.poly = t->poly; T.tri = t->tri; T.nctr = t->nctr; T.nrange = t->nrange; T.nn = t->nn;
  T.max_raycast_dist = t->max_raycast_dist; return T; }

// a larger array with the first `used` bytes of the old one (waits for the device: only when a store grows)
static int grow_keep(void** p, size_t used, size_t bytes)
{
    void* q = nullptr;
    TSL_HIP(hipMalloc(&q, bytes));
    if (*p && used) TSL_HIP(hipMemcpy(q, *p, used, hipMemcpyDeviceToDevice));
    if (*p) (void)hipFree(*p);
    *p = q;
    return TSL_OK;
}

static int topo_reserve(tsl_topo* t, int64_t nf_need, int nn_need)
{
    int rc;
    if (nf_need > t->cap_f) {
        int64_t cap = t->cap_f * 2 > 1024 ? t->cap_f * 2 : 1024;
        if (cap < nf_need) cap = nf_need;
        if (cap > t->max_facelets) cap = t->max_facelets;
        TSL_HIP(hipStreamSynchronize(ms(t->map)));
        const size_t u = (size_t)t->nf, c = (size_t)cap;
        if ((rc = grow_keep((void**)&t->tri, u * 36, c * 36))) return rc;
        float** three[] = { &t->v0, &t->e1, &t->e2, &t->nrm, &t->ctr };
        for (float** p : three) if ((rc = grow_keep((void**)p, u * 12, c * 12))) return rc;
        if ((rc = grow_keep((void**)&t->poly, u * 4, c * 4))) return rc;
        t->cap_f = cap;
    }
    if (nn_need > t->cap_n) {
        int cap = t->cap_n * 2 > 64 ? t->cap_n * 2 : 64;
        if (cap < nn_need) cap = nn_need;
        if (cap > TOPO_MAX_NODES) cap = TOPO_MAX_NODES;
        TSL_HIP(hipStreamSynchronize(ms(t->map)));
        if ((rc = grow_keep((void**)&t->nctr, (size_t)t->nn * 12, (size_t)cap * 12))) return rc;
        if ((rc = grow_keep((void**)&t->nrange, (size_t)t->nn * 8, (size_t)cap * 8))) return rc;
        t->cap_n = cap;
    }
    return TSL_OK;
}

static int rays_launch(tsl_topo* t, hipStream_t q, const float* pos, const float* dir, const int* skip, int n, float max_dist, float backward, int flags, uint8_t* hit,
                       uint8_t* type, float* end_xyz, float* len, int* poly)
{
    hipLaunchKernelGGL(k_topo_rays, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, q, t->map->M, map_q(t->map), topo_dev(t), pos, dir, skip, n, max_dist, backward, flags, hit,
                       type, end_xyz, len, poly);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

// the host-pointer form, after every check
static int rays_host(tsl_topo* t, const float* pos, const float* dir, const int32_t* skip, int n, float max_dist, float backward, int flags, uint8_t* hit, uint8_t* type,
                     float* end_xyz, float* len, int32_t* poly)
{
    tsl_tsdf* m = t->map;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    const size_t c = (size_t)n;
    Stage st(&t->sbuf, &t->sbuf_bytes, q);                                    // the kernel writes every plane: each keeps its room, a null one is not copied back
    const int i_pos = st.in(pos, c * 12), i_dir = st.in(dir, c * 12), i_skip = st.in(skip, c * 4), i_hit = st.out(hit, c, true), i_type = st.out(type, c, true),
              i_end = st.out(end_xyz, c * 12, true), i_len = st.out(len, c * 4, true), i_poly = st.out(poly, c * 4, true);
    int rc = st.upload(); if (rc) return rc;
    if ((rc = rays_launch(t, q, st.ptr<const float>(i_pos), st.ptr<const float>(i_dir), st.ptr<const int>(i_skip), n, max_dist, backward, flags, st.ptr<uint8_t>(i_hit),
                          st.ptr<uint8_t>(i_type), st.ptr<float>(i_end), st.ptr<float>(i_len), st.ptr<int>(i_poly)))) return rc;
    return st.download();
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_topo_create(tsl_tsdf* m, int32_t coll_det_num, float max_raycast_dist, int64_t max_facelets, tsl_topo** out)
{
    TSL_REQUIRE(out, "topo_create: null out"); *out = nullptr;
    TSL_REQUIRE(m, "topo_create: null map");
    TSL_REQUIRE(coll_det_num >= 4 && coll_det_num <= 512, "topo_create: coll_det_num must be 4 .. 512");
    TSL_REQUIRE(max_raycast_dist >= 0.0f && max_raycast_dist <= FLT_MAX, "topo_create: max_raycast_dist is negative or not finite");
    TSL_REQUIRE(max_facelets >= 1 && max_facelets <= (1 << 24), "topo_create: max_facelets must be 1 .. 2^24");
    tsl_topo* t = new tsl_topo();                                             // value-initialised: every pointer null, every count 0
    t->map = m; t->device = m->device; t->coll_det_num = coll_det_num; t->max_raycast_dist = max_raycast_dist; t->max_facelets = max_facelets;
    { std::lock_guard<std::mutex> lk(g_topo_mu); g_topos.push_back(t); }
    *out = t;
    return TSL_OK;
}

void tsl_topo_destroy(tsl_topo* t)
{
    if (!t) return;
    {
        std::lock_guard<std::mutex> lk(g_topo_mu);
        for (size_t i = 0; i < g_topos.size(); ++i) if (g_topos[i] == t) { g_topos.erase(g_topos.begin() + (long)i); break; }
    }
    (void)hipSetDevice(t->device);
    if (t->map && t->map->stream_) (void)hipStreamSynchronize(t->map->stream_);
    void* ptrs[] = { t->tri, t->v0, t->e1, t->e2, t->nrm, t->ctr, t->poly, t->nctr, t->nrange, t->sbuf };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    delete t;
}

int tsl_topo_reset(tsl_topo* t)
{
    int rc = topo_check(t, "topo_reset"); if (rc) return rc;
    t->nf = 0; t->nn = 0;                                                     // the stores keep their memory; launches are stream-ordered, so a later add may overwrite
    return TSL_OK;
}

int tsl_topo_counts(tsl_topo* t, int64_t* n_facelets, int32_t* n_nodes)
{
    int rc = topo_check(t, "topo_counts"); if (rc) return rc;
    if (n_facelets) *n_facelets = t->nf;
    if (n_nodes) *n_nodes = t->nn;
    return TSL_OK;
}

int tsl_topo_rays(tsl_topo* t, const float* pos, const float* dir, const int32_t* skip_idx, int64_t n, float max_dist, float backward, int32_t flags, uint8_t* hit,
                  uint8_t* type, float* end_xyz, float* len, int32_t* poly)
{
    int rc = topo_check(t, "topo_rays"); if (rc) return rc;
    TSL_REQUIRE(n >= 0 && n <= TOPO_MAX_RAYS && (n == 0 || (pos && dir)), "topo_rays: bad argument");
    TSL_REQUIRE((flags & ~1) == 0, "topo_rays: unknown flag");
    if ((rc = topo_check_ray(t, max_dist, backward, "topo_rays"))) return rc;
    if (n == 0) return TSL_OK;
    return rays_host(t, pos, dir, skip_idx, (int)n, max_dist, backward, flags, hit, type, end_xyz, len, poly);
}

int tsl_topo_rays_dev(tsl_topo* t, const void* pos_dev, const void* dir_dev, const void* skip_idx_dev, int64_t n, float max_dist, float backward, int32_t flags,
                      void* hit_dev, void* type_dev, void* end_xyz_dev, void* len_dev, void* poly_dev, void* user_stream)
{
    int rc = topo_check(t, "topo_rays_dev"); if (rc) return rc;
    TSL_REQUIRE(n >= 0 && n <= TOPO_MAX_RAYS && (n == 0 || (pos_dev && dir_dev && hit_dev && type_dev && end_xyz_dev && len_dev && poly_dev)), "topo_rays_dev: bad argument");
    TSL_REQUIRE((flags & ~1) == 0, "topo_rays_dev: unknown flag");
    if ((rc = topo_check_ray(t, max_dist, backward, "topo_rays_dev"))) return rc;
    if (n == 0) return TSL_OK;
    tsl_tsdf* m = t->map;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = rays_launch(t, q, (const float*)pos_dev, (const float*)dir_dev, (const int*)skip_idx_dev, (int)n, max_dist, backward, flags, (uint8_t*)hit_dev, (uint8_t*)type_dev,
                          (float*)end_xyz_dev, (float*)len_dev, (int*)poly_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

int tsl_topo_collide(tsl_topo* t, const float* start, const float* dirs, float thres_size, int32_t* succ, int32_t* black_num, float* black_pos, float* black_dir,
                     float* black_len, int32_t* white_num, float* white_pos, float* node_size)
{
    int rc = topo_check(t, "topo_collide"); if (rc) return rc;
    TSL_REQUIRE(start && dirs && succ && black_num && black_pos && black_dir && black_len, "topo_collide: null argument");
    if ((rc = topo_check_ray(t, t->max_raycast_dist, -0.01f, "topo_collide"))) return rc;
    const int n = t->coll_det_num;
    std::vector<float> pos((size_t)n * 3), end((size_t)n * 3), len((size_t)n);
    std::vector<uint8_t> hit((size_t)n);
    for (int i = 0; i < n; ++i) for (int a = 0; a < 3; ++a) pos[(size_t)i * 3 + a] = start[a];
    if ((rc = rays_host(t, pos.data(), dirs, nullptr, n, t->max_raycast_dist, -0.01f, 0, hit.data(), nullptr, end.data(), len.data(), nullptr))) return rc;
    // detect_collisions  :444-470 in ray order: blacks and whites compacted, the black lengths summed left to right
    int nb = 0, nw = 0; float sum = 0.0f;
    for (int i = 0; i < n; ++i) {
        if (hit[(size_t)i]) {
            for (int a = 0; a < 3; ++a) { black_pos[nb * 3 + a] = end[(size_t)i * 3 + a]; black_dir[nb * 3 + a] = dirs[i * 3 + a]; }
            black_len[nb] = len[(size_t)i];
            sum = sum + len[(size_t)i];
            ++nb;
        } else {
            if (white_pos) for (int a = 0; a < 3; ++a) white_pos[nw * 3 + a] = end[(size_t)i * 3 + a];
            ++nw;
        }
    }
    const float size = sum / (float)nb;                                       // 0 / 0 = NaN when nothing was hit, as in the reference
    *black_num = nb; if (white_num) *white_num = nw; if (node_size) *node_size = size;
    *succ = !(nb == 0 || (nw == 0 && size < thres_size));
    return TSL_OK;
}

int tsl_topo_add_poly(tsl_topo* t, const float* tris, int32_t nf, const float* start, float max_dist, uint8_t* is_frontier, uint8_t* reason, int32_t* neigh, float* centre,
                      int32_t* node_idx)
{
    int rc = topo_check(t, "topo_add_poly"); if (rc) return rc;
    TSL_REQUIRE(tris && start, "topo_add_poly: null argument");
    TSL_REQUIRE(nf >= 1 && nf <= TOPO_MAX_POLY, "topo_add_poly: nf must be 1 .. 4096");
    if ((rc = topo_check_ray(t, max_dist, -0.01f, "topo_add_poly"))) return rc;
    if (t->nf + nf > t->max_facelets) { set_error("topo_add_poly: the facelet store is at max_facelets"); return TSL_ERR_CAPACITY; }
    if (t->nn >= TOPO_MAX_NODES) { set_error("topo_add_poly: the node store is at max_map_node (4096)"); return TSL_ERR_CAPACITY; }
    tsl_tsdf* m = t->map;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);
    if ((rc = topo_reserve(t, t->nf + nf, t->nn + 1))) return rc;
    const size_t c = (size_t)nf;
    Stage st(&t->sbuf, &t->sbuf_bytes, q);                                    // is_frontier and neigh are written whether asked for or not
    const int i_tris = st.in(tris, c * 36), i_fr = st.out(is_frontier, c, true), i_why = st.out(reason, c), i_neigh = st.out(neigh, c * 4, true);
    if ((rc = st.upload())) return rc;
    hipLaunchKernelGGL(k_topo_facelets, dim3((unsigned)((nf + 3) / 4)), dim3(256), 0, q, m->M, map_q(m), topo_dev(t), st.ptr<const float>(i_tris), nf, (int)t->nf, t->nn,
                       start[0], start[1], start[2], max_dist, st.ptr<uint8_t>(i_fr), st.ptr<uint8_t>(i_why), st.ptr<int>(i_neigh));
    TSL_HIP(hipGetLastError());
    // the node (add_mesh :384-405): the left-to-right f32 sum of (v0 + v1) + v2 over the facelets, divided by 3 * nf
    float node[3] = { 0.0f, 0.0f, 0.0f }, count = 0.0f;
    for (size_t f = 0; f < c; ++f) {
        for (int a = 0; a < 3; ++a) { const float s = (tris[f * 9 + a] + tris[f * 9 + 3 + a]) + tris[f * 9 + 6 + a]; node[a] = node[a] + s; }
        count = count + 3.0f;
    }
    for (int a = 0; a < 3; ++a) node[a] = node[a] / count;
    const int range[2] = { (int)t->nf, (int)t->nf + nf };
    TSL_HIP(hipMemcpyAsync(t->nctr + (size_t)t->nn * 3, node, 12, hipMemcpyHostToDevice, q));
    TSL_HIP(hipMemcpyAsync(t->nrange + (size_t)t->nn * 2, range, 8, hipMemcpyHostToDevice, q));
    if ((rc = st.download())) return rc;
    if (centre) for (int a = 0; a < 3; ++a) centre[a] = node[a];
    if (node_idx) *node_idx = t->nn;
    t->nf += nf; t->nn += 1;
    return TSL_OK;
}

int tsl_topo_buffers_dev(tsl_topo* t, void** tri_vertices_dev, void** normal_dev, void** centre_dev, void** poly_dev, int64_t* n_facelets, int32_t* n_nodes)
{
    int rc = topo_check(t, "topo_buffers_dev"); if (rc) return rc;
    if (tri_vertices_dev) *tri_vertices_dev = t->tri;
    if (normal_dev) *normal_dev = t->nrm;
    if (centre_dev) *centre_dev = t->ctr;
    if (poly_dev) *poly_dev = t->poly;
    if (n_facelets) *n_facelets = t->nf;
    if (n_nodes) *n_nodes = t->nn;
    return TSL_OK;
}

int tsl_topo_read_facelets(tsl_topo* t, int64_t first, int64_t n, float* tri_vertices, float* v0, float* edge1, float* edge2, float* normal, float* centre, int32_t* poly)
{
    int rc = topo_check(t, "topo_read_facelets"); if (rc) return rc;
    TSL_REQUIRE(first >= 0 && n >= 0 && first + n <= t->nf, "topo_read_facelets: more facelets than the store holds");
    if (n == 0) return TSL_OK;
    TSL_HIP(hipSetDevice(t->device));
    TSL_HIP(hipStreamSynchronize(ms(t->map)));
    const size_t o = (size_t)first, c = (size_t)n;
    if (tri_vertices) TSL_HIP(hipMemcpy(tri_vertices, t->tri + o * 9, c * 36, hipMemcpyDeviceToHost));
    float* dst[] = { v0, edge1, edge2, normal, centre }; float* src[] = { t->v0, t->e1, t->e2, t->nrm, t->ctr };
    for (int a = 0; a < 5; ++a) if (dst[a]) TSL_HIP(hipMemcpy(dst[a], src[a] + o * 3, c * 12, hipMemcpyDeviceToHost));
    if (poly) TSL_HIP(hipMemcpy(poly, t->poly + o, c * 4, hipMemcpyDeviceToHost));
    return TSL_OK;
}

}  // extern "C"

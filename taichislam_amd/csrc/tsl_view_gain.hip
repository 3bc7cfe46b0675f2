// tsl_view_gain.hip -- many candidate camera poses scored in one call by the unobserved space a sensor there would see before its rays hit something:
// the figure a next-best-view planner ranks its candidates by.  It stands beside tsl_render.hip (one pose, a depth image, no
// counts) and BaseMap.raycast (stops at occupied voxels, says nothing of unknown ones); the reference has nothing of the kind.
//
// Definition (include/taichislam_hip.h "view gain"; tests/view_gain_ref.py restates it in numpy and every integer must equal it).  All f32, no
// contraction, in the written order.  Ray (u, v) of pose k: dc = ((u - cx) / fx, (v - cy) / fy, 1), d = R_k dc (rows summed left to right, NOT
// normalised), samples n = 0 .. S-1 at t_n = t_min + n * dt, p_n = T_k + t_n * d, u_n = p_n / vs.  The voxel of a sample is rnd_i(clamp(u_n)) per axis,
// clamp(x) = max(min(x, 2^24), -2^24) (the clamp of cell_floor: the conversion stays inside an int; a NaN lands on the clamp).  The sample is OUTSIDE
// when p_n is not finite or the voxel is not in the volume, else UNKNOWN / OCCUPIED / FREE as k_fr_mark (tsl_frontier.hip) classes that voxel.  OUTSIDE
// changes nothing; the first OCCUPIED sample ends the ray (hit, not counted); FREE adds 1 and w_n = rnd_i((t_n * t_n) * 1024) to the free sums and clears
// the unknown run; UNKNOWN adds them to the unknown sums and 1 to the run, and with unknown_run > 0 the ray is cut once the run reaches it.  A ray looks
// through a frontier when an UNKNOWN sample's previous non-OUTSIDE sample was FREE.
//
// One lane per ray, a wave covers an 8 x 8 ray tile of one pose (neighbouring rays share bricks and cache lines), a workgroup a 16 x 16 tile, the grid
// is (tiles, poses).  The pose table is in device memory, 12 f32 per pose, read per workgroup (uniform loads), never per lane.  A sample costs one brick
// table lookup and one observed / TSDF gather; the lane keeps its last brick and pool index, so a run of samples in one brick does not go back to the
// table.  The sums stay in registers, are reduced in the wave, then over the four waves in LDS, and one set of global integer atomics per workgroup goes
// to the pose's record (zeroed on the stream before the launch).  No per-lane global atomics, no float atomics, no workgroup waits for another.
//
// Skipping (flags bit 0 switches it off; the result is the same bit for bit).  The argument of tsl_render.hip carries over to the nearest voxel.  Per
// axis the voxel of sample n is a monotone function of n: n -> (float)n * dt and x -> t_min + x are monotone under round-to-nearest, and so are
// x -> T + x * d, x -> x / vs, the clamp, x -> x + copysign(c, x) (for x >= 0 it adds c, for x < 0 it subtracts c, and every value of the first branch
// lies above every value of the second) and the truncating conversion.  So the samples whose voxel lies in one brick -- a box -- or beyond one face of
// the volume -- a half space -- are a contiguous run of n: if samples n and m > n are both there, so is every sample between them.
//   outside the volume   the ray estimates where it crosses the face it has to cross, steps two samples back and CHECKS sample m with the arithmetic of
//                        the walk: if it is beyond the same face, n .. m are all OUTSIDE and the walk resumes at m + 1 with its state untouched.  On an
//                        axis where the ray moves away from the volume (or not at all) every later sample is outside too: the ray ends (range).
//   an unallocated brick the same estimate and check (once per brick entered) give a verified end m of the run.  Samples n .. m are all UNKNOWN: each
//                        still contributes its w and advances the run counter, and the cut is honoured, but with ALU only -- t and w, no position, no
//                        division, no gathers.  They are taken one per turn of the walk's loop like every other sample: a loop of their own would let the
//                        lanes of a tile drift apart (measured: slower than no skipping at all).
// The estimate decides how far a ray jumps, never what it counts.
#include <cmath>
#include "tsl_stage.hpp"

namespace tsl {

#define VG_MAX_POSES 65536
#define VG_CHUNK 32768                 // poses per launch: grid.y stays below its limit of 65535
#define VG_FRONTIER 0x10

struct GainDev {
    float fx, fy, cx, cy;
    float tmin, dt, vs, thres;
    float rvs, big; int fast;          // div_vs (tsl_common.hpp): RN(1 / vs), the bound below which it was verified equal to x / vs, and whether it was
    int h, w, S, run, flags, tiles_x;
};

struct GainState { float* pin; size_t pin_bytes; void* dev; size_t dev_bytes; hipEvent_t copied; bool pending; };      // the pose table: pinned staging, device copy

__device__ __forceinline__ int vg_voxel(float u) { return rnd_i(fmaxf(fminf(u, 16777216.0f), -16777216.0f)); }
// The voxel of a finite position: rnd_i(clamp(p / vs)) per axis.  The three IEEE divisions are a third of a sample's instructions; where the handle has
// verified div_vs against x / vs for every float (tsl_tsdf_create: all x with 2^-100 <= |x| < 2^31 vs) the quotient comes from it -- bit for bit the same
// for those x, and for a smaller |x| both quotients are below 2^-90 and round to voxel 0.  A wave that holds a coordinate beyond the bound divides.
__device__ __forceinline__ void vg_voxels(const GainDev& W, const float p[3], int v[3])
{
    const bool far = !(fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2])) < W.big);
    if (W.fast && !__any(far)) {
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = vg_voxel(div_vs(p[a], W.vs, W.rvs, 1));
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = vg_voxel(p[a] / W.vs);
    }
}
__device__ __forceinline__ int vg_weight(float t) { return rnd_i((t * t) * 1024.0f); }      // t <= 1024: below 2^31

// sample m of the ray: its voxel, with the arithmetic of the walk; false when a coordinate of the position is not finite
__device__ __forceinline__ bool vg_sample(const GainDev& W, const float T[3], const float d[3], int m, int v[3])
{
    const float t = W.tmin + (float)m * W.dt;
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = T[a] + t * d[a];
    vg_voxels(W, p, v);
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// The sample index at which the ray passes from voxel edge - 1 to voxel edge of an axis (the plane edge - 1/2 in voxel units), as a float: an ESTIMATE,
// (edge - 1/2) * ek + ec with the ray's ek = (vs / d) / dt and ec = (-T / d - t_min) / dt -- the divisions are made once per ray, not per brick entered.
struct GainEst { float ek[3], ec[3]; };
__device__ __forceinline__ float vg_plane_sample(const GainEst& E, int a, int edge) { return ((float)edge - 0.5f) * E.ek[a] + E.ec[a]; }

// Sample n has its voxel v in an unallocated brick.  Returns the last sample m >= n verified to lie in the same brick (n .. m are unknown); n when
// there is nothing to gain.
__device__ __forceinline__ int vg_skip_brick(const MapDev& M, const GainDev& W, const GainEst& E, const float T[3], const float d[3], int n, const int v[3])
{
    const int lo[3] = { ((v[0] + M.hN) & ~15) - M.hN, ((v[1] + M.hN) & ~15) - M.hN, ((v[2] + M.hNz) & ~15) - M.hNz };
    float ne = (float)(W.S - 1);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (d[a] != 0.0f) { const float nf = vg_plane_sample(E, a, d[a] > 0.0f ? lo[a] + TSL_BRK : lo[a]); if (nf < ne) ne = nf; }
    if (!(ne >= (float)(n + 4))) return n;                         // nothing to gain (or the estimate is not a number)
    const int m = (int)ne - 2;                                     // rounded down, two samples of margin: the check below nearly always passes
    int c[3];
    if (!vg_sample(W, T, d, m, c)) return n;
    const bool same = c[0] >= lo[0] && c[0] < lo[0] + TSL_BRK && c[1] >= lo[1] && c[1] < lo[1] + TSL_BRK && c[2] >= lo[2] && c[2] < lo[2] + TSL_BRK;
    return same ? m : n;
}

// Sample n has its voxel v outside the volume.  Returns the next sample to evaluate: S when the ray can never re-enter, m + 1 when sample m > n was
// verified to lie beyond the same face, else n + 1.
__device__ __forceinline__ int vg_skip_outside(const MapDev& M, const GainDev& W, const GainEst& E, const float T[3], const float d[3], int n, const int v[3])
{
    const int lo[3] = { -M.hN, -M.hN, -M.hNz }, hi[3] = { M.N - M.hN, M.N - M.hN, M.Nz - M.hNz };      // voxels lo .. hi - 1 are in the volume
    float ne = -1.0f; int ax = 0; bool below = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool under = v[a] < lo[a], over = v[a] >= hi[a];
        if ((under && !(d[a] > 0.0f)) || (over && !(d[a] < 0.0f))) return W.S;
        if (under || over) { const float nf = vg_plane_sample(E, a, under ? lo[a] : hi[a]); if (nf > ne) { ne = nf; ax = a; below = under; } }
    }
    if (!(ne >= (float)(n + 4))) return n + 1;
    if (ne > (float)(W.S - 1)) ne = (float)(W.S - 1);
    const int m = (int)ne - 2;
    if (m <= n) return n + 1;
    int c[3];
    if (!vg_sample(W, T, d, m, c)) return n + 1;
    const int ca = ax == 0 ? c[0] : ax == 1 ? c[1] : c[2], la = ax == 0 ? lo[0] : ax == 1 ? lo[1] : lo[2], ha = ax == 0 ? hi[0] : ax == 1 ? hi[1] : hi[2];
    return (below ? ca < la : ca >= ha) ? m + 1 : n + 1;
}

struct GainRay { int nu, nf, st; bool fr; long long wu, wf; };      // a ray's unknown / free counts, status, "looked through a frontier", the weights

// the walk of ray (px, py) of the pose (R, T) over submap table Tb
__device__ __forceinline__ GainRay vg_walk(const MapDev& M, const int* __restrict__ Tb, const GainDev& W, const float R[9], const float T[3], int px, int py)
{
    GainRay g = { 0, 0, 1, false, 0, 0 };
    const float dc0 = ((float)px - W.cx) / W.fx, dc1 = ((float)py - W.cy) / W.fy, dc2 = 1.0f;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (R[r * 3] * dc0 + R[r * 3 + 1] * dc1) + R[r * 3 + 2] * dc2;
    const bool skip = !(W.flags & 1);
    GainEst E;
#pragma unroll
    for (int a = 0; a < 3; ++a) { E.ek[a] = skip ? (W.vs / d[a]) / W.dt : 0.0f; E.ec[a] = skip ? ((-T[a]) / d[a] - W.tmin) / W.dt : 0.0f; }      // (used where d[a] != 0 only)
    int n = 0, run = 0, cb = -1, cP = TSL_EMPTY;                  // cb / cP: the brick of the lane's last lookup and its pool index
    int mend = -1, eb = -1;                                        // samples n <= mend lie in a brick verified unallocated; eb: the brick of the last estimate
    bool pfree = false;                                            // the previous non-OUTSIDE sample was FREE
    // every lane takes one sample per turn, whatever it is, so that the lanes of a tile stay together
    while (n < W.S) {
        const float t = W.tmin + (float)n * W.dt;
        if (n > mend) {
            float p[3]; int v[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = T[a] + t * d[a];
            if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) { ++n; continue; }                  // OUTSIDE
            vg_voxels(W, p, v);
            if (!in_volume(M, v[0], v[1], v[2])) { n = skip ? vg_skip_outside(M, W, E, T, d, n, v) : n + 1; continue; }      // OUTSIDE
            int l; const int b = brick_of(M, v[0], v[1], v[2], &l);
            if (b != cb) { cb = b; cP = Tb[b]; }
            if (cP >= 0) {
                const size_t x = (size_t)cP * TSL_BRK3 + l;
                const int ob = M.obs[x]; const uint32_t tw = M.tw[x];                                       // both issued before either is used
                if (ob > 0) {
                    if (h2f((h16)(tw & 0xffffu)) < W.thres) { g.st = 0; break; }                            // OCCUPIED: the test of q_occupied
                    ++g.nf; g.wf += vg_weight(t); run = 0; pfree = true; ++n;                               // FREE
                    continue;
                }
            } else if (skip && b != eb) { eb = b; mend = vg_skip_brick(M, W, E, T, d, n, v); }                // one estimate per brick entered
            if (pfree) g.fr = true;
            pfree = false;
        }
        // UNKNOWN; for n <= mend (inside an unallocated brick) with t and w alone: no position, no gathers
        ++g.nu; g.wu += vg_weight(t); ++run;
        if (W.run > 0 && run >= W.run) { g.st = 2; break; }
        ++n;
    }
    return g;
}

__device__ __forceinline__ int vg_wave_sum(int x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o); return x; }

// 7 waves per SIMD: 53 VGPRs, 106 SGPRs (20 more scalars held in lanes of VGPRs), 192 bytes of LDS, no scratch (the compiler's report).  The scalars
// set the limit; __launch_bounds__(256, 8) brings them to 78 for the eighth wave, but then 59 scalars live in VGPR lanes and are moved in and out inside
// the walk: measured never faster and up to 16 % slower, so the bound stays off.  blockIdx.x: the 16 x 16 tile, blockIdx.y + pose0: the pose.
__global__ void __launch_bounds__(256) k_view_gain(MapDev M, int s, GainDev W, const float* __restrict__ poses, int pose0, tsl_view_gain* __restrict__ out,
                                                   int* __restrict__ ray_unknown, uint8_t* __restrict__ ray_status)
{
    __shared__ long long s_ll[4][4];
    __shared__ int s_i[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x % W.tiles_x, ty = blockIdx.x / W.tiles_x, k = pose0 + blockIdx.y;
    const int px = tx * 16 + (wave & 1) * 8 + (lane & 7), py = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool live = px < W.w && py < W.h;
    const int* __restrict__ Tb = M.table + (size_t)s * M.nb3;
    const float* __restrict__ pp = poses + (size_t)k * 12;          // the same address in every lane: scalar loads
    const float R[9] = { pp[0], pp[1], pp[2], pp[3], pp[4], pp[5], pp[6], pp[7], pp[8] }, T[3] = { pp[9], pp[10], pp[11] };

    GainRay g = { 0, 0, 1, false, 0, 0 };
    if (live) {
        g = vg_walk(M, Tb, W, R, T, px, py);
        if (ray_unknown) {
            const size_t o = ((size_t)k * W.h + py) * W.w + px;
            ray_unknown[o] = g.nu; ray_status[o] = (uint8_t)(g.st | (g.fr ? VG_FRONTIER : 0));
        }
    }

    // the wave, then the four waves, then one set of atomics per workgroup
    const long long a0 = wave_sum_ll((long long)g.nu), a1 = wave_sum_ll((long long)g.nf), a2 = wave_sum_ll(g.wu), a3 = wave_sum_ll(g.wf);
    const int b0 = vg_wave_sum(live && g.st == 0 ? 1 : 0), b1 = vg_wave_sum(live && g.st == 1 ? 1 : 0), b2 = vg_wave_sum(live && g.st == 2 ? 1 : 0),
              b3 = vg_wave_sum(g.fr ? 1 : 0);
    if (lane == 0) {
        s_ll[wave][0] = a0; s_ll[wave][1] = a1; s_ll[wave][2] = a2; s_ll[wave][3] = a3;
        s_i[wave][0] = b0; s_i[wave][1] = b1; s_i[wave][2] = b2; s_i[wave][3] = b3;
    }
    __syncthreads();
    tsl_view_gain* o = out + k;
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        const long long sum = (s_ll[0][c] + s_ll[1][c]) + (s_ll[2][c] + s_ll[3][c]);
        if (sum != 0) __hip_atomic_fetch_add((long long*)o + c, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (threadIdx.x < 8) {
        const int c = threadIdx.x - 4;
        const int sum = (s_i[0][c] + s_i[1][c]) + (s_i[2][c] + s_i[3][c]);
        if (sum != 0) __hip_atomic_fetch_add((int*)o + 8 + c, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static_assert(sizeof(tsl_view_gain) == 64, "one record per 64 bytes");

static bool vg_finite(const double* a, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false; return true; }

void gain_release(tsl_tsdf* m)
{
    GainState* G = m->gain;
    if (!G) return;
    if (G->pending) (void)hipEventSynchronize(G->copied);
    if (G->copied) (void)hipEventDestroy(G->copied);
    if (G->pin) (void)hipHostFree(G->pin);
    if (G->dev) (void)hipFree(G->dev);
    delete G;
    m->gain = nullptr;
}

// the checks and defaults both forms share; *go = false: nothing to do (n = 0)
static int gain_check(tsl_tsdf* m, const double* R, const double* T, int32_t n, const tsl_gain_cfg* c, const void* out, const void* ray_unknown,
                      const void* ray_status, GainDev* W, bool* go, const char* who)
{
    const std::string w(who);
    *go = false;
    TSL_REQUIRE(m, w + ": null handle");
    TSL_REQUIRE(n >= 0 && n <= VG_MAX_POSES, w + ": 0 .. 65536 poses");
    if (n == 0) return TSL_OK;
    TSL_REQUIRE(R && T && c && out, w + ": null argument");
    TSL_REQUIRE((ray_unknown != nullptr) == (ray_status != nullptr), w + ": ray_unknown and ray_status go together");
    TSL_REQUIRE(vg_finite(R, 9 * (size_t)n) && vg_finite(T, 3 * (size_t)n), w + ": a pose is not finite");
    TSL_REQUIRE(vg_finite(c->K, 9), w + ": an intrinsic is not finite");
    TSL_REQUIRE(std::isfinite(c->t_min) && std::isfinite(c->t_max) && std::isfinite(c->dt), w + ": t_min / t_max / dt is not finite");
    TSL_REQUIRE(std::isfinite(c->free_thres), w + ": free_thres is not finite");
    TSL_REQUIRE(c->h >= 1 && c->w >= 1 && c->h <= 4096 && c->w <= 4096, w + ": the fan must be 1 .. 4096 rays per side");
    TSL_REQUIRE(c->unknown_run >= 0, w + ": unknown_run is negative");
    bool zero = true; for (int i = 0; i < 9; ++i) zero = zero && c->K[i] == 0.0;
    if (zero) { W->fx = m->P.fx; W->fy = m->P.fy; W->cx = m->P.cx; W->cy = m->P.cy; }           // the map's depth intrinsics
    else { W->fx = (float)c->K[0]; W->fy = (float)c->K[4]; W->cx = (float)c->K[2]; W->cy = (float)c->K[5]; }
    W->vs = m->P.vs;
    W->tmin = c->t_min != 0.0f ? c->t_min : (float)m->cfg.min_ray_length;
    const float tmax = c->t_max != 0.0f ? c->t_max : (float)m->cfg.max_ray_length;
    W->dt = c->dt != 0.0f ? c->dt : 0.75f * W->vs;
    W->thres = c->free_thres != 0.0f ? c->free_thres : m->surf_thres;
    W->rvs = m->P.rvs; W->fast = m->P.fastdiv; W->big = 2147483648.0f * W->vs;                  // the bound of k_verify_div
    TSL_REQUIRE(tmax > W->tmin, w + ": t_max must exceed t_min");
    TSL_REQUIRE(W->dt > 0.0f, w + ": dt must be positive");
    TSL_REQUIRE(tmax <= 1024.0f, w + ": t_max must not exceed 1024 (the weight of a sample is held in 31 bits)");
    const float q = (tmax - W->tmin) / W->dt;
    TSL_REQUIRE(q < 16777216.0f, w + ": more than 2^24 samples per ray");
    W->S = (int)q + 1;
    W->h = c->h; W->w = c->w; W->run = c->unknown_run; W->flags = c->flags; W->tiles_x = (c->w + 15) / 16;
    *go = true;
    return TSL_OK;
}

// the pose table, rounded to f32 once, through the handle's pinned buffer into its device copy on the stream (a buffer of its own: the export staging
// buffer is written by synchronous calls that do not wait for this stream)
static int gain_stage(tsl_tsdf* m, hipStream_t q, const double* R, const double* T, int n, const float** poses)
{
    if (!m->gain) m->gain = new GainState();                      // value-initialised
    GainState* G = m->gain;
    if (!G->copied) TSL_HIP(hipEventCreateWithFlags(&G->copied, hipEventDisableTiming));
    if (G->pending) { TSL_HIP(hipEventSynchronize(G->copied)); G->pending = false; }      // the previous call's table has left the buffer
    const size_t bytes = sizeof(float) * 12 * (size_t)n;
    const int rc = grow(&G->dev, &G->dev_bytes, bytes); if (rc) return rc;      // (frees only behind the device's work)
    if (G->pin_bytes < bytes) {
        if (G->pin) (void)hipHostFree(G->pin);
        G->pin = nullptr; G->pin_bytes = 0;
        TSL_HIP(hipHostMalloc((void**)&G->pin, bytes + bytes / 4 + 4096, hipHostMallocDefault));
        G->pin_bytes = bytes + bytes / 4 + 4096;
    }
    for (int k = 0; k < n; ++k) {
        for (int i = 0; i < 9; ++i) G->pin[(size_t)k * 12 + i] = (float)R[(size_t)k * 9 + i];
        for (int i = 0; i < 3; ++i) G->pin[(size_t)k * 12 + 9 + i] = (float)T[(size_t)k * 3 + i];
    }
    TSL_HIP(hipMemcpyAsync(G->dev, G->pin, bytes, hipMemcpyHostToDevice, q));
    *poses = (const float*)G->dev;
    TSL_HIP(hipEventRecord(G->copied, q));
    G->pending = true;
    return TSL_OK;
}

static int gain_launch(tsl_tsdf* m, hipStream_t q, const GainDev& W, const float* poses, int n, tsl_view_gain* out, int* ray_unknown, uint8_t* ray_status)
{
    TSL_HIP(hipMemsetAsync(out, 0, sizeof(tsl_view_gain) * (size_t)n, q));
    const unsigned tiles = (unsigned)(W.tiles_x * ((W.h + 15) / 16));
    const int s = m->cfg.is_global_map ? 0 : m->active;
    prof_begin(m, TSL_K_VIEW_GAIN, q);
    for (int k0 = 0; k0 < n; k0 += VG_CHUNK)
        hipLaunchKernelGGL(k_view_gain, dim3(tiles, (unsigned)(n - k0 < VG_CHUNK ? n - k0 : VG_CHUNK)), dim3(256), 0, q, m->M, s, W, poses, k0, out, ray_unknown, ray_status);
    prof_end(m, q);
    TSL_HIP(hipGetLastError());
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_tsdf_view_gain(tsl_tsdf* m, const double* R, const double* T, int32_t n, const tsl_gain_cfg* cfg, tsl_view_gain* out, int32_t* ray_unknown,
                       uint8_t* ray_status)
{
    GainDev W; bool go;
    int rc = gain_check(m, R, T, n, cfg, out, ray_unknown, ray_status, &W, &go, "view_gain"); if (rc || !go) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // issues the queued frames
    const size_t rays = (size_t)n * W.h * W.w;
    Stage st(&m->xbuf, &m->xbuf_bytes, q);
    const int i_out = st.out(out, sizeof(tsl_view_gain) * (size_t)n), i_ru = st.out(ray_unknown, rays * 4), i_rs = st.out(ray_status, rays);
    if ((rc = st.upload())) return rc;
    const float* poses;
    if ((rc = gain_stage(m, q, R, T, n, &poses))) return rc;
    if ((rc = gain_launch(m, q, W, poses, n, st.ptr<tsl_view_gain>(i_out), st.ptr<int>(i_ru), st.ptr<uint8_t>(i_rs)))) return rc;
    return st.download();
}

int tsl_tsdf_view_gain_dev(tsl_tsdf* m, const double* R, const double* T, int32_t n, const tsl_gain_cfg* cfg, void* out_dev, void* ray_unknown_dev,
                           void* ray_status_dev, void* user_stream)
{
    GainDev W; bool go;
    int rc = gain_check(m, R, T, n, cfg, out_dev, ray_unknown_dev, ray_status_dev, &W, &go, "view_gain_dev"); if (rc || !go) return rc;
    TSL_HIP(hipSetDevice(m->device));
    const hipStream_t q = ms(m);                               // behind every frame queued so far
    const float* poses;
    if ((rc = order_before(m, (hipStream_t)user_stream, q))) return rc;
    if ((rc = gain_stage(m, q, R, T, n, &poses))) return rc;
    if ((rc = gain_launch(m, q, W, poses, n, (tsl_view_gain*)out_dev, (int*)ray_unknown_dev, (uint8_t*)ray_status_dev))) return rc;
    return order_after(m, (hipStream_t)user_stream, q);
}

}  // extern "C"

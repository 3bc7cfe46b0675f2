// tsl_depth.hip -- depth conditioning (include/taichislam_hip.h "depth conditioning"): a batch of uint16 millimetre frames gets a
// status per pixel (hole, range, sparse, edge, kept), the kept pixels an integer bilateral offset, and the result a pyramid of half-resolution levels.  All
// integer: the answer depends on no schedule, and tests/depth_condition_ref.py restates it byte for byte.  A tsl_depth handle owns the tables, a stream for
// the host-pointer form and two small device buffers; it knows no map.
//
// k_depth_condition: one workgroup of 256 lanes per 64 x 32 tile of one frame (the frame on the grid's third axis).  The tile and its halo of
// H = 1 + erode + radius pixels live in LDS as a u16 depth plane and a u8 status plane of DC_ROWS x DC_PITCH cells; four stages run over shrinking
// regions of that image with a barrier between them:
//     load + gate   the whole haloed region       status HOLE / RANGE / candidate; cells outside the image are OUTSIDE and never count
//     support       the region inset by 1         candidate -> SPARSE
//     erosion       the region inset by 1 + erode candidate -> EDGE
//     smoothing     the tile                      out, status and the counts
// A stage writes only codes that the stage's own readers do not tell apart from the code they replace (support reads "candidate", which SPARSE still is;
// erosion reads "seed", which EDGE never is), so no stage needs a second plane.
//
// LDS banks (MI355X: a u16 / u8 read is serviced like ds_read_b32, two groups of 32 lanes, bank = dword address mod 32): the smoothing stage gives a wave
// one row of 64 consecutive cells, 32 consecutive dwords of depth or 16 of status, two or four lanes per dword (identical addresses broadcast): no
// conflict at any pitch.  The halo stages walk their region by a linear index, so a wave covers the tail of one row and the head of the next: with the
// depth pitch of 40 dwords the two pieces of a 32-lane group span at most 16 + (DC_PITCH - region width) / 2 <= 24 consecutive-or-gapped dwords, less than
// the 32 banks, so they are conflict-free as well; the status pitch of 20 dwords likewise.
#include "tsl_stage.hpp"

namespace tsl {

constexpr int DC_TW = 64, DC_TH = 32, DC_MAX_HALO = 8;
constexpr int DC_PITCH = DC_TW + 2 * DC_MAX_HALO, DC_ROWS = DC_TH + 2 * DC_MAX_HALO;          // 80 x 48 cells: 7680 B of depth, 3840 B of status
constexpr int DC_TAB_DWORDS = 272;                                                          // tol u16 [256], rq u16 [256], ws u8 [32], wr u8 [32]
enum { DS_KEPT = 0, DS_HOLE = 1, DS_RANGE = 2, DS_SPARSE = 3, DS_EDGE = 4, DS_OUTSIDE = 5 };

struct DepthArgs {
    const uint16_t* depth; uint16_t* out; uint8_t* status; long long* counts; const uint32_t* tab;
    int n, h, w, d_min, d_max, min_support, erode, holes;
};

__device__ __forceinline__ bool dc_candidate(int st) { return st == DS_KEPT || st == DS_SPARSE; }

template <int RADIUS>
__global__ __launch_bounds__(256) void k_depth_condition(DepthArgs A)
{
    __shared__ uint32_t s_dw[DC_ROWS * DC_PITCH / 2];
    __shared__ uint32_t s_sw[DC_ROWS * DC_PITCH / 4];
    __shared__ uint32_t s_tab[DC_TAB_DWORDS];
    __shared__ int s_cnt[8];
    uint16_t* s_d = reinterpret_cast<uint16_t*>(s_dw);
    uint8_t* s_st = reinterpret_cast<uint8_t*>(s_sw);
    const uint16_t* s_tol = reinterpret_cast<const uint16_t*>(s_tab);
    const uint16_t* s_rq = s_tol + 256;
    const uint8_t* s_ws = reinterpret_cast<const uint8_t*>(s_tab) + 1024;
    const uint8_t* s_wr = s_ws + 32;

    const int tid = threadIdx.x, f = blockIdx.z;
    const int H = 1 + A.erode + RADIUS;
    const int rw = DC_TW + 2 * H, rh = DC_TH + 2 * H;
    const int x0 = (int)blockIdx.x * DC_TW - H, y0 = (int)blockIdx.y * DC_TH - H;          // the image coordinates of LDS cell (0, 0)

    // ---- every cell OUTSIDE with depth 0; the tables; the counters
    for (int i = tid; i < DC_ROWS * DC_PITCH / 2; i += 256) s_dw[i] = 0u;
    for (int i = tid; i < DC_ROWS * DC_PITCH / 4; i += 256) s_sw[i] = 0x01010101u * DS_OUTSIDE;
    for (int i = tid; i < DC_TAB_DWORDS; i += 256) s_tab[i] = A.tab[i];
    if (tid < 8) s_cnt[tid] = 0;
    __syncthreads();

    // ---- load + gate.  A lane takes one aligned dword, two pixels of a row, when both lie in the clipped row; a single pixel at a row's end is read as u16,
    // so nothing outside the frames is ever read.  mis: the buffer starts in the upper half of a dword.
    {
        const int mis = (int)(((uintptr_t)A.depth >> 1) & 1);
        const uint32_t* wbase = reinterpret_cast<const uint32_t*>(A.depth - mis);
        const int cx0 = max(x0, 0), cx1 = min(x0 + rw, A.w);
        const int SP = (rw >> 1) + 1;                                                       // a run of rw pixels touches at most rw / 2 + 1 dwords
        for (int idx = tid; idx < rh * SP; idx += 256) {
            const int ly = idx / SP, s = idx - ly * SP, y = y0 + ly;
            if (y < 0 || y >= A.h) continue;
            const int rowb = (f * A.h + y) * A.w;                                           // n h w <= 2^28: every linear index fits an int
            const int P = ((rowb + cx0 + mis) >> 1) + s;
            const int xa = 2 * P - mis - rowb, xb = xa + 1;
            const bool ina = xa >= cx0 && xa < cx1, inb = xb >= cx0 && xb < cx1;
            if (!ina && !inb) continue;
            unsigned da = 0, db = 0;
            if (ina && inb) { const uint32_t v = wbase[P]; da = v & 0xffffu; db = v >> 16; }
            else if (ina) da = A.depth[rowb + xa];
            else db = A.depth[rowb + xb];
            const int c = ly * DC_PITCH - x0;
            if (ina) { s_d[c + xa] = (uint16_t)da; s_st[c + xa] = da == 0 ? DS_HOLE : ((int)da < A.d_min || (int)da > A.d_max) ? DS_RANGE : DS_KEPT; }
            if (inb) { s_d[c + xb] = (uint16_t)db; s_st[c + xb] = db == 0 ? DS_HOLE : ((int)db < A.d_min || (int)db > A.d_max) ? DS_RANGE : DS_KEPT; }
        }
    }
    __syncthreads();

    // ---- support: the region inset by 1
    if (A.min_support > 0) {
        const int sw = rw - 2, sh = rh - 2;
        for (int idx = tid; idx < sw * sh; idx += 256) {
            const int ly = idx / sw, c = (ly + 1) * DC_PITCH + (idx - ly * sw) + 1;
            if (s_st[c] != DS_KEPT) continue;
            const int d = s_d[c], t = s_tol[d >> 8];
            int cnt = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dy == 0 && dx == 0) continue;
                    const int q = c + dy * DC_PITCH + dx;
                    cnt += (dc_candidate(s_st[q]) && abs((int)s_d[q] - d) <= t) ? 1 : 0;
                }
            if (cnt < A.min_support) s_st[c] = DS_SPARSE;
        }
        __syncthreads();
    }

    // ---- erosion: the region inset by 1 + erode
    if (A.erode > 0) {
        const int e = A.erode, ew = rw - 2 * (1 + e), eh = rh - 2 * (1 + e);
        for (int idx = tid; idx < ew * eh; idx += 256) {
            const int ly = idx / ew, c = (ly + 1 + e) * DC_PITCH + (idx - ly * ew) + 1 + e;
            if (s_st[c] != DS_KEPT) continue;
            bool seed = false;
            for (int dy = -e; dy <= e; ++dy)
                for (int dx = -e; dx <= e; ++dx) {
                    const int sq = s_st[c + dy * DC_PITCH + dx];
                    seed |= sq == DS_SPARSE || (A.holes && sq == DS_HOLE);
                }
            if (seed) s_st[c] = DS_EDGE;
        }
        __syncthreads();
    }

    // ---- smoothing, output and counts: a wave takes rows wave, wave + 4, ... of the tile, a lane one column
    const int lx = tid & 63, wave = tid >> 6, px = (int)blockIdx.x * DC_TW + lx;
    int cnt[5] = { 0, 0, 0, 0, 0 };
    for (int r = wave; r < DC_TH; r += 4) {
        const int py = (int)blockIdx.y * DC_TH + r;
        const bool inside = px < A.w && py < A.h;
        const int c = (H + r) * DC_PITCH + H + lx;
        const int st = s_st[c], d = s_d[c];
        int o = 0;
        if (st == DS_KEPT) {
            o = d;
            if (RADIUS > 0) {
                const int t = s_tol[d >> 8];
                const unsigned rq = s_rq[d >> 8];
                long long num = 0; int den = 0;
#pragma unroll
                for (int dy = -RADIUS; dy <= RADIUS; ++dy)
#pragma unroll
                    for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
                        const int q = c + dy * DC_PITCH + dx;
                        const int diff = (int)s_d[q] - d, a = abs(diff);
                        const bool ok = s_st[q] == DS_KEPT && a <= t;
                        const unsigned qi = min(((unsigned)a * rq) >> 16, 16u);             // <= 16 for every member; the clamp bounds the read of a non-member
                        const int wgt = ok ? (int)s_ws[(dy < 0 ? -dy : dy) * 5 + (dx < 0 ? -dx : dx)] * (int)s_wr[qi] : 0;
                        num += (long long)wgt * diff;                                       // |wgt * diff| <= 65025 * 32767 < 2^31; the sum needs 64 bits
                        den += wgt;
                    }
                if (num != 0) {                                                             // den > 0: the centre is a member and ws[0][0] wr[0] > 0
                    const long long a2 = 2 * num + den, b2 = 2ll * den;
                    long long off = a2 / b2;
                    if (a2 - off * b2 < 0) --off;                                           // floor
                    o = min(max(d + (int)off, 1), 65535);
                }
            }
        }
        if (inside) {
            const int g = (f * A.h + py) * A.w + px;
            A.out[g] = (uint16_t)o;
            if (A.status) A.status[g] = (uint8_t)st;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) cnt[k] += popc64(__ballot(inside && st == k));
    }
    if (A.counts) {
        if (lane_id() == 0)
#pragma unroll
            for (int k = 0; k < 5; ++k) if (cnt[k]) atomicAdd(&s_cnt[k], cnt[k]);
        __syncthreads();
        if (tid < 5 && s_cnt[tid]) atomic_add_i64(reinterpret_cast<int64_t*>(A.counts) + f * 5 + tid, (long long)s_cnt[tid]);
    }
}

// one level of the pyramid: one lane per output pixel of all n frames
__global__ __launch_bounds__(256) void k_depth_halve(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, const uint16_t* __restrict__ tol, int n, int h, int w,
                                                     int h2, int w2, int min_valid)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n * h2 * w2) return;
    const int x = i % w2, r = i / w2, y = r % h2, f = r / h2;
    const uint16_t* p = src + ((size_t)(f * h + 2 * y) * w + 2 * x);
    unsigned d[4];
    if (((uintptr_t)p & 3) == 0) { const uint32_t v = *reinterpret_cast<const uint32_t*>(p); d[0] = v & 0xffffu; d[1] = v >> 16; }
    else { d[0] = p[0]; d[1] = p[1]; }
    const uint16_t* p1 = p + w;
    if (((uintptr_t)p1 & 3) == 0) { const uint32_t v = *reinterpret_cast<const uint32_t*>(p1); d[2] = v & 0xffffu; d[3] = v >> 16; }
    else { d[2] = p1[0]; d[3] = p1[1]; }
    unsigned ref = 0xffffffffu; int valid = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (d[k]) { ++valid; ref = min(ref, d[k]); }
    unsigned o = 0;
    if (valid >= min_valid) {                                                               // min_valid >= 1: ref is a depth
        const unsigned t = tol[ref >> 8];
        unsigned sum = 0, m = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (d[k] && d[k] - ref <= t) { sum += d[k]; ++m; }
        o = (2 * sum + m) / (2 * m);
    }
    dst[i] = (uint16_t)o;
}

}  // namespace tsl

struct tsl_depth {
    int device;
    hipStream_t stream;
    bool tables_set;
    uint32_t* tab;                       // DC_TAB_DWORDS dwords on the device
    void* sbuf; size_t sbuf_bytes;       // the staging buffer of the host-pointer form
    void* lbuf; size_t lbuf_bytes;       // levels the caller left out but a later level needs
};

namespace tsl {

struct DepthPlan { int n, h, w, levels; size_t px[4]; };     // px[l]: the pixels of all n frames at level l

// every check of both forms; nothing is launched or written before it passes
static int depth_check(tsl_depth* t, const tsl_depth_cfg* c, const void* depth, const void* out, const void* status, void* const* lvl, const char* who, DepthPlan* P)
{
    const std::string w = std::string(who) + ": ";
    TSL_REQUIRE(t, w + "null handle");
    TSL_REQUIRE(c && depth && out, w + "null cfg, depth or out");
    TSL_REQUIRE(t->tables_set, w + "the tables are not set (tsl_depth_set_tables)");
    TSL_REQUIRE(c->n >= 1 && c->n <= 64 && c->h >= 1 && c->h <= 8192 && c->w >= 1 && c->w <= 8192 && (int64_t)c->n * c->h * c->w <= (1ll << 28),
                w + "n must be 1 .. 64, h and w 1 .. 8192, n h w at most 2^28");
    TSL_REQUIRE(c->d_min_mm <= c->d_max_mm, w + "d_min_mm must not exceed d_max_mm");
    TSL_REQUIRE(c->min_support >= 0 && c->min_support <= 8, w + "min_support must be 0 .. 8");
    TSL_REQUIRE(c->erode >= 0 && c->erode <= 3, w + "erode must be 0 .. 3");
    TSL_REQUIRE(c->radius >= 0 && c->radius <= 4, w + "radius must be 0 .. 4");
    TSL_REQUIRE((c->flags & ~1) == 0, w + "unknown flag");
    TSL_REQUIRE(c->levels >= 0 && c->levels <= 3, w + "levels must be 0 .. 3");
    TSL_REQUIRE(c->min_valid >= 1 && c->min_valid <= 4, w + "min_valid must be 1 .. 4");
    TSL_REQUIRE((c->h >> c->levels) >= 1 && (c->w >> c->levels) >= 1, w + "a level asked for has no pixels");
    TSL_REQUIRE((((uintptr_t)depth | (uintptr_t)out) & 1) == 0, w + "depth and out must be 2-byte aligned");
    P->n = c->n; P->h = c->h; P->w = c->w; P->levels = c->levels;
    for (int l = 0; l <= 3; ++l) P->px[l] = l <= c->levels ? (size_t)c->n * (size_t)(c->h >> l) * (size_t)(c->w >> l) : 0;
    const uintptr_t a0 = (uintptr_t)depth, a1 = a0 + 2 * P->px[0];
    const void* outs[5] = { out, status, lvl[0], lvl[1], lvl[2] };
    const size_t bytes[5] = { 2 * P->px[0], P->px[0], 2 * P->px[1], 2 * P->px[2], 2 * P->px[3] };
    for (int k = 0; k < 5; ++k) {
        const uintptr_t b0 = (uintptr_t)outs[k];
        TSL_REQUIRE(!outs[k] || !bytes[k] || b0 >= a1 || b0 + bytes[k] <= a0, w + "an output overlaps the input");
        TSL_REQUIRE(k < 2 || ((uintptr_t)outs[k] & 1) == 0, w + "a level must be 2-byte aligned");
    }
    return TSL_OK;
}

// both forms after the checks: device pointers, everything queued on q
static int depth_launch(tsl_depth* t, hipStream_t q, const tsl_depth_cfg* c, const DepthPlan& P, const uint16_t* depth, uint16_t* out, uint8_t* status, long long* counts,
                        uint16_t* const* lvl)
{
    int last = 0;                                                                           // the last level somebody receives
    for (int l = 1; l <= P.levels; ++l) if (lvl[l - 1]) last = l;
    uint16_t* dst[4] = { out, nullptr, nullptr, nullptr };
    size_t need = 0, off[4] = { 0, 0, 0, 0 };
    for (int l = 1; l <= last; ++l) if (!lvl[l - 1]) { off[l] = need; need += (2 * P.px[l] + 15) & ~(size_t)15; }
    if (need) { const int rc = grow(&t->lbuf, &t->lbuf_bytes, need); if (rc) return rc; }
    for (int l = 1; l <= last; ++l) dst[l] = lvl[l - 1] ? lvl[l - 1] : reinterpret_cast<uint16_t*>((char*)t->lbuf + off[l]);
    if (counts) TSL_HIP(hipMemsetAsync(counts, 0, sizeof(long long) * 5 * (size_t)P.n, q));
    DepthArgs A = { depth, out, status, counts, t->tab, P.n, P.h, P.w, c->d_min_mm, c->d_max_mm, c->min_support, c->erode, c->flags & 1 };
    const dim3 grid((unsigned)((P.w + DC_TW - 1) / DC_TW), (unsigned)((P.h + DC_TH - 1) / DC_TH), (unsigned)P.n);
    switch (c->radius) {
    case 0: hipLaunchKernelGGL(k_depth_condition<0>, grid, dim3(256), 0, q, A); break;
    case 1: hipLaunchKernelGGL(k_depth_condition<1>, grid, dim3(256), 0, q, A); break;
    case 2: hipLaunchKernelGGL(k_depth_condition<2>, grid, dim3(256), 0, q, A); break;
    case 3: hipLaunchKernelGGL(k_depth_condition<3>, grid, dim3(256), 0, q, A); break;
    default: hipLaunchKernelGGL(k_depth_condition<4>, grid, dim3(256), 0, q, A); break;
    }
    TSL_HIP(hipGetLastError());
    for (int l = 1; l <= last; ++l) {
        const int h = P.h >> (l - 1), w = P.w >> (l - 1);
        hipLaunchKernelGGL(k_depth_halve, dim3((unsigned)((P.px[l] + 255) / 256)), dim3(256), 0, q, dst[l - 1], dst[l], reinterpret_cast<const uint16_t*>(t->tab), P.n, h, w,
                           h >> 1, w >> 1, c->min_valid);
        TSL_HIP(hipGetLastError());
    }
    return TSL_OK;
}

}  // namespace tsl

using namespace tsl;

extern "C" {

int tsl_depth_create(int device, tsl_depth** out)
{
    TSL_REQUIRE(out, "tsl_depth_create: null out"); *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available"); return TSL_ERR_NO_DEVICE; }
    TSL_REQUIRE(device >= 0 && device < ndev, "tsl_depth_create: bad device index");
    TSL_HIP(hipSetDevice(device));
    tsl_depth* t = new tsl_depth();                                                         // value-initialised: every pointer null
    t->device = device;
    if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess || hipMalloc((void**)&t->tab, sizeof(uint32_t) * DC_TAB_DWORDS) != hipSuccess) {
        set_error("tsl_depth_create: the stream or the table buffer could not be made");
        tsl_depth_destroy(t);
        return TSL_ERR_HIP;
    }
    *out = t;
    return TSL_OK;
}

void tsl_depth_destroy(tsl_depth* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
    void* ptrs[] = { t->tab, t->sbuf, t->lbuf };
    for (void* p : ptrs) if (p) (void)hipFree(p);                                           // hipFree waits for the device: a _dev call still running on a caller's stream ends first
    delete t;
}

int tsl_depth_set_tables(tsl_depth* t, const uint16_t* tol, const uint8_t* ws, const uint8_t* wr)
{
    TSL_REQUIRE(t, "tsl_depth_set_tables: null handle");
    TSL_REQUIRE(tol && ws && wr, "tsl_depth_set_tables: null table");
    for (int b = 0; b < 256; ++b) TSL_REQUIRE(tol[b] >= 1 && tol[b] <= 32767, "tsl_depth_set_tables: every tol entry must be 1 .. 32767");
    TSL_REQUIRE((int)ws[0] * (int)wr[0] > 0, "tsl_depth_set_tables: ws[0][0] * wr[0] must be positive");
    uint32_t tab[DC_TAB_DWORDS];
    std::memset(tab, 0, sizeof(tab));
    uint16_t* h_tol = reinterpret_cast<uint16_t*>(tab);
    uint8_t* h_w = reinterpret_cast<uint8_t*>(tab) + 1024;
    for (int b = 0; b < 256; ++b) {
        h_tol[b] = tol[b];
        const uint32_t rq = (16u << 16) / tol[b];
        h_tol[256 + b] = (uint16_t)(rq > 65535u ? 65535u : rq);
    }
    std::memcpy(h_w, ws, 25); std::memcpy(h_w + 32, wr, 17);
    TSL_HIP(hipSetDevice(t->device));
    TSL_HIP(hipDeviceSynchronize());                                                        // a _dev call on a caller's stream may still read the old tables
    TSL_HIP(hipMemcpy(t->tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    t->tables_set = true;
    return TSL_OK;
}

int tsl_depth_condition(tsl_depth* t, const tsl_depth_cfg* cfg, const uint16_t* depth, uint16_t* out, uint8_t* status, int64_t* counts, uint16_t* lvl1, uint16_t* lvl2,
                        uint16_t* lvl3)
{
    void* const lv[3] = { lvl1, lvl2, lvl3 };
    DepthPlan P;
    int rc = depth_check(t, cfg, depth, out, status, lv, "tsl_depth_condition", &P); if (rc) return rc;
    TSL_HIP(hipSetDevice(t->device));
    Stage st(&t->sbuf, &t->sbuf_bytes, t->stream);
    const int i_d = st.in(depth, 2 * P.px[0]), i_o = st.out(out, 2 * P.px[0]), i_s = st.out(status, P.px[0]), i_c = st.out(counts, sizeof(int64_t) * 5 * (size_t)P.n);
    int i_l[3];
    for (int l = 1; l <= 3; ++l) i_l[l - 1] = st.out(l <= P.levels ? lv[l - 1] : nullptr, 2 * P.px[l]);
    if ((rc = st.upload())) return rc;
    uint16_t* const dl[3] = { st.ptr<uint16_t>(i_l[0]), st.ptr<uint16_t>(i_l[1]), st.ptr<uint16_t>(i_l[2]) };
    if ((rc = depth_launch(t, t->stream, cfg, P, st.ptr<const uint16_t>(i_d), st.ptr<uint16_t>(i_o), st.ptr<uint8_t>(i_s), st.ptr<long long>(i_c), dl))) return rc;
    return st.download();
}

int tsl_depth_condition_dev(tsl_depth* t, const tsl_depth_cfg* cfg, const void* depth_dev, void* out_dev, void* status_dev, void* counts_dev, void* lvl1_dev,
                            void* lvl2_dev, void* lvl3_dev, void* user_stream)
{
    void* const lv[3] = { lvl1_dev, lvl2_dev, lvl3_dev };
    DepthPlan P;
    int rc = depth_check(t, cfg, depth_dev, out_dev, status_dev, lv, "tsl_depth_condition_dev", &P); if (rc) return rc;
    TSL_REQUIRE(((uintptr_t)counts_dev & 7) == 0, "tsl_depth_condition_dev: counts must be 8-byte aligned");
    TSL_HIP(hipSetDevice(t->device));
    uint16_t* const dl[3] = { (uint16_t*)(P.levels >= 1 ? lvl1_dev : nullptr), (uint16_t*)(P.levels >= 2 ? lvl2_dev : nullptr), (uint16_t*)(P.levels >= 3 ? lvl3_dev : nullptr) };
    return depth_launch(t, (hipStream_t)user_stream, cfg, P, (const uint16_t*)depth_dev, (uint16_t*)out_dev, (uint8_t*)status_dev, (long long*)counts_dev, dl);
}

}  // extern "C"

// tsl_stage.hpp -- how a host-pointer entry point is built from its _dev twin: one Stage per call lays the call's inputs and
// outputs out in ONE device buffer, copies the inputs up on the stream, and after the caller's launch waits for the stream and copies the outputs back.
//
//     Stage st(&m->xbuf, &m->xbuf_bytes, q);                     // q = ms(m)
//     const int i_a = st.in(a, bytes_a), i_b = st.out(b, bytes_b);       // inputs first, then outputs
//     if ((rc = st.upload())) return rc;                         // one grow, the inputs' hipMemcpyAsync on q
//     if ((rc = launch(m, q, ..., st.ptr<const float>(i_a), st.ptr<uint8_t>(i_b)))) return rc;      // the launch function of the _dev form
//     return st.download();                                      // hipStreamSynchronize(q), then the outputs' copies
//
// A null input (or one of 0 bytes) and a null output get no room and a null device pointer, so the launch function skips the plane as it does for the
// _dev form; out(host, bytes, true) keeps the room for a kernel that writes the plane unconditionally.  Every region starts at a multiple of 16 bytes.
//
// The buffer is the handle's staging buffer, xbuf; the topology graph stages in one of its own, sbuf.  Who else lives in xbuf: the sparse export /
// import and pack_pointcloud2 (tsl_tsdf.hip), the ESDF export (tsl_esdf.hip), the accumulator header and the staged image or cloud of the align / track
// calls and the accumulator, poses, scores and list of the register calls (tsl_align*.hip, tsl_register*.hip).  Reuse is safe because every one of them,
// and every call built on Stage, waits for the handle's stream before it returns, so no call finds the buffer in use, and because every copy here is
// queued on that stream, so it is also ordered behind whatever a _dev form left running there; grow() frees through hipFree, which waits for the device.
// The one exception is tsl_esdf_export_dev, which hands pointers INTO xbuf to its caller: they are valid until the next call that stages (its comment
// says so), which now includes the nav family.  The pinned pose table of view_gain (GainState) is another mechanism and is not staged here.
#pragma once
#include <cassert>
#include "tsl_tsdf.hpp"

namespace tsl {

struct Stage {
    enum { MAX_REGIONS = 12 };
    struct Region { void* host; size_t bytes, off; bool out, live; };
    void** buf; size_t* have; hipStream_t q;
    Region r[MAX_REGIONS]; int n = 0; size_t total = 0;

    Stage(void** buf_, size_t* have_, hipStream_t q_) : buf(buf_), have(have_), q(q_) {}

    int in(const void* host, size_t bytes) { return add(const_cast<void*>(host), bytes, false, host && bytes); }
    int out(void* host, size_t bytes, bool always = false) { return add(host, bytes, true, host || always); }

    int upload()
    {
        const int rc = grow(buf, have, total + 64); if (rc) return rc;
        for (int i = 0; i < n; ++i)
            if (r[i].live && !r[i].out) TSL_HIP(hipMemcpyAsync(at(i), r[i].host, r[i].bytes, hipMemcpyHostToDevice, q));
        return TSL_OK;
    }
    template <class T> T* ptr(int i) const { return r[i].live ? (T*)at(i) : nullptr; }      // valid after upload()
    int download()
    {
        TSL_HIP(hipStreamSynchronize(q));
        for (int i = 0; i < n; ++i)
            if (r[i].out && r[i].host) TSL_HIP(hipMemcpy(r[i].host, at(i), r[i].bytes, hipMemcpyDeviceToHost));
        return TSL_OK;
    }

private:
    char* at(int i) const { return (char*)*buf + r[i].off; }
    int add(void* host, size_t bytes, bool out_, bool live)
    {
        assert(n < MAX_REGIONS);
        r[n] = { host, bytes, total, out_, live };
        if (live) total += (bytes + 15) & ~(size_t)15;
        return n++;
    }
};

}  // namespace tsl

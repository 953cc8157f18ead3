// host_util.h -- host-side helpers shared by the *_api.cpp files of libofc.so: scratch that grows on demand, the per-device
// pool it lives in, and the events and streams of the measurement hooks.  Included by .cpp files only; no device code.
#pragma once
#include "ofc_common.h"

namespace ofc {

// room for `need` bytes: allocates only when the buffer is smaller, and keeps the contents otherwise.  Every buffer is
// measured against its own size; a failed allocation leaves it empty (DevBuf::alloc releases first), so the next call
// tries again.
inline int reserve(DevBuf &b, size_t need)
{
    if (b.bytes >= need) return OFC_OK;
    return b.alloc(need);
}

// the library's scratch of type T, one per device
template <class T> T &device_scratch(int device)
{
    static T *pool = new T[16];        // intentionally never destroyed (no HIP calls at exit)
    return pool[device & 15];
}

// a stream of a measurement hook, destroyed whichever way the hook ends
struct ScopedStream {
    hipStream_t s = nullptr;
    ScopedStream() = default;
    ScopedStream(const ScopedStream &) = delete;
    ScopedStream &operator=(const ScopedStream &) = delete;
    ~ScopedStream() { if (s) (void)hipStreamDestroy(s); }
    int create()
    {
        OFC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return OFC_OK;
    }
};

// the two timing events of a measurement hook, destroyed whichever way the hook ends
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int create()
    {
        OFC_HIP(hipEventCreate(&e0));
        OFC_HIP(hipEventCreate(&e1));
        return OFC_OK;
    }
    // waits for e1 and adds the milliseconds from e0 to e1 to `total`
    int add_elapsed(double &total)
    {
        OFC_HIP(hipEventSynchronize(e1));
        float ms = 0;
        OFC_HIP(hipEventElapsedTime(&ms, e0, e1));
        total += ms;
        return OFC_OK;
    }
};

// the block-timed measurement hooks: `warmup` untimed launches, then the average of `iters` by HIP events on the stream
template <class F> int time_launches(hipStream_t s, int iters, F &&launch, float *ms_per_launch, int warmup = 2)
{
    EventPair ev;
    OFC_TRY(ev.create());
    for (int w = 0; w < warmup; w++) OFC_TRY(launch());
    OFC_HIP(hipEventRecord(ev.e0, s));
    for (int i = 0; i < iters; i++) OFC_TRY(launch());
    OFC_HIP(hipEventRecord(ev.e1, s));
    double ms = 0;
    OFC_TRY(ev.add_elapsed(ms));
    *ms_per_launch = (float)ms / iters;
    return OFC_OK;
}

}  // namespace ofc

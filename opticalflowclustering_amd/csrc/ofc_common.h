// ofc_common.h -- shared host-side plumbing of libofc.so (error reporting, HIP checks, device
// buffers).  gfx950 only; no CUDA-compat paths.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ofc.h"

namespace ofc {

void set_error(const char *fmt, ...);
int ensure_device(int device);   // validates + hipSetDevice; returns OFC_OK / OFC_ENODEV

#define OFC_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ofc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                           __LINE__);                                                         \
            return _e == hipErrorOutOfMemory ? OFC_ENOMEM : OFC_EHIP;                         \
        }                                                                                     \
    } while (0)

#define OFC_TRY(expr)                    \
    do {                                 \
        int _rc = (expr);                \
        if (_rc != OFC_OK) return _rc;   \
    } while (0)

#define OFC_REQUIRE(cond, ...)           \
    do {                                 \
        if (!(cond)) {                   \
            ofc::set_error(__VA_ARGS__); \
            return OFC_EINVAL;           \
        }                                \
    } while (0)

// RAII device buffer (host-side bookkeeping only)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t n)
    {
        release();
        if (n == 0) return OFC_OK;
        OFC_HIP(hipMalloc(&p, n));
        bytes = n;
        return OFC_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace ofc

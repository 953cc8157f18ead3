// ofc_api.cpp -- C ABI of libofc.so, the library basics: the error string, device selection, the Farneback geometry and
// constants every flow file shares, and the memory plumbing (ofc_version .. ofc_device_sync).  The flow engine is in
// flow_engine.cpp, its single-stage and bench hooks in flow_stages_api.cpp.
// Declared in include/ofc.h (which cites the reference call each entry point replaces).
#include "flow_host.h"

#include <cfloat>
#include <cmath>

namespace ofc {

static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

int ensure_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no usable GPU (hipGetDeviceCount: %s, count %d); libofc has no CPU fallback",
                  hipGetErrorString(e), n);
        return OFC_ENODEV;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (have %d)", device, n);
        return OFC_ENODEV;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_error("hipSetDevice(%d): %s", device, hipGetErrorString(e));
        return OFC_ENODEV;
    }
    return OFC_OK;
}

// ---- geometry & constants (host) ----
int pyramid_levels(int W, int H, const ofc_fb_params &p)
{
    const int min_size = 32;
    int k;
    double scale = 1;
    for (k = 0; k < p.levels; k++) {
        scale *= p.pyr_scale;
        if (W * scale < min_size || H * scale < min_size) break;
    }
    return k;
}

LevelGeom level_geometry(int W, int H, const ofc_fb_params &p, int k)
{
    double scale = 1;
    for (int i = 0; i < k; i++) scale *= p.pyr_scale;
    LevelGeom g;
    g.sigma = (1. / scale - 1) * 0.5;
    int sz = (int)std::nearbyint(g.sigma * 5) | 1;   // cvRound: half to even
    g.ksize = sz < 3 ? 3 : sz;
    g.w = (int)std::nearbyint(W * scale);
    g.h = (int)std::nearbyint(H * scale);
    return g;
}

void gaussian_kernel(int n, double sigma, float *k)
{
    static const float tab[4][7] = {{1.f},
                                    {0.25f, 0.5f, 0.25f},
                                    {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                    {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    const float *fixed = (n % 2 == 1 && n <= 7 && sigma <= 0) ? tab[n >> 1] : nullptr;
    double sigmaX = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    double scale2X = -0.5 / (sigmaX * sigmaX), sum = 0;
    for (int i = 0; i < n; i++) {
        double x = i - (n - 1) * 0.5;
        double t = fixed ? (double)fixed[i] : std::exp(scale2X * x * x);
        k[i] = (float)t;
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) k[i] = (float)(k[i] * sum);
}

void polyexp_setup(int n, double sigma, PolyConsts &c)
{
    if (sigma < FLT_EPSILON) sigma = n * 0.3;
    std::vector<float> gf(2 * n + 1);
    double s = 0;
    for (int x = -n; x <= n; x++) {
        gf[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma));
        s += gf[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) gf[x + n] = (float)(gf[x + n] * s);
    memset(&c, 0, sizeof(c));
    c.n = n;
    for (int x = 0; x <= n && x < 8; x++) {
        c.g[x] = gf[x + n];
        c.xg[x] = (float)(x * c.g[x]);
        c.xxg[x] = (float)(x * x * c.g[x]);
    }
    double G00 = 0, G11 = 0, G33 = 0, G55 = 0;
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            float gg = gf[y + n] * gf[x + n];
            G00 += gg;
            G11 += gg * x * x;
            G33 += gg * x * x * x * x;
            G55 += gg * x * x * y * y;
        }
    double a = G00, b = G11, cc = G33, e = G55;
    double det = a * (cc * cc - e * e) - 2 * b * b * (cc - e);
    c.ig11 = 1. / G11;
    c.ig03 = -b * (cc - e) / det;
    c.ig33 = (a * cc - b * b) / det;
    c.ig55 = 1. / G55;
}

int check_frame_and_fb_params(const ofc_fb_params &p, int W, int H)
{
    OFC_REQUIRE(W >= 16 && H >= 16 && W <= 16384 && H <= 16384, "frame size %dx%d out of range", W, H);
    OFC_REQUIRE(p.pyr_scale > 0 && p.pyr_scale < 1, "pyr_scale must be in (0,1)");
    OFC_REQUIRE(p.levels >= 0 && p.levels <= 16, "levels out of range");
    OFC_REQUIRE(p.iterations >= 1 && p.iterations <= 64, "iterations out of range");
    if (p.flags != 0) {
        set_error("flags=%d: only the box-filter variant (flags 0) the reference uses is implemented", p.flags);
        return OFC_EUNSUPPORTED;
    }
    if ((p.winsize & 1) && p.winsize > OFC_WINSIZE_MAX) {      // (even windows: OFC_EINVAL where a window is used)
        set_error("winsize %d unsupported (odd 5..%d)", p.winsize, OFC_WINSIZE_MAX);
        return OFC_EUNSUPPORTED;
    }
    return polyexp_n_check(p.poly_n);
}

}  // namespace ofc

using namespace ofc;

// =================================================================================================
// plumbing
// =================================================================================================
extern "C" {

int ofc_version(void) { return OFC_VERSION; }
const char *ofc_last_error(void) { return g_err.c_str(); }

int ofc_device_count(int *n)
{
    OFC_REQUIRE(n, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
    return OFC_OK;
}

int ofc_malloc(int device, size_t bytes, void **dptr)
{
    OFC_REQUIRE(dptr, "null pointer");
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMalloc(dptr, bytes));
    return OFC_OK;
}

int ofc_free(int device, void *dptr)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipFree(dptr));
    return OFC_OK;
}

int ofc_memcpy_h2d(int device, void *dst, const void *src, size_t bytes)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return OFC_OK;
}

int ofc_memcpy_d2h(int device, void *dst, const void *src, size_t bytes)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_memset(int device, void *dst, int value, size_t bytes)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipMemset(dst, value, bytes));
    return OFC_OK;
}

int ofc_device_sync(int device)
{
    OFC_TRY(ensure_device(device));
    OFC_HIP(hipDeviceSynchronize());
    return OFC_OK;
}

void ofc_fb_default_params(ofc_fb_params *p)
{
    if (!p) return;
    p->pyr_scale = 0.5; p->levels = 3; p->winsize = 15; p->iterations = 3;
    p->poly_n = 5; p->poly_sigma = 1.2; p->flags = 0;
}

}  // extern "C"

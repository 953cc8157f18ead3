// traj_step.h -- one step of a followed point (rules 1-4 of the trajectories block of include/ofc.h), shared by the
// trajectory kernel (trajectories.hip) and the tracklet kernels (tracklets.hip).  Device code only.
#pragma once
#include "fb_check.h"

namespace ofc {

// The step of a point at (X, Y) through the field F [H][W] (and the state bytes S [H][W] when STATE).  The four 8-byte tap
// gathers and the state byte are issued together before any is used, and only for a live point; every index comes from the
// position clamped into the frame, whatever X, Y and the field hold.  Returns OFC_TRAJ_RAN and moves (X, Y) when the step is
// taken; otherwise the reason, and (X, Y) stay.  A point that is not live gets OFC_TRAJ_RAN and stays: the caller knows.
template <bool STATE>
__device__ __forceinline__ int traj_step(const float2 *__restrict__ F, const uint8_t *__restrict__ S, int W, int H, unsigned keep,
                                         bool live, int &X, int &Y)
{
    typedef long long i64;
    const int xmax = (W - 1) << 16, ymax = (H - 1) << 16;              // W, H <= 16384: below 2^30
    // everything that indexes comes from the clamped position; a live point past step 0 is inside, so nothing changes for it
    const int Xc = min(max(X, 0), xmax), Yc = min(max(Y, 0), ymax);
    const bool inside = Xc == X && Yc == Y;
    const int ix = Xc >> 16, iy = Yc >> 16;                            // in [0, W-1], [0, H-1]
    const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
    const int rx = min((Xc + 32768) >> 16, W - 1), ry = min((Yc + 32768) >> 16, H - 1);
    float2 f0 = make_float2(0.f, 0.f), f1 = f0, f2 = f0, f3 = f0;
    unsigned sb = 0;
    if (live) {                                                        // the five loads of the step, none used before all are issued
        f0 = F[iy * W + ix];
        f1 = F[iy * W + ix1];
        f2 = F[iy1 * W + ix];
        f3 = F[iy1 * W + ix1];
        if (STATE) sb = S[(size_t)(ry * W + rx)];
    }
    const FbVec q0 = fb_quantise(f0), q1 = fb_quantise(f1), q2 = fb_quantise(f2), q3 = fb_quantise(f3);
    const i64 fx = Xc & 65535, fy = Yc & 65535;
    const i64 w0 = (65536 - fx) * (65536 - fy), w1 = fx * (65536 - fy), w2 = (65536 - fx) * fy, w3 = fx * fy;
    const i64 Sx = w0 * q0.qu + w1 * q1.qu + w2 * q2.qu + w3 * q3.qu;      // |S| <= 2^32 * 2^26
    const i64 Sy = w0 * q0.qv + w1 * q1.qv + w2 * q2.qv + w3 * q3.qv;
    const int Xn = Xc + (int)((Sx + (1ll << 31)) >> 32), Yn = Yc + (int)((Sy + (1ll << 31)) >> 32);   // < 2^30 + 2^26
    int reason = OFC_TRAJ_RAN;
    if (live) {
        const bool trusted = !STATE || (sb < 4u && ((keep >> sb) & 1u));
        const bool valid = q0.valid && q1.valid && q2.valid && q3.valid;
        const bool lands = Xn >= 0 && Xn <= xmax && Yn >= 0 && Yn <= ymax;
        if (!inside) reason = OFC_TRAJ_LEAVES;
        else if (!trusted) reason = OFC_TRAJ_UNTRUSTED;
        else if (!valid) reason = OFC_TRAJ_INVALID;
        else if (!lands) reason = OFC_TRAJ_LEAVES;
        if (reason == OFC_TRAJ_RAN) X = Xn, Y = Yn;
    }
    return reason;
}

}  // namespace ofc

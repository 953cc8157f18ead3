// motion_model.h -- per-pair camera motion (motion_model.hip, motion_api.cpp, stream_api.cpp): the per-pair device record,
// the least-squares solve that the device and the host share, and the launchers.  include/ofc.h has the definition.
#pragma once
#include "ofc_common.h"

namespace ofc {

constexpr int MOTION_NMOM = 13;        // n, SX, SY, SXX, SXY, SYY, Squ, SXqu, SYqu, Sqv, SXqv, SYqv, outside
constexpr int MOTION_SHARE = 2048;     // consecutive vectors of a pair a work-group takes at a time
constexpr int MOTION_MAX_PAIRS = 65535;

// What the kernels know about one pair: the model of the round before (the moment kernel selects by it, the subtraction
// removes it) and where its fit stands.  All zero = "every valid pixel, nothing fitted yet".
struct MotionRec {
    double p[6];
    double c2;       // the squared threshold the next moment launch selects with (use != 0)
    int use;         // 0: every valid pixel; 1: those within c2 of p
    int status;      // 0 fitted; 1 a later round could not be solved, p is the round before's; 2 round 0 could not, p = 0
};

#if defined(__HIPCC__)
#define OFC_HD __host__ __device__
#else
#define OFC_HD
#endif

OFC_HD inline int motion_ilog2(int64_t v)      // floor(log2(v)), v >= 1
{
    int e = 0;
    while ((v >> e) > 1) e++;
    return e;
}
// the power of two 2^-e with 2^e about the root mean square of a coordinate whose squares sum to sqq over n pixels
OFC_HD inline double motion_coord_scale(int64_t sqq, int64_t n)
{
    if (sqq <= 0) return 1.0;
    const int d = motion_ilog2(sqq) - motion_ilog2(n);
    const int e = d >= 0 ? d / 2 : -((1 - d) / 2);
    return ldexp(1.0, -e);
}

// The exact least-squares model of the integer moments m (include/ofc.h), rounded as f64 arithmetic rounds it: the 3 x 3
// normal matrix over (1, X sx, Y sy), sx and sy powers of two so that its entries are O(n), factored once as L D L^T
// (Cholesky without the square roots: the pivots are D's entries) and used for u and for v.  kind 1 translation, 2 affine.
// false (p untouched): fewer than 3 pixels (translation: 1), or a pivot that is not positive.
// Host and device run this one function and must give equal bits: no contraction into fma, which only the device would do.
OFC_HD inline bool motion_solve(const int64_t *m, int kind, double *p)
{
#pragma clang fp contract(off)
    const int64_t n = m[0];
    const double q = 1.0 / 65536.0;
    if (kind == 1) {
        if (n < 1) return false;
        p[0] = (double)m[6] / (double)n * q;
        p[3] = (double)m[9] / (double)n * q;
        p[1] = p[2] = p[4] = p[5] = 0.0;
        return true;
    }
    if (n < 3) return false;
    const double sx = motion_coord_scale(m[3], n), sy = motion_coord_scale(m[5], n);
    const double a00 = (double)n, a01 = (double)m[1] * sx, a02 = (double)m[2] * sy;
    const double a11 = (double)m[3] * sx * sx, a12 = (double)m[4] * sx * sy, a22 = (double)m[5] * sy * sy;
    const double d0 = a00;
    const double l10 = a01 / d0, l20 = a02 / d0;
    const double d1 = a11 - l10 * a01;
    if (!(d1 > 0.0)) return false;
    const double l21 = (a12 - l20 * a01) / d1;
    const double d2 = a22 - l20 * a02 - l21 * l21 * d1;
    if (!(d2 > 0.0)) return false;
    for (int c = 0; c < 2; c++) {
        const int64_t *b = m + 6 + 3 * c;
        const double z0 = (double)b[0], z1 = (double)b[1] * sx - l10 * z0, z2 = (double)b[2] * sy - l20 * z0 - l21 * z1;
        const double x2 = z2 / d2, x1 = z1 / d1 - l21 * x2, x0 = z0 / d0 - l10 * x1 - l20 * x2;
        p[3 * c] = x0 * q;
        p[3 * c + 1] = x1 * sx * (2.0 * q);     // per unit of X/2
        p[3 * c + 2] = x2 * sy * (2.0 * q);
    }
    return true;
}

// Launch geometry of k_motion_moments and k_motion_subtract, in one place for the kernels, the launchers and
// ofc_motion_launch_geometry: a pair's field is nshare shares of MOTION_SHARE vectors, `groups` work-groups per pair take
// `per` consecutive shares each (the last used one what is left, the ones after it none).
OFC_HD inline int motion_nshare(int W, int H) { return (int)(((int64_t)W * H + MOTION_SHARE - 1) / MOTION_SHARE); }
OFC_HD inline int motion_per(int nshare, int groups) { return (nshare + groups - 1) / groups; }
OFC_HD inline int motion_groups_of(int nshare, int npair)
{
    const int want = 2048 / (npair > 1 ? npair : 1);
    const int capped = want < 256 ? want : 256, floored = capped > 16 ? capped : 16;
    return nshare < floored ? nshare : floored;
}

// ---- motion_model.hip ----
// OFC_OK, OFC_EINVAL or OFC_EUNSUPPORTED (message set): what ofc_motion_check documents.  Host only.
int motion_check(int W, int H, int kind);
// the same plus the rounds: T in 0..8, thresholds[0..T) finite and positive (may be NULL when T = 0)
int motion_fit_check(int W, int H, int kind, const double *thresholds, int T);
// work-groups per pair of the moment kernel, and so partial records per pair
int motion_groups(int W, int H, int npair);
// out = groups, per, the groups that get at least one share, the shares of the last of those.  Host only.
void motion_launch_geometry(int W, int H, int npair, int out[4]);
// one launch of the reduction: partial[npair][groups][13].  affine = false leaves the coordinate moments 0.
int launch_motion_moments(const float *flow, int W, int H, int npair, const MotionRec *rec, int64_t *partial, bool affine,
                          hipStream_t s);
// folds the partials of `round`, solves, writes rec for the next round (selecting with c_next) and, where not NULL, the
// history: hist_models[round][npair][6], hist_moments[round][npair][13]
int launch_motion_solve(const int64_t *partial, int groups, int npair, int kind, int round, double c_next, MotionRec *rec,
                        double *hist_models, int64_t *hist_moments, hipStream_t s);
// a whole fit, T + 1 moment launches and T + 1 solves on s, no host round trip: rec (npair, zeroed here) ends as the fit
int motion_fit_async(const float *flow, int W, int H, int npair, int kind, const double *thresholds, int T, MotionRec *rec,
                     int64_t *partial, double *hist_models, int64_t *hist_moments, hipStream_t s);
// dst = flow minus rec's models (dst may be flow)
int launch_motion_subtract(const float *flow, float *dst, int W, int H, int npair, const MotionRec *rec, hipStream_t s);

}  // namespace ofc

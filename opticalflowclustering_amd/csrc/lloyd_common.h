// lloyd_common.h -- device-side state and launcher prototypes of the Lloyd kernels.
#pragma once
#include "ofc_common.h"
#include "lloyd_field.h"

#include <cmath>

namespace ofc {

constexpr int LLOYD_KMAX = 16;   // streaming / batched kernels keep per-lane partials in registers
constexpr int LLOYD_DMAX = 4;

// lives in device memory; centres are stored CENTRED (x - column mean), as sklearn iterates
struct LloydState {
    double mean[LLOYD_DMAX];
    double centers[LLOYD_KMAX * LLOYD_DMAX];      // current (old) centres, row-major k x d
    double centers_new[LLOYD_KMAX * LLOYD_DMAX];
    double cn[LLOYD_KMAX];                        // |c_j|^2 (FMA chain)
    double tol;                                   // sklearn's tol (mean column variance * tol_rel), set by iteration 0
    int halt;                                     // set by k_lloyd_update on convergence / empty cluster: the iterations
    int pad;                                      // that were enqueued speculatively behind it become no-ops
    // tile pruning (lloyd_tiles.hip): decided on the device, iteration by iteration, from the all-reduced tile counts
    int prune_policy;                             // LLOYD_PRUNE_*: set by the host before iteration 0
    int prune_mode;                               // how the NEXT k_lloyd_tiles sweep runs: LLOYD_TILES_*
    int prune_cooldown, prune_backoff;            // full sweeps left before the next probe / its current spacing
};

// how a k_lloyd_tiles sweep treats the 64-sample tiles
enum { LLOYD_TILES_FULL = 0,      // every tile sample by sample (no metadata read)
       LLOYD_TILES_PRUNED = 1,    // box test per tile: cached sums for tiles wholly inside one Voronoi cell, the rest by sample
       LLOYD_TILES_PROBE = 2 };   // box test only counted, every tile still by sample (decides whether to switch to PRUNED)
enum { LLOYD_PRUNE_OFF = 0, LLOYD_PRUNE_AUTO = 1, LLOYD_PRUNE_ON = 2, LLOYD_PRUNE_ALWAYS = 3 };

// written by k_lloyd_update into pinned host memory once per iteration (one slot per iteration of a window)
struct LloydStatus {
    double n_changed;
    double shift_tot;
    int n_empty;
    int valid;        // the iteration ran (0: it was a no-op behind a halt)
    int converged;    // strict or tol stop reached in this iteration
    int strict;       // ... by labels == labels_old
    double tol;
    double counts[LLOYD_KMAX];
    double sqsum[LLOYD_DMAX];     // sum (x-mean)^2 per column (first iteration only)
    double tiles_tested, tiles_pure;   // k_lloyd_tiles: tiles box-tested (or checked for uniform labels while the metadata
    int tiles_mode;                    // is built) / found inside one cell; mode the sweep ran in (-1: not a tile sweep)
    int tiles_next;                    // mode chosen for the next tile sweep (LLOYD_TILES_*)
};

int lloyd_kmax(int k);
int launch_lloyd_colstats(const void *X, int dtype, int64_t N, int d, const double *mean, int pass,
                          double *partial, int nblocks, hipStream_t s);
// halt != nullptr: skip when *halt != 0 (device flag)
int launch_reduce_records(const double *partial, int nblocks, int nv, double *out, hipStream_t s,
                          const int *halt = nullptr);
// mode 0: labels only; 1: labels + M-step record (+ column sums of (x-mean)^2 when first != 0); 2: labels + inertia;
// 3: M-step record only (labels untouched, n_changed = 0)
// record = [kmax*d sums][kmax counts][n_changed][LLOYD_DMAX squared sums][tiles tested][tiles pure]
int launch_lloyd_assign(const void *X, int dtype, int64_t N, int d, int k, const LloydState *st,
                        uint8_t *labels, double *partial, int nblocks, int mode, int first, hipStream_t s);
constexpr int LLOYD_REC_EXTRA = 1 + LLOYD_DMAX + 2;     // slots behind the sums and counts
constexpr int LLOYD_NVMAX = LLOYD_KMAX * LLOYD_DMAX + LLOYD_KMAX + LLOYD_REC_EXTRA;
inline int lloyd_record_len(int kmax, int d) { return kmax * d + kmax + LLOYD_REC_EXTRA; }
// (u,v) stream (f32, d = 2, k <= 8) in 64-sample tiles, see lloyd_tiles.hip.
//   LLOYD_WHAT_PROBE  before anything else: box test of a 1/64 sample of the tiles against the initial centres; sets
//                     st->prune_mode, and st->prune_policy = OFF on the device when the field is too incoherent to pay
//   LLOYD_WHAT_META   before iteration 0: box[N/64] (lo_u, lo_v, hi_u, hi_v), tsum[N/64] (sum of the centred samples),
//                     tsq[N/64] (scatter about the tile's own mean) written; partial[block][2] = column sums of (x-mean)^2
//                     (returns at once, records zeroed, when the probe switched the policy off)
//   LLOYD_WHAT_SWEEP  one label-less iteration in st->prune_mode; meta != nullptr: iteration 0 (meta = the reduced META
//                     record, device pointer: its sums of squares ride along).  Record as launch_lloyd_assign's mode 3
//   LLOYD_WHAT_FINAL  the final E-step (labels written, partial[block] = inertia share)
enum { LLOYD_WHAT_SWEEP = 0, LLOYD_WHAT_META = 1, LLOYD_WHAT_FINAL = 2, LLOYD_WHAT_PROBE = 3 };
bool lloyd_tiles_supported(int dtype, int d, int k);
int launch_lloyd_tiles(const float *X, int64_t N, int k, const LloydState *st, void *box, void *tsum, void *tsq,
                       uint8_t *labels, double *partial, int nblocks, int what, const double *meta, hipStream_t s);
// The same four launches over a stack of fields of width W cut into 2-D tiles under 64 x 8-pixel groups (lloyd_field.h;
// N a multiple of 8 W).  Tile records as above but group-major, N/64 of each; group records gbox / gsum / gsq, N/512 of each.
struct LloydFieldBufs {
    void *box, *tsum, *tsq, *gbox, *gsum, *gsq;
    int W;
};
int launch_lloyd_tiles_field(const float *X, int64_t N, int k, const LloydState *st, const LloydFieldBufs &f, uint8_t *labels,
                             double *partial, int nblocks, int what, const double *meta, hipStream_t s);
// tiles: 0 = the sweep was not a k_lloyd_tiles one, otherwise it ran in st->prune_mode (1: iteration 0)
int launch_lloyd_update(LloydState *st, const double *tot, int k, int d, int after_reloc, int labelled, int first,
                        double n_total, double tol_rel, LloydStatus *status, hipStream_t s, int tiles = 0);
constexpr int LLOYD_WINDOW = 16;    // most iterations enqueued per host synchronisation (windows grow 4, 8, 16, 16, ...)
int launch_lloyd_set_centers(LloydState *st, int k, int d, hipStream_t s, int prune_policy = 0);
int launch_lloyd_inertia(const void *X, int dtype, int64_t N, int d, const LloydState *st,
                         const uint8_t *labels, double *partial, int nblocks, hipStream_t s);
// grid_labels.hip: the E-step's label of every pixel of flow [n_frames][H][W][2] against st (mean, centres, cn set), counted
// per grid cell as launch_grid_label_counts counts a label buffer: counts [n_frames][rows*cols][k], sums (or nullptr)
// [n_frames][rows*cols][k][2]
int launch_grid_assign_counts(const float *flow, const LloydState *st, int W, int H, int n_frames, int rows, int cols, int k,
                              int32_t *counts, double *sums, hipStream_t s);
// OFC_OK, or the refusal of a model both fused entry points share: k outside 1 .. LLOYD_KMAX (OFC_EUNSUPPORTED), a mean
// (may be nullptr) or a centre that is not finite (OFC_EINVAL)
inline int check_uv_model(int k, const double *mean, const double *centers_c)
{
    OFC_REQUIRE(centers_c, "null pointer");
    if (k < 1 || k > LLOYD_KMAX) {
        set_error("k=%d outside the kernel's range (1..%d)", k, LLOYD_KMAX);
        return OFC_EUNSUPPORTED;
    }
    for (int i = 0; i < 2; i++) OFC_REQUIRE(!mean || std::isfinite(mean[i]), "mean[%d] is not finite", i);
    for (int i = 0; i < 2 * k; i++) OFC_REQUIRE(std::isfinite(centers_c[i]), "centre %d is not finite", i / 2);
    return OFC_OK;
}
int launch_lloyd_farthest(const void *X, int dtype, int64_t N, int d, const LloydState *st,
                          const double *c_old, const uint8_t *labels, const int64_t *excl, int n_excl,
                          double *out, int nblocks, hipStream_t s);

// the sweeps with sample weights (lloyd_weighted.hip): W is N weights of w_dtype (OFC_F32 / OFC_F64, 16-byte aligned).
// mode 1 / 2 / 3 and the record as launch_lloyd_assign's, with the weight sums in the count slots and the inertia weighted
int launch_lloyd_assign_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, int k,
                          const LloydState *st, uint8_t *labels, double *partial, int nblocks, int mode, int first,
                          hipStream_t s);
int launch_lloyd_inertia_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, const LloydState *st,
                           const uint8_t *labels, double *partial, int nblocks, hipStream_t s);
// w[i] = |flow[i]| (kind 0) or flow[i] . flow[i] >= thr^2 ? 1 : 0 (kind 1) over n (u,v) vectors, f32
int launch_flow_weights(const float *flow, int64_t n, int kind, float thr, float *w, hipStream_t s);

// k-means++ seeding step; partial: [nblocks][8] potentials per candidate
int launch_kpp_candidates(const void *X, int dtype, int64_t N, int d, const double *mean, const double *cand_centred,
                          int n_cand, const double *closest, double *out, double *partial, int nblocks, hipStream_t s);

// k-means++ seeding on resident samples (lloyd_seed.hip).  closest[N] f64 lives on the device; how a kernel sees it:
enum { KPP_PREV_NONE = 0,     // as stored
       KPP_PREV_APPLY = 1,    // min(stored, d(x, prev)): the previous step's winner is folded in (the sweep stores that)
       KPP_PREV_FIRST = 2 };  // d(x, prev): nothing stored yet, prev is the first centre (the sweep stores that)
constexpr int64_t KPP_NMAX = 1ll << 30;      // samples per rank: k_kpp_sample scans <= 1024 sums of 1024 chunk sums
inline int64_t kpp_chunks(int64_t N) { return (N + OFC_KPP_CHUNK - 1) / OFC_KPP_CHUNK; }
// one seeding step's sweep: cs[c][kpp_chunks(N)] = per-chunk sums of min(closest, d(x, cand c)) for c < max(n_cand, 1)
// (n_cand == 0: of closest itself, slot 0), partial[block][8] = potential shares.  mean, prev, cand_centred: host
int launch_kpp_sweep(const void *X, int dtype, int64_t N, int d, const double *mean, const double *prev, int prev_mode,
                     const double *cand_centred, int n_cand, double *closest, double *cs, double *partial, int nblocks,
                     hipStream_t s);
int launch_kpp_sum1024(const double *in, int64_t n, double *out, hipStream_t s);     // out[b] = sum in[1024 b ..)
// idx[j] = min(smallest i with base + cumsum(closest)[i] >= r[j], N - 1), rows[j][LLOYD_DMAX] = X[idx[j]], j < n <= 8;
// cs = launch_kpp_sweep's chunk sums of that closest, ss = launch_kpp_sum1024 of cs.  X == nullptr: closest is a plain
// weight vector (prev_mode NONE, no rows).  1 <= N <= KPP_NMAX
int launch_kpp_sample(const void *X, int dtype, int64_t N, int d, const double *mean, const double *prev, int prev_mode,
                      const double *closest, const double *cs, const double *ss, const double *r, int n, double base,
                      int64_t *idx, double *rows, hipStream_t s);

// the same with sample weights W (N of w_dtype, OFC_F32 / OFC_F64, 16-byte aligned): closest[] stays unweighted, every
// sum is of w[i] * value[i] with the product rounded on its own
int launch_kpp_sweep_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, const double *mean,
                       const double *prev, int prev_mode, const double *cand_centred, int n_cand, double *closest,
                       double *cs, double *partial, int nblocks, hipStream_t s);
// cs[kpp_chunks(N)] = per-chunk sums of (double)w[i] * v[i] (v == nullptr: of (double)w[i])
int launch_kpp_wchunks(const void *W, int w_dtype, const double *v, int64_t N, double *cs, hipStream_t s);
// total[0] = sum of ss[0..nsuper), nsuper <= 1024, in the order the sampling kernels accumulate it
int launch_kpp_total(const double *ss, int nsuper, double *total, hipStream_t s);
enum { KPP_SIDE_LEFT = 0,     // smallest i with cum[i] >= r, N - 1 when there is none (np.searchsorted, clipped)
       KPP_SIDE_RIGHT = 1,    // smallest i with cum[i] >  r, N - 1 when there is none
       KPP_SIDE_FIRST = 2 };  // the first centre: as RIGHT over rows of positive value only; when rounding leaves no
                              // hit, the last row of positive value (RandomState.choice never returns a p = 0 row)
// launch_kpp_sample over cum = base + cumsum(w * closest) (closest == nullptr: cumsum(w)), cs / ss its chunk sums
int launch_kpp_sample_w(const void *X, int dtype, const void *W, int w_dtype, int64_t N, int d, const double *mean,
                        const double *prev, int prev_mode, const double *closest, const double *cs, const double *ss,
                        const double *r, int n, double base, int side, int64_t *idx, double *rows, hipStream_t s);

// distributed plumbing (dist.cpp): no-ops when no communicator is set up
bool dist_active();
int dist_rank();
int dist_world();
enum { DIST_SUM = 0, DIST_MAX = 1, DIST_MIN = 2, DIST_BCAST = 3 /* a sum to which exactly one rank contributes */ };
int dist_allreduce_f64(double *buf_dev, int count, int op, hipStream_t s);                      // in place
int dist_allreduce_f64(const double *send_dev, double *recv_dev, int count, int op, hipStream_t s);
bool dist_has_comm();
int launch_loopback_reduce(const double *send, double *recv, int count, int world, int sum, hipStream_t s);

}  // namespace ofc

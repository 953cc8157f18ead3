// stream_api.cpp -- C ABI of libofc.so, part 4: streaming ingest with double-buffered pinned uploads
// (BASELINE.json configs[4] shape).  Two slots; while slot A's batch computes on the engine's stream, the host fills
// slot B's pinned buffer and its hipMemcpyAsync runs on the copy stream.  Consecutive batches overlap by one frame.
// With a model (ofc_stream_set_model) every batch's field is also labelled against it and counted per cell, behind the
// cell means on the compute stream, while the field is still where the flow left it.  With a histogram
// (ofc_stream_set_histogram) it is added to the stream's (u,v) table behind those, by uv_hist.hip's kernel.  With a camera
// (ofc_stream_set_camera) every pair's camera motion is fitted and subtracted in place between the flow and the cell means
// (motion_model.hip), so all of the above see the residual field.  With blobs (ofc_stream_set_blobs) every pair's moving
// regions are labelled and described behind all of those (blobs.hip), keyed by the model's label where there is a model.
// With blob links (ofc_stream_set_blob_links) the batch's moves are taken from the field before the camera is subtracted,
// and behind the blobs every transition between consecutive pairs is voted (blob_links.hip): those inside the batch, and
// the one from the previous batch's last pair, whose label map, moves and areas the stream carries over.
// With a photometric check (ofc_stream_set_photo) every pair's vectors are checked against the slot's own frames directly
// behind the flow, before the camera is subtracted (photo_check.hip); with blobs the key map is masked by the check's states.
// With a repair (ofc_stream_set_repair) the batch's field is repaired in place directly behind that check, whose state map it
// takes and updates (flow_repair.hip): before the moves are taken and the camera is fitted, so all of the above see it.
// With a forward-backward check (ofc_stream_set_consist) the batch's flow comes from the engine's bidirectional call, which
// also fills the stream's backward field; the check (fb_check.hip) runs where the photometric one would, and its state map
// plays the same role for the repair and the blobs.  A stream has one of the two checks, not both.
// With trajectories (ofc_stream_set_traj) the stream's points are advected through every batch's field directly behind the
// repair, before the moves and the camera (trajectories.hip): one launch per batch, the last row of the table is the carry.
#include "blob_links.h"
#include "color_common.h"
#include "fb_check.h"
#include "flow_repair.h"
#include "host_util.h"
#include "lloyd_common.h"
#include "motion_model.h"
#include "photo_check.h"
#include "trajectories.h"

#include <memory>

using namespace ofc;

// A table with one row per frame pair of the clip, on the device.  It starts at 256 pairs and doubles when a batch would
// not fit; the rows written so far move to the new buffer behind the compute stream.  Every table grows on its own, so a
// failed allocation leaves each of them either as it was or grown, never half of a group.
struct PairTable {
    DevBuf buf;
    size_t per = 0, cap = 0;           // bytes per pair; pairs there is room for
    explicit PairTable(size_t bytes_per_pair = 0) : per(bytes_per_pair) {}
    int ensure(int need_pairs, int have_pairs, hipStream_t compute)
    {
        if ((size_t)need_pairs <= cap) return OFC_OK;
        const size_t grown = std::max<size_t>(need_pairs, cap ? cap * 2 : 256);
        DevBuf nb;
        OFC_TRY(nb.alloc(grown * per));
        if (buf.p && have_pairs) {
            OFC_HIP(hipStreamSynchronize(compute));
            OFC_HIP(hipMemcpy(nb.p, buf.p, (size_t)have_pairs * per, hipMemcpyDeviceToDevice));
        }
        std::swap(buf.p, nb.p);
        std::swap(buf.bytes, nb.bytes);
        cap = grown;
        return OFC_OK;
    }
    // the table is empty and may change its layout: start over
    void reset()
    {
        buf.release();
        cap = 0;
    }
    void reset(size_t bytes_per_pair)
    {
        reset();
        per = bytes_per_pair;
    }
    template <class T> T *row(size_t pair) const { return reinterpret_cast<T *>(static_cast<char *>(buf.p) + pair * per); }
};

struct ofc_stream {
    int device = 0, W = 0, H = 0, batch = 0, rows = 0, cols = 0;
    ofc_flow_t *flow = nullptr;
    hipStream_t copy = nullptr, compute = nullptr;
    struct Slot {
        uint8_t *pinned = nullptr;     // (batch+1) frames, host
        DevBuf frames, flows;          // device
        hipEvent_t uploaded = nullptr, done = nullptr;
        int n_frames = 0;              // frames currently packed in `pinned`
        int inflight_pairs = 0;        // pairs of the batch in flight from this slot
        bool busy = false;             // a batch of this slot is in flight
    } slot[2];
    int cur = 0;
    PairTable cells;                   // [rows*cols][2] f32 per pair
    int pairs_submitted = 0;
    // the model, when there is one (k > 0): its LloydState on the device, and what it says about every pair so far
    int k = 0;
    bool with_sums = false;
    DevBuf model;                      // LloydState
    PairTable counts, sums;            // [rows*cols][k] int32 and, with_sums, [rows*cols][k][2] f64 per pair
    // the (u,v) histogram, when there is one (hist_bins > 0): every batch adds to it, a finish leaves it alone
    int hist_bins = 0;
    float hist_range = 0.f;
    DevBuf hist;                       // 3 * hist_bins^2 + 1 int64
    // the camera, when there is one (cam_kind > 0): every pair's fit, kept past the finish until the next clip's batches overwrite it
    int cam_kind = 0, cam_T = 0;
    double cam_thr[8] = {};
    PairTable cam_rec{sizeof(MotionRec)};
    DevBuf cam_partial;                // the moment kernel's partials of a batch
    int cam_pairs = 0;                 // pairs of the last finish: what ofc_stream_read_camera delivers
    // the blobs, when there are any (blob_conn > 0): every pair's table, kept past the finish like the camera's fits
    int blob_conn = 0, blob_min_area = 1, blob_max = 0;
    float blob_thr = 0.f;
    DevBuf blob_keys, blob_labels, blob_words, blob_err;   // one batch's key map, label map and area / slot words; the error word
    PairTable blob_table, blob_found{sizeof(int32_t)};     // [blob_max][12] int64 and one int32 per pair
    int blob_pairs = 0;                // pairs of the last finish: what ofc_stream_read_blobs delivers
    // the blob links, when there are any (link_max > 0; only with blobs): transition g leads from pair g to pair g + 1 of the clip
    int link_max = 0;
    DevBuf link_moves, link_areas;     // one batch's moves and areas at the roots, int32 [batch][H][W] each
    DevBuf link_carry;                 // the previous batch's last pair: label map, moves, areas, int32 [3][H][W]
    // [capacity] uint64, [capacity] int32 and one int32 per transition; sized by pairs (one transition fewer, never more)
    PairTable link_keys, link_votes, link_counters{sizeof(int32_t)};
    // the photometric check, when there is one (photo_on): every pair's stats, kept past the finish like the camera's fits
    bool photo_on = false;
    int photo_tau = 0, photo_kappa = 0, photo_keep = 0;
    DevBuf photo_state;                // one batch's state map, u8 [batch][H][W]
    PairTable photo_stats{sizeof(int64_t) * PHOTO_NSTAT};
    int photo_pairs = 0;               // pairs of the last finish: what ofc_stream_read_photo delivers
    // the forward-backward check, when there is one (consist_on; never together with the photometric check): every pair's counts
    bool consist_on = false;
    int64_t consist_alpha = 0, consist_beta = 0;
    int consist_keep = 0;
    DevBuf consist_state;              // one batch's state map, u8 [batch][H][W]
    DevBuf consist_bwd;                // one batch's backward field, f32 [batch][H][W][2]: one for the stream, the check reads it
                                       // behind the flow on the compute stream before the next batch's flow can write it
    PairTable consist_counts{sizeof(int64_t) * FB_NSTATE};
    int consist_pairs = 0;             // pairs of the last finish: what ofc_stream_read_consist delivers
    // the repair, when there is one (repair_on): every pair's counts, kept past the finish like the photometric stats
    bool repair_on = false;
    int repair_keep = 0, repair_radius = 0, repair_rounds = 0, repair_min_count = 0, repair_smooth = 0;
    DevBuf repair_a, repair_b, repair_filled;   // the snapshots and the filled map of a chunk of a batch (RepairScratch)
    PairTable repair_counts{sizeof(int64_t) * REPAIR_NCOUNT};
    int repair_pairs = 0;              // pairs of the last finish: what ofc_stream_read_repair delivers
    // the trajectories, when there are any (traj_P > 0): the positions after every pair, kept past the finish like the camera's fits
    int64_t traj_P = 0;
    bool traj_use_state = false;       // a point ends where the check's state map is not in the check's keep
    DevBuf traj_seeds, traj_len, traj_why;   // int32 [P][2], int32 [P], u8 [P]
    PairTable traj_pos;                // int32 [P][2] per pair: the positions after it; the last row written is the carry
    int traj_pairs = 0;                // pairs of the last finish: what ofc_stream_read_traj delivers
};

namespace {

// entry points that set a stage or read its results need a stream with nothing packed, in flight or undelivered
int require_idle(const ofc_stream *s, const char *what)
{
    OFC_REQUIRE(s->pairs_submitted == 0 && s->slot[0].n_frames == 0 && s->slot[1].n_frames == 0,
                "the stream holds frames or undelivered results: %s", what);
    return OFC_OK;
}

// the tail of a finish: the clip's pair count goes to every stage whose results outlive it, and the next clip starts at 0
void deliver(ofc_stream *s)
{
    s->cam_pairs = s->cam_kind ? s->pairs_submitted : 0;
    s->blob_pairs = s->blob_conn ? s->pairs_submitted : 0;
    s->photo_pairs = s->photo_on ? s->pairs_submitted : 0;
    s->consist_pairs = s->consist_on ? s->pairs_submitted : 0;
    s->repair_pairs = s->repair_on ? s->pairs_submitted : 0;
    s->traj_pairs = s->traj_P ? s->pairs_submitted : 0;
    s->pairs_submitted = 0;
}

// Behind a batch's label maps: its areas, then the votes of the transition from the carried pair (when the clip has one
// before this batch) and of the batch's inner transitions; then the batch's last pair becomes the carried one.
int submit_links(ofc_stream *s, const int32_t *labels, int npair)
{
    const size_t P = (size_t)s->W * s->H;
    const int base = s->pairs_submitted, first = base > 0 ? base - 1 : 0, ntrans = base + npair - 1 - first;
    const int32_t *moves = s->link_moves.as<int32_t>();
    int32_t *areas = s->link_areas.as<int32_t>(), *carry = s->link_carry.as<int32_t>();
    const PairTable &keys = s->link_keys, &votes = s->link_votes, &counters = s->link_counters;
    OFC_TRY(launch_blob_area(labels, s->W, s->H, npair, areas, s->compute));
    OFC_TRY(launch_blob_links_clear(s->link_max, ntrans, keys.row<uint64_t>(first), votes.row<int32_t>(first),
                                    counters.row<int32_t>(first), s->compute));
    if (base > 0)
        OFC_TRY(launch_blob_links(carry, carry + P, carry + 2 * P, labels, areas, s->W, s->H, 1, s->blob_min_area, s->link_max,
                                  keys.row<uint64_t>(first), votes.row<int32_t>(first), counters.row<int32_t>(first), s->compute));
    OFC_TRY(launch_blob_links(labels, moves, areas, labels + P, areas + P, s->W, s->H, npair - 1, s->blob_min_area, s->link_max,
                              keys.row<uint64_t>(base), votes.row<int32_t>(base), counters.row<int32_t>(base), s->compute));
    const size_t last = (size_t)(npair - 1) * P, bytes = sizeof(int32_t) * P;
    OFC_HIP(hipMemcpyAsync(carry, labels + last, bytes, hipMemcpyDeviceToDevice, s->compute));
    OFC_HIP(hipMemcpyAsync(carry + P, moves + last, bytes, hipMemcpyDeviceToDevice, s->compute));
    OFC_HIP(hipMemcpyAsync(carry + 2 * P, areas + last, bytes, hipMemcpyDeviceToDevice, s->compute));
    return OFC_OK;
}

// submit the frames packed in slot `i` (n >= 2): async upload, flow, with a camera its fit and subtraction, cell means,
// with a model the cluster counts, with a histogram the batch's share of the table, and with blobs the pairs' tables
int submit(ofc_stream *s, int i)
{
    ofc_stream::Slot &sl = s->slot[i];
    const int npair = sl.n_frames - 1;
    const size_t P = (size_t)s->W * s->H;
    const int base = s->pairs_submitted;
    // room for this batch's rows in the tables of the stages that are on; what the clip has so far is kept
    auto room = [&](PairTable &t) { return t.ensure(base + npair, base, s->compute); };
    OFC_TRY(room(s->cells));
    if (s->k) OFC_TRY(room(s->counts));
    if (s->with_sums) OFC_TRY(room(s->sums));
    if (s->cam_kind) OFC_TRY(room(s->cam_rec));
    if (s->blob_conn) { OFC_TRY(room(s->blob_table)); OFC_TRY(room(s->blob_found)); }
    if (s->link_max) { OFC_TRY(room(s->link_keys)); OFC_TRY(room(s->link_votes)); OFC_TRY(room(s->link_counters)); }
    if (s->photo_on) OFC_TRY(room(s->photo_stats));
    if (s->consist_on) OFC_TRY(room(s->consist_counts));
    if (s->repair_on) OFC_TRY(room(s->repair_counts));
    if (s->traj_P) OFC_TRY(room(s->traj_pos));
    OFC_HIP(hipMemcpyAsync(sl.frames.p, sl.pinned, P * sl.n_frames, hipMemcpyHostToDevice, s->copy));
    OFC_HIP(hipEventRecord(sl.uploaded, s->copy));
    OFC_HIP(hipStreamWaitEvent(s->compute, sl.uploaded, 0));
    // the state map of the stream's check, if it has one: the photometric or the forward-backward one
    uint8_t *const check_state = s->photo_on ? s->photo_state.as<uint8_t>() : s->consist_on ? s->consist_state.as<uint8_t>() : nullptr;
    const int check_keep = s->photo_on ? s->photo_keep : s->consist_keep;
    if (s->consist_on) {
        // both directions from one front end; the backward pair of a transition across two batches is in the later batch,
        // which carries the earlier frame.  The check compares the whole flows: before the moves and the camera
        OFC_TRY(ofc_flow_calc_frames_dev_bidir(s->flow, sl.frames.as<uint8_t>(), sl.n_frames, sl.flows.as<float>(),
                                               s->consist_bwd.as<float>()));
        OFC_TRY(launch_fb_check(sl.flows.as<float>(), s->consist_bwd.as<float>(), s->W, s->H, npair, false, s->consist_alpha,
                                s->consist_beta, check_state, s->consist_counts.row<int64_t>(base), nullptr, s->compute));
    } else {
        OFC_TRY(ofc_flow_calc_frames_dev(s->flow, sl.frames.as<uint8_t>(), sl.n_frames, sl.flows.as<float>()));
    }
    // the photometric check follows the whole flow into the slot's own next frame: before the camera is subtracted
    if (s->photo_on)
        OFC_TRY(launch_photo_check(sl.frames.as<uint8_t>(), sl.flows.as<float>(), s->W, s->H, npair, s->photo_tau, s->photo_kappa,
                                   s->photo_state.as<uint8_t>(), s->photo_stats.row<int64_t>(base), nullptr, s->compute));
    // the repair takes the check's state map (without a check only invalid vectors are targets) and works in place on both:
    // everything from here on, the moves and the camera included, sees the repaired field and the updated states
    if (s->repair_on) {
        RepairScratch rs;
        rs.a = s->repair_a.as<float>(), rs.b = s->repair_b.as<float>(), rs.filled = s->repair_filled.as<uint8_t>();
        rs.chunk = repair_chunk_pairs(s->W, s->H, s->batch);
        uint8_t *st = check_state;
        OFC_TRY(launch_repair(sl.flows.as<float>(), st, s->W, s->H, npair, s->repair_keep, s->repair_radius, s->repair_rounds,
                              s->repair_min_count, s->repair_smooth != 0, sl.flows.as<float>(), nullptr, st,
                              s->repair_counts.row<int64_t>(base), rs, s->compute));
    }
    // the points land by the whole, repaired flow (the rule of the moves): placed at the clip's first pair, carried by the
    // table's last row afterwards
    if (s->traj_P) {
        OFC_REQUIRE(!s->traj_use_state || check_state, "the trajectories use the state map of a check the stream no longer has");
        int32_t *len = s->traj_len.as<int32_t>();
        uint8_t *why = s->traj_why.as<uint8_t>();
        const int32_t *from = base > 0 ? s->traj_pos.row<int32_t>(base - 1) : s->traj_seeds.as<int32_t>();
        if (base == 0) OFC_TRY(launch_traj_begin(from, s->traj_P, const_cast<int32_t *>(from), len, why, s->compute));
        OFC_TRY(launch_traj_steps(sl.flows.as<float>(), s->traj_use_state ? check_state : nullptr, s->W, s->H, base, npair, s->traj_P,
                                  check_keep, from, s->traj_pos.row<int32_t>(base), len, why, s->compute));
    }
    // where the pixels go is what the whole flow says: the moves are taken before the camera is subtracted
    if (s->link_max) OFC_TRY(launch_blob_moves(sl.flows.as<float>(), s->W, s->H, npair, s->link_moves.as<int32_t>(), s->compute));
    if (s->cam_kind) {
        MotionRec *rec = s->cam_rec.row<MotionRec>(base);
        OFC_TRY(motion_fit_async(sl.flows.as<float>(), s->W, s->H, npair, s->cam_kind, s->cam_thr, s->cam_T, rec,
                                 s->cam_partial.as<int64_t>(), nullptr, nullptr, s->compute));
        OFC_TRY(launch_motion_subtract(sl.flows.as<float>(), sl.flows.as<float>(), s->W, s->H, npair, rec, s->compute));
    }
    OFC_TRY(launch_grid_cell_mean_flow(sl.flows.as<float>(), s->W, s->H, npair, s->rows, s->cols, s->cells.row<float>(base),
                                       s->compute));
    if (s->k)
        OFC_TRY(launch_grid_assign_counts(sl.flows.as<float>(), s->model.as<LloydState>(), s->W, s->H, npair, s->rows, s->cols,
                                          s->k, s->counts.row<int32_t>(base),
                                          s->with_sums ? s->sums.row<double>(base) : nullptr, s->compute));
    if (s->hist_bins)
        OFC_TRY(launch_uv_hist(sl.flows.as<float>(), (int64_t)P * npair, s->hist_bins, s->hist_range, s->hist.as<int64_t>(),
                               s->compute));
    if (s->blob_conn) {
        // moving pixels, keyed by the model's label where there is one: key map, label map, table, all of this batch
        uint8_t *keys = s->blob_keys.as<uint8_t>();
        int32_t *labels = s->blob_labels.as<int32_t>();
        int *err = s->blob_err.as<int>();
        OFC_TRY(launch_blob_keys(sl.flows.as<float>(), s->W, s->H, npair, true, s->blob_thr, s->k ? s->model.as<LloydState>() : nullptr,
                                 s->k, (1u << s->k) - 1u, false, keys, s->compute));
        // a pixel whose vector failed the stream's check belongs to no blob
        if (check_state)
            OFC_TRY(launch_consist_mask(check_state, (int64_t)P * npair, check_keep, keys, nullptr, s->compute));
        OFC_TRY(launch_blob_local(keys, s->W, s->H, npair, s->blob_conn, labels, err, s->compute));
        OFC_TRY(launch_blob_seam(keys, s->W, s->H, npair, s->blob_conn, labels, err, s->compute));
        OFC_TRY(launch_blob_flatten(s->W, s->H, npair, labels, err, s->compute));
        OFC_TRY(launch_blob_table(keys, labels, sl.flows.as<float>(), s->W, s->H, npair, s->blob_min_area, s->blob_max,
                                  s->blob_words.as<int32_t>(), s->blob_table.row<int64_t>(base), s->blob_found.row<int32_t>(base),
                                  s->compute));
        if (s->link_max) OFC_TRY(submit_links(s, labels, npair));
    }
    OFC_HIP(hipEventRecord(sl.done, s->compute));
    sl.busy = true;
    sl.inflight_pairs = npair;
    s->pairs_submitted += npair;
    return OFC_OK;
}

}  // namespace

extern "C" {

hipStream_t ofc_flow_stream_internal(ofc_flow_t *f);   // flow_engine.cpp

int ofc_stream_create(int device, int W, int H, const ofc_fb_params *p, int batch_pairs, int rows, int cols,
                      ofc_stream_t **out)
{
    OFC_REQUIRE(out, "null out pointer");
    *out = nullptr;
    OFC_REQUIRE(batch_pairs >= 1 && rows >= 1 && cols >= 1 && W >= cols && H >= rows, "bad arguments");
    OFC_TRY(ensure_device(device));
    std::unique_ptr<ofc_stream> s(new ofc_stream);
    s->device = device; s->W = W; s->H = H; s->batch = batch_pairs; s->rows = rows; s->cols = cols;
    OFC_TRY(ofc_flow_create(device, W, H, p, batch_pairs, &s->flow));
    s->cells.per = sizeof(float) * 2 * rows * cols;
    s->compute = ofc_flow_stream_internal(s->flow);
    OFC_HIP(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
    const size_t P = (size_t)W * H;
    for (auto &sl : s->slot) {
        OFC_HIP(hipHostMalloc((void **)&sl.pinned, P * (batch_pairs + 1), hipHostMallocDefault));
        OFC_TRY(sl.frames.alloc(P * (batch_pairs + 1)));
        OFC_TRY(sl.flows.alloc(sizeof(float) * 2 * P * batch_pairs));
        OFC_HIP(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
        OFC_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    *out = s.release();
    return OFC_OK;
}

int ofc_stream_push_gray(ofc_stream_t *s, const uint8_t *gray, int *pairs_done)
{
    OFC_REQUIRE(s && gray, "null pointer");
    OFC_TRY(ensure_device(s->device));
    const size_t P = (size_t)s->W * s->H;
    ofc_stream::Slot *sl = &s->slot[s->cur];
    if (sl->busy && sl->n_frames == 0) {            // about to refill a slot whose batch may still be running
        OFC_HIP(hipEventSynchronize(sl->done));
        sl->busy = false;
    }
    memcpy(sl->pinned + P * sl->n_frames, gray, P);
    sl->n_frames++;
    if (sl->n_frames == s->batch + 1) {
        OFC_TRY(submit(s, s->cur));
        // next slot starts with this batch's last frame (one-frame overlap)
        ofc_stream::Slot *nx = &s->slot[s->cur ^ 1];
        if (nx->busy) {
            OFC_HIP(hipEventSynchronize(nx->done));
            nx->busy = false;
        }
        memcpy(nx->pinned, sl->pinned + P * s->batch, P);
        nx->n_frames = 1;
        sl->n_frames = 0;
        s->cur ^= 1;
    }
    if (pairs_done) {
        int done = s->pairs_submitted;
        for (auto &q : s->slot)
            if (q.busy && hipEventQuery(q.done) != hipSuccess) done -= q.inflight_pairs;
        *pairs_done = done;
    }
    return OFC_OK;
}

// flush the partial batch and wait for everything submitted
static int flush(ofc_stream *s)
{
    ofc_stream::Slot &sl = s->slot[s->cur];
    if (sl.n_frames >= 2) {
        if (sl.busy) { OFC_HIP(hipEventSynchronize(sl.done)); sl.busy = false; }
        OFC_TRY(submit(s, s->cur));
    }
    sl.n_frames = 0;
    OFC_HIP(hipStreamSynchronize(s->copy));
    OFC_HIP(hipStreamSynchronize(s->compute));
    for (auto &q : s->slot) q.busy = false;
    return OFC_OK;
}

int ofc_stream_finish(ofc_stream_t *s, float *cell_uv, int max_pairs, int *n_pairs)
{
    OFC_REQUIRE(s && n_pairs, "null pointer");
    OFC_TRY(ensure_device(s->device));
    OFC_TRY(flush(s));
    *n_pairs = s->pairs_submitted;
    if (cell_uv) {
        OFC_REQUIRE(max_pairs >= s->pairs_submitted, "cell_uv holds %d pairs, %d produced", max_pairs, s->pairs_submitted);
        OFC_HIP(hipMemcpy(cell_uv, s->cells.buf.p, s->cells.per * (size_t)s->pairs_submitted, hipMemcpyDeviceToHost));
    }
    deliver(s);
    return OFC_OK;
}

int ofc_stream_set_model(ofc_stream_t *s, int k, const double *mean, const double *centers_c, int with_sums)
{
    OFC_REQUIRE(s, "null pointer");
    if (k != 0) OFC_TRY(check_uv_model(k, mean, centers_c));
    OFC_TRY(require_idle(s, "set the model on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    if (k != 0) {
        LloydState st;
        memset(&st, 0, sizeof(st));
        if (mean) memcpy(st.mean, mean, sizeof(double) * 2);
        memcpy(st.centers, centers_c, sizeof(double) * 2 * k);
        if (!s->model.p) OFC_TRY(s->model.alloc(sizeof(LloydState)));
        // nothing of this stream is in flight (checked above): the state is free to be rewritten
        OFC_HIP(hipMemcpyAsync(s->model.p, &st, sizeof(st), hipMemcpyHostToDevice, s->compute));
        OFC_TRY(launch_lloyd_set_centers(s->model.as<LloydState>(), k, 2, s->compute));
        OFC_HIP(hipStreamSynchronize(s->compute));
    }
    if (k != s->k || (with_sums != 0) != s->with_sums) {       // the buffers' layout changes: they are empty, start over
        const size_t per = sizeof(int32_t) * s->rows * s->cols * k;
        s->counts.reset(per);
        s->sums.reset(per * 4);                                 // two f64 per count
    }
    s->k = k;
    s->with_sums = k != 0 && with_sums != 0;
    return OFC_OK;
}

int ofc_stream_finish_clusters(ofc_stream_t *s, float *cell_uv, int32_t *counts, double *sums, int max_pairs, int *n_pairs)
{
    OFC_REQUIRE(s && n_pairs, "null pointer");
    OFC_REQUIRE(s->k > 0, "the stream has no model (ofc_stream_set_model)");
    OFC_REQUIRE(!sums || s->with_sums, "the model was set without sums");
    OFC_TRY(ensure_device(s->device));
    OFC_TRY(flush(s));
    const size_t n = (size_t)s->pairs_submitted;
    *n_pairs = s->pairs_submitted;
    if (cell_uv || counts || sums)
        OFC_REQUIRE(max_pairs >= s->pairs_submitted, "the outputs hold %d pairs, %d produced", max_pairs, s->pairs_submitted);
    if (n) {
        if (cell_uv) OFC_HIP(hipMemcpy(cell_uv, s->cells.buf.p, s->cells.per * n, hipMemcpyDeviceToHost));
        if (counts) OFC_HIP(hipMemcpy(counts, s->counts.buf.p, s->counts.per * n, hipMemcpyDeviceToHost));
        if (sums) OFC_HIP(hipMemcpy(sums, s->sums.buf.p, s->sums.per * n, hipMemcpyDeviceToHost));
    }
    deliver(s);
    return OFC_OK;
}

int ofc_stream_set_histogram(ofc_stream_t *s, int bins, float range)
{
    OFC_REQUIRE(s, "null pointer");
    if (bins != 0) OFC_TRY(uv_hist_check(bins, range));
    OFC_TRY(require_idle(s, "set the histogram on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    if (bins == 0) {
        s->hist.release();
        s->hist_bins = 0;
        s->hist_range = 0.f;
        return OFC_OK;
    }
    if (bins == s->hist_bins && range == s->hist_range) return OFC_OK;      // the table stays, with what is in it
    DevBuf nb;
    OFC_TRY(nb.alloc(sizeof(int64_t) * (3 * (size_t)bins * bins + 1)));
    OFC_HIP(hipMemsetAsync(nb.p, 0, nb.bytes, s->compute));
    OFC_HIP(hipStreamSynchronize(s->compute));
    std::swap(s->hist.p, nb.p);
    std::swap(s->hist.bytes, nb.bytes);
    s->hist_bins = bins;
    s->hist_range = range;
    return OFC_OK;
}

int ofc_stream_read_histogram(ofc_stream_t *s, int64_t *table_host, int reset)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->hist_bins > 0, "the stream has no histogram (ofc_stream_set_histogram)");
    OFC_TRY(require_idle(s, "read the histogram straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    if (table_host) OFC_HIP(hipMemcpy(table_host, s->hist.p, s->hist.bytes, hipMemcpyDeviceToHost));
    if (reset) {
        OFC_HIP(hipMemsetAsync(s->hist.p, 0, s->hist.bytes, s->compute));
        OFC_HIP(hipStreamSynchronize(s->compute));
    }
    return OFC_OK;
}

int ofc_stream_set_camera(ofc_stream_t *s, int kind, const double *thresholds, int T)
{
    OFC_REQUIRE(s, "null pointer");
    if (kind != 0) OFC_TRY(motion_fit_check(s->W, s->H, kind, thresholds, T));
    OFC_TRY(require_idle(s, "set the camera on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    s->cam_pairs = 0;
    if (kind == 0) {
        s->cam_rec.reset();
        s->cam_partial.release();
        s->cam_kind = 0;
        s->cam_T = 0;
        return OFC_OK;
    }
    // the partials of the largest batch at the most work-groups per pair any batch size gets
    size_t most = 0;
    for (int n = 1; n <= s->batch; n++) most = std::max(most, (size_t)motion_groups(s->W, s->H, n) * n);
    OFC_TRY(s->cam_partial.alloc(sizeof(int64_t) * MOTION_NMOM * most));
    s->cam_kind = kind;
    s->cam_T = T;
    for (int t = 0; t < T; t++) s->cam_thr[t] = thresholds[t];
    return OFC_OK;
}

int ofc_stream_read_camera(ofc_stream_t *s, double *models, int *status, int max_pairs)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->cam_kind > 0, "the stream has no camera (ofc_stream_set_camera)");
    OFC_TRY(require_idle(s, "read the camera straight after a finish"));
    OFC_REQUIRE(max_pairs >= s->cam_pairs, "the outputs hold %d pairs, the last finish delivered %d", max_pairs, s->cam_pairs);
    OFC_TRY(ensure_device(s->device));
    if (!s->cam_pairs || (!models && !status)) return OFC_OK;
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    std::vector<MotionRec> rec(s->cam_pairs);
    OFC_HIP(hipMemcpy(rec.data(), s->cam_rec.buf.p, sizeof(MotionRec) * rec.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < s->cam_pairs; i++) {
        if (models) memcpy(models + 6 * (size_t)i, rec[i].p, sizeof(double) * 6);
        if (status) status[i] = rec[i].status;
    }
    return OFC_OK;
}

// slots: the capacity of a transition's table under the links to come, 0 with none
static void release_links(ofc_stream *s, size_t slots)
{
    for (DevBuf *b : {&s->link_moves, &s->link_areas, &s->link_carry}) b->release();
    s->link_keys.reset(slots * sizeof(uint64_t));
    s->link_votes.reset(slots * sizeof(int32_t));
    s->link_counters.reset();
    s->link_max = 0;
}

int ofc_stream_set_blobs(ofc_stream_t *s, int connectivity, float thr, int min_area, int max_blobs)
{
    OFC_REQUIRE(s, "null pointer");
    if (connectivity != 0) {
        OFC_TRY(blob_check(s->W, s->H, s->batch, connectivity, min_area, max_blobs));
        OFC_REQUIRE(std::isfinite(thr) && thr >= 0, "thr must be finite and >= 0");
    }
    OFC_TRY(require_idle(s, "set the blobs on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    s->blob_pairs = 0;
    // the tables' layout may change: they are empty, start over
    s->blob_table.reset(connectivity ? sizeof(int64_t) * BLOB_NF * max_blobs : 0);
    s->blob_found.reset();
    if (connectivity == 0) {
        s->blob_keys.release();
        s->blob_labels.release();
        s->blob_words.release();
        s->blob_err.release();
        s->blob_conn = 0;
        release_links(s, 0);
        return OFC_OK;
    }
    const size_t n = (size_t)s->W * s->H * s->batch;
    OFC_TRY(reserve(s->blob_keys, n));
    OFC_TRY(reserve(s->blob_labels, n * sizeof(int32_t)));
    OFC_TRY(reserve(s->blob_words, n * sizeof(int32_t)));
    OFC_TRY(reserve(s->blob_err, sizeof(int)));
    OFC_HIP(hipMemsetAsync(s->blob_err.p, 0, sizeof(int), s->compute));
    OFC_HIP(hipStreamSynchronize(s->compute));
    s->blob_conn = connectivity;
    s->blob_thr = thr;
    s->blob_min_area = min_area;
    s->blob_max = max_blobs;
    return OFC_OK;
}

int ofc_stream_read_blobs(ofc_stream_t *s, int64_t *table_host, int32_t *n_host, int32_t *found_host, int max_pairs)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->blob_conn > 0, "the stream has no blobs (ofc_stream_set_blobs)");
    OFC_TRY(require_idle(s, "read the blobs straight after a finish"));
    OFC_REQUIRE(max_pairs >= s->blob_pairs, "the outputs hold %d pairs, the last finish delivered %d", max_pairs, s->blob_pairs);
    OFC_TRY(ensure_device(s->device));
    if (!s->blob_pairs) return OFC_OK;
    OFC_REQUIRE(table_host && n_host && found_host, "null pointer");
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    int e = 0;
    OFC_HIP(hipMemcpy(&e, s->blob_err.p, sizeof(int), hipMemcpyDeviceToHost));
    if (e != 0) {
        set_error("connected components: a capped loop ran out (stages %d); the tables are not valid", e);
        return OFC_EHIP;
    }
    return blob_table_read(s->blob_table.row<int64_t>(0), s->blob_found.row<int32_t>(0), s->blob_pairs, s->blob_max, table_host, n_host,
                           found_host);
}

int ofc_stream_set_blob_links(ofc_stream_t *s, int max_links)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->blob_conn > 0, "the stream has no blobs (ofc_stream_set_blobs): there is nothing to link");
    if (max_links != 0) OFC_TRY(blob_link_check(s->W, s->H, s->batch, s->blob_min_area, max_links));
    OFC_TRY(require_idle(s, "set the links on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    release_links(s, max_links ? blob_link_capacity(max_links) : 0);   // the tables' layout may change: they are empty, start over
    s->blob_pairs = 0;                     // ... and so are the blob tables, as after ofc_stream_set_blobs
    if (max_links == 0) return OFC_OK;
    const size_t P = (size_t)s->W * s->H;
    OFC_TRY(s->link_moves.alloc(sizeof(int32_t) * P * s->batch));
    OFC_TRY(s->link_areas.alloc(sizeof(int32_t) * P * s->batch));
    OFC_TRY(s->link_carry.alloc(sizeof(int32_t) * P * 3));
    s->link_max = max_links;
    return OFC_OK;
}

int ofc_stream_read_blob_links(ofc_stream_t *s, int64_t *links_host, int32_t *nlinks_host, int max_trans)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->link_max > 0, "the stream has no blob links (ofc_stream_set_blob_links)");
    OFC_TRY(require_idle(s, "read the links straight after a finish"));
    const int ntrans = s->blob_pairs > 0 ? s->blob_pairs - 1 : 0;
    OFC_REQUIRE(max_trans >= ntrans, "the outputs hold %d transitions, the last finish delivered %d", max_trans, ntrans);
    OFC_TRY(ensure_device(s->device));
    if (!ntrans) return OFC_OK;
    OFC_REQUIRE(links_host && nlinks_host, "null pointer");
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    return blob_links_read(s->link_keys.row<uint64_t>(0), s->link_votes.row<int32_t>(0), s->link_counters.row<int32_t>(0), ntrans,
                           s->link_max, links_host, nlinks_host);
}

int ofc_stream_set_photo(ofc_stream_t *s, int on, int tau_q, int kappa_q, int keep)
{
    OFC_REQUIRE(s, "null pointer");
    if (on != 0) {
        OFC_TRY(photo_check(s->W, s->H, s->batch, tau_q, kappa_q));
        OFC_REQUIRE(keep >= 1 && keep < (1 << FB_NSTATE), "keep = %d: a set of the four states, 1 .. 15", keep);
        OFC_REQUIRE(!s->consist_on, "the stream has a forward-backward check: one state map per stream, turn that off first");
    }
    OFC_TRY(require_idle(s, "set the photometric check on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    s->photo_pairs = 0;
    if (on == 0) {
        s->photo_state.release();
        s->photo_stats.reset();
        s->photo_on = false;
        return OFC_OK;
    }
    const size_t n = (size_t)s->W * s->H * s->batch;
    OFC_TRY(reserve(s->photo_state, n));
    s->photo_on = true;
    s->photo_tau = tau_q;
    s->photo_kappa = kappa_q;
    s->photo_keep = keep;
    return OFC_OK;
}

int ofc_stream_read_photo(ofc_stream_t *s, int64_t *stats_host, int max_pairs)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->photo_on, "the stream has no photometric check (ofc_stream_set_photo)");
    OFC_TRY(require_idle(s, "read the photometric stats straight after a finish"));
    OFC_REQUIRE(max_pairs >= s->photo_pairs, "the outputs hold %d pairs, the last finish delivered %d", max_pairs, s->photo_pairs);
    OFC_TRY(ensure_device(s->device));
    if (!s->photo_pairs) return OFC_OK;
    OFC_REQUIRE(stats_host, "null pointer");
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    OFC_HIP(hipMemcpy(stats_host, s->photo_stats.buf.p, s->photo_stats.per * (size_t)s->photo_pairs, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_stream_set_consist(ofc_stream_t *s, int on, int64_t alpha_q, int64_t beta_q, int keep)
{
    OFC_REQUIRE(s, "null pointer");
    if (on != 0) {
        OFC_TRY(fb_check(s->W, s->H, s->batch, alpha_q, beta_q));
        OFC_REQUIRE(keep >= 1 && keep < (1 << FB_NSTATE), "keep = %d: a set of the four states, 1 .. 15", keep);
        OFC_REQUIRE(!s->photo_on, "the stream has a photometric check: one state map per stream, turn that off first");
    }
    OFC_TRY(require_idle(s, "set the forward-backward check on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    s->consist_pairs = 0;
    if (on == 0) {
        s->consist_state.release();
        s->consist_bwd.release();
        s->consist_counts.reset();
        s->consist_on = false;
        return OFC_OK;
    }
    const size_t n = (size_t)s->W * s->H * s->batch;
    OFC_TRY(reserve(s->consist_state, n));
    OFC_TRY(reserve(s->consist_bwd, sizeof(float) * 2 * n));
    s->consist_on = true;
    s->consist_alpha = alpha_q;
    s->consist_beta = beta_q;
    s->consist_keep = keep;
    return OFC_OK;
}

int ofc_stream_read_consist(ofc_stream_t *s, int64_t *counts_host, int max_pairs)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->consist_on, "the stream has no forward-backward check (ofc_stream_set_consist)");
    OFC_TRY(require_idle(s, "read the forward-backward counts straight after a finish"));
    OFC_REQUIRE(max_pairs >= s->consist_pairs, "the outputs hold %d pairs, the last finish delivered %d", max_pairs, s->consist_pairs);
    OFC_TRY(ensure_device(s->device));
    if (!s->consist_pairs) return OFC_OK;
    OFC_REQUIRE(counts_host, "null pointer");
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    OFC_HIP(hipMemcpy(counts_host, s->consist_counts.buf.p, s->consist_counts.per * (size_t)s->consist_pairs, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_stream_set_repair(ofc_stream_t *s, int on, int keep, int radius, int rounds, int min_count, int smooth)
{
    OFC_REQUIRE(s, "null pointer");
    if (on != 0) OFC_TRY(repair_check(s->W, s->H, s->batch, keep, radius, rounds, min_count, smooth));
    OFC_TRY(require_idle(s, "set the repair on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    s->repair_pairs = 0;
    if (on == 0) {
        s->repair_a.release();
        s->repair_b.release();
        s->repair_filled.release();
        s->repair_counts.reset();
        s->repair_on = false;
        return OFC_OK;
    }
    // a batch's chunk: one snapshot, a second with more than two sweeps, and the filled map the state kernel reads
    const int chunk = repair_chunk_pairs(s->W, s->H, s->batch);
    const size_t field = repair_field_bytes(s->W, s->H, chunk), map = repair_filled_bytes(s->W, s->H, chunk);
    OFC_TRY(reserve(s->repair_a, field));
    if (rounds + smooth > 2) OFC_TRY(reserve(s->repair_b, field));
    OFC_TRY(reserve(s->repair_filled, map));
    s->repair_on = true;
    s->repair_keep = keep;
    s->repair_radius = radius;
    s->repair_rounds = rounds;
    s->repair_min_count = min_count;
    s->repair_smooth = smooth;
    return OFC_OK;
}

int ofc_stream_read_repair(ofc_stream_t *s, int64_t *counts_host, int max_pairs)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->repair_on, "the stream has no repair (ofc_stream_set_repair)");
    OFC_TRY(require_idle(s, "read the repair counts straight after a finish"));
    OFC_REQUIRE(max_pairs >= s->repair_pairs, "the outputs hold %d pairs, the last finish delivered %d", max_pairs, s->repair_pairs);
    OFC_TRY(ensure_device(s->device));
    if (!s->repair_pairs) return OFC_OK;
    OFC_REQUIRE(counts_host, "null pointer");
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    OFC_HIP(hipMemcpy(counts_host, s->repair_counts.buf.p, s->repair_counts.per * (size_t)s->repair_pairs, hipMemcpyDeviceToHost));
    return OFC_OK;
}

int ofc_stream_set_traj(ofc_stream_t *s, int64_t P, const int32_t *seeds_host, int use_state)
{
    OFC_REQUIRE(s, "null pointer");
    if (P != 0) {
        OFC_TRY(traj_check(s->W, s->H, s->batch, P, 0, 0));
        OFC_REQUIRE(seeds_host, "null pointer");
        OFC_REQUIRE(!use_state || s->photo_on || s->consist_on,
                    "use_state needs the state map of a check (ofc_stream_set_photo or ofc_stream_set_consist)");
    }
    OFC_TRY(require_idle(s, "set the trajectories on a fresh stream or straight after a finish"));
    OFC_TRY(ensure_device(s->device));
    s->traj_pairs = 0;
    s->traj_pos.reset(sizeof(int32_t) * 2 * (size_t)P);      // the table's layout may change: it is empty, start over
    if (P == 0) {
        s->traj_seeds.release();
        s->traj_len.release();
        s->traj_why.release();
        s->traj_P = 0;
        s->traj_use_state = false;
        return OFC_OK;
    }
    s->traj_P = 0;                                           // a failed allocation leaves the stage off
    OFC_TRY(s->traj_seeds.alloc(sizeof(int32_t) * 2 * (size_t)P));
    OFC_TRY(s->traj_len.alloc(sizeof(int32_t) * (size_t)P));
    OFC_TRY(s->traj_why.alloc((size_t)P));
    OFC_HIP(hipMemcpy(s->traj_seeds.p, seeds_host, sizeof(int32_t) * 2 * (size_t)P, hipMemcpyHostToDevice));
    s->traj_P = P;
    s->traj_use_state = use_state != 0;
    return OFC_OK;
}

int ofc_stream_read_traj(ofc_stream_t *s, int32_t *pos_host, int32_t *len_host, uint8_t *why_host, int max_pairs)
{
    OFC_REQUIRE(s, "null pointer");
    OFC_REQUIRE(s->traj_P > 0, "the stream has no trajectories (ofc_stream_set_traj)");
    OFC_TRY(require_idle(s, "read the trajectories straight after a finish"));
    OFC_REQUIRE(max_pairs >= s->traj_pairs, "the outputs hold %d pairs, the last finish delivered %d", max_pairs, s->traj_pairs);
    OFC_TRY(ensure_device(s->device));
    if (!s->traj_pairs) return OFC_OK;
    OFC_REQUIRE(pos_host && len_host && why_host, "null pointer");
    // nothing of this stream is in flight (checked above; a finish has waited for the compute stream)
    const size_t P = (size_t)s->traj_P, row = sizeof(int32_t) * 2 * P;
    OFC_HIP(hipMemcpy(pos_host, s->traj_seeds.p, row, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(pos_host + 2 * P, s->traj_pos.buf.p, row * (size_t)s->traj_pairs, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(len_host, s->traj_len.p, sizeof(int32_t) * P, hipMemcpyDeviceToHost));
    OFC_HIP(hipMemcpy(why_host, s->traj_why.p, P, hipMemcpyDeviceToHost));
    return OFC_OK;
}

void ofc_stream_destroy(ofc_stream_t *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->compute) (void)hipStreamSynchronize(s->compute);
    if (s->copy) { (void)hipStreamSynchronize(s->copy); (void)hipStreamDestroy(s->copy); }
    for (auto &sl : s->slot) {
        if (sl.pinned) (void)hipHostFree(sl.pinned);
        if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    ofc_flow_destroy(s->flow);
    delete s;
}

int ofc_grid_cell_mean_flow(int device, const float *flow, int W, int H, int rows, int cols, float *cell_uv)
{
    OFC_REQUIRE(flow && cell_uv && rows >= 1 && cols >= 1 && W >= cols && H >= rows, "bad arguments");
    OFC_TRY(ensure_device(device));
    DevBuf f, o;
    OFC_TRY(f.alloc(sizeof(float) * 2 * W * H));
    OFC_TRY(o.alloc(sizeof(float) * 2 * rows * cols));
    OFC_HIP(hipMemcpy(f.p, flow, sizeof(float) * 2 * W * H, hipMemcpyHostToDevice));
    OFC_TRY(launch_grid_cell_mean_flow(f.as<float>(), W, H, 1, rows, cols, o.as<float>(), nullptr));
    OFC_HIP(hipMemcpy(cell_uv, o.p, sizeof(float) * 2 * rows * cols, hipMemcpyDeviceToHost));
    return OFC_OK;
}

}  // extern "C"

// blob_links_api.cpp -- C ABI of libofc.so, part 8: the links between the blobs of consecutive pairs (blob_links.hip) on
// device and host buffers, the host forms of its check and of its table's size, and its measurement hook.
#include "blob_links.h"
#include "host_util.h"

#include <mutex>

using namespace ofc;

namespace {

// The library's scratch, one per device: the areas at the roots, and the buffers the host-buffer call and the hook work in.
struct LinkScratch {
    DevBuf areas, labels, flow, moves, links, counters;
    std::mutex mu;
};

LinkScratch &scratch_for(int device) { return device_scratch<LinkScratch>(device); }

// where the votes begin in a links_dev of ntrans transitions (blob_links_bytes' layout)
int32_t *votes_of(const void *links, int max_links, int ntrans)
{
    return reinterpret_cast<int32_t *>(static_cast<uint64_t *>(const_cast<void *>(links)) + blob_link_capacity(max_links) * (size_t)ntrans);
}

// areas of all pairs (the area sweep is run again: nothing of the table stage's words is kept), clears, votes
int links_dev(LinkScratch &sc, const int32_t *labels, const int32_t *moves, int W, int H, int npair, int min_area, int max_links,
              void *links, int32_t *counters, hipStream_t s)
{
    if (npair < 2) return OFC_OK;
    const size_t P = (size_t)W * H;
    uint64_t *keys = static_cast<uint64_t *>(links);
    int32_t *votes = votes_of(links, max_links, npair - 1);
    OFC_TRY(reserve(sc.areas, sizeof(int32_t) * P * npair));
    int32_t *areas = sc.areas.as<int32_t>();
    OFC_TRY(launch_blob_area(labels, W, H, npair, areas, s));
    OFC_TRY(launch_blob_links_clear(max_links, npair - 1, keys, votes, counters, s));
    return launch_blob_links(labels, moves, areas, labels + P, areas + P, W, H, npair - 1, min_area, max_links, keys, votes,
                             counters, s);
}

}  // namespace

namespace ofc {

int blob_links_read(const uint64_t *kd, const int32_t *vd, const int32_t *counters_dev, int ntrans, int max_links,
                    int64_t *links_host, int32_t *nlinks_host)
{
    if (ntrans == 0) return OFC_OK;
    const size_t cap = blob_link_capacity(max_links);
    std::vector<int32_t> counters(ntrans), votes(cap);
    std::vector<uint64_t> keys(cap);
    OFC_HIP(hipMemcpy(counters.data(), counters_dev, sizeof(int32_t) * ntrans, hipMemcpyDeviceToHost));
    bool sound = true;
    for (int t = 0; t < ntrans; t++) {
        const bool over = (counters[t] & BLOB_LINK_COUNT) > max_links;
        if (!over) {
            OFC_HIP(hipMemcpy(keys.data(), kd + cap * (size_t)t, sizeof(uint64_t) * cap, hipMemcpyDeviceToHost));
            OFC_HIP(hipMemcpy(votes.data(), vd + cap * (size_t)t, sizeof(int32_t) * cap, hipMemcpyDeviceToHost));
        }
        sound &= blob_order_links(keys.data(), votes.data(), cap, counters[t], max_links,
                                  links_host + (size_t)t * max_links * BLOB_LINK_NF, nlinks_host + t);
    }
    if (!sound) {
        set_error("blob links: a transition's table does not match its counter (a capped probe loop ran out with room left)");
        return OFC_EHIP;
    }
    return OFC_OK;
}

}  // namespace ofc

extern "C" {

int ofc_blob_link_check(int W, int H, int npair, int min_area, int max_links)
{
    return blob_link_check(W, H, npair, min_area, max_links);
}

size_t ofc_blob_links_bytes(int max_links, int ntrans)
{
    if (max_links < 1 || max_links > BLOB_MAX_LINKS || ntrans < 0) return 0;
    return blob_links_bytes(max_links, ntrans);
}

int ofc_blob_moves_dev(int device, const float *flow_dev, int W, int H, int npair, int32_t *moves_dev)
{
    OFC_REQUIRE(flow_dev && moves_dev, "null pointer");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0 && ((uintptr_t)moves_dev & 3) == 0,
                "flow_dev must be 8-byte and moves_dev 4-byte aligned");
    OFC_TRY(blob_link_check(W, H, npair, 1, 1));
    OFC_TRY(ensure_device(device));
    OFC_TRY(launch_blob_moves(flow_dev, W, H, npair, moves_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_blob_links_dev(int device, const int32_t *labels_dev, const int32_t *moves_dev, int W, int H, int npair, int min_area,
                       int max_links, void *links_dev_, int32_t *nlinks_dev)
{
    OFC_REQUIRE(labels_dev && moves_dev, "null pointer");
    OFC_REQUIRE(npair < 2 || (links_dev_ && nlinks_dev), "null pointer");
    OFC_REQUIRE(((uintptr_t)labels_dev & 3) == 0 && ((uintptr_t)moves_dev & 3) == 0 && ((uintptr_t)nlinks_dev & 3) == 0,
                "labels_dev, moves_dev and nlinks_dev must be 4-byte aligned");
    OFC_REQUIRE(((uintptr_t)links_dev_ & 7) == 0, "links_dev must be 8-byte aligned");
    OFC_TRY(blob_link_check(W, H, npair, min_area, max_links));
    OFC_TRY(ensure_device(device));
    LinkScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(links_dev(sc, labels_dev, moves_dev, W, H, npair, min_area, max_links, links_dev_, nlinks_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_blob_links_read(int device, const void *links_dev_, const int32_t *nlinks_dev, int ntrans, int max_links,
                        int64_t *links_host, int32_t *nlinks_host)
{
    OFC_REQUIRE(ntrans >= 0, "ntrans = %d: not negative", ntrans);
    OFC_TRY(blob_link_check(1, 1, ntrans + 1, 1, max_links));
    OFC_REQUIRE(ntrans == 0 || (links_dev_ && nlinks_dev && links_host && nlinks_host), "null pointer");
    OFC_TRY(ensure_device(device));
    return blob_links_read(static_cast<const uint64_t *>(links_dev_), votes_of(links_dev_, max_links, ntrans), nlinks_dev, ntrans,
                           max_links, links_host, nlinks_host);
}

int ofc_blob_links(int device, const int32_t *labels_host, const float *flow_host, int W, int H, int npair, int min_area,
                   int max_links, int32_t *moves_out, int64_t *links_host, int32_t *nlinks_host)
{
    OFC_REQUIRE(labels_host && flow_host, "null pointer");
    OFC_REQUIRE(npair < 2 || (links_host && nlinks_host), "null pointer");
    OFC_TRY(blob_link_check(W, H, npair, min_area, max_links));
    OFC_TRY(ensure_device(device));
    LinkScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair;
    const int ntrans = npair - 1;
    OFC_TRY(reserve(sc.labels, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.flow, sizeof(float) * 2 * n));
    OFC_TRY(reserve(sc.moves, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.links, std::max<size_t>(blob_links_bytes(max_links, ntrans), 8)));
    OFC_TRY(reserve(sc.counters, sizeof(int32_t) * std::max(ntrans, 1)));
    OFC_HIP(hipMemcpy(sc.labels.p, labels_host, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    OFC_HIP(hipMemcpy(sc.flow.p, flow_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    OFC_TRY(launch_blob_moves(sc.flow.as<float>(), W, H, npair, sc.moves.as<int32_t>(), nullptr));
    OFC_TRY(links_dev(sc, sc.labels.as<int32_t>(), sc.moves.as<int32_t>(), W, H, npair, min_area, max_links, sc.links.p,
                      sc.counters.as<int32_t>(), nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    if (moves_out) OFC_HIP(hipMemcpy(moves_out, sc.moves.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return blob_links_read(sc.links.as<uint64_t>(), votes_of(sc.links.p, max_links, ntrans), sc.counters.as<int32_t>(), ntrans,
                           max_links, links_host, nlinks_host);
}

int ofc_bench_blob_links(int device, const int32_t *labels_dev, const float *flow_dev, int W, int H, int npair, int what,
                         int iters, float *ms_per_run)
{
    OFC_REQUIRE(labels_dev && flow_dev && ms_per_run && iters >= 1 && what >= 0 && what <= 3, "bad arguments");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0 && ((uintptr_t)labels_dev & 3) == 0, "flow_dev must be 8-byte, labels_dev 4-byte aligned");
    constexpr int MAXL = BLOB_MAX_LINKS;
    OFC_TRY(blob_link_check(W, H, npair, 1, MAXL));
    OFC_TRY(ensure_device(device));
    LinkScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t P = (size_t)W * H, n = P * npair;
    const int ntrans = npair - 1;
    OFC_TRY(reserve(sc.moves, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.areas, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.links, std::max<size_t>(blob_links_bytes(MAXL, ntrans), 8)));
    OFC_TRY(reserve(sc.counters, sizeof(int32_t) * std::max(ntrans, 1)));
    hipStream_t s = nullptr;
    EventPair ev;
    OFC_TRY(ev.create());
    int32_t *moves = sc.moves.as<int32_t>(), *areas = sc.areas.as<int32_t>(), *counters = sc.counters.as<int32_t>();
    uint64_t *keys = sc.links.as<uint64_t>();
    int32_t *votes = votes_of(sc.links.p, MAXL, ntrans);
    double total = 0;
    // one run of the chain, the chosen part between the two events
    auto run = [&](bool timed) -> int {
        auto mark = [&](bool begin, bool here) -> int {
            if (timed && here) OFC_HIP(hipEventRecord(begin ? ev.e0 : ev.e1, s));
            return OFC_OK;
        };
        OFC_TRY(mark(true, what == 0 || what == 3));
        OFC_TRY(launch_blob_moves(flow_dev, W, H, npair, moves, s));
        OFC_TRY(mark(false, what == 0));
        OFC_TRY(mark(true, what == 1));
        OFC_TRY(launch_blob_area(labels_dev, W, H, npair, areas, s));
        OFC_TRY(mark(false, what == 1));
        OFC_TRY(mark(true, what == 2));
        OFC_TRY(launch_blob_links_clear(MAXL, ntrans, keys, votes, counters, s));
        OFC_TRY(launch_blob_links(labels_dev, moves, areas, labels_dev + P, areas + P, W, H, ntrans, 1, MAXL, keys, votes, counters, s));
        OFC_TRY(mark(false, what == 2 || what == 3));
        if (timed) OFC_TRY(ev.add_elapsed(total));
        return OFC_OK;
    };
    for (int w = 0; w < 2; w++) OFC_TRY(run(false));
    for (int i = 0; i < iters; i++) OFC_TRY(run(true));
    OFC_HIP(hipStreamSynchronize(s));
    *ms_per_run = (float)(total / iters);
    return OFC_OK;
}

}  // extern "C"

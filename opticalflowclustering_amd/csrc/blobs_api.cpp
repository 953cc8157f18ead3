// blobs_api.cpp -- C ABI of libofc.so, part 7: connected components of a key map (blobs.hip) on device and host buffers,
// the host forms of its checks and of the table's order, and its measurement hook.
#include "blobs.h"
#include "host_util.h"

#include <mutex>

using namespace ofc;

namespace {

// The library's scratch, one per device: the area and slot words of the table stage, the error word of the label stages,
// the model of the key kernel, and the buffers the host-buffer call and the hook work in.  Each grows on demand and is
// measured against its own size.
struct BlobScratch {
    DevBuf words, err, state, keys, labels, flow, table, found;
    std::mutex mu;
};

BlobScratch &scratch_for(int device) { return device_scratch<BlobScratch>(device); }

int check_keys_args(int use_thr, float thr, int k, const double *mean, const double *centers_c)
{
    OFC_REQUIRE(!use_thr || (std::isfinite(thr) && thr >= 0), "thr must be finite and >= 0");
    if (k != 0) OFC_TRY(check_uv_model(k, mean, centers_c));
    return OFC_OK;
}

// the key kernel's model on the device: mean, centred centres, |c|^2
int set_model(BlobScratch &sc, int k, const double *mean, const double *centers_c, hipStream_t s)
{
    OFC_TRY(reserve(sc.state, sizeof(LloydState)));
    LloydState st;
    memset(&st, 0, sizeof(st));
    if (mean) memcpy(st.mean, mean, sizeof(double) * 2);
    memcpy(st.centers, centers_c, sizeof(double) * 2 * k);
    OFC_HIP(hipMemcpy(sc.state.p, &st, sizeof(st), hipMemcpyHostToDevice));
    return launch_lloyd_set_centers(sc.state.as<LloydState>(), k, 2, s);
}

int keys_dev(BlobScratch &sc, const float *flow_dev, int W, int H, int npair, int use_thr, float thr, int k, const double *mean,
             const double *centers_c, uint32_t select, int merge, uint8_t *keys, hipStream_t s)
{
    if (k > 0) OFC_TRY(set_model(sc, k, mean, centers_c, s));
    return launch_blob_keys(flow_dev, W, H, npair, use_thr != 0, thr, k > 0 ? sc.state.as<LloydState>() : nullptr, k, select,
                            merge != 0, keys, s);
}

// the three stages, then the error word: OFC_EHIP when a capped loop ran out
int label_dev(BlobScratch &sc, const uint8_t *keys, int W, int H, int npair, int connectivity, int32_t *labels, hipStream_t s)
{
    OFC_TRY(reserve(sc.err, sizeof(int)));
    int *err = sc.err.as<int>();
    OFC_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    OFC_TRY(launch_blob_local(keys, W, H, npair, connectivity, labels, err, s));
    OFC_TRY(launch_blob_seam(keys, W, H, npair, connectivity, labels, err, s));
    OFC_TRY(launch_blob_flatten(W, H, npair, labels, err, s));
    int e = 0;
    OFC_HIP(hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, s));
    OFC_HIP(hipStreamSynchronize(s));
    if (e != 0) {
        set_error("connected components: a capped loop ran out (stages %d); the label map is not valid", e);
        return OFC_EHIP;
    }
    return OFC_OK;
}

int table_dev(BlobScratch &sc, const uint8_t *keys, const int32_t *labels, const float *flow, int W, int H, int npair,
              int min_area, int max_blobs, int64_t *table, int32_t *found, hipStream_t s)
{
    OFC_TRY(reserve(sc.words, sizeof(int32_t) * (size_t)W * H * npair));
    return launch_blob_table(keys, labels, flow, W, H, npair, min_area, max_blobs, sc.words.as<int32_t>(), table, found, s);
}

}  // namespace

namespace ofc {

int blob_table_read(const int64_t *table_dev_, const int32_t *found_dev, int npair, int max_blobs, int64_t *table_host,
                    int32_t *n_host, int32_t *found_host)
{
    std::vector<int32_t> found(npair);
    OFC_HIP(hipMemcpy(found.data(), found_dev, sizeof(int32_t) * npair, hipMemcpyDeviceToHost));
    std::vector<int64_t> slots;
    for (int i = 0; i < npair; i++) {
        const int have = found[i] >= 0 && found[i] <= max_blobs ? found[i] : 0;
        slots.resize((size_t)have * BLOB_NF);
        if (have)
            OFC_HIP(hipMemcpy(slots.data(), table_dev_ + (size_t)i * max_blobs * BLOB_NF, sizeof(int64_t) * slots.size(),
                              hipMemcpyDeviceToHost));
        blob_order_records(slots.data(), found[i], max_blobs, table_host + (size_t)i * max_blobs * BLOB_NF, n_host + i);
        found_host[i] = found[i];
    }
    return OFC_OK;
}

}  // namespace ofc

extern "C" {

int ofc_blob_check(int W, int H, int npair, int connectivity, int min_area, int max_blobs)
{
    return blob_check(W, H, npair, connectivity, min_area, max_blobs);
}

int ofc_blob_keys_dev(int device, const float *flow_dev, int W, int H, int npair, int use_thr, float thr, int k,
                      const double *mean, const double *centers_c, uint32_t select, int merge, uint8_t *keys_dev_)
{
    OFC_REQUIRE(flow_dev && keys_dev_, "null pointer");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "flow_dev must be 8-byte aligned");
    OFC_TRY(blob_check(W, H, npair, 8, 1, 1));
    OFC_TRY(check_keys_args(use_thr, thr, k, mean, centers_c));
    OFC_TRY(ensure_device(device));
    BlobScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(keys_dev(sc, flow_dev, W, H, npair, use_thr, thr, k, mean, centers_c, select, merge, keys_dev_, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_blob_label_dev(int device, const uint8_t *keys_dev_, int W, int H, int npair, int connectivity, int32_t *labels_dev)
{
    OFC_REQUIRE(keys_dev_ && labels_dev, "null pointer");
    OFC_REQUIRE(((uintptr_t)labels_dev & 3) == 0, "labels_dev must be 4-byte aligned");
    OFC_TRY(blob_check(W, H, npair, connectivity, 1, 1));
    OFC_TRY(ensure_device(device));
    BlobScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    return label_dev(sc, keys_dev_, W, H, npair, connectivity, labels_dev, nullptr);
}

int ofc_blob_table_dev(int device, const uint8_t *keys_dev_, const int32_t *labels_dev, const float *flow_dev, int W, int H,
                       int npair, int min_area, int max_blobs, int64_t *table_dev_, int32_t *found_dev)
{
    OFC_REQUIRE(keys_dev_ && labels_dev && table_dev_ && found_dev, "null pointer");
    OFC_REQUIRE(((uintptr_t)labels_dev & 3) == 0 && ((uintptr_t)found_dev & 3) == 0, "labels_dev and found_dev must be 4-byte aligned");
    OFC_REQUIRE(((uintptr_t)table_dev_ & 7) == 0 && ((uintptr_t)flow_dev & 7) == 0, "table_dev and flow_dev must be 8-byte aligned");
    OFC_TRY(blob_check(W, H, npair, 8, min_area, max_blobs));
    OFC_TRY(ensure_device(device));
    BlobScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    OFC_TRY(table_dev(sc, keys_dev_, labels_dev, flow_dev, W, H, npair, min_area, max_blobs, table_dev_, found_dev, nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    return OFC_OK;
}

int ofc_blob_table_read(int device, const int64_t *table_dev_, const int32_t *found_dev, int npair, int max_blobs,
                        int64_t *table_host, int32_t *n_host, int32_t *found_host)
{
    OFC_REQUIRE(table_dev_ && found_dev && table_host && n_host && found_host, "null pointer");
    OFC_TRY(blob_check(1, 1, npair, 8, 1, max_blobs));
    OFC_TRY(ensure_device(device));
    return blob_table_read(table_dev_, found_dev, npair, max_blobs, table_host, n_host, found_host);
}

int ofc_blobs(int device, const uint8_t *keys_host, const float *flow_host, int W, int H, int npair, int use_thr, float thr,
              int k, const double *mean, const double *centers_c, uint32_t select, int merge, int connectivity, int min_area,
              int max_blobs, int32_t *labels_host, uint8_t *keys_out, int64_t *table_host, int32_t *n_host,
              int32_t *found_host)
{
    OFC_REQUIRE((keys_host || flow_host) && table_host && n_host && found_host, "null pointer");
    OFC_TRY(blob_check(W, H, npair, connectivity, min_area, max_blobs));
    if (!keys_host) OFC_TRY(check_keys_args(use_thr, thr, k, mean, centers_c));
    OFC_TRY(ensure_device(device));
    BlobScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair;
    OFC_TRY(reserve(sc.keys, n));
    OFC_TRY(reserve(sc.labels, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.table, sizeof(int64_t) * BLOB_NF * (size_t)max_blobs * npair));
    OFC_TRY(reserve(sc.found, sizeof(int32_t) * npair));
    if (flow_host) {
        OFC_TRY(reserve(sc.flow, sizeof(float) * 2 * n));
        OFC_HIP(hipMemcpy(sc.flow.p, flow_host, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    }
    const float *flow = flow_host ? sc.flow.as<float>() : nullptr;
    uint8_t *keys = sc.keys.as<uint8_t>();
    if (keys_host) OFC_HIP(hipMemcpy(keys, keys_host, n, hipMemcpyHostToDevice));
    else OFC_TRY(keys_dev(sc, flow, W, H, npair, use_thr, thr, k, mean, centers_c, select, merge, keys, nullptr));
    OFC_TRY(label_dev(sc, keys, W, H, npair, connectivity, sc.labels.as<int32_t>(), nullptr));
    OFC_TRY(table_dev(sc, keys, sc.labels.as<int32_t>(), flow, W, H, npair, min_area, max_blobs, sc.table.as<int64_t>(),
                      sc.found.as<int32_t>(), nullptr));
    OFC_HIP(hipStreamSynchronize(nullptr));
    if (labels_host) OFC_HIP(hipMemcpy(labels_host, sc.labels.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (keys_out) OFC_HIP(hipMemcpy(keys_out, keys, n, hipMemcpyDeviceToHost));
    return blob_table_read(sc.table.as<int64_t>(), sc.found.as<int32_t>(), npair, max_blobs, table_host, n_host, found_host);
}

int ofc_bench_blobs(int device, const uint8_t *keys_dev_, const float *flow_dev, int W, int H, int npair, int connectivity,
                    int what, int iters, float *ms_per_run)
{
    OFC_REQUIRE(keys_dev_ && ms_per_run && iters >= 1 && what >= 0 && what <= 6, "bad arguments");
    OFC_REQUIRE(what != 0 || flow_dev, "the key kernel needs a field");
    OFC_REQUIRE(((uintptr_t)flow_dev & 7) == 0, "flow_dev must be 8-byte aligned");
    constexpr int MAXB = BLOB_MAX_BLOBS;
    OFC_TRY(blob_check(W, H, npair, connectivity, 1, MAXB));
    OFC_TRY(ensure_device(device));
    BlobScratch &sc = scratch_for(device);
    std::lock_guard<std::mutex> lock(sc.mu);
    const size_t n = (size_t)W * H * npair;
    OFC_TRY(reserve(sc.keys, n));
    OFC_TRY(reserve(sc.labels, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.words, sizeof(int32_t) * n));
    OFC_TRY(reserve(sc.table, sizeof(int64_t) * BLOB_NF * (size_t)MAXB * npair));
    OFC_TRY(reserve(sc.found, sizeof(int32_t) * npair));
    OFC_TRY(reserve(sc.err, sizeof(int)));
    OFC_HIP(hipMemset(sc.err.p, 0, sizeof(int)));
    hipStream_t s = nullptr;
    EventPair ev;
    OFC_TRY(ev.create());
    int32_t *labels = sc.labels.as<int32_t>();
    int *err = sc.err.as<int>();
    double total = 0;
    // one run of the chain, the chosen part between the two events
    auto run = [&](bool timed) -> int {
        auto mark = [&](bool begin, int first, int last) -> int {
            if (timed && (begin ? first : last)) OFC_HIP(hipEventRecord(begin ? ev.e0 : ev.e1, s));
            return OFC_OK;
        };
        OFC_TRY(mark(true, what == 0, 0));
        if (what == 0) OFC_TRY(launch_blob_keys(flow_dev, W, H, npair, true, 0.5f, nullptr, 0, 0, false, sc.keys.as<uint8_t>(), s));
        OFC_TRY(mark(false, 0, what == 0));
        OFC_TRY(mark(true, what == 1 || what == 4 || what == 6, 0));
        OFC_TRY(launch_blob_local(keys_dev_, W, H, npair, connectivity, labels, err, s));
        OFC_TRY(mark(false, 0, what == 1));
        OFC_TRY(mark(true, what == 2, 0));
        OFC_TRY(launch_blob_seam(keys_dev_, W, H, npair, connectivity, labels, err, s));
        OFC_TRY(mark(false, 0, what == 2));
        OFC_TRY(mark(true, what == 3, 0));
        OFC_TRY(launch_blob_flatten(W, H, npair, labels, err, s));
        OFC_TRY(mark(false, 0, what == 3 || what == 4));
        OFC_TRY(mark(true, what == 5, 0));
        OFC_TRY(launch_blob_table(keys_dev_, labels, flow_dev, W, H, npair, 1, MAXB, sc.words.as<int32_t>(), sc.table.as<int64_t>(),
                                  sc.found.as<int32_t>(), s));
        OFC_TRY(mark(false, 0, what == 5 || what == 6));
        if (timed) OFC_TRY(ev.add_elapsed(total));
        return OFC_OK;
    };
    for (int w = 0; w < 2; w++) OFC_TRY(run(false));
    for (int i = 0; i < iters; i++) OFC_TRY(run(true));
    OFC_HIP(hipStreamSynchronize(s));
    int e = 0;
    OFC_HIP(hipMemcpy(&e, err, sizeof(int), hipMemcpyDeviceToHost));
    if (e != 0) {
        set_error("connected components: a capped loop ran out (stages %d)", e);
        return OFC_EHIP;
    }
    *ms_per_run = (float)(total / iters);
    return OFC_OK;
}

}  // extern "C"

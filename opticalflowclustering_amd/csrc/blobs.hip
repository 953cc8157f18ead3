// blobs.hip -- connected components of a per-pixel key map and one integer record per component (ofc_blob_*, the
// definition is in include/ofc.h): where the reference read YOLO boxes and contour files, this groups the pixels that
// move against the background, or that carry one cluster label, into regions and describes each.
//
// Label map: a minimum-index union-find (Playne-Hawick / Komura).  parent[i] is an int32 per pixel, -1 for background;
// the invariant parent[i] <= i holds from the first stage on and a set's root is the word that points to itself, so the
// root of a finished set is its smallest index.  Three launches; no work-group ever waits on another, and a stage that
// reads what other work-groups wrote is a launch of its own.
//  1. k_blob_local: a work-group resolves one BLOB_TW x BLOB_TH tile in LDS.  A wave takes a row at a time (BLOB_TW = the
//     wave's width): the start of a pixel's run of equal keys is the highest set bit at or below its lane in the ballot
//     of run starts.  Runs are then united with the row above by atomicMin on LDS words, each pixel walks to its root,
//     and parent[i] = the global index of that tile-local root.
//  2. k_blob_seam: one lane per pixel of a tile's first row or first column unites it with its equal-key neighbours
//     across the border (with connectivity 8 the diagonal ones too, tile corners included).  parent words are touched
//     only by agent-scope atomics here: relaxed loads for the walks, atomicMin for the links.
//  3. k_blob_flatten: every foreground pixel walks to its root and stores it.
// A union is skipped where the definition already implies it through unions other lanes make and connections inside a
// tile; the comments at each test name them (the argument never rests on another skipped union of the same border, so
// it is not circular).
// Table: k_blob_area counts pixels at the roots; k_blob_slots gives each root with area >= min_area a slot from the
// pair's counter (which counts on past max_blobs: its end value is `found`) and writes the record's start; k_blob_accum
// adds box and sums.  Both sweeps combine before they touch memory: a lane keeps a private run while its root repeats,
// the lanes of a wave that share a root fold by shuffles (uv_hist.hip's ballot loop), and the waves of a work-group meet
// in an LDS table keyed by root, written out once.  So a background-sized component costs one atomic per work-group and
// field, not per pixel.
// Every loop that walks parents or retries a link is capped; a cap that is hit sets the error word, and the API call
// returns OFC_EHIP.
#include "blobs.h"
#include "lloyd_device.h"

#include <algorithm>

namespace ofc {

namespace {

constexpr int BL_THREADS = 256, BL_WAVES = BL_THREADS / 64, BL_ROWS = BLOB_TH / BL_WAVES, BL_TILE = BLOB_TW * BLOB_TH;
constexpr int BL_SLOTS = 256, BL_PROBES = 4, BL_UNROLL = BLOB_SHARE / BL_THREADS;
static_assert(BLOB_TW == 64, "a wave resolves one tile row by ballot");
static_assert(BLOB_TH % BL_WAVES == 0 && BL_UNROLL * BL_THREADS == BLOB_SHARE, "tile rows and shares divide evenly");

typedef unsigned long long u64;

// ---- the union-find, on LDS words (SCOPE workgroup) and on global words (SCOPE agent) ----
template <int SCOPE> __device__ __forceinline__ int bl_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE> __device__ __forceinline__ int bl_min(int *p, int v)
{
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
}

// The root of r's set as far as this lane can see.  Terminates: a word only ever holds an index <= its own, so r strictly
// decreases until a word points to itself; a stale read yields an older ancestor of the same set, never a foreign index.
// Anything else (a negative word, a larger one) cannot be read from a foreground pixel; it ends the walk with the error set,
// so that no index ever leaves [0, r].
template <int SCOPE> __device__ __forceinline__ int bl_find(const int *parent, int r, unsigned cap, int *err, int code)
{
    for (unsigned it = 0; it < cap; it++) {
        const int p = bl_load<SCOPE>(parent + r);
        if (p == r) return r;
        if (p < 0 || p > r) break;
        r = p;
    }
    atomicOr(err, code);
    return r;
}

// Unite the sets of a and b.  Terminates: every round replaces the larger of (a, b) by a strictly smaller index (the word's
// old value, which the atomic returns: it corrects a stale walk), so at most max(a, b) rounds.  When the larger was a root
// the link is made and the sets are one; otherwise its old parent is an ancestor in the same set and takes its place.
template <int SCOPE> __device__ __forceinline__ void bl_unite(int *parent, int a, int b, unsigned cap, int *err, int code)
{
    a = bl_find<SCOPE>(parent, a, cap, err, code);
    b = bl_find<SCOPE>(parent, b, cap, err, code);
    for (unsigned it = 0; it < cap; it++) {
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = bl_min<SCOPE>(parent + a, b);
        if (old == a) return;
        if (old < 0 || old > a) break;
        a = bl_find<SCOPE>(parent, old, cap, err, code);
    }
    atomicOr(err, code);
}

constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP, AG = __HIP_MEMORY_SCOPE_AGENT;

// ---- keys ----
// flow [n][2] -> keys [n]; st is dereferenced only when k > 0 (uniform addresses: scalar loads).  VEC (flow 16-byte and keys
// 4-byte aligned): a lane takes four consecutive vectors as two 16-byte loads and stores their keys as one word; the last
// n % 4 vectors, and everything without VEC, go one vector per lane.
template <bool VEC>
__global__ __launch_bounds__(BL_THREADS) void k_blob_keys(const float2 *__restrict__ flow, long long n, int use_thr, float thr2,
                                                          const LloydState *__restrict__ st, int k, unsigned select, int merge,
                                                          uint8_t *__restrict__ keys)
{
    constexpr int KMAX = LLOYD_KMAX;
    double c[2 * KMAX], cn[KMAX], m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        cn[j] = (j < k) ? st->cn[j] : 0.0;
        c[2 * j] = (j < k) ? st->centers[2 * j] : 0.0;
        c[2 * j + 1] = (j < k) ? st->centers[2 * j + 1] : 0.0;
    }
    if (k > 0) { m0 = st->mean[0]; m1 = st->mean[1]; }
    auto key_of = [&](float u, float v) -> unsigned {
        bool fg = !use_thr || flow_is_moving(u, v, thr2);
        int L = 0;
        if (k > 0) {
            const double x[2] = {(double)u - m0, (double)v - m1};
            L = assign_point<2, KMAX>(x, c, cn, k);
            fg = fg && ((select >> L) & 1u);
        }
        return fg ? (merge ? 0u : (unsigned)L) : 255u;
    };
    const long long stride = (long long)gridDim.x * BL_THREADS, t0 = (long long)blockIdx.x * BL_THREADS + threadIdx.x;
    const long long n4 = VEC ? n / 4 : 0;
    for (long long q = t0; q < n4; q += stride) {
        const float4 a = *reinterpret_cast<const float4 *>(flow + 4 * q), b = *reinterpret_cast<const float4 *>(flow + 4 * q + 2);
        *reinterpret_cast<unsigned *>(keys + 4 * q) =
            key_of(a.x, a.y) | (key_of(a.z, a.w) << 8) | (key_of(b.x, b.y) << 16) | (key_of(b.z, b.w) << 24);
    }
    for (long long i = 4 * n4 + t0; i < n; i += stride) {
        const float2 f = flow[i];
        keys[i] = (uint8_t)key_of(f.x, f.y);
    }
}

// ---- stage 1: one tile in LDS ----
template <int CONN>
__global__ __launch_bounds__(BL_THREADS) void k_blob_local(const uint8_t *__restrict__ keys, int W, int H, int ntx,
                                                           int32_t *__restrict__ parent, int *err)
{
    __shared__ int s_lab[BL_TILE];
    __shared__ uint8_t s_key[BL_TILE];
    const size_t base = (size_t)blockIdx.y * (size_t)W * (size_t)H;
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = tx * BLOB_TW, y0 = ty * BLOB_TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    constexpr unsigned CAP = BL_TILE + 1;

    // rows: every pixel starts at the first pixel of its run of equal keys
#pragma unroll
    for (int q = 0; q < BL_ROWS; q++) {
        const int r = wave * BL_ROWS + q, y = y0 + r;
        const bool in = x < W && y < H;
        const int key = in ? (int)keys[base + (size_t)y * W + x] : 255;
        const int left = __shfl_up(key, 1);
        const bool start = key != 255 && (lane == 0 || left != key);
        const u64 starts = __ballot(start);
        const u64 upto = starts & ((2ull << lane) - 1ull);           // lane 63: 2 << 63 wraps to 0, the mask to all ones
        s_key[r * BLOB_TW + lane] = (uint8_t)key;
        s_lab[r * BLOB_TW + lane] = key != 255 ? r * BLOB_TW + (63 - __clzll((long long)upto)) : -1;
    }
    __syncthreads();
    // columns: unite with the row above
#pragma unroll
    for (int q = 0; q < BL_ROWS; q++) {
        const int r = wave * BL_ROWS + q, i = r * BLOB_TW + lane;
        if (r == 0) continue;
        const int key = s_key[i];
        if (key == 255) continue;
        if (s_key[i - BLOB_TW] == key) {
            // skipped when the left pixel and the one above it carry the key too: the left pixel unites those two (or skips
            // for the same reason, down to lane 0 or the first break), and both horizontal pairs share a run
            const bool implied = lane > 0 && s_key[i - 1] == key && s_key[i - BLOB_TW - 1] == key;
            if (!implied) bl_unite<WG>(s_lab, i, i - BLOB_TW, CAP, err, BLOB_ERR_LOCAL);
        } else if (CONN == 8) {
            // a diagonal matters only when the pixel above differs (else it shares a run with both diagonal pixels), and is
            // skipped when the horizontal neighbour on its side carries the key: that neighbour sits right below it
            if (lane > 0 && s_key[i - BLOB_TW - 1] == key && s_key[i - 1] != key)
                bl_unite<WG>(s_lab, i, i - BLOB_TW - 1, CAP, err, BLOB_ERR_LOCAL);
            if (lane < 63 && s_key[i - BLOB_TW + 1] == key && s_key[i + 1] != key)
                bl_unite<WG>(s_lab, i, i - BLOB_TW + 1, CAP, err, BLOB_ERR_LOCAL);
        }
    }
    __syncthreads();
    // nothing writes s_lab any more: every pixel reads its tile-local root and stores that pixel's global index
#pragma unroll
    for (int q = 0; q < BL_ROWS; q++) {
        const int r = wave * BL_ROWS + q, y = y0 + r, i = r * BLOB_TW + lane;
        if (x >= W || y >= H) continue;
        int out = -1;
        if (s_lab[i] >= 0) {
            const int root = bl_find<WG>(s_lab, i, CAP, err, BLOB_ERR_LOCAL);
            out = (y0 + root / BLOB_TW) * W + x0 + (root % BLOB_TW);
        }
        parent[base + (size_t)y * W + x] = out;
    }
}

// ---- stage 2: across the tile borders ----
// seam pixel s of a pair: s < nh: row (s / W + 1) * BLOB_TH, column s % W; else column ((s - nh) / H + 1) * BLOB_TW, row
// (s - nh) % H
template <int CONN>
__global__ __launch_bounds__(BL_THREADS) void k_blob_seam(const uint8_t *__restrict__ keys, int W, int H, int nh, int nseam,
                                                          int32_t *parent, unsigned cap, int *err)
{
    const size_t base = (size_t)blockIdx.y * (size_t)W * (size_t)H;
    const uint8_t *K = keys + base;
    int *p = parent + base;
    int s = blockIdx.x * BL_THREADS + threadIdx.x;
    if (s >= nseam) return;
    if (s < nh) {                                          // first row of a tile: the neighbours are in the row above
        const int j = s / W, x = s - j * W, y = (j + 1) * BLOB_TH, i = y * W + x;
        const int key = K[i];
        if (key == 255) return;
        if (K[i - W] == key) {
            // implied when the left pixel is in this tile and it and the one above it carry the key: the left pixel's lane
            // unites those two, and both horizontal pairs were united inside their tiles
            const bool implied = (x % BLOB_TW) != 0 && K[i - 1] == key && K[i - W - 1] == key;
            if (!implied) bl_unite<AG>(p, i, i - W, cap, err, BLOB_ERR_SEAM);
        } else if (CONN == 8) {
            // skipped when the horizontal neighbour on the diagonal's side carries the key: it lies right below the diagonal
            // pixel and its own lane unites them; this pixel and that neighbour are one run, or one union of a column seam
            // that is never skipped in a tile's first row
            if (x > 0 && K[i - W - 1] == key && K[i - 1] != key) bl_unite<AG>(p, i, i - W - 1, cap, err, BLOB_ERR_SEAM);
            if (x < W - 1 && K[i - W + 1] == key && K[i + 1] != key) bl_unite<AG>(p, i, i - W + 1, cap, err, BLOB_ERR_SEAM);
        }
    } else {                                               // first column of a tile: the neighbours are in the column before
        s -= nh;
        const int j = s / H, y = s - j * H, x = (j + 1) * BLOB_TW, i = y * W + x;
        const int key = K[i];
        if (key == 255) return;
        if (K[i - 1] == key) {
            // implied when the pixel above is in this tile and it and its left neighbour carry the key (the mirror of the above)
            const bool implied = (y % BLOB_TH) != 0 && K[i - W] == key && K[i - W - 1] == key;
            if (!implied) bl_unite<AG>(p, i, i - 1, cap, err, BLOB_ERR_SEAM);
        } else if (CONN == 8) {
            if (y > 0 && K[i - W - 1] == key && K[i - W] != key) bl_unite<AG>(p, i, i - W - 1, cap, err, BLOB_ERR_SEAM);
            if (y < H - 1 && K[i + W - 1] == key && K[i + W] != key) bl_unite<AG>(p, i, i + W - 1, cap, err, BLOB_ERR_SEAM);
        }
    }
}

// ---- stage 3: every pixel to its root ----
// A lane takes four consecutive pixels and keeps the root of the last parent it walked from: neighbours mostly share it.
// Other lanes store roots into words this one walks through; both the old and the new value are ancestors in the same set.
// A pixel's own word is written by its own lane only, so the lane reads and writes it plainly: with VEC (P a multiple of 4
// and the map 16-byte aligned, so every lane's four words are) as one 16-byte load and at most one 16-byte store.  The
// walks go through words other lanes write, by agent-scope atomic loads.
template <bool VEC>
__global__ __launch_bounds__(BL_THREADS) void k_blob_flatten(int32_t *parent, int P, unsigned cap, int *err)
{
    int *p = parent + (size_t)blockIdx.y * (size_t)P;
    const long long i0 = ((long long)blockIdx.x * BL_THREADS + threadIdx.x) * 4;
    if (i0 >= P) return;
    int v[4];
    if (VEC) {
        const int4 t = *reinterpret_cast<const int4 *>(p + i0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = i0 + q < P ? p[i0 + q] : -1;
    }
    int prev = -1, prev_root = -1;
    bool changed = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (v[q] < 0 || v[q] >= (int)(i0 + q)) continue;   // background (or past the end), or a root
        const int root = v[q] == prev ? prev_root : bl_find<AG>(p, v[q], cap, err, BLOB_ERR_FLATTEN);
        prev = v[q];
        prev_root = root;
        if (root != v[q]) {
            changed = true;
            v[q] = root;
            if (!VEC) __hip_atomic_store(p + i0 + q, root, __ATOMIC_RELAXED, AG);
        }
    }
    if (VEC && changed) *reinterpret_cast<int4 *>(p + i0) = make_int4(v[0], v[1], v[2], v[3]);
}

// ---- the table ----
template <class T, class Op> __device__ __forceinline__ T bl_wave(T v, Op op)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}

// the slot of `key` in a work-group's LDS table (claimed by compare-and-swap), or -1 after BL_PROBES slots owned by others
__device__ __forceinline__ int bl_slot(int *s_key, int key)
{
    int slot = (int)(((unsigned)key * 2654435761u) >> 24) & (BL_SLOTS - 1);
    for (int probe = 0; probe < BL_PROBES; probe++, slot = (slot + 1) & (BL_SLOTS - 1)) {
        const int old = atomicCAS(&s_key[slot], -1, key);
        if (old == -1 || old == key) return slot;
    }
    return -1;
}

// labels [npair][P] -> words [npair][P] (zeroed): words[root] = area
__global__ __launch_bounds__(BL_THREADS) void k_blob_area(const int32_t *__restrict__ labels, int P, int32_t *words)
{
    __shared__ int s_key[BL_SLOTS], s_cnt[BL_SLOTS];
    for (int s = threadIdx.x; s < BL_SLOTS; s += BL_THREADS) { s_key[s] = -1; s_cnt[s] = 0; }
    __syncthreads();
    const int32_t *L = labels + (size_t)blockIdx.y * (size_t)P;
    int *Wd = words + (size_t)blockIdx.y * (size_t)P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * BLOB_SHARE + wave * (BLOB_SHARE / BL_WAVES) + lane;
    int r[BL_UNROLL];
#pragma unroll
    for (int q = 0; q < BL_UNROLL; q++) {
        const long long i = i0 + q * 64;
        const int v = i < P ? L[i] : -1;
        r[q] = v < P ? v : -1;                             // a label map of the caller's: nothing outside it is indexed
    }
    auto combine = [&](bool go, int key, int cnt) {        // called by all 64 lanes
        u64 todo = __ballot(go);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k = __builtin_amdgcn_readlane(key, leader);
            const bool mine = go && key == k;
            const int total = bl_wave(mine ? cnt : 0, [](int a, int b) { return a + b; });
            if (lane == leader) {
                const int slot = bl_slot(s_key, k);
                if (slot >= 0) atomicAdd(&s_cnt[slot], total);
                else atomicAdd(&Wd[k], total);
            }
            todo &= ~__ballot(mine);
        }
    };
    int pr = -1, pc = 0;                                   // the lane's run
#pragma unroll
    for (int q = 0; q < BL_UNROLL; q++) {
        const bool ended = pr >= 0 && r[q] >= 0 && r[q] != pr;         // a background pixel ends no run
        if (__ballot(ended)) combine(ended, pr, pc);
        if (ended) pc = 0;
        if (r[q] >= 0) { pr = r[q]; pc++; }
    }
    combine(pr >= 0, pr, pc);
    __syncthreads();
    for (int s = threadIdx.x; s < BL_SLOTS; s += BL_THREADS)
        if (s_key[s] >= 0) atomicAdd(&Wd[s_key[s]], s_cnt[s]);
}

// every root: area -> slot (or -1), the pair's counter, the record's start
__global__ __launch_bounds__(BL_THREADS) void k_blob_slots(const uint8_t *__restrict__ keys, const int32_t *__restrict__ labels,
                                                           int W, int P, int min_area, int max_blobs, int32_t *words,
                                                           long long *__restrict__ table, int32_t *found)
{
    const size_t base = (size_t)blockIdx.y * (size_t)P;
    const long long i = (long long)blockIdx.x * BL_THREADS + threadIdx.x;
    if (i >= P) return;
    if (labels[base + i] != (int)i) return;
    const int area = words[base + i];
    int slot = -1;
    if (area >= min_area) {
        slot = atomicAdd(&found[blockIdx.y], 1);
        if (slot >= max_blobs) slot = -1;
    }
    words[base + i] = slot;
    if (slot < 0) return;
    long long *rec = table + ((size_t)blockIdx.y * max_blobs + slot) * BLOB_NF;
    rec[0] = i;
    rec[1] = keys[base + i];
    rec[2] = area;
    rec[3] = W;                                            // xmin, ymin: above every coordinate
    rec[4] = P;
    rec[5] = -1;                                           // xmax, ymax: below
    rec[6] = -1;
#pragma unroll
    for (int f = 7; f < BLOB_NF; f++) rec[f] = 0;
}

struct BlAcc {
    int x0, y0, x1, y1;
    long long sx, sy, nv, qu, qv;
    __device__ __forceinline__ void clear(int W, int H)
    {
        x0 = W; y0 = H; x1 = -1; y1 = -1;
        sx = sy = nv = qu = qv = 0;
    }
};

// labels, words (slots at the roots), flow (FLOW) -> box and sums of the records
template <bool FLOW>
__global__ __launch_bounds__(BL_THREADS) void k_blob_accum(const int32_t *__restrict__ labels, const int32_t *__restrict__ words,
                                                           const float2 *__restrict__ flow, int W, int H, int max_blobs,
                                                           long long *table)
{
    __shared__ int s_key[BL_SLOTS];
    __shared__ int s_box[4][BL_SLOTS];
    __shared__ u64 s_sum[5][BL_SLOTS];
    const int P = W * H;
    for (int s = threadIdx.x; s < BL_SLOTS; s += BL_THREADS) {
        s_key[s] = -1;
        s_box[0][s] = W; s_box[1][s] = H; s_box[2][s] = -1; s_box[3][s] = -1;
#pragma unroll
        for (int f = 0; f < 5; f++) s_sum[f][s] = 0;
    }
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * (size_t)P;
    const int32_t *L = labels + base, *Wd = words + base;
    long long *T = table + (size_t)blockIdx.y * max_blobs * BLOB_NF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * BLOB_SHARE + wave * (BLOB_SHARE / BL_WAVES) + lane;

    auto to_record = [&](int slot, const BlAcc &a) {       // straight to the table: the LDS table had no room
        long long *rec = T + (size_t)slot * BLOB_NF;
        __hip_atomic_fetch_min(rec + 3, (long long)a.x0, __ATOMIC_RELAXED, AG);
        __hip_atomic_fetch_min(rec + 4, (long long)a.y0, __ATOMIC_RELAXED, AG);
        __hip_atomic_fetch_max(rec + 5, (long long)a.x1, __ATOMIC_RELAXED, AG);
        __hip_atomic_fetch_max(rec + 6, (long long)a.y1, __ATOMIC_RELAXED, AG);
        __hip_atomic_fetch_add(rec + 7, a.sx, __ATOMIC_RELAXED, AG);
        __hip_atomic_fetch_add(rec + 8, a.sy, __ATOMIC_RELAXED, AG);
        if (FLOW) {
            __hip_atomic_fetch_add(rec + 9, a.nv, __ATOMIC_RELAXED, AG);
            __hip_atomic_fetch_add(rec + 10, a.qu, __ATOMIC_RELAXED, AG);
            __hip_atomic_fetch_add(rec + 11, a.qv, __ATOMIC_RELAXED, AG);
        }
    };
    auto combine = [&](bool go, int key, const BlAcc &a) { // called by all 64 lanes
        u64 todo = __ballot(go);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k = __builtin_amdgcn_readlane(key, leader);
            const bool mine = go && key == k;
            auto imin = [](int p, int q) { return p < q ? p : q; };
            auto imax = [](int p, int q) { return p > q ? p : q; };
            auto ladd = [](long long p, long long q) { return p + q; };
            BlAcc t;
            t.x0 = bl_wave(mine ? a.x0 : W, imin);
            t.y0 = bl_wave(mine ? a.y0 : H, imin);
            t.x1 = bl_wave(mine ? a.x1 : -1, imax);
            t.y1 = bl_wave(mine ? a.y1 : -1, imax);
            t.sx = bl_wave(mine ? a.sx : 0ll, ladd);
            t.sy = bl_wave(mine ? a.sy : 0ll, ladd);
            t.nv = t.qu = t.qv = 0;
            if (FLOW) {
                t.nv = bl_wave(mine ? a.nv : 0ll, ladd);
                t.qu = bl_wave(mine ? a.qu : 0ll, ladd);
                t.qv = bl_wave(mine ? a.qv : 0ll, ladd);
            }
            if (lane == leader) {
                const int slot = bl_slot(s_key, k);
                if (slot >= 0) {
                    atomicMin(&s_box[0][slot], t.x0);
                    atomicMin(&s_box[1][slot], t.y0);
                    atomicMax(&s_box[2][slot], t.x1);
                    atomicMax(&s_box[3][slot], t.y1);
                    atomicAdd(&s_sum[0][slot], (u64)t.sx);
                    atomicAdd(&s_sum[1][slot], (u64)t.sy);
                    if (FLOW) {
                        atomicAdd(&s_sum[2][slot], (u64)t.nv);
                        atomicAdd(&s_sum[3][slot], (u64)t.qu);
                        atomicAdd(&s_sum[4][slot], (u64)t.qv);
                    }
                } else {
                    to_record(k, t);
                }
            }
            todo &= ~__ballot(mine);
        }
    };

    int sl[BL_UNROLL];
    float2 f[BL_UNROLL];
#pragma unroll
    for (int q = 0; q < BL_UNROLL; q++) {
        const long long i = i0 + q * 64;
        const int r = i < P ? L[i] : -1;
        const int s = (r >= 0 && r < P) ? Wd[r] : -1;      // labels and words are checked before they index anything
        sl[q] = s < max_blobs ? s : -1;
        f[q] = (FLOW && i < P) ? flow[base + i] : make_float2(0.f, 0.f);
    }
    int ps = -1;                                           // the lane's run: the slot and what it has gathered for it
    BlAcc a;
    a.clear(W, H);
#pragma unroll
    for (int q = 0; q < BL_UNROLL; q++) {
        const bool ended = ps >= 0 && sl[q] >= 0 && sl[q] != ps;
        if (__ballot(ended)) combine(ended, ps, a);
        if (ended) a.clear(W, H);
        if (sl[q] >= 0) {
            const int i = (int)(i0 + q * 64), y = i / W, x = i - y * W;
            ps = sl[q];
            a.x0 = min(a.x0, x); a.y0 = min(a.y0, y); a.x1 = max(a.x1, x); a.y1 = max(a.y1, y);
            a.sx += x;
            a.sy += y;
            if (FLOW) {
                const bool valid = fabsf(f[q].x) < 1024.f && fabsf(f[q].y) < 1024.f;             // NaN and inf fail
                // valid: the fixed-point value is an integer of magnitude < 2^26, exact in f64
                a.nv += valid;
                a.qu += valid ? __double2int_rn((double)f[q].x * 65536.0) : 0;
                a.qv += valid ? __double2int_rn((double)f[q].y * 65536.0) : 0;
            }
        }
    }
    combine(ps >= 0, ps, a);
    __syncthreads();
    for (int s = threadIdx.x; s < BL_SLOTS; s += BL_THREADS) {
        if (s_key[s] < 0) continue;
        BlAcc t;
        t.x0 = s_box[0][s]; t.y0 = s_box[1][s]; t.x1 = s_box[2][s]; t.y1 = s_box[3][s];
        t.sx = (long long)s_sum[0][s]; t.sy = (long long)s_sum[1][s];
        t.nv = (long long)s_sum[2][s]; t.qu = (long long)s_sum[3][s]; t.qv = (long long)s_sum[4][s];
        to_record(s_key[s], t);
    }
}

unsigned walk_cap(int W, int H)
{
    const uint64_t tiles = (uint64_t)cdiv(W, BLOB_TW) * (uint64_t)cdiv(H, BLOB_TH);
    return (unsigned)std::min<uint64_t>(tiles * BL_TILE, 0xffffffffull);
}

}  // namespace

int blob_check(int W, int H, int npair, int connectivity, int min_area, int max_blobs)
{
    OFC_REQUIRE(W >= 1 && H >= 1, "W = %d, H = %d: a frame has at least one pixel", W, H);
    OFC_REQUIRE(npair >= 1, "npair = %d: at least one pair", npair);
    OFC_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity = %d is neither 4 nor 8", connectivity);
    OFC_REQUIRE(min_area >= 1, "min_area = %d: at least 1", min_area);
    OFC_REQUIRE(max_blobs >= 1, "max_blobs = %d: at least 1", max_blobs);
    if ((int64_t)W * H > INT32_MAX) {
        set_error("frames of %dx%d pixels are not supported (more than 2^31 - 1)", W, H);
        return OFC_EUNSUPPORTED;
    }
    if (npair > BLOB_MAX_PAIRS) {
        set_error("npair = %d: at most %d pairs per call", npair, BLOB_MAX_PAIRS);
        return OFC_EUNSUPPORTED;
    }
    if (max_blobs > BLOB_MAX_BLOBS) {
        set_error("max_blobs = %d: at most %d", max_blobs, BLOB_MAX_BLOBS);
        return OFC_EUNSUPPORTED;
    }
    return OFC_OK;
}

int launch_blob_keys(const float *flow, int W, int H, int npair, bool use_thr, float thr, const LloydState *st, int k,
                     uint32_t select, bool merge, uint8_t *keys, hipStream_t s)
{
    const long long n = (long long)W * H * npair;
    const bool vec = ((uintptr_t)flow & 15) == 0 && ((uintptr_t)keys & 3) == 0;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(vec ? cdiv64(n, 4) : n, BL_THREADS), 8192));
    auto kern = vec ? &k_blob_keys<true> : &k_blob_keys<false>;
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(BL_THREADS), 0, s, reinterpret_cast<const float2 *>(flow), n,
                       use_thr ? 1 : 0, thr * thr, st, k, select, merge ? 1 : 0, keys);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_blob_local(const uint8_t *keys, int W, int H, int npair, int connectivity, int32_t *labels, int *err, hipStream_t s)
{
    const int ntx = cdiv(W, BLOB_TW), nty = cdiv(H, BLOB_TH);
    const dim3 grid((unsigned)ntx * nty, npair);
    if (connectivity == 8) hipLaunchKernelGGL(k_blob_local<8>, grid, dim3(BL_THREADS), 0, s, keys, W, H, ntx, labels, err);
    else hipLaunchKernelGGL(k_blob_local<4>, grid, dim3(BL_THREADS), 0, s, keys, W, H, ntx, labels, err);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_blob_seam(const uint8_t *keys, int W, int H, int npair, int connectivity, int32_t *labels, int *err, hipStream_t s)
{
    const int ntx = cdiv(W, BLOB_TW), nty = cdiv(H, BLOB_TH);
    const int nh = (nty - 1) * W, nseam = nh + (ntx - 1) * H;          // < 2^31 / 16 + 2^31 / 64
    if (nseam == 0) return OFC_OK;
    const dim3 grid(cdiv(nseam, BL_THREADS), npair);
    const unsigned cap = walk_cap(W, H);
    if (connectivity == 8)
        hipLaunchKernelGGL(k_blob_seam<8>, grid, dim3(BL_THREADS), 0, s, keys, W, H, nh, nseam, labels, cap, err);
    else
        hipLaunchKernelGGL(k_blob_seam<4>, grid, dim3(BL_THREADS), 0, s, keys, W, H, nh, nseam, labels, cap, err);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_blob_flatten(int W, int H, int npair, int32_t *labels, int *err, hipStream_t s)
{
    const int P = W * H;
    const dim3 grid((unsigned)cdiv64(P, BL_THREADS * 4), npair);
    const bool vec = P % 4 == 0 && ((uintptr_t)labels & 15) == 0;
    auto kern = vec ? &k_blob_flatten<true> : &k_blob_flatten<false>;
    hipLaunchKernelGGL(kern, grid, dim3(BL_THREADS), 0, s, labels, P, walk_cap(W, H), err);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_blob_area(const int32_t *labels, int W, int H, int npair, int32_t *words, hipStream_t s)
{
    const int P = W * H;
    OFC_HIP(hipMemsetAsync(words, 0, sizeof(int32_t) * (size_t)P * npair, s));
    hipLaunchKernelGGL(k_blob_area, dim3((unsigned)cdiv64(P, BLOB_SHARE), npair), dim3(BL_THREADS), 0, s, labels, P, words);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

int launch_blob_table(const uint8_t *keys, const int32_t *labels, const float *flow, int W, int H, int npair, int min_area,
                      int max_blobs, int32_t *words, int64_t *table, int32_t *found, hipStream_t s)
{
    const int P = W * H;
    OFC_HIP(hipMemsetAsync(words, 0, sizeof(int32_t) * (size_t)P * npair, s));
    OFC_HIP(hipMemsetAsync(found, 0, sizeof(int32_t) * npair, s));
    const dim3 shares((unsigned)cdiv64(P, BLOB_SHARE), npair);
    long long *t = reinterpret_cast<long long *>(table);
    hipLaunchKernelGGL(k_blob_area, shares, dim3(BL_THREADS), 0, s, labels, P, words);
    hipLaunchKernelGGL(k_blob_slots, dim3((unsigned)cdiv64(P, BL_THREADS), npair), dim3(BL_THREADS), 0, s, keys, labels, W, P,
                       min_area, max_blobs, words, t, found);
    if (flow)
        hipLaunchKernelGGL(k_blob_accum<true>, shares, dim3(BL_THREADS), 0, s, labels, words,
                           reinterpret_cast<const float2 *>(flow), W, H, max_blobs, t);
    else
        hipLaunchKernelGGL(k_blob_accum<false>, shares, dim3(BL_THREADS), 0, s, labels, words, (const float2 *)nullptr, W, H,
                           max_blobs, t);
    OFC_HIP(hipGetLastError());
    return OFC_OK;
}

}  // namespace ofc

// blob_links_host.h -- the host half of the blob links (blob_links.hip, blob_links_api.cpp): the layout of a transition's
// table on the device and its way into the table of the definition (include/ofc.h).  Plain C++, no HIP: it also builds
// into a stand-alone program.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ofc {

constexpr int BLOB_LINK_NF = 3;                    // OFC_BLOB_LINK_FIELDS: root_a, root_b, votes
constexpr int BLOB_MAX_LINKS = 65536;
constexpr uint64_t BLOB_LINK_EMPTY = ~0ull;        // no key has bit 63 set: roots are below 2^31
// the transition's counter word: distinct links claimed in its low 30 bits (at most the capacity, 2^17), and
// BLOB_LINK_FULL once a probe sequence went through the whole table without finding room
constexpr int32_t BLOB_LINK_FULL = 1 << 30, BLOB_LINK_COUNT = BLOB_LINK_FULL - 1;

// slots of a transition's table: a power of two, at least 2 * max_links
inline size_t blob_link_capacity(int max_links)
{
    size_t cap = 2;
    while (cap < 2 * (size_t)max_links) cap *= 2;
    return cap;
}

// links_dev: uint64 keys [ntrans][cap] ((root_a << 32) | root_b, or BLOB_LINK_EMPTY), then int32 votes [ntrans][cap]
inline size_t blob_links_bytes(int max_links, int ntrans)
{
    return blob_link_capacity(max_links) * (size_t)ntrans * (sizeof(uint64_t) + sizeof(int32_t));
}

// A transition's slots as the device left them -> its table: rows (root_a, root_b, votes) ascending by (root_a, root_b) in
// out [max_links][3], rows past *n zeroed; more than max_links distinct links: *n = -1 and no row.  Returns false when the
// device reported a full table although no more than max_links links were claimed (which the algorithm excludes).
inline bool blob_order_links(const uint64_t *keys, const int32_t *votes, size_t cap, int32_t counter, int max_links, int64_t *out,
                             int32_t *n)
{
    const int32_t claimed = counter & BLOB_LINK_COUNT;
    memset(out, 0, sizeof(int64_t) * BLOB_LINK_NF * (size_t)max_links);
    if (claimed > max_links) {
        *n = -1;
        return true;
    }
    *n = 0;
    if (counter & BLOB_LINK_FULL) return false;
    std::vector<size_t> idx;
    for (size_t s = 0; s < cap; s++)
        if (keys[s] != BLOB_LINK_EMPTY) idx.push_back(s);
    if (idx.size() != (size_t)claimed) return false;       // the counter counts the claims
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    for (size_t i = 0; i < idx.size(); i++) {
        out[i * BLOB_LINK_NF] = (int64_t)(keys[idx[i]] >> 32);
        out[i * BLOB_LINK_NF + 1] = (int64_t)(keys[idx[i]] & 0xffffffffull);
        out[i * BLOB_LINK_NF + 2] = votes[idx[i]];
    }
    *n = claimed;
    return true;
}

}  // namespace ofc

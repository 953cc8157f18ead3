// A stand-alone driver of csrc/blob_links_host.h for test_blob_links_host.py, built there with the address and
// undefined-behaviour sanitizers.  stdin: max_links counter, then the slots as "key votes" pairs (key as a decimal uint64)
// until the end of input; their number must be the capacity of max_links.  stdout: "ok n", then the max_links rows.
#include "../opticalflowclustering_amd/csrc/blob_links_host.h"

#include <cstdio>

int main()
{
    int max_links = 0;
    long long counter = 0;
    if (scanf("%d %lld", &max_links, &counter) != 2 || max_links < 1 || max_links > ofc::BLOB_MAX_LINKS) return 2;
    std::vector<uint64_t> keys;
    std::vector<int32_t> votes;
    unsigned long long k;
    int v;
    while (scanf("%llu %d", &k, &v) == 2) {
        keys.push_back(k);
        votes.push_back(v);
    }
    const size_t cap = ofc::blob_link_capacity(max_links);
    if (keys.size() != cap) return 3;
    if (ofc::blob_links_bytes(max_links, 3) != 3 * cap * 12) return 4;
    std::vector<int64_t> out((size_t)max_links * ofc::BLOB_LINK_NF, -7);
    int32_t n = -7;
    const bool ok = ofc::blob_order_links(keys.data(), votes.data(), cap, (int32_t)counter, max_links, out.data(), &n);
    printf("%s %d\n", ok ? "ok" : "unsound", n);
    for (int i = 0; i < max_links; i++)
        printf("%lld %lld %lld\n", (long long)out[3 * i], (long long)out[3 * i + 1], (long long)out[3 * i + 2]);
    return 0;
}

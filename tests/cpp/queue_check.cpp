// Checks rtw_queue.h's sharded sample queue on the host.  For each total:
//   - the shards' limits sum to the total;
//   - shard_sample(s, j) over j < shard_limit(s, total) and all s is each id
//     of [0, total) exactly once;
//   - queue_drained is true with every shard at its limit and false with any
//     one shard (of a nonzero limit) one short of it.
// Prints one line per total and "OK (<n> totals)"; exit 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rtw_queue.h"

int main() {
    const uint64_t totals[] = {0,    1,    63,   64,   65,   1023, 1024,          1025,
                               8191, 8192, 8193, 8200, 9216, 9217, 25 * 1024 + 5, 100000};
    int bad = 0, n = 0;
    auto fail = [&](uint64_t total, const char* what, uint64_t a, uint64_t b) {
        if (bad++ < 20) std::printf("total %llu: %s (%llu, %llu)\n", (unsigned long long)total, what,
                                    (unsigned long long)a, (unsigned long long)b);
    };
    for (uint64_t total : totals) {
        ++n;
        uint64_t sum = 0;
        for (int s = 0; s < kQShards; ++s) sum += shard_limit(s, total);
        if (sum != total) fail(total, "limits sum to", sum, total);

        std::vector<uint8_t> seen(total, 0);
        for (int s = 0; s < kQShards; ++s)
            for (uint64_t j = 0; j < shard_limit(s, total); ++j) {
                const uint64_t q = shard_sample(s, j);
                if (q >= total)
                    fail(total, "id out of range: shard, id", (uint64_t)s, q);
                else if (seen[q]++)
                    fail(total, "id handed out twice: shard, id", (uint64_t)s, q);
            }
        for (uint64_t q = 0; q < total; ++q)
            if (!seen[q]) fail(total, "id never handed out", q, 0);

        ctrs_t c{};
        for (int s = 0; s < kQShards; ++s) c.qshard[s].v = shard_limit(s, total);
        if (!queue_drained(c, (uint32_t)total)) fail(total, "not drained at the limits", 0, 0);
        for (int s = 0; s < kQShards; ++s) {
            if (c.qshard[s].v == 0) continue;  // (a shard that owns nothing cannot be short)
            --c.qshard[s].v;
            if (queue_drained(c, (uint32_t)total)) fail(total, "drained with a shard one short: shard", (uint64_t)s, 0);
            ++c.qshard[s].v;
        }
        // a shard past its limit (the reservations overshoot a dry shard) is still drained
        for (int s = 0; s < kQShards; ++s) c.qshard[s].v += 64;
        if (!queue_drained(c, (uint32_t)total)) fail(total, "not drained past the limits", 0, 0);
        std::printf("total %llu: limits sum %llu\n", (unsigned long long)total, (unsigned long long)sum);
    }
    if (bad) {
        std::printf("FAILED (%d)\n", bad);
        return 1;
    }
    std::printf("OK (%d totals)\n", n);
    return 0;
}

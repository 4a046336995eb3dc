// rtw_queue.h — the sample queue of a pass and the counters it lives in: what
// the kernels that take samples (k_regen and the four persistent kernels of
// rtw_kernels.hip) and the host's drain test share.
// Plain C++17 (no HIP header): it compiles under g++ (tests/cpp/queue_check.cpp)
// and under hipcc's host and device passes.
#pragma once
#include <stdint.h>
#include "rtw_div.h"  // RTW_HD

// In the unnamed namespace, beside rtw_kernels.hip's own declarations: ctrs_t
// is a parameter type of the wavefront kernels, so its namespace is part of
// their symbol names.
namespace {

// The sample queue is sharded over kQShards counters to spread the atomics:
// shard s owns the chunks c = s, s + kQShards, ... of kQChunk consecutive
// samples, and its j-th sample is  q = ((j / kQChunk) * kQShards + s) * kQChunk
// + j % kQChunk.
constexpr int kQShards = 8;
constexpr uint32_t kQChunk = 1024;

// Counters hit by many workgroups live on 256-byte lines of their own: all
// words of one line are served by one L2 channel, which serialises them
// (one word saturates at ~88 atomics/us).  Shard k is used by the blocks with
// blockIdx % 8 == k, i.e. by one XCD.
struct alignas(256) ctr_line {
    unsigned long long v;
    unsigned long long pad[31];
};

struct ctrs_t {
    ctr_line qshard[kQShards];  // per-shard count of samples handed out
    ctr_line segments[8];       // world hit queries (live paths intersected)
    unsigned int n;                      // slots in the current pool
    unsigned int n_out;                  // compaction output count
    unsigned int pad[4];
};

RTW_HD uint64_t shard_sample(int s, uint64_t j) {
    return ((j / kQChunk) * kQShards + (uint64_t)s) * kQChunk + j % kQChunk;
}
// number of the pass's `total` samples that shard s owns (its ids 0..limit-1)
RTW_HD uint64_t shard_limit(int s, uint64_t total) {
    const uint64_t full = total / kQChunk, rem = total % kQChunk;
    const uint64_t nfull = full > (uint64_t)s ? (full - (uint64_t)s + kQShards - 1) / kQShards : 0;
    return nfull * kQChunk + ((full % kQShards) == (uint64_t)s ? rem : 0);
}

// true once every queue shard has handed out all of its samples
inline bool queue_drained(const ctrs_t& c, uint32_t total) {
    for (int s = 0; s < kQShards; ++s)
        if (c.qshard[s].v < shard_limit(s, total)) return false;
    return true;
}

}  // namespace

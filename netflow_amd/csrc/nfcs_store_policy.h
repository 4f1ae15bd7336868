// The form of a large long-frame plain update, chosen from the store demand its recent calls observed
// (nfcs_api.hip update_device). Plain C++ with no device or runtime dependency, so a
// stand-alone program can test it (tests/cpp/store_policy_test.cpp).
//
//   deferred  sub-batches of a read pass that writes patch records and a write pass that stores them:
//             the fastest form when most frames need their checksum bytes stored;
//   sparse    one read pass over the whole call that stores the few differing fields inline: no
//             records, no write pass, no sub-batches. The fastest form when hardly any frame needs a
//             store (received traffic, whose checksums are already right).
//
// The read pass counts, over a sample of its workgroups, the packets whose frame still needs a store;
// the next call forwards that count to the host with the counted call's generation. The policy sees
// each observation once, in the order the host reads them. It is a pure function of that history:
//   * a context starts deferred;
//   * it turns sparse only when the two newest observations are both under the threshold;
//   * any newer observation at or over the threshold turns it back;
//   * an observation whose generation is not newer than the last one seen (a late or repeated read)
//     and one that sampled no packet are ignored;
//   * reset() (a call on another stream: concurrent calls share the counters) returns to deferred and
//     ignores every generation up to the one given.
// The form changes speed only: bytes, status bytes and records are the same in both.
#pragma once
#include <cstdint>

namespace nfcs {

enum : int { kStoreFormDeferred = 0, kStoreFormSparse = 1 };

// A call is "low" when fewer than kSparseMaxNum / kSparseMaxDen of its sampled packets needed a store.
// The sweep (profiles/store_policy_sweep.jsonl) found the sparse form faster on both C1 (1M)
// and the 4M shard only when nothing stores: with 1/256 to 1/16 of the packets storing, their few inline
// stores scattered through the read stream cost the 4M shard 2-8% against the deferred form (C1 up to 10%
// when calls follow each other without a gap), although from 1/8 upwards inline stores were no slower
// again. So the largest fraction up to which sparse is never slower is below 1/256, the smallest one
// measured, and the constant is half of that: a context runs sparse only while next to nothing stores.
constexpr uint32_t kSparseMaxNum = 1, kSparseMaxDen = 512;
// Observations under the threshold, newest in a row, needed before a context turns sparse.
constexpr uint32_t kSparseLowRun = 2;

struct StorePolicy {
    int form = kStoreFormDeferred;
    uint32_t last_gen = 0;  // the newest generation seen or skipped (generations start at 1, wrap past 0)
    uint32_t low_run = 0;   // observations under the threshold since the last one at or over it
    // the newest observation seen (sampled 0: none yet)
    uint32_t obs_gen = 0, obs_sampled = 0, obs_storing = 0;

    static bool low(uint32_t sampled, uint32_t storing) {
        return (uint64_t)storing * kSparseMaxDen < (uint64_t)sampled * kSparseMaxNum;
    }
    // Whether generation `gen` is newer than the last one seen (serial-number order, so a wrapped
    // counter keeps working).
    bool newer(uint32_t gen) const { return gen != 0 && (int32_t)(gen - last_gen) > 0; }

    void observe(uint32_t gen, uint32_t sampled, uint32_t storing) {
        if (!newer(gen) || sampled == 0) return;
        last_gen = gen;
        obs_gen = gen;
        obs_sampled = sampled;
        obs_storing = storing < sampled ? storing : sampled;
        if (low(sampled, storing)) {
            if (low_run < kSparseLowRun) ++low_run;
            if (low_run >= kSparseLowRun) form = kStoreFormSparse;
        } else {
            low_run = 0;
            form = kStoreFormDeferred;
        }
    }
    void reset(uint32_t ignore_through) {
        form = kStoreFormDeferred;
        low_run = 0;
        last_gen = ignore_through;
        obs_gen = obs_sampled = obs_storing = 0;
    }
};

}  // namespace nfcs

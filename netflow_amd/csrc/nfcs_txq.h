// nfcs_txq.h — the TX queues' host side: what nfcs_txq_create snapshots of the committed egress ports, the
// host copy of the rings, the sequential walks of nfcs_txq_append_host / nfcs_txq_dequeue_host, and the
// closed form of the dequeue (txq_take, txq_rank) that the kernels compute. Pure C++ (no HIP), so it also
// builds into a stand-alone host program (tests/cpp/txq_compile_main.cpp, run under the host sanitizers).
// nfcs_internal.h includes this file, so the port record, the take and the rank below are the kernels' as
// well: one definition each.
#pragma once

#include <stdint.h>

#include <vector>

#include "nfcs.h"
#include "nfcs_egress.h"

namespace nfcs {

// One port as the kernels read it, 16 bytes. A port without a QoS config is all zero: no queue, no ring.
//   queues     num_queues, 1..NFCS_QOS_MAX_QUEUES (0 without a QoS config)
//   max_depth  max_queue_depth: the capacity of each of the port's rings
//   sched      NFCS_SCHED_*
struct alignas(16) TxqPort {
    uint32_t queues, max_depth, sched, pad;
};
static_assert(sizeof(TxqPort) == 16, "one port is one 16-byte load");
constexpr uint32_t kTxqQ = NFCS_QOS_MAX_QUEUES;

NFCS_EG_HD inline uint32_t txq_cap(const TxqPort& p, uint32_t q) { return q < p.queues ? p.max_depth : 0u; }

// The depths the dequeue works with: min(depth, cap) per queue, so a bad depth cannot reach outside a ring.
// Returns their sum.
NFCS_EG_HD inline uint64_t txq_depths(const TxqPort& p, const uint32_t* depth8, uint32_t D[kTxqQ]) {
    uint64_t sum = 0;
    for (uint32_t q = 0; q < kTxqQ; ++q) {
        const uint32_t cap = txq_cap(p, q);
        D[q] = depth8[q] < cap ? depth8[q] : cap;
        sum += D[q];
    }
    return sum;
}

// c(q): queue q's place in the round that starts behind `last` (select_packet_to_dequeue tests the queues
// (last + 1 + i) % num_queues for i = 0..num_queues-1).
NFCS_EG_HD inline uint32_t txq_rr_place(const TxqPort& p, uint32_t last, uint32_t q) {
    return (q + 2u * p.queues - 1u - last % p.queues) % p.queues;
}

// The TX rank of packet r (r < D[q]) of queue q among the port's queued packets: the number of
// select_packet_to_dequeue calls that come before the one that returns it.
NFCS_EG_HD inline uint64_t txq_rank(const TxqPort& p, uint32_t last, const uint32_t D[kTxqQ], uint32_t q, uint32_t r) {
    uint64_t rank = r;
    if (p.sched == NFCS_SCHED_STRICT_PRIORITY) {
        for (uint32_t o = 0; o < kTxqQ; ++o)
            if (o < q) rank += D[o];
        return rank;
    }
    const uint32_t cq = txq_rr_place(p, last, q);
    for (uint32_t o = 0; o < kTxqQ; ++o) {
        if (o == q || o >= p.queues) continue;
        rank += D[o] < r ? D[o] : r;                                    // its packets of the rounds before r
        if (D[o] > r && txq_rr_place(p, last, o) < cq) rank += 1u;      // served earlier in round r
    }
    return rank;
}

// What G select_packet_to_dequeue calls take from each queue (G <= sum D), and the port's last-serviced
// queue afterwards. Every loop is bounded by a constant: at most 8 distinct depths.
NFCS_EG_HD inline void txq_take(const TxqPort& p, uint32_t last, const uint32_t D[kTxqQ], uint32_t G,
                                uint32_t take[kTxqQ], uint32_t* new_last) {
    *new_last = last;
    for (uint32_t q = 0; q < kTxqQ; ++q) take[q] = 0;
    if (G == 0 || p.queues == 0) return;
    if (p.sched == NFCS_SCHED_STRICT_PRIORITY) {  // the lowest-numbered non-empty queue; last is not touched
        uint32_t left = G;
        for (uint32_t q = 0; q < kTxqQ; ++q) {
            take[q] = D[q] < left ? D[q] : left;
            left -= take[q];
        }
        return;
    }
    // Round-robin: round r serves every queue deeper than r. R = the full rounds within G: the largest R
    // with S(R) = sum min(D, R) <= G; S is linear between consecutive distinct depths.
    uint32_t R = 0;
    uint64_t S = 0;
    for (uint32_t step = 0; step <= kTxqQ; ++step) {
        uint32_t next = 0xFFFFFFFFu, active = 0;
        for (uint32_t q = 0; q < kTxqQ; ++q)
            if (D[q] > R) {
                ++active;
                if (D[q] < next) next = D[q];
            }
        if (!active) break;  // G covers everything queued
        const uint64_t s_next = S + (uint64_t)(next - R) * active;
        if (s_next <= G) {
            R = next;
            S = s_next;
            continue;
        }
        const uint32_t full = (uint32_t)((G - S) / active);
        R += full;
        S += (uint64_t)full * active;
        break;
    }
    const uint32_t rem = (uint32_t)(G - S);  // the packets of the round that G ends in; below its queues' count
    uint64_t total = 0;
    for (uint32_t q = 0; q < kTxqQ; ++q) {
        uint32_t t = D[q] < R ? D[q] : R;
        if (D[q] > R && q < p.queues) {
            const uint32_t cq = txq_rr_place(p, last, q);
            uint32_t before = 0;
            for (uint32_t o = 0; o < kTxqQ; ++o)
                if (o < p.queues && D[o] > R && txq_rr_place(p, last, o) < cq) ++before;
            if (before < rem) ++t;
        }
        take[q] = t;
        total += t;
    }
    for (uint32_t q = 0; q < kTxqQ; ++q)  // the queue of the packet with rank total - 1
        if (take[q] && txq_rank(p, last, D, q, take[q] - 1u) + 1u == total) *new_last = q;
}

// The tx_cap rule: port p wants `want`, the ports before it want W in all (64 bits); it gets the part of
// [W, W + want) below tx_cap, and its segment starts at min(W, tx_cap).
NFCS_EG_HD inline uint32_t txq_grant(uint64_t W, uint32_t want, uint32_t tx_cap, uint32_t* start) {
    const uint64_t a = W < tx_cap ? W : tx_cap, e = W + want < tx_cap ? W + want : tx_cap;
    *start = (uint32_t)a;
    return (uint32_t)(e - a);
}

NFCS_EG_HD inline uint64_t txq_desc_handle(uint32_t off16, uint32_t len) { return off16 | ((uint64_t)len << 32); }

// ---- the host object ---------------------------------------------------------------------------------

struct TxqTables {
    std::vector<TxqPort> port;        // `ports` records
    std::vector<uint64_t> ring_base;  // keys + 1: the exclusive prefix of cap; ring_base[keys] = ring_slots
    uint32_t ports = 0, keys = 0;
    uint64_t ring_slots = 0;
};

struct TxqState {
    std::vector<uint64_t> ring;  // ring_slots handles
    std::vector<uint32_t> head;  // keys, each in [0, cap)
    std::vector<uint8_t> last;   // ports: port_last_serviced_queue_
};

inline void txq_compile(const EgressTables& e, TxqTables& t) {
    t = TxqTables{};
    t.ports = e.ports;
    t.keys = e.keys;
    t.port.assign(t.ports, TxqPort{0, 0, NFCS_SCHED_STRICT_PRIORITY, 0});
    t.ring_base.assign((size_t)t.keys + 1u, 0);
    for (uint32_t p = 0; p < t.ports; ++p) {
        const EgressRec& r = e.recs[p];
        if (r.flags & kEgQos) {
            t.port[p].queues = r.queues;
            t.port[p].max_depth = r.max_depth;
        }
        for (uint32_t q = 0; q < kTxqQ; ++q) {
            t.ring_base[p * kTxqQ + q] = t.ring_slots;
            t.ring_slots += txq_cap(t.port[p], q);
        }
    }
    t.ring_base[t.keys] = t.ring_slots;
}

inline void txq_state_init(const TxqTables& t, TxqState& s) {
    s.ring.assign((size_t)t.ring_slots, 0);
    s.head.assign(t.keys, 0);
    s.last.assign(t.ports, 0);
}

// enqueue_packet's emplace_back for the burst (nfcs.h nfcs_txq_append_host). Read-only on head and depth.
inline void txq_append(const TxqTables& t, TxqState& s, const uint32_t* order, const uint32_t* key_start,
                       const uint32_t* depth, const uint64_t* handle, const nfcs_desc* desc, uint32_t n) {
    for (uint32_t k = 0; k < t.keys; ++k) {
        const uint32_t b = key_start[k], e = key_start[k + 1];
        if (e <= b || e > n) continue;
        const uint32_t cnt = e - b, cap = txq_cap(t.port[k / kTxqQ], k % kTxqQ);
        if (cap == 0 || depth[k] < cnt || depth[k] > cap) continue;  // inconsistent input: nothing for this key
        const uint64_t first = (uint64_t)s.head[k] + (depth[k] - cnt);
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t i = order[b + j];
            if (i >= n) continue;
            const uint64_t pos = (first + j) % cap;
            s.ring[(size_t)(t.ring_base[k] + pos)] = handle ? handle[i] : txq_desc_handle(desc[i].off16, desc[i].len);
        }
    }
}

// select_packet_to_dequeue on the port's clamped depths D: the queue it takes from, or kTxqQ for nullopt.
// Updates D and last as the reference does.
inline uint32_t txq_select(const TxqPort& p, uint32_t D[kTxqQ], uint8_t* last) {
    if (p.queues == 0) return kTxqQ;
    if (p.sched == NFCS_SCHED_STRICT_PRIORITY) {
        for (uint32_t i = 0; i < p.queues; ++i)
            if (D[i]) {
                --D[i];
                return i;
            }
        return kTxqQ;
    }
    for (uint32_t i = 0; i < p.queues; ++i) {
        const uint32_t q = (*last + 1u + i) % p.queues;
        if (D[q]) {
            --D[q];
            *last = (uint8_t)q;
            return q;
        }
    }
    return kTxqQ;
}

// The sequential definition of the dequeue (nfcs.h nfcs_txq_dequeue_host): the literal walk.
inline void txq_dequeue_walk(const TxqTables& t, TxqState& s, const uint32_t* budget, uint32_t budget_all,
                             uint32_t* depth, uint64_t* tx, uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start,
                             uint32_t* dequeued) {
    uint32_t written = 0;
    for (uint32_t p = 0; p < t.ports; ++p) {
        const TxqPort& pr = t.port[p];
        tx_start[p] = written;
        uint32_t D[kTxqQ], taken[kTxqQ] = {0};
        txq_depths(pr, depth + (size_t)p * kTxqQ, D);
        const uint32_t b = budget ? budget[p] : budget_all;
        for (uint32_t c = 0; c < b && written < tx_cap; ++c) {
            const uint32_t q = txq_select(pr, D, &s.last[p]);
            if (q == kTxqQ) break;
            const uint32_t k = p * kTxqQ + q;
            tx[written] = s.ring[(size_t)(t.ring_base[k] + ((uint64_t)s.head[k] + taken[q]) % pr.max_depth)];
            if (tx_queue) tx_queue[written] = (uint8_t)q;
            ++taken[q];
            ++written;
        }
        for (uint32_t q = 0; q < kTxqQ; ++q) {
            const uint32_t k = p * kTxqQ + q;
            if (dequeued) dequeued[k] = taken[q];
            if (!taken[q]) continue;
            depth[k] -= taken[q];
            s.head[k] = (uint32_t)(((uint64_t)s.head[k] + taken[q]) % pr.max_depth);
        }
    }
    tx_start[t.ports] = written;
}

// The same dequeue by the closed form, step for step what the three kernels do (plan, gather, commit). The
// stand-alone host program holds it to the walk.
inline void txq_dequeue_closed(const TxqTables& t, TxqState& s, const uint32_t* budget, uint32_t budget_all,
                               uint32_t* depth, uint64_t* tx, uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start,
                               uint32_t* dequeued) {
    uint64_t W = 0;
    for (uint32_t p = 0; p < t.ports; ++p) {
        const TxqPort& pr = t.port[p];
        uint32_t D[kTxqQ], take[kTxqQ], new_last, start;
        const uint64_t sum = txq_depths(pr, depth + (size_t)p * kTxqQ, D);
        const uint32_t b = budget ? budget[p] : budget_all;
        const uint32_t want = (uint32_t)(sum < b ? sum : b);
        const uint32_t G = txq_grant(W, want, tx_cap, &start);
        W += want;
        tx_start[p] = start;
        txq_take(pr, s.last[p], D, G, take, &new_last);
        for (uint32_t q = 0; q < kTxqQ; ++q) {
            const uint32_t k = p * kTxqQ + q;
            for (uint32_t r = 0; r < take[q]; ++r) {
                const uint64_t e = start + txq_rank(pr, s.last[p], D, q, r);
                tx[e] = s.ring[(size_t)(t.ring_base[k] + ((uint64_t)s.head[k] + r) % pr.max_depth)];
                if (tx_queue) tx_queue[e] = (uint8_t)q;
            }
            if (dequeued) dequeued[k] = take[q];
            if (!take[q]) continue;
            depth[k] -= take[q];
            s.head[k] = (uint32_t)(((uint64_t)s.head[k] + take[q]) % pr.max_depth);
        }
        s.last[p] = (uint8_t)new_last;
    }
    tx_start[t.ports] = (uint32_t)(W < tx_cap ? W : tx_cap);
}

}  // namespace nfcs

// txq_compile_main.cpp — the TX queues' host code (netflow_amd/csrc/nfcs_txq.h: the tables, the append,
// the literal dequeue walk and the closed form the kernels compute) as a stand-alone program with its own
// main: no HIP, nothing loaded into Python. tests/test_txq.py compiles it with the host sanitizers and runs
// it. The rings and every array sit in heap blocks of their exact sizes, so an access past one is reported.
// Two copies of the state are driven in lockstep, one by the walk and one by the closed form, and both are
// held to a direct restatement with one std::deque per queue; inconsistent inputs are fed in as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "nfcs_txq.h"

namespace {

uint64_t g_s = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_s ^= g_s << 13;
    g_s ^= g_s >> 7;
    g_s ^= g_s << 17;
    return (uint32_t)(g_s >> 32);
}

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

}  // namespace

int main() {
    const uint32_t Q = NFCS_QOS_MAX_QUEUES;
    nfcs::EgressInputs in;
    const uint32_t kPorts = 23;
    in.ports.resize(kPorts);
    for (uint32_t p = 0; p < kPorts; ++p) {
        if (p % 7 == 3) continue;  // never set
        nfcs_egress_port& e = in.ports[p].port;
        in.ports[p].set = true;
        e.port_id = p;
        e.has_qos = p % 6 != 1;
        e.num_queues = (uint8_t)(p % 9);  // 0..8
        const uint32_t depths[] = {0, 1, 2, 5, 7};
        e.max_queue_depth = depths[p % 5];
    }
    nfcs::EgressTables et;
    nfcs::egress_compile(in, et);
    nfcs::TxqTables t;
    nfcs::txq_compile(et, t);
    CHECK(t.ports == kPorts && t.keys == kPorts * Q && t.ring_base.size() == t.keys + 1u);
    uint64_t slots = 0;
    for (uint32_t p = 0; p < kPorts; ++p) {
        t.port[p].sched = p % 3;
        slots += (uint64_t)t.port[p].queues * t.port[p].max_depth;
    }
    CHECK(slots == t.ring_slots && t.ring_base[t.keys] == slots);
    nfcs::TxqState walk, closed;
    nfcs::txq_state_init(t, walk);
    nfcs::txq_state_init(t, closed);
    CHECK(walk.ring.size() == slots);

    std::vector<std::deque<uint64_t>> model(t.keys);
    std::vector<uint8_t> model_last(kPorts, 0);
    std::vector<uint32_t> depth_w(t.keys, 0), depth_c(t.keys, 0);
    uint64_t next_handle = 1;
    for (uint32_t tick = 0; tick < 60; ++tick) {
        // a burst through the egress enqueue, then the append on both copies
        const uint32_t n = rnd() % 400;
        std::vector<uint32_t> port(n), order(n), key_start(t.keys + 1u), dropped(t.keys);
        std::vector<uint8_t> queue(n), result(n);
        std::vector<uint64_t> handle(n);
        std::vector<nfcs_desc> desc(n);
        for (uint32_t i = 0; i < n; ++i) {
            port[i] = rnd() % (kPorts + 1u);
            queue[i] = (uint8_t)(rnd() % Q);
            handle[i] = next_handle++;
            desc[i].off16 = (uint32_t)handle[i];
            desc[i].len = (uint32_t)(handle[i] >> 32);
        }
        std::vector<uint32_t> d0 = depth_w;
        nfcs::egress_enqueue(et, port.data(), queue.data(), n, depth_w.data(), result.data(), order.data(),
                             key_start.data(), dropped.data());
        depth_c = depth_w;
        std::vector<uint32_t> used(order.begin(), order.begin() + key_start[t.keys]);  // exactly the entries written
        const bool by_desc = tick % 2;
        nfcs::txq_append(t, walk, used.data(), key_start.data(), depth_w.data(), by_desc ? nullptr : handle.data(),
                         by_desc ? desc.data() : nullptr, n);
        nfcs::txq_append(t, closed, used.data(), key_start.data(), depth_c.data(), by_desc ? nullptr : handle.data(),
                         by_desc ? desc.data() : nullptr, n);
        for (uint32_t i = 0; i < n; ++i)
            if (result[i] == NFCS_EQ_ENQUEUED) model[port[i] * Q + queue[i]].push_back(handle[i]);
        for (uint32_t k = 0; k < t.keys; ++k) CHECK(model[k].size() == depth_w[k]);
        CHECK(walk.ring == closed.ring);

        // the dequeue: the walk on one copy, the closed form on the other, the deques as the judge
        std::vector<uint32_t> budget(kPorts);
        const uint32_t kinds[] = {0, 1, 2, 3, 5, 9, 100000, 0xFFFFFFFFu};
        for (uint32_t p = 0; p < kPorts; ++p) budget[p] = kinds[rnd() % 8];
        const uint32_t caps[] = {0, 7, 64, 5000};
        const uint32_t tx_cap = caps[rnd() % 4];
        const bool all = tick % 3 == 0;
        std::vector<uint64_t> tx_w(tx_cap, ~0ull), tx_c(tx_cap, ~0ull);
        std::vector<uint8_t> q_w(tx_cap, 0xEE), q_c(tx_cap, 0xEE);
        std::vector<uint32_t> s_w(kPorts + 1u), s_c(kPorts + 1u), n_w(t.keys), n_c(t.keys);
        nfcs::txq_dequeue_walk(t, walk, all ? nullptr : budget.data(), budget[0], depth_w.data(), tx_w.data(), tx_cap,
                               q_w.data(), s_w.data(), n_w.data());
        nfcs::txq_dequeue_closed(t, closed, all ? nullptr : budget.data(), budget[0], depth_c.data(), tx_c.data(), tx_cap,
                                 q_c.data(), s_c.data(), n_c.data());
        CHECK(tx_w == tx_c && q_w == q_c && s_w == s_c && n_w == n_c && depth_w == depth_c);
        CHECK(walk.head == closed.head && walk.last == closed.last);
        uint32_t written = 0;
        for (uint32_t p = 0; p < kPorts; ++p) {
            CHECK(s_w[p] == written);
            const nfcs::TxqPort& pr = t.port[p];
            const uint32_t b = all ? budget[0] : budget[p];
            for (uint32_t c = 0; c < b && written < tx_cap; ++c) {
                uint32_t got = Q;
                for (uint32_t i = 0; i < pr.queues && got == Q; ++i) {
                    const uint32_t q = pr.sched == NFCS_SCHED_STRICT_PRIORITY ? i : (model_last[p] + 1u + i) % pr.queues;
                    if (!model[p * Q + q].empty()) got = q;
                }
                if (got == Q) break;
                if (pr.sched != NFCS_SCHED_STRICT_PRIORITY) model_last[p] = (uint8_t)got;
                CHECK(tx_w[written] == model[p * Q + got].front() && q_w[written] == got);
                model[p * Q + got].pop_front();
                ++written;
            }
        }
        CHECK(s_w[kPorts] == written);
        for (uint32_t e = written; e < tx_cap; ++e) CHECK(tx_w[e] == ~0ull && q_w[e] == 0xEE);  // left alone
        for (uint32_t k = 0; k < t.keys; ++k) {
            CHECK(model[k].size() == depth_w[k]);
            const uint32_t cap = nfcs::txq_cap(t.port[k / Q], k % Q);
            CHECK(cap == 0 ? walk.head[k] == 0 : walk.head[k] < cap);
        }
        CHECK(walk.last == model_last);
    }

    // inconsistent input: depths above the cap, below cnt, order entries >= n, ranges past n, queues that do
    // not exist. Nothing may be stored or read outside the rings (the sanitizer is the judge), and a key
    // with bad counters appends nothing.
    for (uint32_t round = 0; round < 200; ++round) {
        const uint32_t n = 1u + rnd() % 50;
        std::vector<uint32_t> order(n), key_start(t.keys + 1u), depth(t.keys);
        std::vector<uint64_t> handle(n, 0xABCDull);
        uint32_t run = 0;
        for (uint32_t k = 0; k < t.keys; ++k) {
            key_start[k] = run;
            if (rnd() % 8 == 0) run += rnd() % 5;
            depth[k] = rnd() % 3 == 0 ? rnd() : rnd() % 9;
        }
        key_start[t.keys] = run;  // may exceed n
        for (uint32_t i = 0; i < n; ++i) order[i] = rnd() % 4 == 0 ? rnd() : rnd() % n;
        std::vector<uint32_t> ord(order);
        ord.resize(run > n ? run : n, 0xFFFFFFFFu);
        const std::vector<uint64_t> ring_before = walk.ring;
        nfcs::txq_append(t, walk, ord.data(), key_start.data(), depth.data(), handle.data(), nullptr, n);
        for (uint32_t k = 0; k < t.keys; ++k) {
            const uint32_t cap = nfcs::txq_cap(t.port[k / Q], k % Q), cnt = key_start[k + 1] - key_start[k];
            if (cap && depth[k] >= cnt && depth[k] <= cap && key_start[k + 1] <= n) continue;
            for (uint64_t s = t.ring_base[k]; s < t.ring_base[k + 1]; ++s) CHECK(walk.ring[s] == ring_before[s]);
        }
        closed.ring = walk.ring;
        closed.head = walk.head;
        closed.last = walk.last;
        const uint32_t tx_cap = rnd() % 300;
        std::vector<uint64_t> tx_w(tx_cap), tx_c(tx_cap);
        std::vector<uint32_t> s_w(kPorts + 1u), s_c(kPorts + 1u), depth_c(depth);
        const uint32_t budget_all = rnd() % 40;  // depths above the cap are read as the cap by both forms
        nfcs::txq_dequeue_walk(t, walk, nullptr, budget_all, depth.data(), tx_w.data(), tx_cap, nullptr, s_w.data(), nullptr);
        nfcs::txq_dequeue_closed(t, closed, nullptr, budget_all, depth_c.data(), tx_c.data(), tx_cap, nullptr, s_c.data(),
                                 nullptr);
        CHECK(s_w[kPorts] <= tx_cap && s_w == s_c && depth == depth_c);
        tx_w.resize(s_w[kPorts]);
        tx_c.resize(s_w[kPorts]);
        CHECK(tx_w == tx_c && walk.head == closed.head && walk.last == closed.last);
    }
    printf("txq compile OK: %u ports, %llu ring slots\n", kPorts, (unsigned long long)slots);
    return 0;
}

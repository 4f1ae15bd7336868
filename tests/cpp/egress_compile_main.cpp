// egress_compile_main.cpp — the egress stage's host code (netflow_amd/csrc/nfcs_egress.h: the compile
// step, the one-frame plan, the sequential enqueue) as a stand-alone program with its own main: no HIP,
// nothing loaded into Python. tests/test_egress.py compiles it with the host sanitizers and runs it. Every
// frame sits in a heap block of exactly its length, so a read past a frame's end is reported; the results
// are checked against a direct restatement with one std::deque per queue.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <vector>

#include "nfcs_egress.h"

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

bool tagged(const std::vector<uint8_t>& f) { return f.size() >= 18 && f[12] == 0x81 && f[13] == 0x00; }

}  // namespace

int main() {
    nfcs::EgressInputs in;
    const uint32_t kPorts = 40;
    in.ports.resize(kPorts);
    for (uint32_t p = 0; p < kPorts; ++p) {
        if (p % 7 == 3) continue;  // never set
        nfcs_egress_port& e = in.ports[p].port;
        in.ports[p].set = true;
        e.port_id = p;
        e.has_vlan_config = p % 5 != 0;
        e.type = (uint8_t)(p % 3);
        e.tag_native = (p / 3) % 2;
        e.has_qos = p % 6 != 1;
        e.native_vlan = (uint16_t)(p % 4 == 0 ? 10 : 20);
        e.num_queues = (uint8_t)(p % 9);  // 0..8
        e.max_queue_depth = p % 4 == 2 ? 0 : 1 + p % 11;
    }
    nfcs::EgressTables t;
    nfcs::egress_compile(in, t);
    CHECK(t.ports == kPorts && t.keys == kPorts * NFCS_QOS_MAX_QUEUES && t.recs.size() == kPorts);

    // frames in heap blocks of their exact length
    const uint32_t n = 6000;
    const uint32_t lens[] = {0, 1, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 64};
    std::vector<std::unique_ptr<uint8_t[]>> blocks(n);
    std::vector<std::vector<uint8_t>> frames(n);
    std::vector<uint32_t> port(n);
    std::vector<uint8_t> queue(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = lens[rnd() % (sizeof(lens) / sizeof(lens[0]))];
        std::vector<uint8_t>& f = frames[i];
        f.resize(len);
        for (uint8_t& b : f) b = (uint8_t)rnd();
        const uint32_t kind = rnd() % 4;
        auto put = [&](uint32_t o, uint8_t v) { if (o < len) f[o] = v; };
        if (kind >= 1) {
            const uint32_t vid = rnd() % 2 ? 10 : 20;
            put(12, 0x81), put(13, 0x00), put(14, (uint8_t)((rnd() % 8) << 5 | (vid >> 8))), put(15, (uint8_t)vid);
        }
        if (kind >= 2) put(16, 0x81), put(17, 0x00);
        blocks[i].reset(len ? new uint8_t[len] : nullptr);
        if (len) memcpy(blocks[i].get(), f.data(), len);
        port[i] = rnd() % 16 == 0 ? NFCS_IF_NONE : rnd() % (kPorts + 3);
    }

    // the plan against a restatement that edits a copy of the frame
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t op = 77, q = 77;
        nfcs::egress_plan(t, port[i], blocks[i].get(), (uint32_t)frames[i].size(), &op, &q);
        queue[i] = (uint8_t)q;
        if (port[i] == NFCS_IF_NONE) {
            CHECK(op == NFCS_VLAN_NOP && q == NFCS_QUEUE_NONE);
            continue;
        }
        const bool set = port[i] < kPorts && in.ports[port[i]].set;
        const nfcs_egress_port e = set ? in.ports[port[i]].port : nfcs_egress_port{};
        std::vector<uint8_t> f = frames[i];
        bool pop = false;
        if (e.has_vlan_config && tagged(f)) {
            const uint32_t vid = (((uint32_t)f[14] << 8) | f[15]) & 0x0FFFu;
            pop = vid == e.native_vlan && (e.type == 0 || !e.tag_native);
        }
        if (pop) f.erase(f.begin() + 12, f.begin() + 16);
        uint32_t want = 0;
        if (e.has_qos) {
            const uint32_t nq = e.num_queues ? e.num_queues : 1;
            if (tagged(f)) {
                const uint32_t pcp = f[14] >> 5;
                want = nq == 4 ? (pcp >= 6 ? 0 : pcp >= 4 ? 1 : pcp >= 2 ? 2 : 3) : (uint32_t)(((7 - pcp) * nq) / 8.0);
                if (want >= nq) want = nq - 1;
            } else {
                want = nq - 1;
            }
        }
        CHECK(op == (pop ? NFCS_VLAN_POP : NFCS_VLAN_NOP));
        CHECK(q == want);
        if (rnd() % 32 == 0) queue[i] = (uint8_t)(rnd() % 10);  // some bad queues for the enqueue
    }

    // the enqueue, two bursts chained on one depth array, against deques
    std::vector<uint32_t> depth(t.keys);
    for (uint32_t& d : depth) d = rnd() % 14;  // some at, some above the cap
    std::vector<uint32_t> model_depth = depth;
    for (uint32_t burst = 0; burst < 2; ++burst) {
        const uint32_t b0 = burst * (n / 2), bn = n / 2;
        std::vector<uint8_t> result(bn, 0xEE);
        std::vector<uint32_t> order(bn, 0xEEEEEEEEu), key_start(t.keys + 1, 0xEEEEEEEEu), dropped(t.keys, 0xEEEEEEEEu);
        nfcs::egress_enqueue(t, port.data() + b0, queue.data() + b0, bn, depth.data(), result.data(), order.data(),
                             key_start.data(), dropped.data());
        std::map<uint32_t, std::deque<uint32_t>> qs;
        std::vector<uint32_t> want_dropped(t.keys, 0);
        for (uint32_t i = 0; i < bn; ++i) {
            const uint32_t p = port[b0 + i], q = queue[b0 + i];
            uint32_t want;
            const bool set = p < kPorts && in.ports[p].set;
            if (p == NFCS_IF_NONE) want = NFCS_EQ_SKIP;
            else if (!set || !in.ports[p].port.has_qos) want = NFCS_EQ_DROP_NO_CONFIG;
            else {
                const nfcs_egress_port& e = in.ports[p].port;
                const uint32_t nq = e.num_queues ? e.num_queues : 1, cap = e.max_queue_depth ? e.max_queue_depth : 1;
                const uint32_t k = p * NFCS_QOS_MAX_QUEUES + q;
                if (q >= nq) want = NFCS_EQ_BAD_QUEUE;
                else if (model_depth[k] >= cap) want = NFCS_EQ_DROP_FULL, ++want_dropped[k];
                else want = NFCS_EQ_ENQUEUED, qs[k].push_back(i), ++model_depth[k];
            }
            CHECK(result[i] == want);
        }
        uint32_t at = 0;
        for (uint32_t k = 0; k < t.keys; ++k) {
            CHECK(key_start[k] == at);
            for (uint32_t i : qs[k]) CHECK(order[at++] == i);
            CHECK(dropped[k] == want_dropped[k]);
            CHECK(depth[k] == model_depth[k]);
        }
        CHECK(key_start[t.keys] == at);
        for (uint32_t i = at; i < bn; ++i) CHECK(order[i] == 0xEEEEEEEEu);
    }

    // an empty table and an empty burst
    nfcs::EgressTables none;
    nfcs::egress_compile(nfcs::EgressInputs{}, none);
    uint32_t ks[1] = {5}, op = 0, q = 0;
    nfcs::egress_enqueue(none, nullptr, nullptr, 0, nullptr, nullptr, nullptr, ks, nullptr);
    CHECK(ks[0] == 0);
    nfcs::egress_plan(none, 3, nullptr, 0, &op, &q);
    CHECK(op == NFCS_VLAN_NOP && q == 0);
    printf("egress compile OK: %u ports, %u keys, %u frames\n", t.ports, t.keys, n);
    return 0;
}

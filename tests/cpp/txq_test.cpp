// txq_test.cpp — the C++ host API's TX queues (include/netflow_amd/packet.hpp): egress ports built by
// make_egress_from and schedulers set by set_schedulers_from over mirror types with the reference's member
// names (a QosConfig that does have `scheduler`), ChecksumEngine::make_txq, then per tick
// egress_plan_batch -> egress_enqueue_batch -> txq_append_batch -> txq_dequeue_batch over netflow_amd::Packet
// objects. The handle of a packet is its sequence number over all ticks. Driven by tests/test_gpu_txq_cpp.py.
//
// stdin, one record per line (numbers decimal): "P port_id has_qos num_queues scheduler max_queue_depth",
// then per tick "F egress_port frame(hex)" for each frame and "B budget[0] .. budget[num_ports-1]", which
// ends the tick.
// stdout, per tick: "S tx_start[0] .. tx_start[ports]", "X handles", "Q the queue of each handle",
// "N dequeued[0] .. dequeued[keys-1]", "Z depth[0] .. depth[keys-1]".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <optional>
#include <sstream>
#include <string>
#include <vector>

#include "netflow_amd/packet.hpp"

namespace {

std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return v;
}

// mirror types: the member names make_egress_from and set_schedulers_from read of VlanManager and QosManager
enum class PortType { ACCESS, TRUNK, HYBRID };
enum class SchedulerType { STRICT_PRIORITY, WEIGHTED_ROUND_ROBIN, DEFICIT_ROUND_ROBIN };
struct PortConfig { PortType type = PortType::ACCESS; uint16_t native_vlan = 1; bool tag_native = false; };
struct QosConfig {
    uint8_t num_queues = 4;
    SchedulerType scheduler = SchedulerType::STRICT_PRIORITY;
    uint32_t max_queue_depth = 1000;
};
struct Vlans {
    std::optional<PortConfig> get_port_config(uint32_t) const { return std::nullopt; }
};
struct Qos {
    std::map<uint32_t, QosConfig> m;
    std::optional<QosConfig> get_port_qos_config(uint32_t p) const {
        auto it = m.find(p);
        return it == m.end() ? std::nullopt : std::optional<QosConfig>(it->second);
    }
};

template <class T>
void print_row(const char* tag, const std::vector<T>& v, size_t n) {
    std::printf("%s", tag);
    for (size_t i = 0; i < n; ++i) std::printf(" %llu", (unsigned long long)v[i]);
    std::printf("\n");
}

#define MUST(call)                                                              \
    do {                                                                        \
        const int rc_ = (call);                                                 \
        if (rc_) {                                                              \
            std::fprintf(stderr, "%s:%d: %s rc=%d\n", __FILE__, __LINE__, #call, rc_); \
            return 2;                                                           \
        }                                                                       \
    } while (0)

}  // namespace

int main() {
    Vlans vlans;
    Qos qos;
    uint32_t num_ports = 0;
    nfcs_egress* eg = nullptr;
    nfcs_txq* txq = nullptr;
    uint32_t ports = 0, keys = 0;
    std::vector<uint32_t> depth;
    netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
    std::vector<uint32_t> port;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    uint64_t next_seq = 0;
    uint32_t tick = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "P") {
            uint32_t id = 0, has_qos = 0, nq = 0, sched = 0, d = 0;
            in >> id >> has_qos >> nq >> sched >> d;
            if (has_qos) qos.m[id] = QosConfig{(uint8_t)nq, static_cast<SchedulerType>(sched), d};
            if (id + 1 > num_ports) num_ports = id + 1;
        } else if (kind == "F") {
            uint32_t p = 0;
            in >> p >> h;
            port.push_back(p);
            const std::vector<uint8_t> f = unhex(h);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        } else if (kind == "B") {
            if (!txq) {  // the first tick: the tables, the upload, the queues and their schedulers
                MUST(netflow_amd::make_egress_from(vlans, qos, num_ports, &eg));
                if (eng.make_txq(nullptr, &txq) != NFCS_EINVAL) return 3;
                MUST(eng.upload_egress(eg));
                MUST(eng.make_txq(eg, &txq));
                MUST(netflow_amd::set_schedulers_from(qos, num_ports, txq));
                uint64_t slots = 0;
                MUST(nfcs_txq_info(txq, &ports, &keys, &slots));
                if (ports != num_ports || keys != ports * NFCS_QOS_MAX_QUEUES || slots == 0) return 3;
                depth.assign(keys, 0);
            }
            std::vector<uint32_t> budget;
            for (uint32_t b = 0; in >> b;) budget.push_back(b);
            if (budget.size() != ports) return 2;
            std::vector<netflow_amd::Packet*> raw;
            for (auto& p : pkts) raw.push_back(p.get());
            const size_t n = raw.size();
            std::vector<uint32_t> ops(n), order(n), key_start(keys + 1);
            std::vector<uint8_t> queue(n), result(n);
            std::vector<uint64_t> handle(n);
            for (size_t i = 0; i < n; ++i) handle[i] = next_seq++;
            MUST(eng.egress_plan_batch(raw.data(), n, eg, port.data(), ops.data(), queue.data()));
            MUST(eng.egress_enqueue_batch(eg, port.data(), queue.data(), n, depth.data(), result.data(), order.data(),
                                          key_start.data()));
            const uint32_t tx_cap = 4096;
            std::vector<uint64_t> tx(tx_cap, ~0ull);
            std::vector<uint8_t> tx_queue(tx_cap, 0xEE);
            std::vector<uint32_t> tx_start(ports + 1), dequeued(keys);
            if (tick % 2) {  // the free functions on the process-wide engine
                MUST(netflow_amd::txq_append_batch(txq, order.data(), key_start.data(), depth.data(), handle.data(), n));
                MUST(netflow_amd::txq_dequeue_batch(txq, budget.data(), 0, depth.data(), tx.data(), tx_cap, tx_queue.data(),
                                                    tx_start.data(), dequeued.data()));
            } else {
                MUST(eng.txq_append_batch(txq, order.data(), key_start.data(), depth.data(), handle.data(), n));
                MUST(eng.txq_dequeue_batch(txq, budget.data(), 0, depth.data(), tx.data(), tx_cap, tx_queue.data(),
                                           tx_start.data(), dequeued.data()));
            }
            const uint32_t total = tx_start[ports];
            for (uint32_t e = total; e < tx_cap; ++e)
                if (tx[e] != ~0ull || tx_queue[e] != 0xEE) return 4;  // entries past the total are left alone
            print_row("S", tx_start, ports + 1);
            print_row("X", tx, total);
            print_row("Q", tx_queue, total);
            print_row("N", dequeued, keys);
            print_row("Z", depth, keys);
            port.clear();
            pkts.clear();
            bufs.clear();
            ++tick;
        }
    }
    if (txq) nfcs_txq_destroy(txq);
    if (eg) nfcs_egress_destroy(eg);
    return 0;
}

// egress_test.cpp — the C++ host API's egress path (include/netflow_amd/packet.hpp): egress ports built by
// make_egress_from over mirror types with the reference's member names, ChecksumEngine::upload_egress, then
// egress_plan_batch -> vlan_batch(ops) -> egress_enqueue_batch over netflow_amd::Packet objects. Driven by
// tests/test_gpu_egress_cpp.py.
//
// stdin, one record per line: "P port(hex of one 16-byte nfcs_egress_port)", "D key depth" (a queue's depth
// before the burst; the others are 0), "F egress_port frame(hex)" (numbers decimal).
// stdout: per frame "F op queue result frame_after(hex)", then "K key_start[0] .. key_start[keys]",
// "O order[0] ..", "X key_dropped[0] ..", "Z depth[0] ..".
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

// mirror types: the member names make_egress_from reads of VlanManager and QosManager
enum class PortType { ACCESS, TRUNK, HYBRID };
struct PortConfig { PortType type = PortType::ACCESS; uint16_t native_vlan = 1; bool tag_native = false; };
struct QosConfig { uint8_t num_queues = 4; uint32_t max_queue_depth = 1000; };
struct Vlans {
    std::map<uint32_t, PortConfig> m;
    std::optional<PortConfig> get_port_config(uint32_t p) const {
        auto it = m.find(p);
        return it == m.end() ? std::nullopt : std::optional<PortConfig>(it->second);
    }
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
    for (size_t i = 0; i < n; ++i) std::printf(" %u", (unsigned)v[i]);
    std::printf("\n");
}

}  // namespace

int main() {
    Vlans vlans;
    Qos qos;
    uint32_t num_ports = 0;
    std::map<uint32_t, uint32_t> depth_in;
    std::vector<uint32_t> port;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "P") {
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            if (b.size() != sizeof(nfcs_egress_port)) return 2;
            nfcs_egress_port p;
            std::memcpy(&p, b.data(), sizeof p);
            if (p.has_vlan_config) vlans.m[p.port_id] = PortConfig{static_cast<PortType>(p.type), p.native_vlan, p.tag_native != 0};
            if (p.has_qos) qos.m[p.port_id] = QosConfig{p.num_queues, p.max_queue_depth};
            if (p.port_id + 1 > num_ports) num_ports = p.port_id + 1;
        } else if (kind == "D") {
            uint32_t k = 0, d = 0;
            in >> k >> d;
            depth_in[k] = d;
        } else if (kind == "F") {
            uint32_t p = 0;
            in >> p >> h;
            port.push_back(p);
            const std::vector<uint8_t> f = unhex(h);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        }
    }
    nfcs_egress* eg = nullptr;
    int rc = netflow_amd::make_egress_from(vlans, qos, num_ports, &eg);
    if (rc || !eg) { std::fprintf(stderr, "make_egress_from rc=%d\n", rc); return 2; }
    uint32_t ports = 0, keys = 0;
    if (nfcs_egress_keys(eg, &ports, &keys) || ports != num_ports || keys != ports * NFCS_QOS_MAX_QUEUES) return 2;

    std::vector<netflow_amd::Packet*> raw;
    for (auto& p : pkts) raw.push_back(p.get());
    const size_t n = raw.size();
    std::vector<uint32_t> ops(n, 0xEEEEEEEEu), order(n, 0xEEEEEEEEu), key_start(keys + 1, 0xEEEEEEEEu), dropped(keys, 0xEEEEEEEEu);
    std::vector<uint32_t> depth(keys, 0);
    for (const auto& kd : depth_in)
        if (kd.first < keys) depth[kd.first] = kd.second;
    std::vector<uint8_t> queue(n, 0xEE), result(n, 0xEE);
    netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
    // before the upload the plan is an argument error, not a launch
    if (eng.egress_plan_batch(raw.data(), n, eg, port.data(), ops.data(), queue.data()) != NFCS_EINVAL) {
        std::fprintf(stderr, "no EINVAL\n");
        return 3;
    }
    if ((rc = eng.upload_egress(eg))) { std::fprintf(stderr, "upload rc=%d\n", rc); return 2; }
    rc = eng.egress_plan_batch(raw.data(), n, eg, port.data(), ops.data(), queue.data());
    if (!rc) rc = eng.vlan_batch(raw.data(), ops.data(), n);
    // the free function on the process-wide engine
    if (!rc) rc = netflow_amd::egress_enqueue_batch(eg, port.data(), queue.data(), n, depth.data(), result.data(),
                                                    order.data(), key_start.data(), dropped.data());
    if (rc) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
    for (size_t i = 0; i < n; ++i) {
        std::printf("F %u %u %u ", ops[i], queue[i], result[i]);
        const uint8_t* d = bufs[i]->get_data_start_ptr();
        for (size_t b = 0; b < bufs[i]->get_data_length(); ++b) std::printf("%02x", d[b]);
        std::printf("\n");
    }
    print_row("K", key_start, keys + 1);
    print_row("O", order, key_start[keys]);
    print_row("X", dropped, keys);
    print_row("Z", depth, keys);
    nfcs_egress_destroy(eg);
    return 0;
}

// icmp_respond_test.cpp — the C++ host API's ICMP responder (include/netflow_amd/packet.hpp): tables built through
// the C ABI and through make_icmp_from over a stand-in for the interface manager, ChecksumEngine::upload_fib /
// upload_icmp, route_lookup_batch over netflow_amd::Packet objects and then icmp_respond_batch on its verdicts.
// Driven by tests/test_gpu_icmp_cpp.py.
//
// stdin, one record per line (numbers decimal, blobs hex): "I ingress_port", "N num_ports",
// "R route(16-byte nfcs_fib_route)", "A arp(12-byte nfcs_fib_arp)", "M if_mac(12-byte nfcs_fib_if_mac)", "L local_ip",
// "C if_id link_up mac(6 bytes) ip ..." (one configured interface), "F ip_id frame".
// stdout: "T messages messages_needed echo_replies errors msg_bytes", "S status ..." (per packet), then per message
// "src port len bytes(hex)".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "netflow_amd/packet.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return v;
}

// InterfaceManager's two members that make_icmp_from reads, with its types' member names
struct Mac { uint8_t bytes[6]; };
struct IpConf { uint32_t address; };
struct PortCfg { Mac mac_address; std::vector<IpConf> ip_configurations; };
struct Ifm {
    std::map<uint32_t, PortCfg> cfg;
    std::map<uint32_t, bool> up;
    std::map<uint32_t, PortCfg> get_all_port_configs() const { return cfg; }
    bool is_port_link_up(uint32_t id) const { auto it = up.find(id); return it != up.end() && it->second; }
};

template <class T>
static bool blob(const std::string& h, std::vector<T>& out) {
    const std::vector<uint8_t> b = unhex(h);
    if (b.size() != sizeof(T)) return false;
    T t;
    std::memcpy(&t, b.data(), sizeof t);
    out.push_back(t);
    return true;
}

int main() {
    uint32_t ingress = 0, num_ports = 0;
    std::vector<nfcs_fib_route> routes;
    std::vector<nfcs_fib_arp> arp;
    std::vector<nfcs_fib_if_mac> ifm;
    std::vector<uint32_t> local;
    std::vector<uint16_t> ids;
    Ifm mgr;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "I") in >> ingress;
        else if (kind == "N") in >> num_ports;
        else if (kind == "R") { in >> h; if (!blob(h, routes)) return 2; }
        else if (kind == "A") { in >> h; if (!blob(h, arp)) return 2; }
        else if (kind == "M") { in >> h; if (!blob(h, ifm)) return 2; }
        else if (kind == "L") { uint32_t ip; in >> ip; local.push_back(ip); }
        else if (kind == "C") {
            uint32_t id, up;
            in >> id >> up >> h;
            const std::vector<uint8_t> m = unhex(h);
            if (m.size() != 6) return 2;
            PortCfg c;
            std::memcpy(c.mac_address.bytes, m.data(), 6);
            for (uint32_t ip; in >> ip;) c.ip_configurations.push_back(IpConf{ip});
            mgr.cfg[id] = c;
            mgr.up[id] = up != 0;
        } else if (kind == "F") {
            uint32_t id;
            in >> id >> h;
            const std::vector<uint8_t> f = unhex(h);
            ids.push_back((uint16_t)id);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        }
    }
    nfcs_fib* fib = nullptr;
    nfcs_icmp* icmp = nullptr;
    int rc = nfcs_fib_create(&fib);
    if (!rc) rc = nfcs_fib_set_routes(fib, routes.data(), (uint32_t)routes.size());
    if (!rc) rc = nfcs_fib_set_arp(fib, arp.data(), (uint32_t)arp.size());
    if (!rc) rc = nfcs_fib_set_if_macs(fib, ifm.data(), (uint32_t)ifm.size());
    if (!rc) rc = nfcs_fib_set_local_ips(fib, local.data(), (uint32_t)local.size());
    if (!rc) rc = nfcs_fib_commit(fib);
    if (!rc) rc = netflow_amd::make_icmp_from(mgr, num_ports, &icmp);
    if (rc) { std::fprintf(stderr, "tables rc=%d\n", rc); return 2; }

    std::vector<netflow_amd::Packet*> raw;
    for (auto& p : pkts) raw.push_back(p.get());
    const size_t n = raw.size();
    std::vector<uint32_t> nh(n);
    std::vector<uint8_t> verdict(n, 0xEE);
    netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
    netflow_amd::ChecksumEngine::IcmpMessages msgs, again, none;
    if (eng.icmp_respond_batch(raw.data(), n, icmp, fib, ingress, verdict.data(), ids.data(), &msgs) != NFCS_EINVAL) {
        std::fprintf(stderr, "no EINVAL before the uploads\n");
        return 3;
    }
    if ((rc = eng.upload_fib(fib)) || (rc = eng.upload_icmp(icmp))) { std::fprintf(stderr, "upload rc=%d\n", rc); return 2; }
    if ((rc = eng.route_lookup_batch(raw.data(), n, fib, nh.data(), nullptr, verdict.data()))) return 2;
    if ((rc = eng.icmp_respond_batch(raw.data(), n, icmp, fib, ingress, verdict.data(), ids.data(), &msgs))) {
        std::fprintf(stderr, "respond rc=%d\n", rc);
        return 2;
    }
    // through the free function, a second time: the same messages
    if ((rc = netflow_amd::icmp_respond_batch(raw.data(), n, icmp, fib, ingress, verdict.data(), ids.data(), &again))) return 2;
    if (again.bytes != msgs.bytes || again.src != msgs.src || again.status != msgs.status) {
        std::fprintf(stderr, "the second call differs\n");
        return 4;
    }
    if (eng.icmp_respond_batch(raw.data(), 0, icmp, fib, ingress, verdict.data(), nullptr, &none) || !none.src.empty()) return 4;
    std::printf("T %u %u %u %u %llu\n", msgs.totals.messages, msgs.totals.messages_needed, msgs.totals.echo_replies,
                msgs.totals.errors, (unsigned long long)msgs.totals.msg_bytes);
    std::printf("S");
    for (uint8_t s : msgs.status) std::printf(" %u", s);
    std::printf("\n");
    for (size_t k = 0; k < msgs.src.size(); ++k) {
        std::printf("%u %u %u ", msgs.src[k], msgs.port[k], msgs.len[k]);
        for (uint32_t j = 0; j < msgs.len[k]; ++j) std::printf("%02x", msgs.bytes[msgs.off[k] + j]);
        std::printf("\n");
    }
    nfcs_icmp_destroy(icmp);
    nfcs_fib_destroy(fib);
    return 0;
}

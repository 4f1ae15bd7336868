// dispatch_test.cpp — the C++ host API's ingress dispatch (include/netflow_amd/packet.hpp): the port state built
// through the C ABI, ChecksumEngine::upload_fdb, then ingress_dispatch_batch over netflow_amd::Packet objects.
// Driven by tests/test_gpu_dispatch_cpp.py.
//
// stdin, one record per line: "I ingress_port", "N num_ports", "A 0|1" (whether the port has an ingress list),
// "P port(hex of one 12-byte nfcs_l2_port)", "F rt_verdict action redirect next_hop l2_port l2_verdict frame(hex)"
// (numbers decimal; a frame of no bytes is "-").
// stdout: "rx packets bytes drops", then per frame "class bypass next_hop l2_port l2_verdict".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "netflow_amd/packet.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return v;
}

int main() {
    nfcs_fdb* fdb = nullptr;
    int rc = nfcs_fdb_create(&fdb);
    if (rc) return 2;
    uint32_t ingress = 0, num_ports = 0, has_list = 0;
    std::vector<uint8_t> rt, action, l2v;
    std::vector<uint32_t> redirect, nh, l2p;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "I") {
            in >> ingress;
        } else if (kind == "N") {
            in >> num_ports;
        } else if (kind == "A") {
            in >> has_list;
        } else if (kind == "P") {
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            if (b.size() != sizeof(nfcs_l2_port)) return 2;
            nfcs_l2_port p;
            std::memcpy(&p, b.data(), sizeof p);
            if ((rc = nfcs_fdb_set_port(fdb, &p, nullptr, 0))) return 2;
        } else if (kind == "F") {
            uint32_t v[6] = {0, 0, 0, 0, 0, 0};
            for (uint32_t& x : v) in >> x;
            in >> h;
            rt.push_back((uint8_t)v[0]), action.push_back((uint8_t)v[1]), redirect.push_back(v[2]);
            nh.push_back(v[3]), l2p.push_back(v[4]), l2v.push_back((uint8_t)v[5]);
            const std::vector<uint8_t> f = unhex(h);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        }
    }
    if ((rc = nfcs_fdb_commit(fdb))) { std::fprintf(stderr, "fdb rc=%d\n", rc); return 2; }

    std::vector<netflow_amd::Packet*> raw;
    for (auto& p : pkts) raw.push_back(p.get());
    const size_t n = raw.size();
    netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
    std::vector<uint32_t> nh0 = nh, l2p0 = l2p;
    std::vector<uint8_t> l2v0 = l2v, cls(n, 0xEE), bypass(n, 0xEE);
    const uint8_t* act = has_list ? action.data() : nullptr;
    const uint32_t* red = has_list ? redirect.data() : nullptr;
    // before the upload the call is an argument error, not a launch, and changes nothing
    if (eng.ingress_dispatch_batch(raw.data(), n, fdb, ingress, num_ports, rt.data(), nh0.data(), l2p0.data(), l2v0.data(), act, red) !=
            NFCS_EINVAL || nh0 != nh) {
        std::fprintf(stderr, "no EINVAL\n");
        return 3;
    }
    if ((rc = eng.upload_fdb(fdb))) { std::fprintf(stderr, "upload rc=%d\n", rc); return 2; }
    // without the optional outputs: the three in/out arrays alone
    if ((rc = eng.ingress_dispatch_batch(raw.data(), n, fdb, ingress, num_ports, rt.data(), nh0.data(), l2p0.data(), l2v0.data(), act,
                                         red))) {
        std::fprintf(stderr, "rc=%d\n", rc);
        return 2;
    }
    // the free function on the process-wide engine, with every output; the counters start above zero
    nfcs_rx_stats rx = {1000, 100000, 10};
    rc = netflow_amd::ingress_dispatch_batch(raw.data(), n, fdb, ingress, num_ports, rt.data(), nh.data(), l2p.data(), l2v.data(), act, red,
                                             cls.data(), bypass.data(), &rx);
    if (rc) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
    if (nh0 != nh || l2p0 != l2p || l2v0 != l2v) { std::fprintf(stderr, "the arrays differ without the optional outputs\n"); return 4; }
    std::printf("rx %llu %llu %llu\n", (unsigned long long)rx.rx_packets - 1000, (unsigned long long)rx.rx_bytes - 100000,
                (unsigned long long)rx.rx_drops - 10);
    for (size_t i = 0; i < n; ++i) std::printf("%u %u %u %u %u\n", cls[i], bypass[i], nh[i], l2p[i], l2v[i]);
    nfcs_fdb_destroy(fdb);
    return 0;
}

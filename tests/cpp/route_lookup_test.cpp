// route_lookup_test.cpp — the C++ host API's lookup -> forward path (include/netflow_amd/packet.hpp):
// a forwarding table built through the C ABI, ChecksumEngine::upload_fib, route_lookup_batch over
// netflow_amd::Packet objects, then l3_forward_batch with the next hops it returned and the fib's own
// next-hop table. Driven by tests/test_gpu_route_cpp.py.
//
// stdin, one record per line: "R network mask next_hop if", "A ip mac(hex)", "I if mac(hex)", "L ip",
// "F frame(hex)" (numbers decimal). stdout: "T table(hex)", then per frame
// "verdict next_hop egress_if forward_status frame_after(hex)".
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
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return v;
}
static std::string hex(const unsigned char* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}

int main() {
    std::vector<nfcs_fib_route> routes;
    std::vector<nfcs_fib_arp> arp;
    std::vector<nfcs_fib_if_mac> ifm;
    std::vector<uint32_t> local;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "R") {
            nfcs_fib_route r{};
            in >> r.network >> r.mask >> r.next_hop_ip >> r.egress_if;
            routes.push_back(r);
        } else if (kind == "A") {
            nfcs_fib_arp a{};
            in >> a.ip >> h;
            std::memcpy(a.mac, unhex(h).data(), 6);
            arp.push_back(a);
        } else if (kind == "I") {
            nfcs_fib_if_mac m{};
            in >> m.egress_if >> h;
            std::memcpy(m.mac, unhex(h).data(), 6);
            ifm.push_back(m);
        } else if (kind == "L") {
            uint32_t a = 0;
            in >> a;
            local.push_back(a);
        } else if (kind == "F") {
            in >> h;
            const std::vector<uint8_t> f = unhex(h);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        }
    }
    nfcs_fib* fib = nullptr;
    int rc = nfcs_fib_create(&fib);
    if (!rc) rc = nfcs_fib_set_routes(fib, routes.data(), (uint32_t)routes.size());
    if (!rc) rc = nfcs_fib_set_arp(fib, arp.data(), (uint32_t)arp.size());
    if (!rc) rc = nfcs_fib_set_if_macs(fib, ifm.data(), (uint32_t)ifm.size());
    if (!rc) rc = nfcs_fib_set_local_ips(fib, local.data(), (uint32_t)local.size());
    if (!rc) rc = nfcs_fib_commit(fib);
    if (rc) { std::fprintf(stderr, "fib rc=%d\n", rc); return 2; }
    uint32_t table_n = 0;
    nfcs_fib_nexthops_host(fib, nullptr, 0, &table_n);
    std::vector<nfcs_nexthop> table(table_n ? table_n : 1);
    nfcs_fib_nexthops_host(fib, table.data(), table_n, &table_n);

    std::vector<netflow_amd::Packet*> raw;
    for (auto& p : pkts) raw.push_back(p.get());
    const size_t n = raw.size();
    std::vector<uint32_t> nh(n, 0xEEEEEEEEu), eif(n, 0xEEEEEEEEu);
    std::vector<uint8_t> verdict(n, 0xEE), status(n, 0xEE);
    {
        netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
        // before the upload the lookup is an argument error, not a launch
        if (eng.route_lookup_batch(raw.data(), n, fib, nh.data()) != NFCS_EINVAL) { std::fprintf(stderr, "no EINVAL\n"); return 3; }
        if ((rc = eng.upload_fib(fib))) { std::fprintf(stderr, "upload rc=%d\n", rc); return 2; }
    }
    rc = netflow_amd::route_lookup_batch(raw.data(), n, fib, nh.data(), eif.data(), verdict.data());
    if (!rc) rc = netflow_amd::l3_forward_batch(raw.data(), nh.data(), n, table.data(), table_n, status.data());
    if (rc) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
    std::printf("T %s\n", hex(reinterpret_cast<const uint8_t*>(table.data()), table_n * sizeof(nfcs_nexthop)).c_str());
    for (size_t i = 0; i < n; ++i)
        std::printf("%u %u %u %u %s\n", verdict[i], nh[i], eif[i], status[i],
                    hex(bufs[i]->get_data_start_ptr(), bufs[i]->get_data_length()).c_str());
    nfcs_fib_destroy(fib);
    return 0;
}

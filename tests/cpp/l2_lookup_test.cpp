// l2_lookup_test.cpp — the C++ host API's L2 path (include/netflow_amd/packet.hpp): a forwarding database
// built through the C ABI, ChecksumEngine::upload_fdb, then l2_lookup_batch over netflow_amd::Packet
// objects. Driven by tests/test_gpu_l2_cpp.py.
//
// stdin, one record per line: "I ingress_port", "E entry(hex of one 16-byte nfcs_fdb_entry)",
// "P port(hex of one 12-byte nfcs_l2_port) allowed_vlan ..." (numbers decimal), "F rt_verdict frame(hex)".
// stdout per frame: "verdict egress_port vlan learn skipped_verdict", the last from a second call that
// passes the route verdicts.
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

int main() {
    nfcs_fdb* fdb = nullptr;
    int rc = nfcs_fdb_create(&fdb);
    if (rc) return 2;
    uint32_t ingress = 0;
    std::vector<nfcs_fdb_entry> entries;
    std::vector<uint8_t> rt;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "I") {
            in >> ingress;
        } else if (kind == "E") {
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            if (b.size() != sizeof(nfcs_fdb_entry)) return 2;
            nfcs_fdb_entry e;
            std::memcpy(&e, b.data(), sizeof e);
            entries.push_back(e);
        } else if (kind == "P") {
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            if (b.size() != sizeof(nfcs_l2_port)) return 2;
            nfcs_l2_port p;
            std::memcpy(&p, b.data(), sizeof p);
            std::vector<uint16_t> allowed;
            for (uint32_t v; in >> v;) allowed.push_back((uint16_t)v);
            if ((rc = nfcs_fdb_set_port(fdb, &p, allowed.data(), (uint32_t)allowed.size()))) return 2;
        } else if (kind == "F") {
            uint32_t v = 0;
            in >> v >> h;
            rt.push_back((uint8_t)v);
            const std::vector<uint8_t> f = unhex(h);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        }
    }
    rc = nfcs_fdb_set_entries(fdb, entries.data(), (uint32_t)entries.size());
    if (!rc) rc = nfcs_fdb_commit(fdb);
    if (rc) { std::fprintf(stderr, "fdb rc=%d\n", rc); return 2; }

    std::vector<netflow_amd::Packet*> raw;
    for (auto& p : pkts) raw.push_back(p.get());
    const size_t n = raw.size();
    std::vector<uint32_t> port(n, 0xEEEEEEEEu), only(n, 0xEEEEEEEEu), port2(n, 0xEEEEEEEEu);
    std::vector<uint16_t> vlan(n, 0xEEEE);
    std::vector<uint8_t> verdict(n, 0xEE), learn(n, 0xEE), skipped(n, 0xEE);
    netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
    // before the upload the lookup is an argument error, not a launch
    if (eng.l2_lookup_batch(raw.data(), n, fdb, ingress, port.data()) != NFCS_EINVAL) { std::fprintf(stderr, "no EINVAL\n"); return 3; }
    if ((rc = eng.upload_fdb(fdb))) { std::fprintf(stderr, "upload rc=%d\n", rc); return 2; }
    // without the optional outputs: the ports alone
    if ((rc = eng.l2_lookup_batch(raw.data(), n, fdb, ingress, only.data()))) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
    rc = eng.l2_lookup_batch(raw.data(), n, fdb, ingress, port.data(), verdict.data(), vlan.data(), learn.data());
    if (!rc && only != port) { std::fprintf(stderr, "ports differ without the optional outputs\n"); return 4; }
    // the free function on the process-wide engine, fed the route verdicts
    if (!rc) rc = netflow_amd::l2_lookup_batch(raw.data(), n, fdb, ingress, port2.data(), skipped.data(), nullptr, nullptr, rt.data());
    if (rc) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
    for (size_t i = 0; i < n; ++i) std::printf("%u %u %u %u %u\n", verdict[i], port[i], vlan[i], learn[i], skipped[i]);
    nfcs_fdb_destroy(fdb);
    return 0;
}

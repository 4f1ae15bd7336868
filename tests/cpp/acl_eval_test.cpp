// acl_eval_test.cpp — the C++ host API's ACL -> forward path (include/netflow_amd/packet.hpp): a rule
// list built through the C ABI, ChecksumEngine::upload_acl, acl_eval_batch over netflow_amd::Packet
// objects masking a next-hop vector, then l3_forward_batch with the masked next hops. Driven by
// tests/test_gpu_acl_cpp.py.
//
// stdin, one record per line: "A rule(hex of one 52-byte nfcs_acl_rule)", "T next_hop(hex, 12 bytes)",
// "F next_hop_index frame(hex)" (numbers decimal). stdout per frame:
// "action rule redirect_port next_hop_after forward_status frame_after(hex)".
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
    std::vector<nfcs_acl_rule> rules;
    std::vector<nfcs_nexthop> table;
    std::vector<uint32_t> nh;
    std::vector<std::unique_ptr<netflow_amd::PacketBuffer>> bufs;
    std::vector<std::unique_ptr<netflow_amd::Packet>> pkts;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, h;
        in >> kind;
        if (kind == "A") {
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            if (b.size() != sizeof(nfcs_acl_rule)) return 2;
            nfcs_acl_rule r;
            std::memcpy(&r, b.data(), sizeof r);
            rules.push_back(r);
        } else if (kind == "T") {
            in >> h;
            const std::vector<uint8_t> b = unhex(h);
            if (b.size() != sizeof(nfcs_nexthop)) return 2;
            nfcs_nexthop t;
            std::memcpy(&t, b.data(), sizeof t);
            table.push_back(t);
        } else if (kind == "F") {
            uint32_t k = 0;
            in >> k >> h;
            nh.push_back(k);
            const std::vector<uint8_t> f = unhex(h);
            bufs.emplace_back(new netflow_amd::PacketBuffer(f.size() + 96, 32, f.size()));
            if (!f.empty()) std::memcpy(bufs.back()->get_data_start_ptr(), f.data(), f.size());
            pkts.emplace_back(new netflow_amd::Packet(bufs.back().get()));
        }
    }
    nfcs_acl* acl = nullptr;
    int rc = nfcs_acl_create(&acl);
    if (!rc) rc = nfcs_acl_set_rules(acl, rules.data(), (uint32_t)rules.size());
    if (!rc) rc = nfcs_acl_commit(acl);
    if (rc) { std::fprintf(stderr, "acl rc=%d\n", rc); return 2; }

    std::vector<netflow_amd::Packet*> raw;
    for (auto& p : pkts) raw.push_back(p.get());
    const size_t n = raw.size();
    std::vector<uint32_t> rule(n, 0xEEEEEEEEu), port(n, 0xEEEEEEEEu);
    std::vector<uint8_t> action(n, 0xEE), status(n, 0xEE);
    {
        netflow_amd::ChecksumEngine& eng = netflow_amd::ChecksumEngine::instance();
        // before the upload the evaluation is an argument error, not a launch
        if (eng.acl_eval_batch(raw.data(), n, acl, action.data()) != NFCS_EINVAL) { std::fprintf(stderr, "no EINVAL\n"); return 3; }
        if ((rc = eng.upload_acl(acl))) { std::fprintf(stderr, "upload rc=%d\n", rc); return 2; }
        // without the optional outputs: the actions alone
        std::vector<uint8_t> only(n, 0xEE);
        if ((rc = eng.acl_eval_batch(raw.data(), n, acl, only.data()))) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
        rc = eng.acl_eval_batch(raw.data(), n, acl, action.data(), rule.data(), port.data(), nh.data());
        if (!rc && only != action) { std::fprintf(stderr, "actions differ without the optional outputs\n"); return 4; }
    }
    if (!rc) rc = netflow_amd::l3_forward_batch(raw.data(), nh.data(), n, table.data(), (uint32_t)table.size(), status.data());
    if (rc) { std::fprintf(stderr, "rc=%d\n", rc); return 2; }
    for (size_t i = 0; i < n; ++i)
        std::printf("%u %u %u %u %u %s\n", action[i], rule[i], port[i], nh[i], status[i],
                    hex(bufs[i]->get_data_start_ptr(), bufs[i]->get_data_length()).c_str());
    nfcs_acl_destroy(acl);
    return 0;
}

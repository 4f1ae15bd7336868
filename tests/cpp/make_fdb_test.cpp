// make_fdb_test.cpp — host-only check of netflow_amd::make_fdb_from (include/netflow_amd/packet.hpp), the
// work behind netflow_adapter.hpp's make_fdb(ForwardingDatabase, VlanManager, link_up, stp_forwarding,
// num_ports, ...): mirror types with the reference's member names (get_all_entries() of entries with mac,
// vlan_id, port, is_static; get_port_config(port) returning an optional config with an enum type,
// native_vlan and a std::set of allowed VLANs), then the decisions of the database it builds. No GPU: the
// database is host code until it is uploaded. Built and run by tests/test_l2_fdb.py. Prints "make_fdb OK"
// and exits 0 when every check holds.
#include <cstdio>
#include <map>
#include <optional>
#include <set>
#include <vector>

#include "netflow_amd/packet.hpp"

namespace {

struct Mac { uint8_t bytes[6]; };
struct Entry {
    Mac mac;
    uint32_t port;
    uint16_t vlan_id;
    long timestamp;
    bool is_static;
};
struct Fdb {
    std::vector<Entry> entries;
    const std::vector<Entry>& get_all_entries() const { return entries; }
};
enum class PortType { ACCESS, TRUNK, HYBRID };
struct PortConfig {
    PortType type = PortType::ACCESS;
    uint16_t native_vlan = 1;
    std::set<uint16_t> allowed_vlans;
    bool tag_native = false;
};
struct Vlans {
    std::map<uint32_t, PortConfig> cfg;
    std::optional<PortConfig> get_port_config(uint32_t p) const {
        auto it = cfg.find(p);
        return it == cfg.end() ? std::nullopt : std::optional<PortConfig>(it->second);
    }
};

std::vector<uint8_t> frame(uint8_t dst_last, uint8_t src_last, int vlan) {
    std::vector<uint8_t> f(64, 0);
    f[0] = f[6] = 2;
    f[5] = dst_last, f[11] = src_last;
    f[12] = 0x88, f[13] = 0xB5;
    if (vlan >= 0) f[12] = 0x81, f[13] = 0x00, f[14] = (uint8_t)(vlan >> 8), f[15] = (uint8_t)vlan;
    return f;
}

int g_bad = 0;
void expect(const nfcs_fdb* fdb, uint32_t ingress, const std::vector<uint8_t>& f, uint32_t verdict, uint32_t port,
            uint32_t vlan, uint32_t learn) {
    uint32_t v = 99, p = 99, vl = 99, le = 99;
    const int rc = nfcs_fdb_lookup_host(fdb, ingress, f.data(), (uint32_t)f.size(), &v, &p, &vl, &le);
    if (rc != 0 || v != verdict || p != port || vl != vlan || le != learn) {
        std::printf("rc %d verdict %u (want %u) port %u (want %u) vlan %u (want %u) learn %u (want %u)\n", rc, v, verdict,
                    p, port, vl, vlan, le, learn);
        ++g_bad;
    }
}

}  // namespace

int main() {
    Fdb fdb;
    fdb.entries.push_back(Entry{Mac{{2, 0, 0, 0, 0, 1}}, 1, 10, 0, false});
    fdb.entries.push_back(Entry{Mac{{2, 0, 0, 0, 0, 2}}, 2, 20, 0, true});
    fdb.entries.push_back(Entry{Mac{{2, 0, 0, 0, 0, 3}}, 3, 10, 0, false});  // port 3: link down
    fdb.entries.push_back(Entry{Mac{{2, 0, 0, 0, 0, 4}}, 4, 10, 0, false});  // port 4: not STP-forwarding
    fdb.entries.push_back(Entry{Mac{{2, 0, 0, 0, 0, 5}}, 5, 10, 0, false});  // port 5: no VLAN config
    fdb.entries.push_back(Entry{Mac{{2, 0, 0, 0, 0, 6}}, 0, 10, 0, false});  // on the ingress port
    Vlans vl;
    vl.cfg[0].native_vlan = 10;
    vl.cfg[1].native_vlan = 10;
    vl.cfg[2].type = PortType::TRUNK;
    vl.cfg[2].allowed_vlans = {10, 20};
    vl.cfg[3].native_vlan = 10;
    vl.cfg[4].native_vlan = 10;
    vl.cfg[6].type = PortType::HYBRID;
    vl.cfg[6].native_vlan = 7;
    vl.cfg[6].allowed_vlans = {20};
    auto link_up = [](uint32_t p) { return p != 3; };
    auto stp_forwarding = [](uint32_t p) { return p != 4; };
    nfcs_fdb* f = nullptr;
    if (netflow_amd::make_fdb_from(fdb, vl, link_up, stp_forwarding, 7, &f) != NFCS_OK || !f) return 2;
    if (netflow_amd::make_fdb_from(fdb, vl, link_up, stp_forwarding, 7, (nfcs_fdb**)nullptr) != NFCS_EINVAL) return 3;
    expect(f, 0, frame(1, 9, -1), NFCS_L2_FORWARD, 1, 10, NFCS_L2_LEARN_NEW);
    expect(f, 0, frame(1, 6, 10), NFCS_L2_FORWARD, 1, 10, NFCS_L2_LEARN_REFRESH);
    expect(f, 0, frame(2, 1, 20), NFCS_L2_DROP_VLAN, NFCS_IF_NONE, 20, NFCS_L2_LEARN_NEW);  // ACCESS 10 takes no VLAN 20
    expect(f, 6, frame(2, 2, 20), NFCS_L2_FORWARD, 2, 20, NFCS_L2_LEARN_NONE);              // HYBRID allows 20; static source
    expect(f, 6, frame(2, 2, -1), NFCS_L2_FLOOD, NFCS_IF_NONE, 7, NFCS_L2_LEARN_NEW);       // its native VLAN 7
    expect(f, 0, frame(3, 1, -1), NFCS_L2_DROP_LINK_DOWN, NFCS_IF_NONE, 10, NFCS_L2_LEARN_MOVED);
    expect(f, 0, frame(4, 1, -1), NFCS_L2_DROP_STP, NFCS_IF_NONE, 10, NFCS_L2_LEARN_MOVED);
    expect(f, 0, frame(5, 1, -1), NFCS_L2_DROP_VLAN, NFCS_IF_NONE, 10, NFCS_L2_LEARN_MOVED);
    expect(f, 0, frame(6, 1, -1), NFCS_L2_DROP_SAME_PORT, NFCS_IF_NONE, 10, NFCS_L2_LEARN_MOVED);
    expect(f, 5, frame(1, 9, -1), NFCS_L2_FLOOD, NFCS_IF_NONE, 1, NFCS_L2_LEARN_NEW);  // no config: PortConfig()'s VLAN 1
    expect(f, 0, std::vector<uint8_t>(10, 0), NFCS_L2_NO_ETH, NFCS_IF_NONE, 0, NFCS_L2_LEARN_NONE);
    uint32_t ports[8], n = 0;
    if (nfcs_fdb_flood_ports_host(f, 0, 10, 7, ports, 8, &n) != NFCS_OK || n != 2 || ports[0] != 1 || ports[1] != 2) {
        std::printf("flood list: %u ports\n", n);
        ++g_bad;
    }
    nfcs_fdb_destroy(f);
    // no ports and no entries is a valid database; more ports than the library holds is an error that
    // leaves no database behind
    if (netflow_amd::make_fdb_from(Fdb{}, Vlans{}, link_up, stp_forwarding, 0, &f) != NFCS_OK || !f) return 4;
    expect(f, 0, frame(1, 9, -1), NFCS_L2_FLOOD, NFCS_IF_NONE, 1, NFCS_L2_LEARN_NEW);
    nfcs_fdb_destroy(f);
    if (netflow_amd::make_fdb_from(fdb, vl, link_up, stp_forwarding, NFCS_L2_MAX_PORTS + 1, &f) != NFCS_EINVAL || f) return 5;
    std::printf(g_bad ? "FAIL\n" : "make_fdb OK\n");
    return g_bad ? 1 : 0;
}

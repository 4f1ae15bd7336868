// make_fib_test.cpp — host-only check of netflow_amd::make_fib_from (include/netflow_amd/packet.hpp),
// the work behind netflow_adapter.hpp's make_fib(const netflow::RoutingManager&, ...): a stand-in
// routing table with the member names make_fib_from reads (get_routing_table() of entries with
// destination_network, subnet_mask, next_hop_ip, egress_interface_id) and a MAC type with bytes[6],
// then the decisions of the table it builds. No GPU: the table is host code until it is uploaded.
// Built and run by tests/test_route_fib.py. Prints "make_fib OK" and exits 0 when every check holds.
#include <cstdio>
#include <vector>

#include "netflow_amd/packet.hpp"

namespace {

struct Entry { uint32_t destination_network, subnet_mask, next_hop_ip, egress_interface_id; int metric; };
struct Table {
    std::vector<Entry> entries;
    std::vector<Entry> get_routing_table() const { return entries; }
};
struct Mac { uint8_t bytes[6]; };

uint32_t ip(unsigned a, unsigned b, unsigned c, unsigned d) { return a | (b << 8) | (c << 16) | (d << 24); }

int g_bad = 0;
void expect(const nfcs_fib* fib, const nfcs_nexthop* table, uint32_t dst, uint32_t ttl, uint32_t verdict, uint32_t eif,
            uint8_t dmac, uint8_t smac) {
    uint32_t v = 99, nh = 99, e = 99;
    int rc = nfcs_fib_lookup_host(fib, dst, ttl, &v, &nh, &e);
    bool ok = rc == 0 && v == verdict && e == eif && (v == NFCS_RT_FORWARD) == (nh != NFCS_NH_NONE);
    if (ok && v == NFCS_RT_FORWARD) ok = table[nh].dst_mac[0] == dmac && table[nh].src_mac[0] == smac;
    if (!ok) {
        std::printf("dst %08x ttl %u: rc %d verdict %u (want %u) if %u (want %u) nh %u\n", dst, ttl, rc, v, verdict, e, eif, nh);
        ++g_bad;
    }
}

}  // namespace

int main() {
    Table rm;
    // in lookup order: a connected /24, a /8 through a gateway, the default route through another
    rm.entries = {{ip(10, 1, 2, 0), ip(255, 255, 255, 0), 0, 3, 1},
                  {ip(10, 0, 0, 0), ip(255, 0, 0, 0), ip(10, 1, 2, 254), 2, 1},
                  {0, 0, ip(192, 0, 2, 1), 9, 5}};
    const std::vector<std::pair<uint32_t, Mac>> arp = {{ip(10, 1, 2, 7), Mac{{0x11}}}, {ip(10, 1, 2, 254), Mac{{0x22}}},
                                                      {ip(10, 1, 2, 7), Mac{{0x33}}}};  // a duplicate: the last wins
    const std::vector<std::pair<uint32_t, Mac>> ifm = {{3u, Mac{{0xA3}}}, {2u, Mac{{0xA2}}}};
    nfcs_fib* fib = nullptr;
    if (netflow_amd::make_fib_from(rm, arp, ifm, {ip(10, 1, 2, 1)}, &fib) != NFCS_OK || !fib) return 2;
    if (netflow_amd::make_fib_from(rm, arp, ifm, {}, nullptr) != NFCS_EINVAL) return 3;
    nfcs_nexthop table[8] = {};
    uint32_t tn = 0;
    if (nfcs_fib_nexthops_host(fib, table, 8, &tn) != NFCS_OK || tn != 3) return 4;  // two addresses, one gateway route
    expect(fib, table, ip(10, 1, 2, 7), 64, NFCS_RT_FORWARD, 3, 0x33, 0xA3);
    expect(fib, table, ip(10, 9, 9, 9), 64, NFCS_RT_FORWARD, 2, 0x22, 0xA2);
    expect(fib, table, ip(10, 1, 2, 8), 64, NFCS_RT_ARP_MISS, NFCS_IF_NONE, 0, 0);
    expect(fib, table, ip(8, 8, 8, 8), 64, NFCS_RT_ARP_MISS, NFCS_IF_NONE, 0, 0);  // the default's gateway has no entry
    expect(fib, table, ip(10, 1, 2, 1), 1, NFCS_RT_LOCAL, NFCS_IF_NONE, 0, 0);
    expect(fib, table, ip(10, 1, 2, 7), 1, NFCS_RT_TTL_EXPIRED, NFCS_IF_NONE, 0, 0);
    nfcs_fib_destroy(fib);
    std::printf(g_bad ? "FAIL\n" : "make_fib OK\n");
    return g_bad ? 1 : 0;
}

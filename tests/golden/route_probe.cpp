// route_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_route_golden.py).
//
// Runs the reference's L3 decision (switch.hpp:259-301) over a list of frames with the reference's
// own code: the routes go through RoutingManager::add_static_route and come back through
// get_routing_table(); every frame is a netflow::Packet whose ethernet() / vlan() / ipv4() accessors
// and RoutingManager::lookup_route decide. ARP entries and interface MACs live in std::map as in
// ArpProcessor / InterfaceManager (their lookups are map finds; both classes log and take the whole
// switch as context, so only their containers are mirrored). Compiled against the reference's headers
// in place plus src/netflow++/routing_manager.cpp; the binary goes to oracle/_ref/ (git-ignored).
//
// stdin (little-endian): u32 nr, nr x {net, mask, next_hop, if, metric}; u32 na, na x {ip, mac[6], pad[2]};
//   u32 ni, ni x {if, mac[6], pad[2]}; u32 nl, nl x ip; u32 nf, nf x {u32 len, len bytes}
// stdout: u32 nt, nt x {net, mask, next_hop, if, metric} (get_routing_table() order);
//   nf x {u32 verdict, u32 egress_if, dst_mac[6], src_mac[6]}
#include <netflow++/packet.hpp>
#include <netflow++/routing_manager.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <optional>
#include <set>
#include <vector>

namespace {

// verdict numbering of include/nfcs.h NFCS_RT_* (BAD_DESC = 1 is about arenas, not frames)
enum { FORWARD = 0, NOT_IPV4 = 2, LOCAL = 3, TTL_EXPIRED = 4, NO_ROUTE = 5, ARP_MISS = 6, NO_IF_MAC = 7 };

struct Window {  // a PacketBuffer whose data window is the caller's frame (as oracle/ref_shim.cpp)
    netflow::PacketBuffer pb;
    unsigned char* own;
    Window() : pb(16, 0, 0), own(pb.raw_data_ptr_) {}
    ~Window() { pb.raw_data_ptr_ = own; }
    void point(uint8_t* frame, size_t len) {
        pb.raw_data_ptr_ = frame;
        pb.capacity_ = len;
        pb.data_offset_ = 0;
        pb.data_len_ = len;
    }
};

bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
void wr(const void* p, size_t n) { if (n) fwrite(p, 1, n, stdout); }
uint32_t rd32() { uint32_t v = 0; rd(&v, 4); return v; }
void wr32(uint32_t v) { wr(&v, 4); }

}  // namespace

int main() {
    netflow::RoutingManager rm;
    std::map<netflow::IpAddress, netflow::MacAddress> arp;
    std::map<uint32_t, netflow::MacAddress> if_mac;
    std::set<netflow::IpAddress> my_ips;

    const uint32_t nr = rd32();
    for (uint32_t i = 0; i < nr; ++i) {
        uint32_t r[5];
        if (!rd(r, sizeof r)) return 2;
        rm.add_static_route(r[0], r[1], r[2], r[3], (int)r[4]);
    }
    const uint32_t na = rd32();
    for (uint32_t i = 0; i < na; ++i) {
        uint32_t ip = rd32();
        uint8_t m[8];
        if (!rd(m, 8)) return 2;
        arp[ip] = netflow::MacAddress(m);
    }
    const uint32_t ni = rd32();
    for (uint32_t i = 0; i < ni; ++i) {
        uint32_t id = rd32();
        uint8_t m[8];
        if (!rd(m, 8)) return 2;
        if_mac[id] = netflow::MacAddress(m);
    }
    const uint32_t nl = rd32();
    for (uint32_t i = 0; i < nl; ++i) my_ips.insert(rd32());

    const std::vector<netflow::RouteEntry> table = rm.get_routing_table();
    wr32((uint32_t)table.size());
    for (const netflow::RouteEntry& e : table) {
        wr32(e.destination_network);
        wr32(e.subnet_mask);
        wr32(e.next_hop_ip);
        wr32(e.egress_interface_id);
        wr32((uint32_t)e.metric);
    }

    const uint32_t nf = rd32();
    std::vector<uint8_t> frame;
    for (uint32_t i = 0; i < nf; ++i) {
        const uint32_t len = rd32();
        frame.assign(len + 16, 0);
        if (!rd(frame.data(), len)) return 2;
        Window w;
        w.point(frame.data(), len);
        netflow::Packet pkt(&w.pb);
        uint32_t verdict = NOT_IPV4, egress = 0xFFFFFFFFu;
        uint8_t macs[12] = {0};
        // the decision sequence of switch.hpp:259-301, each step through the reference's accessor
        const netflow::EthernetHeader* eth = pkt.ethernet();
        uint16_t l3_type = eth ? ntohs(eth->ethertype) : 0;
        if (l3_type == netflow::ETHERTYPE_VLAN)
            if (const netflow::VlanHeader* tag = pkt.vlan()) l3_type = ntohs(tag->ethertype);
        const netflow::IPv4Header* ip = l3_type == netflow::ETHERTYPE_IPV4 ? pkt.ipv4() : nullptr;
        if (ip) {
            const netflow::IpAddress dst = ip->dst_ip;
            const std::optional<netflow::RouteEntry> route =
                (my_ips.count(dst) || ip->ttl <= 1) ? std::nullopt : rm.lookup_route(dst);
            if (my_ips.count(dst)) verdict = LOCAL;
            else if (ip->ttl <= 1) verdict = TTL_EXPIRED;
            else if (!route) verdict = NO_ROUTE;
            else {
                const auto a = arp.find(route->next_hop_ip == 0 ? dst : route->next_hop_ip);
                const auto s = if_mac.find(route->egress_interface_id);
                if (a == arp.end()) verdict = ARP_MISS;
                else if (s == if_mac.end()) verdict = NO_IF_MAC;
                else {
                    verdict = FORWARD;
                    egress = route->egress_interface_id;
                    memcpy(macs, a->second.bytes, 6);
                    memcpy(macs + 6, s->second.bytes, 6);
                }
            }
        }
        wr32(verdict);
        wr32(egress);
        wr(macs, 12);
    }
    return fflush(stdout) == 0 ? 0 : 3;
}

// icmp_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_icmp_golden.py).
//
// Constructs a real netflow::Switch and drives its own icmp_processor_ at the three call sites of
// Switch::process_received_packet, which the reference leaves as comments:
//   switch.hpp:271  is_my_ip(dst), protocol ICMP  -> icmp_processor_.process_icmp_packet(pkt, ingress)
//   switch.hpp:279  ttl <= 1                      -> icmp_processor_.send_time_exceeded(pkt, ingress)
//   switch.hpp:301  no route                      -> icmp_processor_.send_destination_unreachable(pkt, ingress, 0)
// The decision between them (259-301) is restated here through the reference's own accessors. What the
// processor sends is captured through test_packet_send_hook, which send_control_plane_packet calls after its
// port test; the ARP requests the error path sends on an ARP miss go through the same hook and are dropped
// here by their EtherType. Interfaces go through InterfaceManager::configure_port / add_ip_address /
// simulate_port_link_up, routes through RoutingManager::add_static_route, ARP entries through
// ArpProcessor::process_arp_packet on ARP replies (its cache has no public setter). Per frame the probe also
// names the step at which the reference stops, asking the reference's accessors in icmp_processor.cpp's order.
// `extra local` addresses are addresses the caller's lookup calls local that no interface holds: the
// processor's own is_my_ip then says "not for us". Frames whose IPv4 header runs past the frame are not fed
// (the reference would copy past its buffer). Links against src/netflow++/*.cpp without isis/; the binary
// goes to oracle/_ref/ (git-ignored). Run it in an empty directory (the constructor looks for
// default_switch_config.json). The loggers print to stdout, so the results go to the file named by argv[1].
//
// stdin (little-endian):
//   u32 num_ports, u32 ingress, u32 seed (srand)
//   u32 n_if, n_if x {u32 id, u8 link_up, u8 pad[3], mac[6], u8 pad[2], u32 n_ip, n_ip x u32 ip}
//   u32 n_routes, n_routes x {net, mask, next_hop, if}
//   u32 n_arp, n_arp x {u32 ip, mac[6], u8 pad[2]}
//   u32 n_extra, n_extra x u32 ip
//   u32 nf, nf x {u32 len, bytes}
// argv[1] (little-endian):
//   u32 n_if, n_if x {u32 id, u8 link_up, u8 pad[3], mac[6], u8 pad[2], u32 n_ip, n_ip x u32 ip}  (get_all_port_configs)
//   u32 n_routes, n_routes x {net, mask, next_hop, if}                                        (get_routing_table)
//   u32 n_arp, n_arp x {u32 ip, mac[6], u8 pad[2]}                                 (lookup_mac per distinct address)
//   nf x {u32 verdict (NFCS_RT_*: 3, 4, 5, or 0 for anything else), u32 status (NFCS_ICMP_ST_*), u32 sent (0 / 1),
//         u32 port, u32 len, len bytes}
#include <netflow++/switch.hpp>

#include <arpa/inet.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <set>
#include <vector>

namespace {

enum : uint32_t { RT_OTHER = 0, RT_LOCAL = 3, RT_TTL = 4, RT_NO_ROUTE = 5 };
enum : uint32_t { ST_NONE = 0, ST_ECHO = 1, ST_TIME = 2, ST_UNREACH = 3, ST_TO_CPU = 4, ST_IGNORED = 5, ST_NO_LOCAL_MAC = 6,
                  ST_SRC_NO_ROUTE = 7, ST_SRC_NO_IF_IP = 8, ST_SRC_ARP_MISS = 9, ST_SRC_NO_IF_MAC = 10, ST_PORT_DOWN = 11 };

FILE* g_out = nullptr;
bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
void wr(const void* p, size_t n) { if (n) fwrite(p, 1, n, g_out); }
uint32_t rd32() { uint32_t v = 0; rd(&v, 4); return v; }
void wr32(uint32_t v) { wr(&v, 4); }

struct Sent { uint32_t port; std::vector<uint8_t> bytes; };

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    const uint32_t num_ports = rd32(), ingress = rd32(), seed = rd32();
    std::vector<std::unique_ptr<netflow::PacketBuffer>> bufs;  // declared before the switch: its queues refer to them
    netflow::Switch sw(num_ports, 0x02AA00000001ull);
    std::vector<Sent> sent;
    sw.test_packet_send_hook = [&](const netflow::Packet& pkt, uint32_t port) {
        const netflow::PacketBuffer* b = pkt.get_buffer();
        const uint8_t* d = b->get_data_start_ptr();
        const size_t len = b->get_data_length();
        if (len < 14 || d[12] != 0x08 || d[13] != 0x00) return;  // an ARP request of the error path
        sent.push_back(Sent{port, std::vector<uint8_t>(d, d + len)});
    };
    auto buffer_of = [&](const uint8_t* data, size_t len) {
        bufs.push_back(std::make_unique<netflow::PacketBuffer>(len + 16, 0, len));
        memset(bufs.back()->get_data_start_ptr(), 0, len + 16);
        memcpy(bufs.back()->get_data_start_ptr(), data, len);
        return bufs.back().get();
    };

    const uint32_t n_if = rd32();
    for (uint32_t i = 0; i < n_if; ++i) {
        const uint32_t id = rd32();
        uint8_t f[4], m[8];
        if (!rd(f, 4) || !rd(m, 8)) return 2;
        netflow::InterfaceManager::PortConfig cfg;
        cfg.admin_up = f[0] != 0;
        cfg.mac_address = netflow::MacAddress(m);
        sw.interface_manager_.configure_port(id, cfg);
        const uint32_t n_ip = rd32();
        for (uint32_t k = 0; k < n_ip; ++k) sw.interface_manager_.add_ip_address(id, rd32(), htonl(0xFFFFFF00u));
        if (f[0]) sw.interface_manager_.simulate_port_link_up(id);
        else sw.interface_manager_.simulate_port_link_down(id);
    }
    const uint32_t n_routes = rd32();
    for (uint32_t i = 0; i < n_routes; ++i) {
        uint32_t r[4];
        if (!rd(r, sizeof r)) return 2;
        sw.routing_manager_.add_static_route(r[0], r[1], r[2], r[3], 1);
    }
    const uint32_t n_arp = rd32();
    std::set<uint32_t> arp_ips;
    for (uint32_t i = 0; i < n_arp; ++i) {
        const uint32_t ip = rd32();
        arp_ips.insert(ip);
        uint8_t m[8];
        if (!rd(m, 8)) return 2;
        uint8_t f[42] = {0};  // an ARP reply from (ip, mac): process_arp_packet learns its sender
        memset(f, 0xFF, 6);
        memcpy(f + 6, m, 6);
        f[12] = 0x08; f[13] = 0x06;
        f[14] = 0; f[15] = 1; f[16] = 0x08; f[17] = 0x00; f[18] = 6; f[19] = 4; f[20] = 0; f[21] = 2;
        memcpy(f + 22, m, 6);
        memcpy(f + 28, &ip, 4);
        netflow::Packet pkt(buffer_of(f, sizeof f));
        sw.arp_processor_.process_arp_packet(pkt, ingress);
    }
    std::set<uint32_t> extra;
    for (uint32_t i = rd32(); i > 0; --i) extra.insert(rd32());

    // what the reference's managers hold
    const auto cfgs = sw.interface_manager_.get_all_port_configs();
    wr32((uint32_t)cfgs.size());
    for (const auto& kv : cfgs) {
        wr32(kv.first);
        const uint8_t f[4] = {(uint8_t)(sw.interface_manager_.is_port_link_up(kv.first) ? 1 : 0), 0, 0, 0};
        uint8_t m[8] = {0};
        memcpy(m, kv.second.mac_address.bytes, 6);
        wr(f, 4);
        wr(m, 8);
        wr32((uint32_t)kv.second.ip_configurations.size());
        for (const auto& c : kv.second.ip_configurations) wr32(c.address);
    }
    const std::vector<netflow::RouteEntry> table = sw.routing_manager_.get_routing_table();
    wr32((uint32_t)table.size());
    for (const netflow::RouteEntry& e : table) {
        wr32(e.destination_network);
        wr32(e.subnet_mask);
        wr32(e.next_hop_ip);
        wr32(e.egress_interface_id);
    }
    wr32((uint32_t)arp_ips.size());  // the cache has no public reader either: lookup_mac per address fed
    for (const uint32_t ip : arp_ips) {
        const std::optional<netflow::MacAddress> mac = sw.arp_processor_.lookup_mac(ip);
        if (!mac) return 7;
        uint8_t m[8] = {0};
        memcpy(m, mac->bytes, 6);
        wr32(ip);
        wr(m, 8);
    }

    srand(seed);
    const uint32_t nf = rd32();
    std::vector<uint8_t> frame;
    for (uint32_t i = 0; i < nf; ++i) {
        const uint32_t len = rd32();
        frame.resize(len);
        if (!rd(frame.data(), len)) return 2;
        netflow::Packet pkt(buffer_of(frame.data(), len));
        uint32_t verdict = RT_OTHER, status = ST_NONE;
        sent.clear();
        // switch.hpp:250-301
        const netflow::EthernetHeader* eth = pkt.ethernet();
        uint16_t l3_type = eth ? ntohs(eth->ethertype) : 0;
        if (l3_type == netflow::ETHERTYPE_VLAN)
            if (const netflow::VlanHeader* tag = pkt.vlan()) l3_type = ntohs(tag->ethertype);
        netflow::IPv4Header* ip = l3_type == netflow::ETHERTYPE_IPV4 ? pkt.ipv4() : nullptr;
        if (ip) {
            const size_t l2 = (const uint8_t*)ip - pkt.get_buffer()->get_data_start_ptr();
            if (l2 + ip->get_header_length() > len) return 5;  // not a frame for this fixture
            auto after_resolve = [&](uint32_t ok) {
                // icmp_processor.cpp:212-251 in its order, through the accessors it calls
                const auto route = sw.routing_manager_.lookup_route(ip->src_ip);
                if (!route) return (uint32_t)ST_SRC_NO_ROUTE;
                if (!sw.interface_manager_.get_interface_ip(route->egress_interface_id)) return (uint32_t)ST_SRC_NO_IF_IP;
                if (!sw.arp_processor_.lookup_mac(route->next_hop_ip == 0 ? ip->src_ip : route->next_hop_ip))
                    return (uint32_t)ST_SRC_ARP_MISS;
                if (!sw.interface_manager_.get_interface_mac(route->egress_interface_id)) return (uint32_t)ST_SRC_NO_IF_MAC;
                return ok;
            };
            if (sw.interface_manager_.is_my_ip(ip->dst_ip) || extra.count(ip->dst_ip)) {
                verdict = RT_LOCAL;
                if (ip->protocol != netflow::IPPROTO_ICMP) status = ST_TO_CPU;
                else {
                    const netflow::IcmpHeader* ic = pkt.icmp();
                    if (!ic || ic->type != netflow::IcmpHeader::TYPE_ECHO_REQUEST || ic->code != 0) status = ST_IGNORED;
                    else if (!sw.interface_manager_.is_my_ip(ip->dst_ip) || !sw.interface_manager_.get_mac_for_ip(ip->dst_ip))
                        status = ST_NO_LOCAL_MAC;
                    else if (ntohs(ip->total_length) < ip->get_header_length() + netflow::IcmpHeader::MIN_SIZE) status = ST_IGNORED;
                    else status = ST_ECHO;
                    sw.icmp_processor_.process_icmp_packet(pkt, ingress);
                }
            } else if (ip->ttl <= 1) {
                verdict = RT_TTL;
                status = after_resolve(ST_TIME);
                sw.icmp_processor_.send_time_exceeded(pkt, ingress);
            } else if (!sw.routing_manager_.lookup_route(ip->dst_ip)) {
                verdict = RT_NO_ROUTE;
                status = after_resolve(ST_UNREACH);
                sw.icmp_processor_.send_destination_unreachable(pkt, ingress, 0);
            }
        }
        if (sent.size() > 1) return 4;
        const bool would = status == ST_ECHO || status == ST_TIME || status == ST_UNREACH;
        if (!would && !sent.empty()) return 6;  // the probe's reading of the reference's order is wrong
        if (would && sent.empty()) status = ST_PORT_DOWN;
        wr32(verdict);
        wr32(status);
        wr32((uint32_t)sent.size());
        wr32(sent.empty() ? 0xFFFFFFFFu : sent[0].port);
        wr32(sent.empty() ? 0u : (uint32_t)sent[0].bytes.size());
        if (!sent.empty()) wr(sent[0].bytes.data(), sent[0].bytes.size());
    }
    return fclose(g_out) == 0 ? 0 : 3;
}

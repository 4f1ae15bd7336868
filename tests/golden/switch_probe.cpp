// switch_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_switch_golden.py).
//
// Constructs a real netflow::Switch, configures it through its managers' own setters and feeds it bursts of
// frames through Switch::process_received_packet (switch.hpp:213-329), so that process_egress_pipeline (113-139)
// and flood_packet (174-206) run as the reference wrote them: nothing of the pipeline is restated here. After
// each burst every port's TX loop runs QosManager::select_packet_to_dequeue up to that port's budget.
//   interfaces   InterfaceManager::configure_port / add_ip_address / simulate_port_link_up / _down
//   VLAN, QoS    VlanManager::configure_port, QosManager::configure_port_qos
//   routes, ARP  RoutingManager::add_static_route; ArpProcessor::process_arp_packet on ARP replies (its cache
//                has no public setter)
//   FDB          ForwardingDatabase::learn_mac / add_static_entry
//   ACLs         AclManager::create_acl / add_rule / compile_rules, InterfaceManager::apply_acl_to_interface
//   STP          the reference's StpManager starts every port BLOCKING and its bodies that would change that are
//                placeholders, so its switch never forwards or floods an L2 frame. The probe sets the state
//                field of StpManager's own per-port record to FORWARDING for the ports named so (the member is
//                private; it is reached through an explicit template instantiation, which may name it).
//                get_port_stp_state, which the switch asks, then answers from that record as always.
// Per frame the probe also says where the reference stops (`code`), by asking the reference's accessors in
// switch.hpp's order BEFORE the frame is processed, and what the switch then did, read from the reference's own
// counters before and after the call: one event per enqueue, tail drop or egress deny. A code that sends nothing
// with events, or a unicast code with more than one, ends the probe (exit 6): its reading of the order would be
// wrong. A dequeued packet is traced to its source frame by the marker the generator plants in the last four
// bytes of every frame (flood copies are the switch's own buffers). Links against src/netflow++/*.cpp without
// isis/; the binary goes to oracle/_ref/ (git-ignored). Run it in an empty directory (the constructor looks for
// default_switch_config.json). The loggers print to stdout, so the results go to the file named by argv[1].
//
// A rule record: the 56 bytes of tests/golden/acl_probe.cpp (nfcs_acl_rule, then i32 priority).
// stdin (little-endian):
//   u32 num_ports
//   u32 n_if, n_if x {u32 id, u8 link_up, u8 stp_forwarding, u8 pad[2], mac[6], u8 pad[2], u32 n_ip, n_ip x u32 ip}
//   u32 n_vlan, n_vlan x {u32 id, u8 type, u8 tag_native, u16 native, u32 n_allowed, n_allowed x u16 (padded to 4)}
//   u32 n_qos, n_qos x {u32 id, u8 num_queues, u8 scheduler, u8 pad[2], u32 max_queue_depth}
//   u32 n_routes, n_routes x {net, mask, next_hop, if}
//   u32 n_arp, n_arp x {u32 ip, mac[6], u8 pad[2]}
//   u32 n_fdb, n_fdb x {u8 kind (0 learn_mac, 1 add_static_entry), u8 pad, mac[6], u16 vlan, u16 pad, u32 port}
//   u32 n_lists, n_lists x {u32 list id, u32 nr, nr x record}
//   u32 n_bind, n_bind x {u32 port, u32 direction (0 ingress, 1 egress), u32 list id}
//   u32 n_bursts, n_bursts x {u32 ingress, u32 nf, num_ports x u32 budget, nf x {u32 len, bytes}}
// argv[1] (little-endian):
//   u32 n_if, n_if x {u32 id, u8 link_up, u8 stp_forwarding, u8 pad[2], mac[6], u8 pad[2], u32 ingress list id or
//        0xFFFFFFFF, u32 egress list id or 0xFFFFFFFF, u32 n_ip, n_ip x u32 ip}   get_all_port_configs,
//        is_port_link_up, get_port_stp_state, get_applied_acl_name
//   num_ports x {u8 has, u8 type, u8 tag_native, u8 pad, u16 native, u16 n_allowed, n_allowed x u16 (padded to 4)}
//        VlanManager::get_port_config
//   num_ports x {u8 has, u8 num_queues, u8 scheduler, u8 pad, u32 max_queue_depth}   get_port_qos_config
//   u32 n_routes, n_routes x {net, mask, next_hop, if}                               get_routing_table
//   u32 n_arp, n_arp x {u32 ip, mac[6], u8 pad[2]}                      lookup_mac per distinct address fed
//   u32 ne, ne x {mac[6], u16 vlan_id, u32 port, u8 is_static, u8 pad[3]}            get_all_entries
//   n_lists x {u32 list id, u32 nt, nt x record}                                     get_all_rules
//   per burst:
//     nf x {u32 code, u32 port or 0xFFFFFFFF, u32 1 if the frame parses as IPv4, u32 action of the egress port's
//           list on the frame as the switch left it (unicast codes; 0xFFFFFFFF otherwise or without a list),
//           u32 n_events, n_events x u32 (kind << 16 | port << 8 | queue; kind 0 enqueued, 1 tail drop, 2 egress deny)}
//     num_ports x {u32 count, count x {u32 source frame (the marker), u32 len, len bytes}}   the TX loops
//     num_ports x 8 x {u32 packets_enqueued, u32 packets_dropped_full, u32 current_depth} (0xFFFFFFFF x 3 where
//           get_queue_stats returns nullopt), after the TX loops, cumulative
//     num_ports x {u64 rx_packets, rx_bytes, rx_drops, tx_packets, tx_bytes, tx_drops}       get_port_stats
#include <netflow++/switch.hpp>

#include <arpa/inet.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <set>
#include <string>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
enum : uint32_t { C_UNHANDLED = 0, C_RX_DOWN, C_IN_DENY, C_RED_OK, C_RED_DOWN, C_RED_RANGE, C_LLDP, C_ZERO_MAC, C_ARP,
                  C_LOCAL, C_TTL, C_NO_ROUTE, C_ARP_MISS, C_NO_IF_MAC, C_L3_FWD, C_L2_FWD, C_L2_FLOOD, C_SAME_PORT,
                  C_LINK_DOWN, C_STP, C_VLAN };
enum : uint32_t { EV_ENQ = 0, EV_FULL = 1, EV_EDENY = 2 };

#pragma pack(push, 1)
struct Rec {
    uint32_t fields, rule_id;
    uint8_t src_mac[6], dst_mac[6];
    uint16_t vlan_id, ethertype;
    uint32_t src_ip, dst_ip, unused[2];
    uint16_t src_port, dst_port;
    uint8_t protocol, action, pad[2];
    uint32_t redirect_port;
    int32_t priority;
};
#pragma pack(pop)
static_assert(sizeof(Rec) == 56, "record layout");

// StpManager::port_stp_info_ is private and has no setter; an explicit instantiation may name it.
using StpMap = std::map<uint32_t, netflow::StpManager::StpPortInfo>;
StpMap netflow::StpManager::* stp_ports_member();
template <StpMap netflow::StpManager::* M>
struct StpAccess {
    friend StpMap netflow::StpManager::* stp_ports_member() { return M; }
};
template struct StpAccess<&netflow::StpManager::port_stp_info_>;

FILE* g_out = nullptr;
bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
void wr(const void* p, size_t n) { if (n) fwrite(p, 1, n, g_out); }
uint32_t rd32() { uint32_t v = 0; rd(&v, 4); return v; }
uint16_t rd16() { uint16_t v = 0; rd(&v, 2); return v; }
void wr32(uint32_t v) { wr(&v, 4); }
void wr16(uint16_t v) { wr(&v, 2); }
void wr64(uint64_t v) { wr(&v, 8); }

netflow::AclRule to_rule(const Rec& r) {
    netflow::AclRule a(r.rule_id, r.priority, static_cast<netflow::AclActionType>(r.action));
    if (r.fields & 1u) a.src_mac = netflow::MacAddress(r.src_mac);
    if (r.fields & 2u) a.dst_mac = netflow::MacAddress(r.dst_mac);
    if (r.fields & 4u) a.vlan_id = r.vlan_id;
    if (r.fields & 8u) a.ethertype = r.ethertype;
    if (r.fields & 16u) a.src_ip = r.src_ip;
    if (r.fields & 32u) a.dst_ip = r.dst_ip;
    if (r.fields & 64u) a.protocol = r.protocol;
    if (r.fields & 128u) a.src_port = r.src_port;
    if (r.fields & 256u) a.dst_port = r.dst_port;
    if (r.redirect_port != NONE) a.redirect_port_id = r.redirect_port;
    return a;
}

Rec from_rule(const netflow::AclRule& a) {
    Rec r;
    memset(&r, 0, sizeof r);
    r.rule_id = a.rule_id;
    r.priority = a.priority;
    r.action = (uint8_t)static_cast<int>(a.action);
    if (a.src_mac) { r.fields |= 1u; memcpy(r.src_mac, a.src_mac->bytes, 6); }
    if (a.dst_mac) { r.fields |= 2u; memcpy(r.dst_mac, a.dst_mac->bytes, 6); }
    if (a.vlan_id) { r.fields |= 4u; r.vlan_id = *a.vlan_id; }
    if (a.ethertype) { r.fields |= 8u; r.ethertype = *a.ethertype; }
    if (a.src_ip) { r.fields |= 16u; r.src_ip = *a.src_ip; }
    if (a.dst_ip) { r.fields |= 32u; r.dst_ip = *a.dst_ip; }
    if (a.protocol) { r.fields |= 64u; r.protocol = *a.protocol; }
    if (a.src_port) { r.fields |= 128u; r.src_port = *a.src_port; }
    if (a.dst_port) { r.fields |= 256u; r.dst_port = *a.dst_port; }
    r.redirect_port = a.redirect_port_id ? *a.redirect_port_id : NONE;
    return r;
}

std::string list_name(uint32_t id) { return "list" + std::to_string(id); }
uint32_t list_id(const std::optional<std::string>& name) {
    return name.has_value() && name->size() > 4 ? (uint32_t)atoi(name->c_str() + 4) : NONE;
}

struct Counters { uint64_t enq[64][8], full[64][8], tx_drops[64]; };

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    const uint32_t num_ports = rd32();
    if (num_ports > 64) return 2;
    std::vector<std::unique_ptr<netflow::PacketBuffer>> bufs;  // declared before the switch: its queues refer to them
    netflow::Switch sw(num_ports, 0x02AA00000001ull);
    sw.logger_.set_min_log_level(netflow::LogLevel::CRITICAL);
    auto buffer_of = [&](const uint8_t* data, size_t len) {
        bufs.push_back(std::make_unique<netflow::PacketBuffer>(len + 16, 0, len));
        memset(bufs.back()->get_data_start_ptr(), 0, len + 16);
        memcpy(bufs.back()->get_data_start_ptr(), data, len);
        return bufs.back().get();
    };

    // ---- configuration, through the managers' own setters
    const uint32_t n_if = rd32();
    for (uint32_t i = 0; i < n_if; ++i) {
        const uint32_t id = rd32();
        uint8_t f[4], m[8];
        if (!rd(f, 4) || !rd(m, 8)) return 2;
        netflow::InterfaceManager::PortConfig cfg;
        cfg.admin_up = f[0] != 0;
        cfg.mac_address = netflow::MacAddress(m);
        sw.interface_manager_.configure_port(id, cfg);
        for (uint32_t k = rd32(); k > 0; --k) sw.interface_manager_.add_ip_address(id, rd32(), htonl(0xFFFFFF00u));
        if (f[0]) sw.interface_manager_.simulate_port_link_up(id);
        else sw.interface_manager_.simulate_port_link_down(id);
        if (f[1]) {
            StpMap& ports = sw.stp_manager.*stp_ports_member();
            const auto it = ports.find(id);
            if (it != ports.end()) it->second.state = netflow::StpManager::PortState::FORWARDING;
        }
    }
    for (uint32_t i = rd32(); i > 0; --i) {
        const uint32_t id = rd32();
        uint8_t f[2];
        if (!rd(f, 2)) return 2;
        netflow::VlanManager::PortConfig cfg;
        cfg.type = static_cast<netflow::PortType>(f[0]);
        cfg.tag_native = f[1] != 0;
        cfg.native_vlan = rd16();
        cfg.allowed_vlans.clear();
        const uint32_t n_allowed = rd32();
        for (uint32_t k = 0; k < n_allowed; ++k) cfg.allowed_vlans.insert(rd16());
        if (n_allowed & 1u) rd16();
        sw.vlan_manager.configure_port(id, cfg);
    }
    for (uint32_t i = rd32(); i > 0; --i) {
        const uint32_t id = rd32();
        uint8_t f[4];
        if (!rd(f, 4)) return 2;
        netflow::QosConfig qc;
        qc.num_queues = f[0];
        qc.scheduler = static_cast<netflow::SchedulerType>(f[1]);
        qc.max_queue_depth = rd32();
        sw.qos_manager_.configure_port_qos(id, qc);
    }
    for (uint32_t i = rd32(); i > 0; --i) {
        uint32_t r[4];
        if (!rd(r, sizeof r)) return 2;
        sw.routing_manager_.add_static_route(r[0], r[1], r[2], r[3], 1);
    }
    std::set<uint32_t> arp_ips;
    for (uint32_t i = rd32(); i > 0; --i) {
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
        sw.arp_processor_.process_arp_packet(pkt, 0);
    }
    for (uint32_t i = rd32(); i > 0; --i) {
        uint8_t kind_pad[2], mac[6];
        if (!rd(kind_pad, 2) || !rd(mac, 6)) return 2;
        const uint16_t vlan = rd16();
        rd16();
        const uint32_t port = rd32();
        if (kind_pad[0] == 1) sw.fdb.add_static_entry(netflow::MacAddress(mac), port, vlan);
        else sw.fdb.learn_mac(netflow::MacAddress(mac), port, vlan);
    }
    std::vector<uint32_t> lists(rd32());
    for (uint32_t& id : lists) {
        id = rd32();
        const uint32_t nr = rd32();
        if (!sw.acl_manager_.create_acl(list_name(id))) return 2;
        for (uint32_t i = 0; i < nr; ++i) {
            Rec r;
            if (!rd(&r, sizeof r)) return 2;
            if (!sw.acl_manager_.add_rule(list_name(id), to_rule(r))) return 2;
        }
        sw.acl_manager_.compile_rules(list_name(id));
    }
    for (uint32_t i = rd32(); i > 0; --i) {
        const uint32_t port = rd32(), dir = rd32(), id = rd32();
        if (!sw.interface_manager_.apply_acl_to_interface(
                port, list_name(id), dir ? netflow::AclDirection::EGRESS : netflow::AclDirection::INGRESS))
            return 2;
    }

    // ---- what the reference's managers hold
    auto stp_forwarding = [&](uint32_t p) {
        return sw.stp_manager.get_port_stp_state(p) == netflow::StpManager::PortState::FORWARDING;
    };
    const auto cfgs = sw.interface_manager_.get_all_port_configs();
    wr32((uint32_t)cfgs.size());
    for (const auto& kv : cfgs) {
        wr32(kv.first);
        const uint8_t f[4] = {(uint8_t)(sw.interface_manager_.is_port_link_up(kv.first) ? 1 : 0),
                              (uint8_t)(stp_forwarding(kv.first) ? 1 : 0), 0, 0};
        uint8_t m[8] = {0};
        memcpy(m, kv.second.mac_address.bytes, 6);
        wr(f, 4);
        wr(m, 8);
        wr32(list_id(sw.interface_manager_.get_applied_acl_name(kv.first, netflow::AclDirection::INGRESS)));
        wr32(list_id(sw.interface_manager_.get_applied_acl_name(kv.first, netflow::AclDirection::EGRESS)));
        wr32((uint32_t)kv.second.ip_configurations.size());
        for (const auto& c : kv.second.ip_configurations) wr32(c.address);
    }
    for (uint32_t p = 0; p < num_ports; ++p) {
        const auto c = sw.vlan_manager.get_port_config(p);
        const uint8_t f[4] = {(uint8_t)(c ? 1 : 0), (uint8_t)(c ? static_cast<int>(c->type) : 0),
                              (uint8_t)(c && c->tag_native ? 1 : 0), 0};
        wr(f, 4);
        wr16(c ? c->native_vlan : 0);
        const uint16_t n_allowed = c ? (uint16_t)c->allowed_vlans.size() : 0;
        wr16(n_allowed);
        if (c) for (const uint16_t v : c->allowed_vlans) wr16(v);
        if (n_allowed & 1u) wr16(0);
    }
    for (uint32_t p = 0; p < num_ports; ++p) {
        const auto c = sw.qos_manager_.get_port_qos_config(p);
        const uint8_t f[4] = {(uint8_t)(c ? 1 : 0), (uint8_t)(c ? c->num_queues : 0),
                              (uint8_t)(c ? static_cast<int>(c->scheduler) : 0), 0};
        wr(f, 4);
        wr32(c ? c->max_queue_depth : 0);
    }
    const std::vector<netflow::RouteEntry> table = sw.routing_manager_.get_routing_table();
    wr32((uint32_t)table.size());
    for (const netflow::RouteEntry& e : table) {
        wr32(e.destination_network);
        wr32(e.subnet_mask);
        wr32(e.next_hop_ip);
        wr32(e.egress_interface_id);
    }
    wr32((uint32_t)arp_ips.size());
    for (const uint32_t ip : arp_ips) {
        const std::optional<netflow::MacAddress> mac = sw.arp_processor_.lookup_mac(ip);
        if (!mac) return 7;
        uint8_t m[8] = {0};
        memcpy(m, mac->bytes, 6);
        wr32(ip);
        wr(m, 8);
    }
    const std::vector<netflow::FdbEntry>& all = sw.fdb.get_all_entries();
    wr32((uint32_t)all.size());
    for (const netflow::FdbEntry& e : all) {
        uint8_t rec[16] = {0};
        memcpy(rec, e.mac.bytes, 6);
        memcpy(rec + 6, &e.vlan_id, 2);
        memcpy(rec + 8, &e.port, 4);
        rec[12] = e.is_static ? 1 : 0;
        wr(rec, 16);
    }
    for (const uint32_t id : lists) {
        const std::vector<netflow::AclRule> rules = sw.acl_manager_.get_all_rules(list_name(id));
        wr32(id);
        wr32((uint32_t)rules.size());
        for (const netflow::AclRule& a : rules) {
            const Rec r = from_rule(a);
            wr(&r, sizeof r);
        }
    }

    auto snapshot = [&](Counters& c) {
        for (uint32_t p = 0; p < num_ports; ++p) {
            c.tx_drops[p] = sw.interface_manager_.get_port_stats(p).tx_drops;
            for (uint32_t q = 0; q < 8; ++q) {
                const auto s = sw.qos_manager_.get_queue_stats(p, (uint8_t)q);
                c.enq[p][q] = s ? s->packets_enqueued : 0;
                c.full[p][q] = s ? s->packets_dropped_full : 0;
            }
        }
    };
    auto egress_action = [&](const netflow::Packet& pkt, uint32_t port) {
        const auto name = sw.interface_manager_.get_applied_acl_name(port, netflow::AclDirection::EGRESS);
        if (!name.has_value() || name->empty()) return NONE;
        uint32_t unused = 0;
        return (uint32_t)static_cast<int>(sw.acl_manager_.evaluate(*name, pkt, unused));
    };

    // ---- the bursts
    const uint32_t n_bursts = rd32();
    std::vector<uint8_t> frame;
    for (uint32_t b = 0; b < n_bursts; ++b) {
        const uint32_t ingress = rd32(), nf = rd32();
        std::vector<uint32_t> budget(num_ports);
        for (uint32_t& x : budget) x = rd32();
        for (uint32_t i = 0; i < nf; ++i) {
            const uint32_t len = rd32();
            frame.resize(len);
            if (!rd(frame.data(), len)) return 2;
            netflow::PacketBuffer* pb = buffer_of(frame.data(), len);
            uint32_t code = C_UNHANDLED, port = NONE, is_v4 = 0, eg_action = NONE;
            {
                // where switch.hpp:213-329 stops, asked of the reference's accessors in its order
                netflow::Packet pkt(pb);
                const netflow::EthernetHeader* eth = pkt.ethernet();
                const uint16_t l2_type = eth ? ntohs(eth->ethertype) : 0;
                uint16_t l3_type = l2_type;
                if (l2_type == netflow::ETHERTYPE_VLAN)
                    if (const netflow::VlanHeader* tag = pkt.vlan()) l3_type = ntohs(tag->ethertype);
                netflow::IPv4Header* ip = l3_type == netflow::ETHERTYPE_IPV4 ? pkt.ipv4() : nullptr;
                is_v4 = ip ? 1 : 0;
                netflow::AclActionType action = netflow::AclActionType::PERMIT;
                uint32_t redirect = 0;
                const auto in_name = sw.interface_manager_.get_applied_acl_name(ingress, netflow::AclDirection::INGRESS);
                if (in_name.has_value() && !in_name->empty()) action = sw.acl_manager_.evaluate(*in_name, pkt, redirect);
                if (!sw.interface_manager_.is_port_link_up(ingress)) code = C_RX_DOWN;
                else if (action == netflow::AclActionType::DENY) code = C_IN_DENY;
                else if (action == netflow::AclActionType::REDIRECT) {
                    port = redirect;
                    code = redirect >= num_ports ? C_RED_RANGE
                                                 : !sw.interface_manager_.is_port_link_up(redirect) ? C_RED_DOWN : C_RED_OK;
                } else if (eth && l2_type == netflow::LLDP_ETHERTYPE) code = C_LLDP;
                else if (eth && eth->dst_mac == netflow::MacAddress()) code = C_ZERO_MAC;
                else if (l3_type == netflow::ETHERTYPE_ARP) code = C_ARP;
                else if (ip) {
                    if (sw.interface_manager_.is_my_ip(ip->dst_ip)) code = C_LOCAL;
                    else if (ip->ttl <= 1) code = C_TTL;
                    else {
                        const auto route = sw.routing_manager_.lookup_route(ip->dst_ip);
                        if (!route) code = C_NO_ROUTE;
                        else if (!sw.arp_processor_.lookup_mac(route->next_hop_ip == 0 ? ip->dst_ip : route->next_hop_ip))
                            code = C_ARP_MISS;
                        else if (!sw.interface_manager_.get_interface_mac(route->egress_interface_id)) code = C_NO_IF_MAC;
                        else { code = C_L3_FWD; port = route->egress_interface_id; }
                    }
                } else if (eth && pkt.dst_mac().has_value()) {
                    const uint16_t vlan = pkt.vlan_id().value_or(
                        sw.vlan_manager.get_port_config(ingress).value_or(netflow::VlanManager::PortConfig()).native_vlan);
                    const std::optional<uint32_t> hit = sw.fdb.lookup_port(pkt.dst_mac().value(), vlan);
                    if (!hit) code = C_L2_FLOOD;
                    else if (*hit == ingress) code = C_SAME_PORT;
                    else if (!sw.interface_manager_.is_port_link_up(*hit)) code = C_LINK_DOWN;
                    else if (!stp_forwarding(*hit)) code = C_STP;
                    else if (!sw.vlan_manager.should_forward(ingress, *hit, vlan)) code = C_VLAN;
                    else { code = C_L2_FWD; port = *hit; }
                }
            }
            Counters before, after;
            snapshot(before);
            sw.process_received_packet(ingress, pb);
            snapshot(after);
            std::vector<uint32_t> events;
            for (uint32_t p = 0; p < num_ports; ++p) {
                for (uint64_t k = before.tx_drops[p]; k < after.tx_drops[p]; ++k) events.push_back(EV_EDENY << 16 | p << 8);
                for (uint32_t q = 0; q < 8; ++q) {
                    for (uint64_t k = before.enq[p][q]; k < after.enq[p][q]; ++k) events.push_back(EV_ENQ << 16 | p << 8 | q);
                    for (uint64_t k = before.full[p][q]; k < after.full[p][q]; ++k) events.push_back(EV_FULL << 16 | p << 8 | q);
                }
            }
            const bool unicast = code == C_RED_OK || code == C_L3_FWD || code == C_L2_FWD;
            if (unicast) {
                netflow::Packet pkt(pb);
                eg_action = egress_action(pkt, port);
                if (events.size() > 1 || (events.size() == 1 && ((events[0] >> 8) & 0xFF) != port)) return 6;
            } else if (code != C_L2_FLOOD && !events.empty()) {
                return 6;
            }
            wr32(code);
            wr32(port);
            wr32(is_v4);
            wr32(eg_action);
            wr32((uint32_t)events.size());
            wr(events.data(), events.size() * 4);
        }
        for (uint32_t p = 0; p < num_ports; ++p) {
            std::vector<uint8_t> out;
            uint32_t count = 0;
            for (uint32_t k = 0; k < budget[p]; ++k) {
                auto pkt = sw.qos_manager_.select_packet_to_dequeue(p);
                if (!pkt) break;
                const netflow::PacketBuffer* pb = pkt->get_buffer();
                const uint32_t len = (uint32_t)pb->get_data_length();
                const uint8_t* d = pb->get_data_start_ptr();
                uint32_t src = NONE;
                if (len >= 4) memcpy(&src, d + len - 4, 4);
                const uint8_t* h[2] = {(const uint8_t*)&src, (const uint8_t*)&len};
                out.insert(out.end(), h[0], h[0] + 4);
                out.insert(out.end(), h[1], h[1] + 4);
                out.insert(out.end(), d, d + len);
                ++count;
            }
            wr32(count);
            wr(out.data(), out.size());
        }
        for (uint32_t p = 0; p < num_ports; ++p)
            for (uint32_t q = 0; q < 8; ++q) {
                const auto s = sw.qos_manager_.get_queue_stats(p, (uint8_t)q);
                wr32(s ? (uint32_t)s->packets_enqueued : NONE);
                wr32(s ? (uint32_t)s->packets_dropped_full : NONE);
                wr32(s ? (uint32_t)s->current_depth : NONE);
            }
        for (uint32_t p = 0; p < num_ports; ++p) {
            const netflow::InterfaceManager::PortStats s = sw.interface_manager_.get_port_stats(p);
            wr64(s.rx_packets); wr64(s.rx_bytes); wr64(s.rx_drops);
            wr64(s.tx_packets); wr64(s.tx_bytes); wr64(s.tx_drops);
        }
    }
    return fclose(g_out) == 0 ? 0 : 3;
}

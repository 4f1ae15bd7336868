// egress_acl_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_egress_acl_golden.py).
//
// Walks Switch::process_egress_pipeline (switch.hpp:113-139) WITH its egress ACL over a list of (frame,
// egress port) pairs, with the reference's own objects: the lists go through AclManager::create_acl / add_rule
// / compile_rules (and delete_acl for a list marked deleted, after it was bound); the ports through
// InterfaceManager::configure_port and apply_acl_to_interface(port, name, EGRESS), VlanManager::configure_port
// and QosManager::configure_port_qos. The few lines that join them are written afresh here, per pair in order:
//   egress VLAN    VlanManager::process_egress(pkt, port)
//   applied name   InterfaceManager::get_applied_acl_name(port, EGRESS); absent or empty: no ACL
//   evaluate       AclManager::evaluate(name, pkt, redirect); DENY: _increment_tx_stats(port, length, false,
//                  true) and the packet is gone
//   enqueue        otherwise QosManager::enqueue_packet(pkt, port)
// evaluate() does not say which rule decided, so — as tests/golden/acl_probe.cpp does — every rule also
// stands alone in a single-rule ACL deciding DENY, and the probe reports the first rule of the port's list, in
// get_all_rules() order, whose single-rule ACL answers DENY; it fails (exit 4) unless evaluate()'s action and
// port are what that rule implies. Besides, the same list is evaluated on an un-popped copy of the frame.
// Compiled against the reference's headers in place plus src/netflow++/acl_manager.cpp,
// interface_manager.cpp, vlan_manager.cpp and qos_manager.cpp; the binary goes to oracle/_ref/ (git-ignored).
// The logger is set to CRITICAL; the results go to the file named by argv[1], not to stdout, where the
// logger would write.
//
// A rule record: the 56 bytes of tests/golden/acl_probe.cpp (nfcs_acl_rule, then i32 priority).
// stdin (little-endian):
//   u32 n_lists, n_lists x {u32 list id, u32 compile, u32 deleted, u32 nr, nr x record}
//   u32 n_ports, n_ports x {nfcs_egress_port (16 bytes: u32 port_id, u8 has_vlan_config, u8 type, u8 tag_native,
//                           u8 has_qos, u16 native_vlan, u8 num_queues, u8 pad, u32 depth), u32 bound list id or
//                           0xFFFFFFFF}
//   u32 num_ports (the port ids the per-port outputs cover: 0..num_ports-1)
//   u32 np, np x {u32 port, u32 len, bytes}
// argv[1] (little-endian):
//   n_lists x {u32 nt, nt x record}   get_all_rules() order, before any delete_acl
//   np x {u32 action (REDIRECT without a port arrives as DENY), u32 index of the deciding rule in the port's
//         list or 0xFFFFFFFF, u32 redirect port or 0xFFFFFFFF, u32 length after process_egress, u32 action of
//         the same list on the un-popped copy, u32 1 when enqueue_packet was called,
//         u32 classify_packet_to_queue(pkt, port) on the frame after process_egress}
//   num_ports x {u64 tx_packets, u64 tx_bytes, u64 tx_drops}   get_port_stats
//   num_ports x 8 x {u32 packets_enqueued, u32 packets_dropped_full, u32 current_depth} (0xFFFFFFFF x 3 where
//         get_queue_stats returns nullopt)
//   num_ports x 8 x {u32 count, count x {u32 pair index, u32 len, 64 bytes of the frame (zero padded)}}
//         dequeue_packet(port, queue) until it returns nullopt
#include <netflow++/acl_manager.hpp>
#include <netflow++/interface_manager.hpp>
#include <netflow++/logger.hpp>
#include <netflow++/packet.hpp>
#include <netflow++/qos_manager.hpp>
#include <netflow++/vlan_manager.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;

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
struct PortRec {
    uint32_t id;
    uint8_t has_vlan, type, tag_native, has_qos;
    uint16_t native;
    uint8_t queues, pad;
    uint32_t depth, list;
};
#pragma pack(pop)
static_assert(sizeof(Rec) == 56 && sizeof(PortRec) == 20, "record layouts");

FILE* g_out = nullptr;
bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
void wr(const void* p, size_t n) { if (n) fwrite(p, 1, n, g_out); }
uint32_t rd32() { uint32_t v = 0; rd(&v, 4); return v; }
void wr32(uint32_t v) { wr(&v, 4); }
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
std::string alone_name(uint32_t id, size_t k) { return "list" + std::to_string(id) + "_rule" + std::to_string(k); }

struct Pair { uint32_t port; std::unique_ptr<netflow::PacketBuffer> pb, raw; };

std::unique_ptr<netflow::PacketBuffer> buffer_of(const uint8_t* data, uint32_t len) {
    auto pb = std::make_unique<netflow::PacketBuffer>(len + 16, 0, len);
    memset(pb->get_data_start_ptr(), 0, len + 16);
    memcpy(pb->get_data_start_ptr(), data, len);
    return pb;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    netflow::SwitchLogger logger(netflow::LogLevel::CRITICAL);
    netflow::AclManager acl(logger);
    netflow::InterfaceManager ifm(logger, acl);
    netflow::VlanManager vm;
    std::vector<Pair> pairs;  // declared before the QosManager: its queues refer to these buffers
    {
        netflow::QosManager qos(logger);
        // the lists; what get_all_rules() returns is kept, since a deleted list no longer answers
        std::map<uint32_t, std::vector<netflow::AclRule>> rules_of;
        std::vector<uint32_t> to_delete;
        const uint32_t n_lists = rd32();
        for (uint32_t l = 0; l < n_lists; ++l) {
            const uint32_t id = rd32(), compile = rd32(), deleted = rd32(), nr = rd32();
            if (!acl.create_acl(list_name(id))) return 2;
            for (uint32_t i = 0; i < nr; ++i) {
                Rec r;
                if (!rd(&r, sizeof r)) return 2;
                if (!acl.add_rule(list_name(id), to_rule(r))) return 2;
            }
            if (compile) acl.compile_rules(list_name(id));
            const std::vector<netflow::AclRule> rules = acl.get_all_rules(list_name(id));
            wr32((uint32_t)rules.size());
            for (size_t k = 0; k < rules.size(); ++k) {
                const Rec r = from_rule(rules[k]);
                wr(&r, sizeof r);
                netflow::AclRule alone = rules[k];  // the rule alone, deciding DENY
                alone.action = netflow::AclActionType::DENY;
                alone.redirect_port_id.reset();
                acl.create_acl(alone_name(id, k));
                acl.add_rule(alone_name(id, k), alone);
            }
            rules_of[id] = rules;
            if (deleted) to_delete.push_back(id);
        }
        // the ports
        std::map<uint32_t, uint32_t> bound;
        const uint32_t n_ports = rd32();
        for (uint32_t i = 0; i < n_ports; ++i) {
            PortRec p;
            if (!rd(&p, sizeof p)) return 2;
            netflow::InterfaceManager::PortConfig pc;
            pc.admin_up = true;
            ifm.configure_port(p.id, pc);
            if (p.list != NONE) {
                if (!ifm.apply_acl_to_interface(p.id, list_name(p.list), netflow::AclDirection::EGRESS)) return 2;
                bound[p.id] = p.list;
            }
            if (p.has_vlan) {
                netflow::VlanManager::PortConfig cfg;
                cfg.type = static_cast<netflow::PortType>(p.type);
                cfg.tag_native = p.tag_native != 0;
                cfg.native_vlan = p.native;
                cfg.allowed_vlans.insert(p.native);
                vm.configure_port(p.id, cfg);
            }
            if (p.has_qos) {
                netflow::QosConfig qc;
                qc.num_queues = p.queues;
                qc.max_queue_depth = p.depth;
                qos.configure_port_qos(p.id, qc);
            }
        }
        for (const uint32_t id : to_delete) {  // the binding stays
            if (!acl.delete_acl(list_name(id))) return 2;
            rules_of[id].clear();
        }
        const uint32_t num_ports = rd32();
        pairs.resize(rd32());
        std::vector<uint8_t> bytes;
        for (Pair& pr : pairs) {
            pr.port = rd32();
            const uint32_t len = rd32();
            bytes.assign(len + 1, 0);
            if (!rd(bytes.data(), len)) return 2;
            pr.pb = buffer_of(bytes.data(), len);
            pr.raw = buffer_of(bytes.data(), len);
        }
        std::map<const netflow::PacketBuffer*, uint32_t> index_of;
        for (uint32_t i = 0; i < pairs.size(); ++i) {
            Pair& pr = pairs[i];
            index_of[pr.pb.get()] = i;
            netflow::Packet pkt(pr.pb.get()), raw(pr.raw.get());
            vm.process_egress(pkt, pr.port);
            const uint32_t queue = qos.classify_packet_to_queue(pkt, pr.port);
            uint32_t action = 0, first = NONE, redirect = NONE, action_raw = 0, enq = 1;
            const std::optional<std::string> name = ifm.get_applied_acl_name(pr.port, netflow::AclDirection::EGRESS);
            if (name.has_value() && !name->empty()) {
                uint32_t port_out = NONE, unused = 0;
                const netflow::AclActionType act = acl.evaluate(*name, pkt, port_out);
                if (act != netflow::AclActionType::REDIRECT) port_out = NONE;
                action_raw = (uint32_t)static_cast<int>(acl.evaluate(*name, raw, unused));
                const std::vector<netflow::AclRule>& rules = rules_of[bound[pr.port]];
                for (size_t k = 0; k < rules.size() && first == NONE; ++k)
                    if (acl.evaluate(alone_name(bound[pr.port], k), pkt, unused) == netflow::AclActionType::DENY)
                        first = (uint32_t)k;
                netflow::AclActionType want = netflow::AclActionType::PERMIT;
                uint32_t want_port = NONE;
                if (first != NONE) {
                    want = rules[first].action;
                    if (want == netflow::AclActionType::REDIRECT) {
                        if (rules[first].redirect_port_id) want_port = *rules[first].redirect_port_id;
                        else want = netflow::AclActionType::DENY;
                    }
                }
                if (want != act || want_port != port_out) {
                    fprintf(stderr, "pair %u: evaluate() %d port %u, first matching rule %u implies %d port %u\n", i,
                            static_cast<int>(act), port_out, first, static_cast<int>(want), want_port);
                    return 4;
                }
                action = (uint32_t)static_cast<int>(act);
                redirect = port_out;
                if (act == netflow::AclActionType::DENY) {
                    ifm._increment_tx_stats(pr.port, pr.pb->get_data_length(), false, true);
                    enq = 0;
                }
            }
            if (enq) qos.enqueue_packet(pkt, pr.port);
            wr32(action);
            wr32(first);
            wr32(redirect);
            wr32((uint32_t)pr.pb->get_data_length());
            wr32(action_raw);
            wr32(enq);
            wr32(queue);
        }
        for (uint32_t p = 0; p < num_ports; ++p) {
            const netflow::InterfaceManager::PortStats s = ifm.get_port_stats(p);
            wr64(s.tx_packets);
            wr64(s.tx_bytes);
            wr64(s.tx_drops);
        }
        for (uint32_t p = 0; p < num_ports; ++p)
            for (uint32_t q = 0; q < 8; ++q) {
                const auto s = qos.get_queue_stats(p, (uint8_t)q);
                wr32(s ? (uint32_t)s->packets_enqueued : NONE);
                wr32(s ? (uint32_t)s->packets_dropped_full : NONE);
                wr32(s ? (uint32_t)s->current_depth : NONE);
            }
        for (uint32_t p = 0; p < num_ports; ++p)
            for (uint32_t q = 0; q < 8; ++q) {
                std::vector<uint8_t> out;
                uint32_t count = 0;
                while (auto pkt = qos.dequeue_packet(p, (uint8_t)q)) {
                    const netflow::PacketBuffer* b = pkt->get_buffer();
                    const auto it = index_of.find(b);
                    if (it == index_of.end() || pairs[it->second].port != p) return 4;
                    uint8_t rec[72] = {0};
                    const uint32_t len = (uint32_t)b->get_data_length();
                    memcpy(rec, &it->second, 4);
                    memcpy(rec + 4, &len, 4);
                    memcpy(rec + 8, b->get_data_start_ptr(), len < 64 ? len : 64);
                    out.insert(out.end(), rec, rec + 72);
                    ++count;
                }
                wr32(count);
                wr(out.data(), out.size());
            }
    }
    return fclose(g_out) == 0 ? 0 : 3;
}

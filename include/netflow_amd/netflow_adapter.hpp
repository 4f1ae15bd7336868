// netflow_amd/netflow_adapter.hpp — the GPU batch entry points over NetFlow++'s OWN types.
//
// A NetFlow++ caller holds netflow::Packet (include/netflow++/packet.hpp:344-357) over
// netflow::PacketBuffer (packet_buffer.hpp:10-111): the switch's transit forward
// (switch.hpp:279-294), the VLAN manager (vlan_manager.cpp:90,159,174), the ICMP processor
// (icmp_processor.cpp:180,336). Including this header in such a translation unit (with NetFlow++'s
// include/ on the include path, as its own sources have it) gives it the batched forms of the
// reference's per-packet calls on those very objects, run on the gfx950 engine through the C ABI
// (include/nfcs.h); no change to the Packet type:
//
//   reference, per packet                     here, per burst (std::vector<netflow::Packet*> or ptr + n)
//   pkt.update_checksums()  packet.hpp:722    netflow_amd::update_checksums_batch(pkts[, status])
//   pkt.push_vlan(v, p) / pkt.pop_vlan()      netflow_amd::vlan_batch(pkts, ops, ok[, status])
//        packet.hpp:655-720                   (ops[i] = NFCS_VLAN_PUSH_OP(v, p) / NFCS_VLAN_POP / NOP)
//   the switch's TTL--, MAC rewrite and       netflow_amd::l3_forward_batch(pkts, next_hop, table,
//   update_checksums() switch.hpp:279-294     table_n[, status])
//   extract_flow_key + hash_flow              netflow_amd::flow_keys_batch(pkts, keys[, hashes])
//        packet_classifier.cpp:12-108
//   is_my_ip, lookup_route, lookup_mac,       netflow_amd::route_lookup_batch(pkts, fib, next_hop[, egress_if,
//   get_interface_mac  switch.hpp:259-301     verdict]) with fib = netflow_amd::make_fib(routing_manager, arp,
//                                             if_macs, local_ips): its next hops feed l3_forward_batch
//   AclManager::evaluate                      netflow_amd::acl_eval_batch(pkts, acl, action[, rule_index,
//        acl_manager.cpp:161-278              redirect_port, next_hop]) with acl = netflow_amd::make_acl(
//                                             acl_manager.get_all_rules(name)): masks next_hop for l3_forward_batch
//   fdb.lookup_port, the same-port / link /   netflow_amd::l2_lookup_batch(pkts, fdb, ingress_port, egress_port[,
//   STP / should_forward checks, flood        verdict, vlan, learn, rt_verdict]) with fdb = netflow_amd::make_fdb(
//        switch.hpp:305-326                   fdb, vlan_manager, link_up, stp_forwarding, num_ports)
//   vlan_manager.process_egress(pkt, port) +  netflow_amd::egress_plan_batch(pkts, eg, egress_port, ops, queue), then
//   qos_manager.enqueue_packet(pkt, port)     vlan_batch(pkts, ops) and egress_enqueue_batch(eg, egress_port, queue, ...)
//        switch.hpp:113-139                   with eg = netflow_amd::make_egress(vlan_manager, qos_manager, num_ports)
//   qos_manager.select_packet_to_dequeue(port)  netflow_amd::txq_append_batch(txq, order, key_start, depth, handles)
//        qos_manager.cpp:197-240              after each egress_enqueue_batch, then txq_dequeue_batch(txq, budget, ...)
//                                             with txq = netflow_amd::make_txq(qos_manager, num_ports, eg)
//
// Every entry returns 0 or a negative NFCS_E* code and never throws (the reference's calls are
// void / bool and never throw); per-packet outcomes are the NFCS_ST_* status bytes. The bytes
// written into each PacketBuffer are the reference's, bit for bit. A VLAN edit changes the buffer's
// data length as push_vlan / pop_vlan do; the Packet's cached l2_header_size_ (packet.hpp:916) is
// not touched — every reference accessor recomputes it through ethernet() before use.
//
// Single packets stay where the reference has them: call pkt.update_checksums() on the CPU, as
// before. Link with -lnfcs (netflow_amd/libnfcs.so); the engine is the process-wide one on device 0
// unless one is passed (ChecksumEngine(device) per GPU for multi-GPU hosts).
#pragma once

#include <netflow++/packet.hpp>

#include <cstring>
#include <utility>
#include <vector>

#include "netflow_amd/packet.hpp"

namespace netflow {
class RoutingManager;  // <netflow++/routing_manager.hpp>, for make_fib below
struct AclRule;        // <netflow++/acl_manager.hpp>, for make_acl below
class ForwardingDatabase;  // <netflow++/forwarding_database.hpp>, for make_fdb below
class VlanManager;         // <netflow++/vlan_manager.hpp>, for make_fdb and make_egress below
class QosManager;          // <netflow++/qos_manager.hpp>, for make_egress below
}

namespace netflow_amd {

// On the process-wide engine (device 0): NFCS_ENODEV instead of an exception when there is none.
inline int update_checksums_batch(netflow::Packet* const* pkts, size_t n, uint8_t* status = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.update_checksums_batch(pkts, n, status); });
}
inline int update_checksums_batch(const std::vector<netflow::Packet*>& pkts, uint8_t* status = nullptr) {
    return update_checksums_batch(pkts.data(), pkts.size(), status);
}
inline int vlan_batch(netflow::Packet* const* pkts, const uint32_t* ops, size_t n, bool* ok = nullptr,
                      uint8_t* status = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.vlan_batch(pkts, ops, n, ok, status); });
}
inline int vlan_batch(const std::vector<netflow::Packet*>& pkts, const uint32_t* ops, bool* ok = nullptr,
                      uint8_t* status = nullptr) {
    return vlan_batch(pkts.data(), ops, pkts.size(), ok, status);
}
inline int l3_forward_batch(netflow::Packet* const* pkts, const uint32_t* next_hop, size_t n,
                            const nfcs_nexthop* table, uint32_t table_n, uint8_t* status = nullptr) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.l3_forward_batch(pkts, next_hop, n, table, table_n, status); });
}
inline int l3_forward_batch(const std::vector<netflow::Packet*>& pkts, const uint32_t* next_hop,
                            const nfcs_nexthop* table, uint32_t table_n, uint8_t* status = nullptr) {
    return l3_forward_batch(pkts.data(), next_hop, pkts.size(), table, table_n, status);
}
inline int flow_keys_batch(netflow::Packet* const* pkts, size_t n, nfcs_flow_key* keys,
                           uint32_t* hashes = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.flow_keys_batch(pkts, n, keys, hashes); });
}
inline int flow_keys_batch(const std::vector<netflow::Packet*>& pkts, nfcs_flow_key* keys,
                           uint32_t* hashes = nullptr) {
    return flow_keys_batch(pkts.data(), pkts.size(), keys, hashes);
}

inline int route_lookup_batch(netflow::Packet* const* pkts, size_t n, const nfcs_fib* fib, uint32_t* next_hop,
                              uint32_t* egress_if = nullptr, uint8_t* verdict = nullptr) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.route_lookup_batch(pkts, n, fib, next_hop, egress_if, verdict); });
}
inline int route_lookup_batch(const std::vector<netflow::Packet*>& pkts, const nfcs_fib* fib, uint32_t* next_hop,
                              uint32_t* egress_if = nullptr, uint8_t* verdict = nullptr) {
    return route_lookup_batch(pkts.data(), pkts.size(), fib, next_hop, egress_if, verdict);
}

// A committed forwarding table (nfcs_fib) from the switch's own state: the routes are
// RoutingManager::get_routing_table() as it is — the order lookup_route scans, which is the order
// contract of nfcs_fib_set_routes (the reference's sort is not redone here) — plus the ARP cache
// entries {ip, mac} (ArpProcessor keeps them in a std::map; of duplicates the last one wins), the
// interface MACs {interface id, mac} (InterfaceManager::get_interface_mac) and the switch's own
// addresses (InterfaceManager::is_my_ip). Returns NFCS_OK and the table in *out (nfcs_fib_destroy it;
// upload it with ChecksumEngine::upload_fib before route_lookup_batch), or a negative NFCS_E* code.
// A template, so that this header needs neither <netflow++/routing_manager.hpp> nor, at link time,
// routing_manager.cpp unless make_fib is used: the caller includes that header (RoutingManager must be
// complete where make_fib is called) and links what get_routing_table() lives in, as any user of
// RoutingManager does. The work is netflow_amd::make_fib_from (packet.hpp), which any class with a
// get_routing_table() of such entries can use.
template <class RoutingManagerT = netflow::RoutingManager>
inline int make_fib(const RoutingManagerT& rm,
                    const std::vector<std::pair<netflow::IpAddress, netflow::MacAddress>>& arp_entries,
                    const std::vector<std::pair<uint32_t, netflow::MacAddress>>& interface_macs,
                    const std::vector<netflow::IpAddress>& local_ips, nfcs_fib** out) {
    return make_fib_from(rm, arp_entries, interface_macs, local_ips, out);
}

inline int acl_eval_batch(netflow::Packet* const* pkts, size_t n, const nfcs_acl* acl, uint8_t* action,
                          uint32_t* rule_index = nullptr, uint32_t* redirect_port = nullptr,
                          uint32_t* next_hop = nullptr) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.acl_eval_batch(pkts, n, acl, action, rule_index, redirect_port, next_hop); });
}
inline int acl_eval_batch(const std::vector<netflow::Packet*>& pkts, const nfcs_acl* acl, uint8_t* action,
                          uint32_t* rule_index = nullptr, uint32_t* redirect_port = nullptr,
                          uint32_t* next_hop = nullptr) {
    return acl_eval_batch(pkts.data(), pkts.size(), acl, action, rule_index, redirect_port, next_hop);
}

// A committed rule list (nfcs_acl) from one of the switch's named ACLs: AclManager::get_all_rules(name)
// as it is — the order evaluate walks, compiled or not, which is the order contract of
// nfcs_acl_set_rules (compile_rules' sort is not redone here). Each engaged std::optional of a rule
// becomes its NFCS_ACL_F_* bit, the addresses stay in host byte order as AclRule holds them, and the
// address masks are full (the reference matches addresses exactly). Returns NFCS_OK and the list in *out
// (nfcs_acl_destroy it; upload it with ChecksumEngine::upload_acl before acl_eval_batch), or a negative
// NFCS_E* code. A template, so that this header does not need <netflow++/acl_manager.hpp> unless
// make_acl is used: the caller includes it (AclRule must be complete where make_acl is called). The work
// is netflow_amd::make_acl_from (packet.hpp), which any rule struct with AclRule's members can use.
template <class AclRuleT = netflow::AclRule>
inline int make_acl(const std::vector<AclRuleT>& rules, nfcs_acl** out) {
    return make_acl_from(rules, out);
}

// A committed set of egress ACLs (nfcs_aclset, for nfcs_egress_acl_device) from the switch's named ACLs and
// its bindings: lists[name] = AclManager::get_all_rules(name), port_to_name = (port,
// *InterfaceManager::get_applied_acl_name(port, AclDirection::EGRESS)) for every port that has a name. A bound
// name without a list (a deleted ACL) permits, as AclManager::evaluate does. The work is
// netflow_amd::make_acl_set_from (packet.hpp).
template <class AclRuleT = netflow::AclRule>
inline int make_acl_set(const std::map<std::string, std::vector<AclRuleT>>& lists,
                        const std::vector<std::pair<uint32_t, std::string>>& port_to_name, nfcs_aclset** out) {
    return make_acl_set_from(lists, port_to_name, out);
}

inline int l2_lookup_batch(netflow::Packet* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                           uint32_t* egress_port, uint8_t* verdict = nullptr, uint16_t* vlan = nullptr,
                           uint8_t* learn = nullptr, const uint8_t* rt_verdict = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.l2_lookup_batch(pkts, n, fdb, ingress_port, egress_port, verdict, vlan, learn, rt_verdict);
    });
}
inline int l2_lookup_batch(const std::vector<netflow::Packet*>& pkts, const nfcs_fdb* fdb, uint32_t ingress_port,
                           uint32_t* egress_port, uint8_t* verdict = nullptr, uint16_t* vlan = nullptr,
                           uint8_t* learn = nullptr, const uint8_t* rt_verdict = nullptr) {
    return l2_lookup_batch(pkts.data(), pkts.size(), fdb, ingress_port, egress_port, verdict, vlan, learn, rt_verdict);
}

// What process_received_packet does between the stages, for the burst the three lookups just decided
// (ChecksumEngine::ingress_dispatch_batch, packet.hpp): the ingress link test, DENY / REDIRECT and the LLDP,
// zero-MAC and ARP early returns masking next_hop, l2_port and l2_verdict, and the RX counters. As with the other
// overloads over netflow::Packet*, the tested path is the same template over netflow_amd::Packet
// (tests/cpp/dispatch_test.cpp).
inline int ingress_dispatch_batch(netflow::Packet* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                                  uint32_t num_ports, const uint8_t* rt_verdict, uint32_t* next_hop, uint32_t* l2_port,
                                  uint8_t* l2_verdict, const uint8_t* action = nullptr,
                                  const uint32_t* redirect_port = nullptr, uint8_t* cls = nullptr,
                                  uint8_t* bypass = nullptr, nfcs_rx_stats* rx = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.ingress_dispatch_batch(pkts, n, fdb, ingress_port, num_ports, rt_verdict, next_hop, l2_port, l2_verdict,
                                        action, redirect_port, cls, bypass, rx);
    });
}
inline int ingress_dispatch_batch(const std::vector<netflow::Packet*>& pkts, const nfcs_fdb* fdb, uint32_t ingress_port,
                                  uint32_t num_ports, const uint8_t* rt_verdict, uint32_t* next_hop, uint32_t* l2_port,
                                  uint8_t* l2_verdict, const uint8_t* action = nullptr,
                                  const uint32_t* redirect_port = nullptr, uint8_t* cls = nullptr,
                                  uint8_t* bypass = nullptr, nfcs_rx_stats* rx = nullptr) {
    return ingress_dispatch_batch(pkts.data(), pkts.size(), fdb, ingress_port, num_ports, rt_verdict, next_hop, l2_port,
                                  l2_verdict, action, redirect_port, cls, bypass, rx);
}

// A committed forwarding database (nfcs_fdb) from the switch's own L2 state: ForwardingDatabase::
// get_all_entries() as it is, and for the ports 0 .. num_ports - 1 VlanManager::get_port_config plus the
// two predicates the L2 block asks per port — link_up(port) for InterfaceManager::is_port_link_up and
// stp_forwarding(port) for StpManager::get_port_stp_state(port) == PortState::FORWARDING, as callables,
// so that this header needs neither manager. Returns NFCS_OK and the database in *out (nfcs_fdb_destroy
// it; upload it with ChecksumEngine::upload_fdb before l2_lookup_batch), or a negative NFCS_E* code. A
// template, so that <netflow++/forwarding_database.hpp> and <netflow++/vlan_manager.hpp> are needed only
// where make_fdb is used: the caller includes them and links forwarding_database.cpp and
// vlan_manager.cpp, as any user of those classes does. The work is netflow_amd::make_fdb_from
// (packet.hpp), which any types with the same member names can use.
template <class ForwardingDatabaseT = netflow::ForwardingDatabase, class VlanManagerT = netflow::VlanManager,
          class LinkUp, class StpForwarding>
inline int make_fdb(const ForwardingDatabaseT& fdb, const VlanManagerT& vlans, LinkUp&& link_up,
                    StpForwarding&& stp_forwarding, uint32_t num_ports, nfcs_fdb** out) {
    return make_fdb_from(fdb, vlans, link_up, stp_forwarding, num_ports, out);
}

// Flood replication for the burst l2_lookup_batch just decided (ChecksumEngine::flood_expand_batch, packet.hpp):
// the egress work items in the reference's processing order, flood copies included, with the copies' bytes for
// the caller to wrap in PacketBuffers of its own (BufferPool::allocate_buffer + memcpy, as flood_packet does).
// This overload over netflow::Packet* was compiled and run against the reference's real types by hand only;
// the tested path is the same template over netflow_amd::Packet (tests/cpp/flood_test.cpp).
inline int flood_expand_batch(netflow::Packet* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                              uint32_t num_ports, const uint32_t* egress_port, const uint8_t* l2_verdict,
                              const uint16_t* l2_vlan, ChecksumEngine::FloodItems* out) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.flood_expand_batch(pkts, n, fdb, ingress_port, num_ports, egress_port, l2_verdict, l2_vlan, out);
    });
}
inline int flood_expand_batch(const std::vector<netflow::Packet*>& pkts, const nfcs_fdb* fdb, uint32_t ingress_port,
                              uint32_t num_ports, const uint32_t* egress_port, const uint8_t* l2_verdict,
                              const uint16_t* l2_vlan, ChecksumEngine::FloodItems* out) {
    return flood_expand_batch(pkts.data(), pkts.size(), fdb, ingress_port, num_ports, egress_port, l2_verdict, l2_vlan, out);
}

// The switch's ICMP answers for the burst route_lookup_batch just decided (ChecksumEngine::icmp_respond_batch,
// packet.hpp): echo replies for NFCS_RT_LOCAL echo requests, ICMP 11/0 for NFCS_RT_TTL_EXPIRED and 3/0 for
// NFCS_RT_NO_ROUTE, built and checksummed on the device, with the messages' bytes for the caller to wrap in
// PacketBuffers of its own and hand to send_control_plane_packet(pkt, out->port[k]) — the call sites the
// reference leaves as comments at switch.hpp:271 / 279 / 301. This overload over netflow::Packet* has not been
// run against the reference's real types; the tested path is the same template over netflow_amd::Packet
// (tests/cpp/icmp_respond_test.cpp).
inline int icmp_respond_batch(netflow::Packet* const* pkts, size_t n, const nfcs_icmp* icmp, const nfcs_fib* fib,
                              uint32_t ingress_port, const uint8_t* rt_verdict, const uint16_t* ip_id,
                              ChecksumEngine::IcmpMessages* out) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.icmp_respond_batch(pkts, n, icmp, fib, ingress_port, rt_verdict, ip_id, out);
    });
}
// A committed nfcs_icmp from the switch's InterfaceManager (make_icmp_from, packet.hpp). A template, so that
// <netflow++/interface_manager.hpp> is needed only where make_icmp is used.
template <class InterfaceManagerT>
inline int make_icmp(const InterfaceManagerT& ifm, uint32_t num_ports, nfcs_icmp** out) {
    return make_icmp_from(ifm, num_ports, out);
}

inline int egress_plan_batch(netflow::Packet* const* pkts, size_t n, const nfcs_egress* eg, const uint32_t* egress_port,
                             uint32_t* ops, uint8_t* queue) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.egress_plan_batch(pkts, n, eg, egress_port, ops, queue); });
}
inline int egress_plan_batch(const std::vector<netflow::Packet*>& pkts, const nfcs_egress* eg,
                             const uint32_t* egress_port, uint32_t* ops, uint8_t* queue) {
    return egress_plan_batch(pkts.data(), pkts.size(), eg, egress_port, ops, queue);
}

// Committed egress ports (nfcs_egress) from the switch's own state: for the ports 0 .. num_ports - 1
// VlanManager::get_port_config (type, native_vlan, tag_native) and QosManager::get_port_qos_config
// (num_queues, max_queue_depth, as configure_port_qos normalised them). Returns NFCS_OK and the object in
// *out (nfcs_egress_destroy it; upload it with ChecksumEngine::upload_egress before egress_plan_batch), or a
// negative NFCS_E* code. A template, so that <netflow++/vlan_manager.hpp> and <netflow++/qos_manager.hpp>
// are needed only where make_egress is used: the caller includes them and links vlan_manager.cpp and
// qos_manager.cpp. The work is netflow_amd::make_egress_from (packet.hpp), which any types with the same
// member names can use.
template <class VlanManagerT = netflow::VlanManager, class QosManagerT = netflow::QosManager>
inline int make_egress(const VlanManagerT& vlans, const QosManagerT& qos, uint32_t num_ports, nfcs_egress** out) {
    return make_egress_from(vlans, qos, num_ports, out);
}

// The TX queues of those ports (nfcs_txq) with QosConfig::scheduler of each port from
// QosManager::get_port_qos_config: the rings behind enqueue_packet and the scheduler of
// select_packet_to_dequeue, on `eng`'s device (the process-wide engine by default). eg is what make_egress
// returned for the same managers. Returns NFCS_OK and the object in *out (nfcs_txq_destroy it before the
// engine), or a negative NFCS_E* code. The work is make_txq and set_schedulers_from (packet.hpp).
template <class QosManagerT = netflow::QosManager>
inline int make_txq(ChecksumEngine& eng, const QosManagerT& qos, uint32_t num_ports, const nfcs_egress* eg,
                    nfcs_txq** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    nfcs_txq* x = nullptr;
    int rc = eng.make_txq(eg, &x);
    if (!rc) rc = set_schedulers_from(qos, num_ports, x);
    if (rc && x) nfcs_txq_destroy(x);
    else *out = x;
    return rc;
}
template <class QosManagerT = netflow::QosManager>
inline int make_txq(const QosManagerT& qos, uint32_t num_ports, const nfcs_egress* eg, nfcs_txq** out) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return make_txq(e, qos, num_ports, eg, out); });
}

// On an engine of the caller's (another device; one engine per GPU, one host thread each).
inline int update_checksums_batch(ChecksumEngine& eng, netflow::Packet* const* pkts, size_t n,
                                  uint8_t* status = nullptr) {
    return eng.update_checksums_batch(pkts, n, status);
}

}  // namespace netflow_amd

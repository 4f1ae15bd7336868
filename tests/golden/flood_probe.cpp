// flood_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_flood_golden.py).
//
// Walks the L2 block of Switch::process_received_packet with its flood branch over a list of frames, with
// the reference's own ForwardingDatabase, VlanManager, QosManager, Packet and PacketBuffer. The few lines of
// switch.hpp that join them are restated here:
//   305-326  the lookup VLAN, lookup_port, the || chain of checks, flood on a miss;
//   174-204  flood_packet: the flood VLAN, the port loop, a fresh buffer per port, the memcpy of
//            get_data_length() bytes, process_egress_pipeline(copy, port);
//   113-139  process_egress_pipeline without its ACL: VlanManager::process_egress, QosManager::enqueue_packet.
// The FDB is built through learn_mac / add_static_entry, the ports through VlanManager::configure_port and
// QosManager::configure_port_qos; link and STP state are booleans the probe holds itself (the reference has no
// setter for an STP state), a port not listed being link down and not STP-forwarding. For each frame in order:
// on a hit that passes the checks, process_egress + enqueue_packet on the frame's own buffer; on a miss the
// flood loop, each copy in a PacketBuffer of its own. The probe keeps its own map from buffer to (source
// index, port): frame bytes are not borrowed for an index, since the destination MAC matters here. Every run
// (one ingress port) starts with fresh copies of the frames and a fresh QosManager. Compiled against the
// reference's headers in place plus src/netflow++/forwarding_database.cpp, vlan_manager.cpp and
// qos_manager.cpp; the binary goes to oracle/_ref/ (git-ignored). The logger is set to CRITICAL; the results
// go to the file named by argv[1], not to stdout, where the logger would write.
//
// stdin (little-endian):
//   u32 n_ops, n_ops x {u8 kind (0 learn_mac, 1 add_static_entry), u8 pad, mac[6], u16 vlan, u16 pad, u32 port}
//   u32 n_ports, n_ports x {u32 port_id, u8 link_up, u8 stp_forwarding, u8 has_vlan_config, u8 type,
//                           u16 native_vlan, u16 n_allowed, n_allowed x u16 (padded to 4 bytes),
//                           u8 tag_native, u8 has_qos, u8 num_queues, u8 pad, u32 max_queue_depth}
//   u32 num_ports (the switch's port count, for the flood loop)
//   u32 n_runs, n_runs x u32 ingress port
//   u32 nf, nf x {u32 len, bytes}
// argv[1] (little-endian):
//   u32 ne, ne x {mac[6], u16 vlan_id, u32 port, u8 is_static, u8 pad[3]}   (get_all_entries() order)
//   per run:
//     nf x {u32 verdict (NFCS_L2_*), u32 egress port or 0xFFFFFFFF, u32 vlan, u32 n_flood, n_flood x u32 port}
//     num_ports x 8 x {u32 packets_enqueued, u32 packets_dropped_full, u32 current_depth} (0xFFFFFFFF x 3
//            where get_queue_stats returns nullopt)
//     num_ports x 8 x {u32 count, count x {u32 source index, u32 port, u32 len, 64 bytes of the frame (zero
//            padded)}}   dequeue_packet(port, queue) until it returns nullopt
#include <netflow++/forwarding_database.hpp>
#include <netflow++/logger.hpp>
#include <netflow++/packet.hpp>
#include <netflow++/qos_manager.hpp>
#include <netflow++/vlan_manager.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

namespace {

enum : uint32_t { FORWARD = 0, NO_ETH = 3, FLOOD = 4, SAME_PORT = 5, LINK_DOWN = 6, STP = 7, VLAN = 8 };
constexpr uint32_t NONE = 0xFFFFFFFFu;

FILE* g_out = nullptr;
bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
void wr(const void* p, size_t n) { if (n) fwrite(p, 1, n, g_out); }
uint32_t rd32() { uint32_t v = 0; rd(&v, 4); return v; }
uint16_t rd16() { uint16_t v = 0; rd(&v, 2); return v; }
void wr32(uint32_t v) { wr(&v, 4); }

struct PortState { bool link = false, stp = false; };
struct Qos { uint32_t port; uint8_t queues; uint32_t depth; };
std::map<uint32_t, PortState> g_state;
bool link_up(uint32_t p) { auto it = g_state.find(p); return it != g_state.end() && it->second.link; }
bool stp_fwd(uint32_t p) { auto it = g_state.find(p); return it != g_state.end() && it->second.stp; }

struct Sent { uint32_t src, port; };

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    netflow::SwitchLogger logger(netflow::LogLevel::CRITICAL);
    netflow::ForwardingDatabase fdb;
    netflow::VlanManager vm;
    std::vector<Qos> qos_cfg;
    const uint32_t n_ops = rd32();
    for (uint32_t i = 0; i < n_ops; ++i) {
        uint8_t kind_pad[2], mac[6];
        if (!rd(kind_pad, 2) || !rd(mac, 6)) return 2;
        const uint16_t vlan = rd16();
        rd16();
        const uint32_t port = rd32();
        if (kind_pad[0] == 1) fdb.add_static_entry(netflow::MacAddress(mac), port, vlan);
        else fdb.learn_mac(netflow::MacAddress(mac), port, vlan);
    }
    const uint32_t n_ports = rd32();
    for (uint32_t i = 0; i < n_ports; ++i) {
        const uint32_t id = rd32();
        uint8_t b[4], q[4];
        if (!rd(b, 4)) return 2;
        const uint16_t native = rd16(), n_allowed = rd16();
        netflow::VlanManager::PortConfig cfg;
        cfg.type = static_cast<netflow::PortType>(b[3]);
        cfg.native_vlan = native;
        cfg.allowed_vlans.clear();
        for (uint16_t k = 0; k < n_allowed; ++k) cfg.allowed_vlans.insert(rd16());
        if (n_allowed & 1u) rd16();
        if (!rd(q, 4)) return 2;
        const uint32_t depth = rd32();
        cfg.tag_native = q[0] != 0;
        g_state[id].link = b[0] != 0;
        g_state[id].stp = b[1] != 0;
        if (b[2]) vm.configure_port(id, cfg);
        if (q[1]) qos_cfg.push_back(Qos{id, q[2], depth});
    }
    const uint32_t num_ports = rd32();
    std::vector<uint32_t> runs(rd32());
    for (uint32_t& r : runs) r = rd32();
    const uint32_t nf = rd32();
    std::vector<std::vector<uint8_t>> frames(nf);
    for (uint32_t i = 0; i < nf; ++i) {
        frames[i].resize(rd32());
        if (!rd(frames[i].data(), frames[i].size())) return 2;
    }

    const std::vector<netflow::FdbEntry>& all = fdb.get_all_entries();
    wr32((uint32_t)all.size());
    for (const netflow::FdbEntry& e : all) {
        uint8_t rec[16] = {0};
        memcpy(rec, e.mac.bytes, 6);
        memcpy(rec + 6, &e.vlan_id, 2);
        memcpy(rec + 8, &e.port, 4);
        rec[12] = e.is_static ? 1 : 0;
        wr(rec, 16);
    }

    for (const uint32_t ingress : runs) {
        std::vector<std::unique_ptr<netflow::PacketBuffer>> bufs;  // declared before the QosManager: its queues refer to them
        std::map<const netflow::PacketBuffer*, Sent> sent;
        auto buffer_of = [&](const uint8_t* data, size_t len) {
            bufs.push_back(std::make_unique<netflow::PacketBuffer>(len + 16, 0, len));
            memset(bufs.back()->get_data_start_ptr(), 0, len + 16);
            memcpy(bufs.back()->get_data_start_ptr(), data, len);
            return bufs.back().get();
        };
        netflow::QosManager qos(logger);
        for (const Qos& q : qos_cfg) {
            netflow::QosConfig qc;
            qc.num_queues = q.queues;
            qc.max_queue_depth = q.depth;
            qos.configure_port_qos(q.port, qc);
        }
        // switch.hpp:113-139 without the ACL
        auto egress_pipeline = [&](netflow::Packet& pkt, uint32_t port, uint32_t src) {
            sent[pkt.get_buffer()] = Sent{src, port};
            vm.process_egress(pkt, port);
            qos.enqueue_packet(pkt, port);
        };
        for (uint32_t i = 0; i < nf; ++i) {
            netflow::PacketBuffer* pb = buffer_of(frames[i].data(), frames[i].size());
            netflow::Packet pkt(pb);
            uint32_t verdict = NO_ETH, egress = NONE, vlan = 0;
            std::vector<uint32_t> flood;
            netflow::EthernetHeader* eth_hdr = pkt.ethernet();
            if (eth_hdr && pkt.dst_mac().has_value()) {
                // switch.hpp:305-326
                const uint16_t vlan_for_lookup = pkt.vlan_id().value_or(
                    vm.get_port_config(ingress).value_or(netflow::VlanManager::PortConfig()).native_vlan);
                vlan = vlan_for_lookup;
                const std::optional<uint32_t> egress_port_opt = fdb.lookup_port(pkt.dst_mac().value(), vlan_for_lookup);
                if (egress_port_opt.has_value()) {
                    const uint32_t port = egress_port_opt.value();
                    if (port == ingress) verdict = SAME_PORT;
                    else if (!link_up(port)) verdict = LINK_DOWN;
                    else if (!stp_fwd(port)) verdict = STP;
                    else if (!vm.should_forward(ingress, port, vlan_for_lookup)) verdict = VLAN;
                    else {
                        verdict = FORWARD;
                        egress = port;
                        egress_pipeline(pkt, port, i);
                    }
                } else {
                    verdict = FLOOD;
                    // switch.hpp:174-204
                    const uint16_t vlan_id_for_flooding = pkt.vlan_id().value_or(
                        vm.get_port_config(ingress).value_or(netflow::VlanManager::PortConfig()).native_vlan);
                    for (uint32_t p = 0; p < num_ports; ++p) {
                        if (p == ingress) continue;
                        if (!link_up(p) || !stp_fwd(p) || !vm.should_forward(ingress, p, vlan_id_for_flooding)) continue;
                        netflow::PacketBuffer* pb_copy = buffer_of(pkt.get_buffer()->get_data_start_ptr(),
                                                                   pkt.get_buffer()->get_data_length());
                        netflow::Packet flood_pkt_copy(pb_copy);
                        flood.push_back(p);
                        egress_pipeline(flood_pkt_copy, p, i);
                    }
                }
            }
            wr32(verdict);
            wr32(egress);
            wr32(vlan);
            wr32((uint32_t)flood.size());
            wr(flood.data(), flood.size() * 4);
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
                    const auto it = sent.find(b);
                    if (it == sent.end() || it->second.port != p) return 4;
                    uint8_t rec[76] = {0};
                    const uint32_t len = (uint32_t)b->get_data_length();
                    memcpy(rec, &it->second.src, 4);
                    memcpy(rec + 4, &it->second.port, 4);
                    memcpy(rec + 8, &len, 4);
                    memcpy(rec + 12, b->get_data_start_ptr(), len < 64 ? len : 64);
                    out.insert(out.end(), rec, rec + 76);
                    ++count;
                }
                wr32(count);
                wr(out.data(), out.size());
            }
    }
    return fclose(g_out) == 0 ? 0 : 3;
}

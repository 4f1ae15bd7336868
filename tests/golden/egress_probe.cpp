// egress_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_egress_golden.py).
//
// Walks the two halves of Switch::process_egress_pipeline (switch.hpp:113-139) over a list of frames with
// the reference's own code: the ports go through VlanManager::configure_port and
// QosManager::configure_port_qos; every frame is a netflow::Packet over its own PacketBuffer, handed to
// VlanManager::process_egress(pkt, port) and then to QosManager::enqueue_packet(pkt, port), in order. A
// warm-up list goes through the same two calls first, so the queues are not empty when the burst starts.
// Every frame carries a 32-bit index in its bytes 0..3 (the destination MAC, which nothing here reads or
// edits); warm-up frames have bit 31 of it set. Compiled against the reference's headers in place plus
// src/netflow++/vlan_manager.cpp and qos_manager.cpp (the logger is header-only); the binary goes to
// oracle/_ref/ (git-ignored). The logger is set to CRITICAL, so nothing but the results leaves the
// program; the results go to the file named by argv[1], not to stdout, where the logger would write.
//
// stdin (little-endian):
//   u32 n_ports, n_ports x nfcs_egress_port {u32 port_id, u8 has_vlan_config, u8 type, u8 tag_native,
//                                            u8 has_qos, u16 native_vlan, u8 num_queues, u8 pad, u32 depth}
//   u32 n_warm, n_warm x {u32 port, u32 len, bytes}
//   u32 nf, nf x {u32 port, u32 len, bytes}
// argv[1] (little-endian):
//   n_ports x 8 x {u32 packets_enqueued, u32 packets_dropped_full, u32 current_depth}   get_queue_stats
//            after the warm-up (0xFFFFFFFF x 3 where it returns nullopt)
//   nf x {u32 len after process_egress, 64 bytes of the frame after it (zero padded),
//         u32 classify_packet_to_queue(pkt, port) on the edited frame}
//   n_ports x 8 x the same three counters after the burst
//   n_ports x 8 x {u32 count, count x u32 index}   dequeue_packet(port, queue) until it returns nullopt
#include <netflow++/logger.hpp>
#include <netflow++/packet.hpp>
#include <netflow++/qos_manager.hpp>
#include <netflow++/vlan_manager.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

namespace {

FILE* g_out = nullptr;
bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
void wr(const void* p, size_t n) { if (n) fwrite(p, 1, n, g_out); }
uint32_t rd32() { uint32_t v = 0; rd(&v, 4); return v; }
void wr32(uint32_t v) { wr(&v, 4); }

struct Port { uint32_t id; uint8_t b[4]; uint16_t native; uint8_t queues, pad; uint32_t depth; };
struct Frame { uint32_t port; std::unique_ptr<netflow::PacketBuffer> pb; };

bool read_frames(std::vector<Frame>& v) {
    v.resize(rd32());
    for (Frame& f : v) {
        f.port = rd32();
        const uint32_t len = rd32();
        f.pb = std::make_unique<netflow::PacketBuffer>(len + 16, 0, len);
        memset(f.pb->get_data_start_ptr(), 0, len + 16);
        if (!rd(f.pb->get_data_start_ptr(), len)) return false;
    }
    return true;
}

void stats(const netflow::QosManager& qos, const std::vector<Port>& ports) {
    for (const Port& p : ports)
        for (uint32_t q = 0; q < 8; ++q) {
            const auto s = qos.get_queue_stats(p.id, (uint8_t)q);
            wr32(s ? (uint32_t)s->packets_enqueued : 0xFFFFFFFFu);
            wr32(s ? (uint32_t)s->packets_dropped_full : 0xFFFFFFFFu);
            wr32(s ? (uint32_t)s->current_depth : 0xFFFFFFFFu);
        }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    netflow::SwitchLogger logger(netflow::LogLevel::CRITICAL);
    netflow::VlanManager vm;
    std::vector<Frame> warm, frames;  // declared before the QosManager: its queues refer to these buffers
    {
        netflow::QosManager qos(logger);
        std::vector<Port> ports(rd32());
        for (Port& p : ports) {
            p.id = rd32();
            if (!rd(p.b, 4) || !rd(&p.native, 2) || !rd(&p.queues, 1) || !rd(&p.pad, 1)) return 2;
            p.depth = rd32();
            if (p.b[0]) {
                netflow::VlanManager::PortConfig cfg;
                cfg.type = static_cast<netflow::PortType>(p.b[1]);
                cfg.tag_native = p.b[2] != 0;
                cfg.native_vlan = p.native;
                cfg.allowed_vlans.insert(p.native);
                vm.configure_port(p.id, cfg);
            }
            if (p.b[3]) {
                netflow::QosConfig qc;
                qc.num_queues = p.queues;
                qc.max_queue_depth = p.depth;
                qos.configure_port_qos(p.id, qc);
            }
        }
        if (!read_frames(warm) || !read_frames(frames)) return 2;
        for (Frame& f : warm) {
            netflow::Packet pkt(f.pb.get());
            vm.process_egress(pkt, f.port);
            qos.enqueue_packet(pkt, f.port);
        }
        stats(qos, ports);
        for (Frame& f : frames) {
            netflow::Packet pkt(f.pb.get());
            vm.process_egress(pkt, f.port);
            const uint32_t len = (uint32_t)f.pb->get_data_length();
            uint8_t out[64] = {0};
            memcpy(out, f.pb->get_data_start_ptr(), len < 64 ? len : 64);
            wr32(len);
            wr(out, 64);
            wr32(qos.classify_packet_to_queue(pkt, f.port));
            qos.enqueue_packet(pkt, f.port);
        }
        stats(qos, ports);
        for (const Port& p : ports)
            for (uint32_t q = 0; q < 8; ++q) {
                std::vector<uint32_t> idx;
                while (auto pkt = qos.dequeue_packet(p.id, (uint8_t)q)) {
                    uint32_t i = 0;
                    memcpy(&i, pkt->get_buffer()->get_data_start_ptr(), 4);
                    idx.push_back(i);
                }
                wr32((uint32_t)idx.size());
                wr(idx.data(), idx.size() * 4);
            }
    }
    return fclose(g_out) == 0 ? 0 : 3;
}

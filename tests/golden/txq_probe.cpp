// txq_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_txq_golden.py).
//
// Drives the reference's QosManager over several ticks with its own code: the ports go through
// QosManager::configure_port_qos (with their scheduler); in each tick a burst of frames, each a
// netflow::Packet over its own PacketBuffer, goes through classify_packet_to_queue and enqueue_packet in
// order, and then every port gets its budget of select_packet_to_dequeue calls, stopping at the first
// nullopt. Every frame carries a 32-bit sequence number in its bytes 18..21 (the payload behind the tag
// and the EtherType). Compiled against the reference's headers in place plus src/netflow++/qos_manager.cpp
// (the logger is header-only); the binary goes to oracle/_ref/ (git-ignored). The logger is set to
// CRITICAL; the results go to the file named by argv[1], not to stdout, where the logger would write.
//
// stdin (little-endian):
//   u32 n_ports, n_ports x {u32 port_id, u8 has_qos, u8 num_queues, u8 scheduler, u8 pad, u32 max_queue_depth}
//   u32 ticks, ticks x { u32 nf, nf x {u32 port, u32 len, bytes}, n_ports x u32 budget }
// argv[1] (little-endian), per tick:
//   nf x u32 classify_packet_to_queue(pkt, port)
//   n_ports x 8 x {u32 packets_enqueued, u32 packets_dropped_full, u32 packets_dequeued, u32 current_depth}
//            get_queue_stats after the burst (0xFFFFFFFF x 4 where it returns nullopt)
//   n_ports x {u32 count, count x u32 sequence number}   the packets select_packet_to_dequeue returned
//   n_ports x 8 x the same four counters after the dequeues
#include <netflow++/logger.hpp>
#include <netflow++/packet.hpp>
#include <netflow++/qos_manager.hpp>

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

struct Port { uint32_t id; uint8_t has_qos, queues, sched, pad; uint32_t depth; };

void stats(const netflow::QosManager& qos, const std::vector<Port>& ports) {
    for (const Port& p : ports)
        for (uint32_t q = 0; q < 8; ++q) {
            const auto s = qos.get_queue_stats(p.id, (uint8_t)q);
            wr32(s ? (uint32_t)s->packets_enqueued : 0xFFFFFFFFu);
            wr32(s ? (uint32_t)s->packets_dropped_full : 0xFFFFFFFFu);
            wr32(s ? (uint32_t)s->packets_dequeued : 0xFFFFFFFFu);
            wr32(s ? (uint32_t)s->current_depth : 0xFFFFFFFFu);
        }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    netflow::SwitchLogger logger(netflow::LogLevel::CRITICAL);
    std::vector<std::unique_ptr<netflow::PacketBuffer>> bufs;  // before the QosManager: its queues refer to these
    {
        netflow::QosManager qos(logger);
        std::vector<Port> ports(rd32());
        for (Port& p : ports) {
            p.id = rd32();
            if (!rd(&p.has_qos, 1) || !rd(&p.queues, 1) || !rd(&p.sched, 1) || !rd(&p.pad, 1)) return 2;
            p.depth = rd32();
            if (p.has_qos) {
                netflow::QosConfig qc;
                qc.num_queues = p.queues;
                qc.max_queue_depth = p.depth;
                qc.scheduler = static_cast<netflow::SchedulerType>(p.sched);
                qos.configure_port_qos(p.id, qc);
            }
        }
        const uint32_t ticks = rd32();
        for (uint32_t t = 0; t < ticks; ++t) {
            const uint32_t nf = rd32();
            for (uint32_t i = 0; i < nf; ++i) {
                const uint32_t port = rd32(), len = rd32();
                bufs.push_back(std::make_unique<netflow::PacketBuffer>(len + 16, 0, len));
                netflow::PacketBuffer* pb = bufs.back().get();
                memset(pb->get_data_start_ptr(), 0, len + 16);
                if (!rd(pb->get_data_start_ptr(), len)) return 2;
                netflow::Packet pkt(pb);
                wr32(qos.classify_packet_to_queue(pkt, port));
                qos.enqueue_packet(pkt, port);
            }
            stats(qos, ports);
            for (const Port& p : ports) {
                const uint32_t budget = rd32();
                std::vector<uint32_t> seq;
                for (uint32_t c = 0; c < budget; ++c) {
                    auto pkt = qos.select_packet_to_dequeue(p.id);
                    if (!pkt) break;
                    uint32_t s = 0;
                    memcpy(&s, pkt->get_buffer()->get_data_start_ptr() + 18, 4);
                    seq.push_back(s);
                }
                wr32((uint32_t)seq.size());
                wr(seq.data(), seq.size() * 4);
            }
            stats(qos, ports);
        }
    }
    return fclose(g_out) == 0 ? 0 : 3;
}

// l2_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_l2_golden.py).
//
// Walks the L2 data plane of Switch::process_received_packet (switch.hpp:305-326) over a list of frames
// with the reference's own code: the FDB is built through ForwardingDatabase::learn_mac and
// add_static_entry and comes back through get_all_entries(); the ports go through
// VlanManager::configure_port; every frame is a netflow::Packet whose dst_mac() / src_mac() / vlan_id()
// feed lookup_port and should_forward in the switch's order. Link and STP state are booleans the probe
// holds itself (the reference has no setter for an STP state); a port not listed is link down and not
// STP-forwarding, the reference's defaults. The learn class of a frame comes from get_all_entries()
// before and after learn_mac(src_mac, ingress, vlan) on a COPY of the FDB. The flood list restates
// flood_packet's port loop (switch.hpp:180-186) with the reference's should_forward. Compiled against
// the reference's headers in place plus src/netflow++/forwarding_database.cpp and vlan_manager.cpp;
// the binary goes to oracle/_ref/ (git-ignored).
//
// stdin (little-endian):
//   u32 n_ops, n_ops x {u8 kind (0 learn_mac, 1 add_static_entry), u8 pad, mac[6], u16 vlan, u16 pad, u32 port}
//   u32 n_ports, n_ports x {u32 port_id, u8 link_up, u8 stp_forwarding, u8 has_vlan_config, u8 type,
//                           u16 native_vlan, u16 n_allowed, n_allowed x u16}
//   u32 num_ports (the switch's port count, for the flood loop)
//   u32 n_runs, n_runs x u32 ingress port
//   u32 n_vlans, n_vlans x u16 (the VLANs to list flood ports for), padded to a multiple of 4 bytes
//   u32 nf, nf x {u32 len, bytes}
// stdout:
//   u32 ne, ne x {mac[6], u16 vlan_id, u32 port, u8 is_static, u8 pad[3]}   (get_all_entries() order)
//   per run: nf x {u32 verdict, u32 egress port or 0xFFFFFFFF, u32 vlan, u32 learn class}
//   per run, per listed VLAN: u32 count, count x u32 port
// Verdicts and learn classes carry the values of include/nfcs.h NFCS_L2_* / NFCS_L2_LEARN_*.
#include <netflow++/forwarding_database.hpp>
#include <netflow++/packet.hpp>
#include <netflow++/vlan_manager.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

namespace {

enum : uint32_t { FORWARD = 0, NO_ETH = 3, FLOOD = 4, SAME_PORT = 5, LINK_DOWN = 6, STP = 7, VLAN = 8 };
enum : uint32_t { LEARN_NONE = 0, LEARN_NEW = 1, LEARN_REFRESH = 2, LEARN_MOVED = 3 };
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Window {  // a PacketBuffer whose data window is the caller's frame (as tests/golden/acl_probe.cpp)
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
uint16_t rd16() { uint16_t v = 0; rd(&v, 2); return v; }
void wr32(uint32_t v) { wr(&v, 4); }

struct PortState { bool link = false, stp = false; };
std::map<uint32_t, PortState> g_state;
bool link_up(uint32_t p) { auto it = g_state.find(p); return it != g_state.end() && it->second.link; }
bool stp_fwd(uint32_t p) { auto it = g_state.find(p); return it != g_state.end() && it->second.stp; }

const netflow::FdbEntry* find(const std::vector<netflow::FdbEntry>& v, const netflow::MacAddress& m, uint16_t vlan) {
    for (const netflow::FdbEntry& e : v)
        if (e.mac == m && e.vlan_id == vlan) return &e;
    return nullptr;
}

}  // namespace

int main() {
    netflow::ForwardingDatabase fdb;
    netflow::VlanManager vm;
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
        uint8_t b[4];
        if (!rd(b, 4)) return 2;
        const uint16_t native = rd16(), n_allowed = rd16();
        netflow::VlanManager::PortConfig cfg;
        cfg.type = static_cast<netflow::PortType>(b[3]);
        cfg.native_vlan = native;
        cfg.allowed_vlans.clear();
        for (uint16_t k = 0; k < n_allowed; ++k) cfg.allowed_vlans.insert(rd16());
        if (n_allowed & 1u) rd16();
        g_state[id].link = b[0] != 0;
        g_state[id].stp = b[1] != 0;
        if (b[2]) vm.configure_port(id, cfg);
    }
    const uint32_t num_ports = rd32();
    std::vector<uint32_t> runs(rd32());
    for (uint32_t& r : runs) r = rd32();
    std::vector<uint16_t> vlans(rd32());
    for (uint16_t& v : vlans) v = rd16();
    if (vlans.size() & 1u) rd16();
    const uint32_t nf = rd32();
    std::vector<std::vector<uint8_t>> frames(nf);
    std::vector<uint32_t> lens(nf);
    for (uint32_t i = 0; i < nf; ++i) {
        lens[i] = rd32();
        frames[i].assign(lens[i] + 16, 0);
        if (!rd(frames[i].data(), lens[i])) return 2;
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
        for (uint32_t i = 0; i < nf; ++i) {
            Window w;
            w.point(frames[i].data(), lens[i]);
            netflow::Packet pkt(&w.pb);
            uint32_t verdict = NO_ETH, egress = NONE, vlan = 0, learn = LEARN_NONE;
            netflow::EthernetHeader* eth_hdr = pkt.ethernet();
            if (eth_hdr && pkt.dst_mac().has_value()) {
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
                    else { verdict = FORWARD; egress = port; }
                } else {
                    verdict = FLOOD;
                }
                // learn_mac on a copy, classified from the entries before and after
                const netflow::MacAddress src = pkt.src_mac().value();
                netflow::ForwardingDatabase copy = fdb;
                const netflow::FdbEntry* before = find(all, src, vlan_for_lookup);
                const bool was_new = copy.learn_mac(src, ingress, vlan_for_lookup);
                const std::vector<netflow::FdbEntry>& now = copy.get_all_entries();
                const netflow::FdbEntry* after = find(now, src, vlan_for_lookup);
                if (!after) return 4;
                if (!before) {
                    if (!was_new || now.size() != all.size() + 1) return 4;
                    learn = LEARN_NEW;
                } else {
                    if (was_new || now.size() != all.size()) return 4;
                    if (after->port != before->port) learn = LEARN_MOVED;
                    else learn = after->is_static ? LEARN_NONE : LEARN_REFRESH;
                    if (after->is_static && after->port != before->port) return 4;
                    if (!after->is_static && after->port != ingress) return 4;
                }
            }
            wr32(verdict);
            wr32(egress);
            wr32(vlan);
            wr32(learn);
        }
    }
    for (const uint32_t ingress : runs) {
        for (const uint16_t vlan : vlans) {
            std::vector<uint32_t> out;
            for (uint32_t i = 0; i < num_ports; ++i) {
                if (i == ingress) continue;
                if (!link_up(i) || !stp_fwd(i) || !vm.should_forward(ingress, i, vlan)) continue;
                out.push_back(i);
            }
            wr32((uint32_t)out.size());
            wr(out.data(), out.size() * 4);
        }
    }
    return fflush(stdout) == 0 ? 0 : 3;
}

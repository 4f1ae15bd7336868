// acl_probe.cpp — FIXTURE GENERATION ONLY (tests/golden/make_acl_golden.py).
//
// Runs the reference's ACL decision over a list of frames with the reference's own code: the rules go
// through AclManager::add_rule (and compile_rules when asked) and come back through get_all_rules();
// every frame is a netflow::Packet that AclManager::evaluate decides. evaluate() returns the action
// and the redirect port but not WHICH rule decided, so the probe also asks the reference whether each
// rule alone matches the frame — one single-rule ACL per rule, the rule's action replaced by DENY, so
// that evaluate() returns DENY exactly when check_match holds — and reports the first such rule in
// get_all_rules() order. It fails (exit 4) unless the action and port of the full evaluate() are what
// that first rule implies, so "the first match in vector order decides" is itself checked against the
// reference here. Compiled against the reference's headers in place plus
// src/netflow++/acl_manager.cpp; the binary goes to oracle/_ref/ (git-ignored).
//
// A rule record (little-endian, 56 bytes): u32 fields (bit k = optional k engaged, in the order src_mac,
//   dst_mac, vlan_id, ethertype, src_ip, dst_ip, protocol, src_port, dst_port), u32 rule_id, src_mac[6],
//   dst_mac[6], u16 vlan_id, u16 ethertype, u32 src_ip, u32 dst_ip (host order), u32 x 2 unused, u16
//   src_port, u16 dst_port, u8 protocol, u8 action, u8 pad[2], u32 redirect port (0xFFFFFFFF = absent),
//   i32 priority.
// stdin: u32 nr, nr x record; u32 compile (1 = compile_rules after adding); u32 nf, nf x {u32 len, bytes}
// stdout: u32 nt, nt x record (get_all_rules() order);
//   nf x {u32 action (REDIRECT without a port arrives as DENY), u32 index of the deciding rule in that
//   order or 0xFFFFFFFF, u32 redirect port or 0xFFFFFFFF}
#include <netflow++/acl_manager.hpp>
#include <netflow++/logger.hpp>
#include <netflow++/packet.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

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
    if (r.redirect_port != 0xFFFFFFFFu) a.redirect_port_id = r.redirect_port;
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
    r.redirect_port = a.redirect_port_id ? *a.redirect_port_id : 0xFFFFFFFFu;
    return r;
}

}  // namespace

int main() {
    netflow::SwitchLogger logger(netflow::LogLevel::CRITICAL);
    netflow::AclManager mgr(logger);
    mgr.create_acl("acl");
    const uint32_t nr = rd32();
    for (uint32_t i = 0; i < nr; ++i) {
        Rec r;
        if (!rd(&r, sizeof r)) return 2;
        if (!mgr.add_rule("acl", to_rule(r))) return 2;
    }
    if (rd32() == 1u) mgr.compile_rules("acl");
    const std::vector<netflow::AclRule> rules = mgr.get_all_rules("acl");
    wr32((uint32_t)rules.size());
    for (size_t i = 0; i < rules.size(); ++i) {
        const Rec r = from_rule(rules[i]);
        wr(&r, sizeof r);
        // the rule alone, deciding DENY: evaluate() == DENY <=> check_match(pkt, rule)
        netflow::AclRule alone = rules[i];
        alone.action = netflow::AclActionType::DENY;
        alone.redirect_port_id.reset();
        const std::string name = "rule" + std::to_string(i);
        mgr.create_acl(name);
        mgr.add_rule(name, alone);
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
        uint32_t port = 0xFFFFFFFFu;
        const netflow::AclActionType act = mgr.evaluate("acl", pkt, port);
        if (act != netflow::AclActionType::REDIRECT) port = 0xFFFFFFFFu;
        uint32_t first = 0xFFFFFFFFu;
        for (size_t k = 0; k < rules.size() && first == 0xFFFFFFFFu; ++k) {
            uint32_t unused = 0;
            if (mgr.evaluate("rule" + std::to_string(k), pkt, unused) == netflow::AclActionType::DENY) first = (uint32_t)k;
        }
        // what the first matching rule implies, against what evaluate() returned
        netflow::AclActionType want = netflow::AclActionType::PERMIT;
        uint32_t want_port = 0xFFFFFFFFu;
        if (first != 0xFFFFFFFFu) {
            want = rules[first].action;
            if (want == netflow::AclActionType::REDIRECT) {
                if (rules[first].redirect_port_id) want_port = *rules[first].redirect_port_id;
                else want = netflow::AclActionType::DENY;
            }
        }
        if (want != act || want_port != port) {
            fprintf(stderr, "frame %u: evaluate() %d port %u, first matching rule %u implies %d port %u\n", i,
                    static_cast<int>(act), port, first, static_cast<int>(want), want_port);
            return 4;
        }
        wr32((uint32_t)static_cast<int>(act));
        wr32(first);
        wr32(port);
    }
    return fflush(stdout) == 0 ? 0 : 3;
}

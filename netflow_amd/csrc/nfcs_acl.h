// nfcs_acl.h — the ACL's host side: the compile step of nfcs_acl_commit and the one-frame decision of
// nfcs_acl_eval_host. Pure C++ (no HIP), so it also builds into a stand-alone host program
// (tests/cpp/acl_compile_main.cpp, run under the host sanitizers). The device side (upload, launch)
// is in nfcs_api.hip / nfcs_kernels.hip.
//
// AclManager::check_match (acl_manager.cpp:198-278) is a chain of std::optional tests against the
// Packet accessors. Here a frame becomes a KEY of eight dwords once — its fields, zero where the
// accessor would return nothing, plus presence bits that say which accessors returned something — and
// a rule becomes value[8] / mask[8]: it matches when ((key[i] ^ value[i]) & mask[i]) == 0 for all i.
// A field the rule sets puts its bits in mask and its value in value, together with the presence bit
// the reference's accessor chain requires for it.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "nfcs.h"

namespace nfcs {

// Key dwords. Frame bytes 0..11 (the MACs) as three little-endian dwords, then numbers.
enum : uint32_t {
    kAkMac0 = 0,   // frame bytes 0..3: dst_mac[0..3]
    kAkMac1 = 1,   // frame bytes 4..7: dst_mac[4..5], src_mac[0..1]
    kAkMac2 = 2,   // frame bytes 8..11: src_mac[2..5]
    kAkL2 = 3,     // vlan id | effective EtherType << 16
    kAkSrcIp = 4,  // ntohl(src_ip)
    kAkDstIp = 5,  // ntohl(dst_ip)
    kAkPorts = 6,  // src port | dst port << 16 (host-order numbers)
    kAkMeta = 7    // protocol | presence bits
};
// Presence bits of key[kAkMeta]: what the reference's accessors return for this frame.
constexpr uint32_t kApEth = 1u << 8;     // ethernet(): len >= 14 (src_mac(), dst_mac())
constexpr uint32_t kApVlan = 1u << 9;    // vlan_id(): bytes 12-13 == 0x8100 and len >= 18
constexpr uint32_t kApEtype = 1u << 10;  // the effective EtherType is known (untagged, or tagged with len >= 18)
constexpr uint32_t kApIpv4 = 1u << 11;   // effective EtherType 0x0800 and ipv4(): l2 + 20 <= len
constexpr uint32_t kApPorts = 1u << 12;  // tcp() (protocol 6, l4 + 19 <= len) or udp() (17, l4 + 8 <= len)
constexpr uint32_t kApNever = 1u << 31;  // never set in a key: a padding rule asks for it
// Never set in a key either, and only ever set in a rule's MASK (its value bit stays 0, so it changes no
// match): the rule tests one of the dwords 0..3 (MACs, VLAN id, EtherType). The kernel reads those halves
// of a trip's rules only when one of them says so; a list of address / port rules never does.
constexpr uint32_t kApNeedL2 = 1u << 30;

// The scan reads kAclGroup rules per trip; the array is padded to a multiple with rules no key matches.
constexpr uint32_t kAclGroup = 4;

struct AclRec {  // 64 bytes: one compiled rule
    uint32_t value[8];
    uint32_t mask[8];
};
static_assert(sizeof(AclRec) == 64, "a compiled ACL rule is a 64-byte record");

struct AclAct {  // per rule: the decision it makes when it matches
    uint32_t action;    // NFCS_ACL_PERMIT / DENY / REDIRECT, REDIRECT without a port already folded to DENY
    uint32_t redirect;  // the port of NFCS_ACL_REDIRECT, else NFCS_IF_NONE
};

// What the evaluation reads (host copies; the kernel reads the same arrays from device memory).
struct AclTables {
    std::vector<AclRec> rec;  // in scan order, padded to a multiple of kAclGroup
    std::vector<AclAct> act;  // per rule (no padding)
    uint32_t rules = 0;       // entries before the padding
};

inline void acl_compile(const std::vector<nfcs_acl_rule>& in, AclTables& t) {
    t = AclTables{};
    t.rules = (uint32_t)in.size();
    for (const nfcs_acl_rule& r : in) {
        AclRec c{};
        auto want = [&](uint32_t word, uint32_t mask, uint32_t value) {
            c.mask[word] |= mask;
            c.value[word] |= value & mask;
        };
        const uint32_t f = r.fields;
        if (f & NFCS_ACL_F_DST_MAC) {  // pkt.dst_mac() present and equal (acl_manager.cpp:203-206)
            want(kAkMac0, 0xFFFFFFFFu, r.dst_mac[0] | (r.dst_mac[1] << 8) | (r.dst_mac[2] << 16) | ((uint32_t)r.dst_mac[3] << 24));
            want(kAkMac1, 0x0000FFFFu, r.dst_mac[4] | (r.dst_mac[5] << 8));
            want(kAkMeta, kApEth, kApEth);
        }
        if (f & NFCS_ACL_F_SRC_MAC) {  // 199-202
            want(kAkMac1, 0xFFFF0000u, ((uint32_t)r.src_mac[0] << 16) | ((uint32_t)r.src_mac[1] << 24));
            want(kAkMac2, 0xFFFFFFFFu, r.src_mac[2] | (r.src_mac[3] << 8) | (r.src_mac[4] << 16) | ((uint32_t)r.src_mac[5] << 24));
            want(kAkMeta, kApEth, kApEth);
        }
        if (f & NFCS_ACL_F_VLAN_ID) {  // 207-210; the key's id is at most 0x0FFF, so a larger value never matches
            want(kAkL2, 0x0000FFFFu, r.vlan_id);
            want(kAkMeta, kApVlan, kApVlan);
        }
        const uint32_t ip_fields = NFCS_ACL_F_SRC_IP | NFCS_ACL_F_DST_IP | NFCS_ACL_F_PROTOCOL | NFCS_ACL_F_SRC_PORT |
                                   NFCS_ACL_F_DST_PORT;
        // 212-233: with no Ethernet header, or behind a tag without a VLAN header, a rule that sets any
        // of these fails; one that sets none goes on
        if (f & (NFCS_ACL_F_ETHERTYPE | ip_fields)) want(kAkMeta, kApEtype, kApEtype);
        if (f & NFCS_ACL_F_ETHERTYPE) want(kAkL2, 0xFFFF0000u, (uint32_t)r.ethertype << 16);
        if (f & ip_fields) want(kAkMeta, kApIpv4, kApIpv4);  // 236-245: EtherType 0x0800 and ipv4()
        if (f & NFCS_ACL_F_SRC_IP) want(kAkSrcIp, r.src_ip_mask, r.src_ip);  // 248, with the mask extension
        if (f & NFCS_ACL_F_DST_IP) want(kAkDstIp, r.dst_ip_mask, r.dst_ip);
        if (f & NFCS_ACL_F_PROTOCOL) want(kAkMeta, 0xFFu, r.protocol);  // 250-252 (256-258 says the same again)
        if (f & (NFCS_ACL_F_SRC_PORT | NFCS_ACL_F_DST_PORT)) want(kAkMeta, kApPorts, kApPorts);  // 259-271
        if (f & NFCS_ACL_F_SRC_PORT) want(kAkPorts, 0x0000FFFFu, r.src_port);
        if (f & NFCS_ACL_F_DST_PORT) want(kAkPorts, 0xFFFF0000u, (uint32_t)r.dst_port << 16);
        if (c.mask[kAkMac0] | c.mask[kAkMac1] | c.mask[kAkMac2] | c.mask[kAkL2]) c.mask[kAkMeta] |= kApNeedL2;
        t.rec.push_back(c);
        // evaluate(), 180-189: REDIRECT without redirect_port_id returns DENY at this rule
        AclAct a{r.action, NFCS_IF_NONE};
        if (r.action == NFCS_ACL_REDIRECT) {
            if (r.redirect_port == NFCS_IF_NONE) a.action = NFCS_ACL_DENY;
            else a.redirect = r.redirect_port;
        }
        t.act.push_back(a);
    }
    AclRec never{};
    never.value[kAkMeta] = never.mask[kAkMeta] = kApNever;
    while (t.rec.size() % kAclGroup) t.rec.push_back(never);
}

// The key of one frame: every field check_match can read, through the reference's bounds
// (packet.hpp:405-643: 14-byte EthernetHeader, 4-byte VlanHeader, 20-byte IPv4Header, 19-byte
// TcpHeader, 8-byte UdpHeader; l4 = l2 + IHL*4 whatever IHL says). The kernel builds the same key
// from LDS (nfcs_kernels.hip acl_eval_kernel).
inline void acl_key(const uint8_t* b, uint32_t len, uint32_t k[8]) {
    for (uint32_t i = 0; i < 8; ++i) k[i] = 0;
    if (len < 14) return;
    auto be16 = [&](uint32_t o) { return ((uint32_t)b[o] << 8) | b[o + 1]; };
    auto le32 = [&](uint32_t o) { return b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24); };
    auto be32 = [&](uint32_t o) { return (be16(o) << 16) | be16(o + 2); };
    uint32_t meta = kApEth;
    k[kAkMac0] = le32(0);
    k[kAkMac1] = le32(4);
    k[kAkMac2] = le32(8);
    const uint32_t e12 = be16(12);
    const bool tagged = e12 == 0x8100u;
    const uint32_t l2 = tagged ? 18u : 14u;
    uint32_t et = e12, vlan = 0;
    bool known = true;
    if (tagged) {
        known = len >= 18;
        if (known) {
            vlan = be16(14) & 0x0FFFu;
            et = be16(16);
            meta |= kApVlan;
        } else {
            et = 0;
        }
    }
    if (known) meta |= kApEtype;
    k[kAkL2] = vlan | (et << 16);
    if (known && et == 0x0800u && l2 + 20u <= len) {
        meta |= kApIpv4;
        k[kAkSrcIp] = be32(l2 + 12u);
        k[kAkDstIp] = be32(l2 + 16u);
        const uint32_t proto = b[l2 + 9u];
        meta |= proto;
        const uint32_t l4 = l2 + (b[l2] & 15u) * 4u;
        if ((proto == 6 && l4 + 19u <= len) || (proto == 17 && l4 + 8u <= len)) {
            meta |= kApPorts;
            k[kAkPorts] = be16(l4) | (be16(l4 + 2u) << 16);
        }
    }
    k[kAkMeta] = meta;
}

// AclManager::evaluate over the compiled rules: the first rule in order that matches, or NFCS_ACL_NO_MATCH.
inline uint32_t acl_first_match(const AclTables& t, const uint32_t k[8]) {
    for (uint32_t r = 0; r < t.rules; ++r) {
        const AclRec& c = t.rec[r];
        uint32_t d = 0;
        for (uint32_t i = 0; i < 8; ++i) d |= (k[i] ^ c.value[i]) & c.mask[i];
        if (d == 0) return r;
    }
    return NFCS_ACL_NO_MATCH;
}

inline void acl_decide(const AclTables& t, const uint8_t* frame, uint32_t len, uint32_t* action, uint32_t* rule_index,
                       uint32_t* redirect_port) {
    uint32_t k[8];
    acl_key(frame, len, k);
    const uint32_t r = acl_first_match(t, k);
    if (action) *action = r == NFCS_ACL_NO_MATCH ? NFCS_ACL_PERMIT : t.act[r].action;
    if (rule_index) *rule_index = r;
    if (redirect_port) *redirect_port = r == NFCS_ACL_NO_MATCH ? NFCS_IF_NONE : t.act[r].redirect;
}

}  // namespace nfcs

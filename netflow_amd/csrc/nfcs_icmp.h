// nfcs_icmp.h — the ICMP responder's host side: inputs, the compile step of nfcs_icmp_commit, the one-packet
// plan (which message a packet calls for, and every header byte of it) and the sequential walk of
// nfcs_icmp_respond_host. Pure C++ (no HIP), so it also builds into a stand-alone host program
// (tests/cpp/icmp_test.cpp, run under the host sanitizers). The plan is ONE definition for host and device
// (NFCS_HD): the kernels of nfcs_kernels.hip call icmp_plan on the frame in device memory and differ from the
// walk below only in how the bytes behind the header are moved and summed. The device side (upload, launch)
// is in nfcs_api.hip / nfcs_kernels.hip.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "nfcs.h"
#include "nfcs_fdb.h"  // flood_sat_add, flood_round_up: the region arithmetic is the flood stage's
#include "nfcs_fib.h"

namespace nfcs {

constexpr uint32_t kIcmpHdr = 42;       // Ethernet 14 + IPv4 20 + ICMP 8: every message starts with these
constexpr uint32_t kIcmpHdrDwords = 11; // the plan fixes message bytes 0..43
constexpr uint32_t kIcmpMaxPorts = NFCS_L2_MAX_PORTS;

struct IcmpInputs {
    std::vector<nfcs_icmp_local> local;
    std::vector<nfcs_icmp_if_ip> if_ips;
    std::vector<uint32_t> up;
    uint32_t num_ports = 0;
};

// What the responder reads (host copies; the kernels read the same arrays from device memory).
struct IcmpTables {
    std::vector<uint32_t> local_ip;   // distinct addresses ascending as u32; of duplicates the first given wins
    std::vector<U2> local_mac;        // per address: MAC bytes 0-3 in x, bytes 4-5 in the low half of y
    std::vector<uint32_t> if_id;      // distinct interfaces ascending; of duplicates the first given wins
    std::vector<uint32_t> if_ip;      // per interface: its first address
    std::vector<uint32_t> up;         // (num_ports + 31) / 32 words: bit p = port p is up; at least one word
    uint32_t num_ports = 0;
};

struct IcmpView {
    const uint32_t* local_ip;
    const U2* local_mac;
    uint32_t locals;
    const uint32_t* if_id;
    const uint32_t* if_ip;
    uint32_t ifs;
    const uint32_t* up;
    uint32_t num_ports;
};
inline IcmpView icmp_view(const IcmpTables& t) {
    return IcmpView{t.local_ip.data(), t.local_mac.data(), (uint32_t)t.local_ip.size(), t.if_id.data(), t.if_ip.data(),
                    (uint32_t)t.if_id.size(), t.up.data(), t.num_ports};
}

inline void icmp_compile(const IcmpInputs& in, IcmpTables& t) {
    t = IcmpTables{};
    std::vector<uint32_t> order(in.local.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return in.local[a].ip < in.local[b].ip; });
    for (uint32_t i : order) {
        if (!t.local_ip.empty() && t.local_ip.back() == in.local[i].ip) continue;  // stable: the first given stays
        const uint8_t* m = in.local[i].mac;
        t.local_ip.push_back(in.local[i].ip);
        t.local_mac.push_back(U2{(uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24),
                                 (uint32_t)m[4] | ((uint32_t)m[5] << 8)});
    }
    order.resize(in.if_ips.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return in.if_ips[a].egress_if < in.if_ips[b].egress_if; });
    for (uint32_t i : order) {
        if (!t.if_id.empty() && t.if_id.back() == in.if_ips[i].egress_if) continue;
        t.if_id.push_back(in.if_ips[i].egress_if);
        t.if_ip.push_back(in.if_ips[i].ip);
    }
    t.num_ports = in.num_ports;
    t.up.assign((in.num_ports + 31u) / 32u + 1u, 0u);
    for (uint32_t p : in.up)
        if (p < in.num_ports) t.up[p >> 5] |= 1u << (p & 31u);  // a port >= num_ports can never send (switch.hpp:143)
}

// send_control_plane_packet's test (switch.hpp:143).
NFCS_HD inline bool icmp_port_ok(const IcmpView& t, uint32_t port) {
    return port < t.num_ports && ((t.up[port >> 5] >> (port & 31u)) & 1u);
}

// Which message one packet calls for, and message bytes 0..43 with both checksum fields zero.
struct IcmpPlan {
    uint32_t status;   // NFCS_ICMP_ST_* before the overflow rule
    uint32_t msg_len;  // 0: no message
    uint32_t port;     // send_control_plane_packet's port
    int32_t shift;     // message byte b >= 44 (and below msg_len) is frame byte b + shift; a multiple of 4
    uint32_t hdr[kIcmpHdrDwords];  // little-endian dwords of message bytes 0..43 (bytes at or past msg_len: zero)
};

NFCS_HD inline uint32_t icmp_be16(const uint8_t* f, uint32_t o) { return ((uint32_t)f[o] << 8) | f[o + 1]; }
NFCS_HD inline uint32_t icmp_le32(const uint8_t* f, uint32_t o) {
    return (uint32_t)f[o] | ((uint32_t)f[o + 1] << 8) | ((uint32_t)f[o + 2] << 16) | ((uint32_t)f[o + 3] << 24);
}
// Frame byte o, or 0 at and past `end` (end <= len: nothing past the frame is read).
NFCS_HD inline uint32_t icmp_byte(const uint8_t* f, uint32_t o, uint32_t end) { return o < end ? f[o] : 0u; }

// The reference's fold over a big-endian sum (packet.hpp:907-911), as the two bytes in memory order packed
// little-endian (byte 0 in bits 0-7).
NFCS_HD inline uint32_t icmp_fin_le(uint32_t be_sum) {
    while (be_sum >> 16) be_sum = (be_sum & 0xFFFFu) + (be_sum >> 16);
    const uint32_t c = (~be_sum) & 0xFFFFu;
    return (c >> 8) | ((c & 0xFFu) << 8);
}

// f: the frame's bytes (len of them, len below 2^32), live. verdict: NFCS_RT_* of the route lookup. ip_id: the
// IPv4 identification of an error message (host order).
NFCS_HD inline IcmpPlan icmp_plan(const IcmpView& t, const FibView& fib, uint32_t ingress, const uint8_t* f, uint32_t len,
                                  uint32_t verdict, uint32_t ip_id) {
    IcmpPlan p;
    p.status = NFCS_ICMP_ST_NONE;
    p.msg_len = 0u;
    p.port = NFCS_IF_NONE;
    p.shift = 0;
    for (uint32_t i = 0; i < kIcmpHdrDwords; ++i) p.hdr[i] = 0u;
    if (verdict != NFCS_RT_LOCAL && verdict != NFCS_RT_TTL_EXPIRED && verdict != NFCS_RT_NO_ROUTE) return p;
    // the lookup's predicate again (the three verdicts imply it; a caller's array is not trusted with reads)
    if (len < 34u) return p;
    const bool tagged = icmp_be16(f, 12) == 0x8100u;
    const uint32_t l2 = tagged ? 18u : 14u;
    if (l2 + 20u > len || icmp_be16(f, l2 - 2u) != 0x0800u) return p;
    const uint32_t ihl4 = (f[l2] & 15u) * 4u, l4 = l2 + ihl4;
    const uint32_t src = icmp_le32(f, l2 + 12u), dst = icmp_le32(f, l2 + 16u);  // network order as a u32
    uint32_t mac_d0, mac_d1, mac_s0, mac_s1;  // bytes 0-3 / 4-5 of the two MACs
    uint32_t ip_src, ip_dst, type, body;      // body: ICMP bytes beyond type/code/checksum start at message byte 38
    if (verdict == NFCS_RT_LOCAL) {
        if (f[l2 + 9u] != 1u) { p.status = NFCS_ICMP_ST_TO_CPU; return p; }
        p.status = NFCS_ICMP_ST_IGNORED;
        if (l4 + 8u > len) return p;                       // icmp() is null
        if (f[l4] != 8u || f[l4 + 1u] != 0u) return p;     // not an echo request
        const uint32_t li = fib_find(t.local_ip, t.locals, dst);
        if (li == NFCS_NH_NONE) { p.status = NFCS_ICMP_ST_NO_LOCAL_MAC; return p; }
        const uint32_t tl = icmp_be16(f, l2 + 2u);
        if (tl < ihl4 + 8u) return p;
        uint32_t payload = tl - ihl4 - 8u;
        if (l4 + 8u + payload > len) payload = 0u;         // icmp_processor.cpp:117-122
        if (28u + payload > 65535u) { p.status = NFCS_ICMP_ST_TOO_LONG; return p; }
        if (!icmp_port_ok(t, ingress)) { p.status = NFCS_ICMP_ST_PORT_DOWN; return p; }
        p.status = NFCS_ICMP_ST_ECHO_REPLY;
        p.msg_len = kIcmpHdr + payload;
        p.port = ingress;
        p.shift = (int32_t)(l4 + 8u) - (int32_t)kIcmpHdr;
        mac_d0 = icmp_le32(f, 6);
        mac_d1 = (uint32_t)f[10] | ((uint32_t)f[11] << 8);
        mac_s0 = t.local_mac[li].x;
        mac_s1 = t.local_mac[li].y;
        ip_src = dst;
        ip_dst = src;
        type = 0u;
        ip_id = 0u;
        // identifier, sequence number and the first two payload bytes: frame bytes l4 + 4 .. l4 + 9
        const uint32_t end = l4 + 8u + payload;
        body = icmp_le32(f, l4 + 4u);
        p.hdr[10] = (body >> 16) | (icmp_byte(f, l4 + 8u, end) << 16) | (icmp_byte(f, l4 + 9u, end) << 24);
        body <<= 16;  // bytes 38-39 of dword 9
    } else {
        uint32_t rv, nh, eif;
        fib_resolve(fib, src, &rv, &nh, &eif);                // icmp_processor.cpp:212-251, in its order
        if (rv == NFCS_RT_NO_ROUTE) { p.status = NFCS_ICMP_ST_SRC_NO_ROUTE; return p; }
        uint32_t ii = NFCS_NH_NONE;
        {
            uint32_t lo = 0, hi = t.ifs;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (t.if_id[mid] < eif) lo = mid + 1u;
                else hi = mid;
            }
            if (lo < t.ifs && t.if_id[lo] == eif) ii = lo;
        }
        if (ii == NFCS_NH_NONE) { p.status = NFCS_ICMP_ST_SRC_NO_IF_IP; return p; }
        if (rv == NFCS_RT_ARP_MISS) { p.status = NFCS_ICMP_ST_SRC_ARP_MISS; return p; }
        if (rv != NFCS_RT_FORWARD) { p.status = NFCS_ICMP_ST_SRC_NO_IF_MAC; return p; }
        if (l4 > len) { p.status = NFCS_ICMP_ST_OOB; return p; }  // the reference copies past its buffer
        if (!icmp_port_ok(t, eif)) { p.status = NFCS_ICMP_ST_PORT_DOWN; return p; }
        const uint32_t avail = len - l4, copied = ihl4 + (avail < 8u ? avail : 8u);  // 255-265
        const bool ttl = verdict == NFCS_RT_TTL_EXPIRED;
        p.status = ttl ? NFCS_ICMP_ST_TIME_EXCEEDED : NFCS_ICMP_ST_UNREACHABLE;
        p.msg_len = kIcmpHdr + copied;
        p.port = eif;
        p.shift = (int32_t)l2 - (int32_t)kIcmpHdr;
        const uint8_t* m = fib.table[nh].dst_mac;
        const uint8_t* s = fib.table[nh].src_mac;
        mac_d0 = icmp_le32(m, 0);
        mac_d1 = (uint32_t)m[4] | ((uint32_t)m[5] << 8);
        mac_s0 = icmp_le32(s, 0);
        mac_s1 = (uint32_t)s[4] | ((uint32_t)s[5] << 8);
        ip_src = t.if_ip[ii];
        ip_dst = src;
        type = ttl ? 11u : 3u;
        body = 0u;
        const uint32_t end = l2 + copied;
        p.hdr[10] = (icmp_byte(f, l2, end) << 16) | (icmp_byte(f, l2 + 1u, end) << 24);
    }
    const uint32_t tot = p.msg_len - 14u;  // the IPv4 total length, at most 65535
    p.hdr[0] = mac_d0;
    p.hdr[1] = mac_d1 | (mac_s0 << 16);
    p.hdr[2] = (mac_s0 >> 16) | (mac_s1 << 16);
    p.hdr[3] = 0x00450008u;                                              // 08 00 | 45 00
    p.hdr[4] = (tot >> 8) | ((tot & 0xFFu) << 8) | ((ip_id >> 8) & 0xFFu) << 16 | (ip_id & 0xFFu) << 24;
    p.hdr[5] = 0x01400000u;                                              // no fragment | TTL 64, protocol 1
    p.hdr[6] = ip_src << 16;                                             // header checksum 0 | source
    p.hdr[7] = (ip_src >> 16) | (ip_dst << 16);
    p.hdr[8] = (ip_dst >> 16) | (type << 16);                            // | type, code 0
    p.hdr[9] = body;                                                     // ICMP checksum 0 | bytes 38-39
    // the IPv4 header checksum from the message's own bytes 14..33 (update_checksums, packet.hpp:738-745)
    uint32_t s = 0;
    for (uint32_t w = 7; w < 17u; ++w) {  // big-endian words at bytes 2w
        const uint32_t h = (p.hdr[w >> 1] >> (16u * (w & 1u))) & 0xFFFFu;
        s += ((h & 0xFFu) << 8) | (h >> 8);
    }
    p.hdr[6] |= icmp_fin_le(s);
    return p;
}

// Message bytes 34.. as the reference sums them (calculate_checksum: big-endian words, an odd last byte added
// as the LOW byte, packet.hpp:898-905), for the walk below. m: the message with its ICMP checksum bytes zero.
inline uint32_t icmp_sum_be(const uint8_t* m, uint32_t len) {
    uint32_t s = 0, i = 34u;
    for (; i + 1u < len; i += 2u) s += ((uint32_t)m[i] << 8) | m[i + 1u];
    if (i < len) s += m[i];
    return s;
}

inline bool icmp_args_ok(uint64_t arena_bytes, uint64_t msg_base, uint32_t msg_align) {
    return msg_align >= 16u && !(msg_align & (msg_align - 1u)) && !(msg_base & (msg_align - 1u)) && msg_base <= arena_bytes;
}

// The three call sites (switch.hpp:271/279/301) over the burst, one packet after another (nfcs.h,
// nfcs_icmp_respond_device: the rules). The message arrays have `cap` entries; entries [messages, cap) are
// written inert. A message's bytes [msg_len, round_up(msg_len, 16)) are written zero, the rest of its slot is
// not written.
inline void icmp_respond(const IcmpTables& it, const FibTables& ft, uint32_t ingress, uint8_t* arena, uint64_t arena_bytes,
                         uint64_t msg_base, uint32_t msg_align, const nfcs_desc* desc, uint32_t n, const uint8_t* rt_verdict,
                         const uint16_t* ip_id, uint32_t cap, nfcs_desc* msg_desc, uint32_t* msg_port, uint32_t* msg_src,
                         uint8_t* status, nfcs_icmp_totals* tot) {
    const IcmpView iv = icmp_view(it);
    const FibView fv = fib_view(ft);
    nfcs_icmp_totals r{};
    uint64_t k = 0, used = 0;  // messages called for so far; slot bytes called for so far
    bool open = true;          // every message so far was emitted
    std::vector<uint8_t> m;
    for (uint32_t i = 0; i < n; ++i) {
        if (status) status[i] = NFCS_ICMP_ST_NONE;
        const uint64_t off = (uint64_t)desc[i].off16 * 16u, len = desc[i].len;
        if (off + flood_round_up(len, 16u) > msg_base) continue;  // not live
        const uint8_t* f = arena + off;
        const IcmpPlan p = icmp_plan(iv, fv, ingress, f, desc[i].len, rt_verdict[i], ip_id ? ip_id[i] : 0u);
        if (status) status[i] = (uint8_t)p.status;
        if (!p.msg_len) continue;
        const uint64_t slot = flood_round_up(p.msg_len, msg_align), at = flood_sat_add(msg_base, used);
        used = flood_sat_add(used, slot);
        open = open && k < cap && flood_sat_add(msg_base, used) <= arena_bytes;
        ++k;
        if (!open) {
            if (status) status[i] = NFCS_ICMP_ST_OVERFLOW;
            continue;
        }
        const uint32_t padded = (uint32_t)flood_round_up(p.msg_len, 16u);
        m.assign(padded, 0);
        for (uint32_t b = 0; b < 44u && b < p.msg_len; ++b) m[b] = (uint8_t)(p.hdr[b >> 2] >> (8u * (b & 3u)));
        for (uint32_t b = 44u; b < p.msg_len; ++b) m[b] = f[(int64_t)b + p.shift];
        const uint32_t c = icmp_fin_le(icmp_sum_be(m.data(), p.msg_len));
        m[36] = (uint8_t)c;
        m[37] = (uint8_t)(c >> 8);
        memcpy(arena + at, m.data(), padded);
        msg_desc[k - 1u] = nfcs_desc{(uint32_t)(at / 16u), p.msg_len};
        msg_port[k - 1u] = p.port;
        msg_src[k - 1u] = i;
        ++r.messages;
        if (p.status == NFCS_ICMP_ST_ECHO_REPLY) ++r.echo_replies;
        else ++r.errors;
        r.msg_bytes += slot;
    }
    r.messages_needed = (uint32_t)k;
    r.msg_bytes_needed = used;
    for (uint64_t j = r.messages; j < cap; ++j) {
        msg_desc[j] = nfcs_desc{0u, 0u};
        msg_port[j] = NFCS_IF_NONE;
        msg_src[j] = NFCS_ITEM_NONE;
    }
    *tot = r;
}

}  // namespace nfcs

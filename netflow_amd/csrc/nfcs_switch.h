// nfcs_switch.h — the ingress dispatch stage: the lines of Switch::process_received_packet (switch.hpp:213-329)
// that belong to no manager, written once for the host walk of nfcs_ingress_dispatch_host and for the kernel
// (nfcs_kernels.hip ingress_dispatch_kernel): sw_classify below is compiled for both. Pure C/C++ (no HIP, no
// allocation), so it also builds into a stand-alone host program (tests/cpp/switch_dispatch_main.cpp, run under
// the host sanitizers). The order of the tests is the reference's; each line cites its switch.hpp line.
#pragma once

#include <stdint.h>
#include <string.h>

#include "nfcs.h"

#if defined(__HIPCC__)
#define NFCS_SW_HD __host__ __device__
#else
#define NFCS_SW_HD
#endif

namespace nfcs {

constexpr uint32_t kSwLinkUp = 1u;  // nfcs_fdb.h kL2LinkUp: the port state byte's is_port_link_up bit

NFCS_SW_HD inline uint32_t sw_be16(uint32_t lo16) { return ((lo16 & 0xFFu) << 8) | ((lo16 >> 8) & 0xFFu); }

// Whether the frame of a descriptor may be read: its 16-byte chunks lie inside the arena.
NFCS_SW_HD inline bool sw_desc_live(uint32_t off16, uint32_t len, uint64_t arena_bytes) {
    return (uint64_t)off16 * 16u + (((uint64_t)len + 15u) & ~15ull) <= arena_bytes;
}

// Which frames are read at all, and how far: a permitted frame with an Ethernet header (250), bytes 0..15, and
// bytes 16..19 where the inner EtherType lies inside the frame (pkt.vlan() needs len >= 18, 262).
NFCS_SW_HD inline bool sw_bad(uint32_t action, uint32_t rt, bool live) {
    return action == NFCS_ACL_BAD_DESC || rt == NFCS_RT_BAD_DESC || !live;
}
NFCS_SW_HD inline bool sw_reads_head(uint32_t action, uint32_t rt, bool live, uint32_t len) {
    return !sw_bad(action, rt, live) && action == NFCS_ACL_PERMIT && len >= 14u;
}
NFCS_SW_HD inline bool sw_reads_inner(uint32_t action, uint32_t rt, bool live, uint32_t len) {
    return sw_reads_head(action, rt, live, len) && len >= 18u;
}

// One frame of a burst whose ingress link is up. w0, w1, w3: the little-endian words at bytes 0, 4 and 12 of the
// frame, w4: the one at byte 16; each is 0 where sw_reads_head / sw_reads_inner say it is not read. red_up: the
// redirect port's link (looked up only for redirect < num_ports).
NFCS_SW_HD inline uint32_t sw_classify(uint32_t len, bool live, uint32_t action, uint32_t redirect, uint32_t num_ports,
                                       bool red_up, uint32_t rt, uint32_t l2v, uint32_t w0, uint32_t w1, uint32_t w3,
                                       uint32_t w4) {
    if (sw_bad(action, rt, live)) return NFCS_SW_BAD_DESC;  // the frame is not read; not a drop
    if (action == NFCS_ACL_DENY) return NFCS_SW_IN_DENY;    // 226-229
    if (action == NFCS_ACL_REDIRECT) {                      // 231-243
        if (redirect >= num_ports) return NFCS_SW_RED_RANGE;  // 233, first term
        if (!red_up) return NFCS_SW_RED_DOWN;                 // 233, second term
        return NFCS_SW_RED_OK;                                // 239-242
    }
    if (action != NFCS_ACL_PERMIT) return NFCS_SW_BAD_DESC;  // no such action: handled as an unreadable frame
    if (len >= 14u) {  // eth_hdr (250)
        const uint32_t outer = sw_be16(w3 & 0xFFFFu);
        if (outer == 0x88CCu) return NFCS_SW_LLDP;                          // 252
        if (w0 == 0u && (w1 & 0xFFFFu) == 0u) return NFCS_SW_ZERO_MAC;      // 253: MacAddress() is all zero
        const uint32_t l3 = (outer == 0x8100u && len >= 18u) ? sw_be16(w4 & 0xFFFFu) : outer;  // 259-264
        if (l3 == 0x0806u) return NFCS_SW_ARP;                              // 266
    }
    switch (rt) {  // 267-303
        case NFCS_RT_FORWARD: return NFCS_SW_L3_FWD;
        case NFCS_RT_LOCAL: return NFCS_SW_LOCAL;          // 270-276
        case NFCS_RT_TTL_EXPIRED: return NFCS_SW_TTL;      // 279
        case NFCS_RT_NO_ROUTE: return NFCS_SW_NO_ROUTE;    // 301
        case NFCS_RT_ARP_MISS: return NFCS_SW_ARP_MISS;    // 300
        case NFCS_RT_NO_IF_MAC: return NFCS_SW_NO_IF_MAC;  // 292
        default: break;                                    // NFCS_RT_NOT_IPV4: the L2 block (305-326)
    }
    switch (l2v) {
        case NFCS_L2_FORWARD: return NFCS_SW_L2_FWD;              // 320
        case NFCS_L2_FLOOD: return NFCS_SW_L2_FLOOD;              // 323
        case NFCS_L2_DROP_SAME_PORT: return NFCS_SW_SAME_PORT;    // 314
        case NFCS_L2_DROP_LINK_DOWN: return NFCS_SW_LINK_DOWN;    // 314
        case NFCS_L2_DROP_STP: return NFCS_SW_STP;                // 315
        case NFCS_L2_DROP_VLAN: return NFCS_SW_VLAN;              // 316
        case NFCS_L2_BAD_DESC: return NFCS_SW_BAD_DESC;
        default: return NFCS_SW_UNHANDLED;                        // 328: no Ethernet header
    }
}

// What a class means for the three in/out arrays and the counters.
NFCS_SW_HD inline bool sw_masked(uint32_t cls) {  // no forward, no port, no flood
    return cls == NFCS_SW_RX_DOWN || cls == NFCS_SW_BAD_DESC || cls == NFCS_SW_IN_DENY || cls == NFCS_SW_RED_RANGE ||
           cls == NFCS_SW_RED_DOWN || cls == NFCS_SW_LLDP || cls == NFCS_SW_ZERO_MAC || cls == NFCS_SW_ARP;
}
NFCS_SW_HD inline bool sw_drop(uint32_t cls) {  // _increment_rx_stats(port, len, false, true) at 228 and 235
    return cls == NFCS_SW_IN_DENY || cls == NFCS_SW_RED_RANGE || cls == NFCS_SW_RED_DOWN;
}

// The sequential definition (nfcs_ingress_dispatch_host). port_state: `ports` state bytes (FdbTables).
inline void sw_dispatch(const uint8_t* port_state, uint32_t ports, uint32_t ingress, uint32_t num_ports,
                        const uint8_t* arena, uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n,
                        const uint8_t* action, const uint32_t* redirect, const uint8_t* rt_verdict, uint32_t* nh,
                        uint32_t* l2_port, uint8_t* l2_verdict, uint8_t* cls_out, uint8_t* bypass,
                        nfcs_rx_stats* rx_stats) {
    const bool rx_up = ingress < ports && (port_state[ingress] & kSwLinkUp);  // 215
    nfcs_rx_stats add = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t cls = NFCS_SW_RX_DOWN, red = NFCS_IF_NONE;
        if (rx_up) {
            const uint32_t len = desc[i].len, act = action ? action[i] : NFCS_ACL_PERMIT, rt = rt_verdict[i];
            red = redirect ? redirect[i] : NFCS_IF_NONE;
            const bool live = sw_desc_live(desc[i].off16, len, arena_bytes);
            add.rx_packets += 1u;  // 216
            add.rx_bytes += len;
            uint32_t w[5] = {0, 0, 0, 0, 0};
            const uint8_t* f = arena + (uint64_t)desc[i].off16 * 16u;
            if (sw_reads_head(act, rt, live, len)) memcpy(w, f, len < 16u ? len : 16u);
            if (sw_reads_inner(act, rt, live, len)) memcpy(w + 4, f + 16, len < 20u ? len - 16u : 4u);
            const bool red_up = red < num_ports && red < ports && (port_state[red] & kSwLinkUp);
            cls = sw_classify(len, live, act, red, num_ports, red_up, rt, l2_verdict[i], w[0], w[1], w[3], w[4]);
            if (sw_drop(cls)) {  // 228, 235: all three counters once more
                add.rx_packets += 1u;
                add.rx_bytes += len;
                add.rx_drops += 1u;
            }
        }
        if (sw_masked(cls) || cls == NFCS_SW_RED_OK) {
            nh[i] = NFCS_NH_NONE;
            l2_port[i] = cls == NFCS_SW_RED_OK ? red : NFCS_IF_NONE;  // 239-240: the redirect port takes the packet
            l2_verdict[i] = NFCS_L2_SKIP;
        }
        if (cls_out) cls_out[i] = (uint8_t)cls;
        if (bypass) bypass[i] = cls == NFCS_SW_RED_OK;  // 238: no egress ACL on the redirect port
    }
    if (rx_stats && rx_up) {
        rx_stats[ingress].rx_packets += add.rx_packets;
        rx_stats[ingress].rx_bytes += add.rx_bytes;
        rx_stats[ingress].rx_drops += add.rx_drops;
    }
}

}  // namespace nfcs

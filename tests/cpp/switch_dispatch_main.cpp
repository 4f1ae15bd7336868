// switch_dispatch_main.cpp — the ingress dispatch's host definition (netflow_amd/csrc/nfcs_switch.h) as a
// stand-alone program, for the host sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Inetflow_amd/csrc
//       tests/cpp/switch_dispatch_main.cpp -o switch_dispatch_main && ./switch_dispatch_main
// Every frame lies in a heap block of exactly the arena's bytes, so a read past the arena is a report. The edge
// list is that of tests/dispatch_common.py (EDGES); the expected classes are written down here again.
#include <cstdio>
#include <cstring>
#include <vector>

#include "nfcs_switch.h"

namespace {

struct Edge {
    const char* what;
    std::vector<uint8_t> frame;
    uint32_t action, redirect, rt, l2v, cls;
};

std::vector<uint8_t> eth(uint32_t et, size_t len, int tci = -1, bool zero_dst = false) {
    std::vector<uint8_t> b;
    for (int i = 0; i < 6; ++i) b.push_back(zero_dst ? 0 : (i == 0 ? 2 : i == 5 ? 9 : 0));
    for (int i = 0; i < 6; ++i) b.push_back(i == 0 ? 2 : i == 5 ? 1 : 0);
    if (tci >= 0) {
        b.push_back(0x81), b.push_back(0x00), b.push_back((uint8_t)(tci >> 8)), b.push_back((uint8_t)tci);
    }
    b.push_back((uint8_t)(et >> 8)), b.push_back((uint8_t)et);
    b.resize(b.size() + 64, 0x5A);
    b.resize(len);
    return b;
}

int fails = 0;
void expect(bool ok, const char* what, const char* detail) {
    if (!ok) {
        std::fprintf(stderr, "FAIL %s: %s\n", what, detail);
        ++fails;
    }
}

}  // namespace

int main() {
    const uint32_t P = NFCS_ACL_PERMIT, D = NFCS_ACL_DENY, R = NFCS_ACL_REDIRECT, NONE = 0xFFFFFFFFu;
    const uint32_t NIP = NFCS_RT_NOT_IPV4, FWD = NFCS_RT_FORWARD, num_ports = 6;
    const uint8_t state[6] = {1, 1, 1, 0, 1, 1};  // port 3 is down
    const std::vector<Edge> edges = {
        {"0 bytes", {}, P, NONE, NIP, NFCS_L2_NO_ETH, NFCS_SW_UNHANDLED},
        {"13 bytes", eth(0x88CC, 13), P, NONE, NIP, NFCS_L2_NO_ETH, NFCS_SW_UNHANDLED},
        {"14 bytes LLDP", eth(0x88CC, 14), P, NONE, NIP, NFCS_L2_FLOOD, NFCS_SW_LLDP},
        {"14 bytes ARP", eth(0x0806, 14), P, NONE, NIP, NFCS_L2_FLOOD, NFCS_SW_ARP},
        {"17 bytes tagged, inner cut", eth(0x0806, 17, 5), P, NONE, NIP, NFCS_L2_FORWARD, NFCS_SW_L2_FWD},
        {"18 bytes tagged ARP", eth(0x0806, 18, 5), P, NONE, NIP, NFCS_L2_FLOOD, NFCS_SW_ARP},
        {"0x88CC behind a tag", eth(0x88CC, 60, 7), P, NONE, NIP, NFCS_L2_FORWARD, NFCS_SW_L2_FWD},
        {"IPv4 to the zero MAC", eth(0x0800, 60, -1, true), P, NONE, FWD, NFCS_L2_SKIP, NFCS_SW_ZERO_MAC},
        {"redirect == num_ports", eth(0x0800, 60), R, num_ports, FWD, NFCS_L2_SKIP, NFCS_SW_RED_RANGE},
        {"redirect == num_ports - 1", eth(0x0800, 60), R, num_ports - 1, FWD, NFCS_L2_SKIP, NFCS_SW_RED_OK},
        {"redirect == 0xFFFFFFFF", eth(0x0800, 60), R, NONE, FWD, NFCS_L2_SKIP, NFCS_SW_RED_RANGE},
        {"redirect to a down port", eth(0x0800, 60), R, 3, NIP, NFCS_L2_FLOOD, NFCS_SW_RED_DOWN},
        {"a denied ARP frame", eth(0x0806, 60), D, NONE, NIP, NFCS_L2_FLOOD, NFCS_SW_IN_DENY},
        {"ACL_BAD_DESC", eth(0x88CC, 60), NFCS_ACL_BAD_DESC, NONE, NFCS_RT_BAD_DESC, NFCS_L2_BAD_DESC, NFCS_SW_BAD_DESC},
        {"forwarded, 1500 bytes", eth(0x0800, 1500), P, NONE, FWD, NFCS_L2_SKIP, NFCS_SW_L3_FWD},
        {"the last frame ends with the arena: 18 bytes tagged", eth(0x0800, 18, 5), P, NONE, NIP, NFCS_L2_DROP_VLAN, NFCS_SW_VLAN},
    };
    const uint32_t n = (uint32_t)edges.size();
    std::vector<nfcs_desc> desc(n);
    size_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        desc[i] = nfcs_desc{(uint32_t)(pos / 16), (uint32_t)edges[i].frame.size()};
        pos += (edges[i].frame.size() + 15) / 16 * 16;
    }
    // the last frame's slot is cut to its length: the arena ends with the frame (arena_bytes still covers the slot)
    const size_t arena_bytes = pos, held = pos - 16 + 18 - 16;
    std::vector<uint8_t> store(held);
    uint8_t* arena = store.data();  // heap: the sanitizer sees every byte past `held`
    for (uint32_t i = 0; i < n; ++i)
        if (!edges[i].frame.empty()) std::memcpy(arena + (size_t)desc[i].off16 * 16, edges[i].frame.data(), edges[i].frame.size());

    for (int pass = 0; pass < 4; ++pass) {
        // pass 0: every output; 1: no optional output, no ingress list; 2: the ingress link down; 3: no such port
        const uint32_t ingress = pass == 2 ? 3u : pass == 3 ? 6u : 0u;
        std::vector<uint8_t> action(n), rt(n), l2v(n), cls(n, 0xEE), byp(n, 0xEE);
        std::vector<uint32_t> redirect(n), nh(n), l2p(n);
        for (uint32_t i = 0; i < n; ++i) {
            action[i] = (uint8_t)edges[i].action, rt[i] = (uint8_t)edges[i].rt, l2v[i] = (uint8_t)edges[i].l2v;
            redirect[i] = edges[i].redirect, nh[i] = 100 + i, l2p[i] = 200 + i;
        }
        nfcs_rx_stats rx[7] = {};
        const bool bare = pass == 1;
        nfcs::sw_dispatch(state, 6, ingress, num_ports, arena, arena_bytes, desc.data(), n, bare ? nullptr : action.data(),
                          bare ? nullptr : redirect.data(), rt.data(), nh.data(), l2p.data(), l2v.data(), bare ? nullptr : cls.data(),
                          bare ? nullptr : byp.data(), bare ? nullptr : rx);
        uint64_t pk = 0, by = 0, dr = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const Edge& e = edges[i];
            if (pass == 0) {
                const bool drop = e.cls == NFCS_SW_IN_DENY || e.cls == NFCS_SW_RED_DOWN || e.cls == NFCS_SW_RED_RANGE;
                pk += drop ? 2 : 1, by += (drop ? 2 : 1) * e.frame.size(), dr += drop;
                expect(cls[i] == e.cls, e.what, "class");
                expect(byp[i] == (e.cls == NFCS_SW_RED_OK), e.what, "bypass");
                const bool gone = nfcs::sw_masked(e.cls) || e.cls == NFCS_SW_RED_OK;
                expect(nh[i] == (gone ? NFCS_NH_NONE : 100 + i), e.what, "nh");
                expect(l2p[i] == (e.cls == NFCS_SW_RED_OK ? e.redirect : gone ? NFCS_IF_NONE : 200 + i), e.what, "l2_port");
                expect(l2v[i] == (gone ? (uint32_t)NFCS_L2_SKIP : e.l2v), e.what, "l2_verdict");
            } else if (pass >= 2) {
                expect(cls[i] == NFCS_SW_RX_DOWN && byp[i] == 0 && nh[i] == NFCS_NH_NONE && l2p[i] == NFCS_IF_NONE &&
                           l2v[i] == NFCS_L2_SKIP, e.what, "ingress down: not masked");
            }
        }
        if (pass == 0) expect(rx[0].rx_packets == pk && rx[0].rx_bytes == by && rx[0].rx_drops == dr && dr == 4, "counters", "pass 0");
        for (int p = pass == 0 ? 1 : 0; p < 7; ++p)
            expect(!rx[p].rx_packets && !rx[p].rx_bytes && !rx[p].rx_drops, "counters", "a counter that must not move did");
    }
    if (fails) return 1;
    std::printf("switch_dispatch_main: %u edges, 4 passes, ok\n", n);
    return 0;
}

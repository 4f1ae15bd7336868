// nfcs_fib.h — the forwarding table's host side: inputs, the compile step of nfcs_fib_commit and
// the one-address decision of nfcs_fib_lookup_host. Pure C++ (no HIP), so it also builds into a
// stand-alone host program (tests/cpp/fib_compile_main.cpp, run under the host sanitizers). The
// device side (upload, launch) is in nfcs_api.hip / nfcs_kernels.hip.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "nfcs.h"

#if defined(__HIPCC__)
#define NFCS_HD __host__ __device__
#else
#define NFCS_HD
#endif

namespace nfcs {

// What a route's word says (FibTables::rt_info[r].x): a next-hop index, or one of these.
constexpr uint32_t kRtConnected = 0xFFFFFFFEu;   // next_hop_ip == 0: ARP for the destination itself
constexpr uint32_t kRtGwArpMiss = 0xFFFFFFFDu;   // the gateway has no ARP entry
constexpr uint32_t kRtGwNoIfMac = 0xFFFFFFFCu;   // the gateway resolves, the interface has no MAC
constexpr uint32_t kRtCodeMin = kRtGwNoIfMac;    // words below are next-hop indexes
// The route scan reads {network, mask} pairs in groups of kRtGroup; the array is padded to a multiple
// with pairs no address matches ((dst & 0) == 1 never holds).
constexpr uint32_t kRtGroup = 8;
constexpr uint32_t kRtPadNetwork = 1u, kRtPadMask = 0u;

struct U2 { uint32_t x, y; };

// What the lookup reads (host copies; the kernel reads the same arrays from device memory).
struct FibTables {
    std::vector<U2> rt_nm;          // {network, mask} in lookup order, padded to a multiple of kRtGroup
    std::vector<U2> rt_info;        // per route: {next-hop index or kRt* code, egress_if}
    uint32_t routes = 0;            // entries before the padding
    std::vector<uint32_t> arp_ip;   // distinct ARP addresses, ascending as u32
    std::vector<uint32_t> arp_nh;   // per address: its next-hop index (its own position) or NFCS_NH_NONE
    std::vector<uint32_t> local_ip; // the switch's addresses, ascending, distinct
    std::vector<nfcs_nexthop> table;  // arp_ip.size() entries, then one per gateway route
};

struct FibInputs {
    std::vector<nfcs_fib_route> routes;
    std::vector<nfcs_fib_arp> arp;
    std::vector<nfcs_fib_if_mac> if_macs;
    std::vector<uint32_t> local_ips;
};

// Index of key in the ascending array a[0..n), or NFCS_NH_NONE. The kernel's search is the same loop.
NFCS_HD inline uint32_t fib_find(const uint32_t* a, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return (lo < n && a[lo] == key) ? lo : NFCS_NH_NONE;
}

// RoutingManager::lookup_route: the first entry in order that matches, or NFCS_NH_NONE.
inline uint32_t fib_first_route(const FibTables& t, uint32_t dst) {
    for (uint32_t r = 0; r < t.routes; ++r)
        if ((dst & t.rt_nm[r].y) == t.rt_nm[r].x) return r;
    return NFCS_NH_NONE;
}

inline void fib_compile(const FibInputs& in, FibTables& t) {
    t = FibTables{};
    // ARP: distinct addresses ascending; of duplicates the last one given wins
    std::vector<uint32_t> order(in.arp.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return in.arp[a].ip < in.arp[b].ip; });
    std::vector<uint32_t> pick;  // input index per distinct address
    for (uint32_t i = 0; i < order.size(); ++i) {
        if (!pick.empty() && in.arp[pick.back()].ip == in.arp[order[i]].ip) pick.back() = order[i];
        else pick.push_back(order[i]);
    }
    for (uint32_t i : pick) t.arp_ip.push_back(in.arp[i].ip);
    t.local_ip = in.local_ips;
    std::sort(t.local_ip.begin(), t.local_ip.end());
    t.local_ip.erase(std::unique(t.local_ip.begin(), t.local_ip.end()), t.local_ip.end());
    // interface MACs: the last one given wins
    auto if_mac = [&](uint32_t ifid) -> const uint8_t* {
        for (size_t i = in.if_macs.size(); i-- > 0;)
            if (in.if_macs[i].egress_if == ifid) return in.if_macs[i].mac;
        return nullptr;
    };
    t.routes = (uint32_t)in.routes.size();
    for (const nfcs_fib_route& r : in.routes) t.rt_nm.push_back(U2{r.network, r.mask});
    while (t.rt_nm.size() % kRtGroup) t.rt_nm.push_back(U2{kRtPadNetwork, kRtPadMask});
    const uint32_t arps = (uint32_t)t.arp_ip.size();
    t.table.assign(arps, nfcs_nexthop{});
    t.arp_nh.assign(arps, NFCS_NH_NONE);
    // ARP entry a as a directly connected destination: its one first-matching route decides
    for (uint32_t a = 0; a < arps; ++a) {
        const uint32_t r = fib_first_route(t, t.arp_ip[a]);
        if (r == NFCS_NH_NONE || in.routes[r].next_hop_ip != 0) continue;
        const uint8_t* sm = if_mac(in.routes[r].egress_if);
        if (!sm) continue;
        memcpy(t.table[a].dst_mac, in.arp[pick[a]].mac, 6);
        memcpy(t.table[a].src_mac, sm, 6);
        t.arp_nh[a] = a;
    }
    // routes: a gateway resolves once (ARP first, then the interface MAC: switch.hpp:286-292)
    for (const nfcs_fib_route& r : in.routes) {
        uint32_t word = kRtConnected;
        if (r.next_hop_ip != 0) {
            const uint32_t a = fib_find(t.arp_ip.data(), arps, r.next_hop_ip);
            const uint8_t* sm = if_mac(r.egress_if);
            if (a == NFCS_NH_NONE) word = kRtGwArpMiss;
            else if (!sm) word = kRtGwNoIfMac;
            else {
                nfcs_nexthop nh{};
                memcpy(nh.dst_mac, in.arp[pick[a]].mac, 6);
                memcpy(nh.src_mac, sm, 6);
                word = (uint32_t)t.table.size();
                t.table.push_back(nh);
            }
        }
        t.rt_info.push_back(U2{word, r.egress_if});
    }
}

// What a matching route says about one address: route word `word` (rt_info[r].x), the ARP arrays, the
// address the route was matched for. FORWARD (with the next-hop index), ARP_MISS or NO_IF_MAC
// (switch.hpp:285-292; icmp_processor.cpp:231-251 has the same two steps). Host and device, this one
// definition: fib_decide, fib_resolve, route_lookup_kernel and the ICMP stage's kernels call it.
NFCS_HD inline uint32_t fib_route_word(uint32_t word, const uint32_t* arp_ip, const uint32_t* arp_nh, uint32_t arps,
                                       uint32_t ip, uint32_t* nh) {
    *nh = NFCS_NH_NONE;
    if (word == kRtGwArpMiss) return NFCS_RT_ARP_MISS;
    if (word == kRtGwNoIfMac) return NFCS_RT_NO_IF_MAC;
    if (word == kRtConnected) {  // ARP for the address itself
        const uint32_t a = fib_find(arp_ip, arps, ip);
        if (a == NFCS_NH_NONE) return NFCS_RT_ARP_MISS;
        *nh = arp_nh[a];
        return *nh == NFCS_NH_NONE ? (uint32_t)NFCS_RT_NO_IF_MAC : (uint32_t)NFCS_RT_FORWARD;
    }
    *nh = word;
    return NFCS_RT_FORWARD;
}

// The compiled arrays as plain pointers: the host's vectors or the device copy of nfcs_fib_upload.
struct FibView {
    const U2* rt_nm;
    const U2* rt_info;
    uint32_t routes_padded;  // a multiple of kRtGroup; the padding pairs match nothing
    const uint32_t* arp_ip;
    const uint32_t* arp_nh;
    uint32_t arps;
    const nfcs_nexthop* table;
};
inline FibView fib_view(const FibTables& t) {
    return FibView{t.rt_nm.data(), t.rt_info.data(), (uint32_t)t.rt_nm.size(), t.arp_ip.data(), t.arp_nh.data(),
                   (uint32_t)t.arp_ip.size(), t.table.data()};
}

// Route -> next hop -> ARP -> interface MAC for one address, without fib_decide's is_my_ip and TTL steps
// (nfcs_fib_resolve_host; the source address of an ICMP error, icmp_processor.cpp:212-251). *verdict is
// FORWARD, NO_ROUTE, ARP_MISS or NO_IF_MAC; *egress_if is the first matching route's interface whenever a
// route matches, whatever the verdict (the ICMP stage tests the interface's address before ARP).
NFCS_HD inline void fib_resolve(const FibView& t, uint32_t ip, uint32_t* verdict, uint32_t* nh, uint32_t* egress_if) {
    uint32_t r = NFCS_NH_NONE;
    for (uint32_t i = 0; i < t.routes_padded && r == NFCS_NH_NONE; ++i)
        if ((ip & t.rt_nm[i].y) == t.rt_nm[i].x) r = i;
    *verdict = NFCS_RT_NO_ROUTE;
    *nh = NFCS_NH_NONE;
    *egress_if = NFCS_IF_NONE;
    if (r == NFCS_NH_NONE) return;
    *egress_if = t.rt_info[r].y;
    *verdict = fib_route_word(t.rt_info[r].x, t.arp_ip, t.arp_nh, t.arps, ip, nh);
}

// The decision after the header predicate (switch.hpp:270-301) for one destination and TTL.
inline void fib_decide(const FibTables& t, uint32_t dst, uint32_t ttl, uint32_t* verdict, uint32_t* nh,
                       uint32_t* egress_if) {
    uint32_t v, h = NFCS_NH_NONE, e = NFCS_IF_NONE;
    if (fib_find(t.local_ip.data(), (uint32_t)t.local_ip.size(), dst) != NFCS_NH_NONE) v = NFCS_RT_LOCAL;
    else if (ttl <= 1) v = NFCS_RT_TTL_EXPIRED;
    else {
        const uint32_t r = fib_first_route(t, dst);
        if (r == NFCS_NH_NONE) v = NFCS_RT_NO_ROUTE;
        else {
            v = fib_route_word(t.rt_info[r].x, t.arp_ip.data(), t.arp_nh.data(), (uint32_t)t.arp_ip.size(), dst, &h);
            if (v == NFCS_RT_FORWARD) e = t.rt_info[r].y;
        }
    }
    if (verdict) *verdict = v;
    if (nh) *nh = h;
    if (egress_if) *egress_if = e;
}

}  // namespace nfcs

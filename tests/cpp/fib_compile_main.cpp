// fib_compile_main.cpp — stand-alone host program over netflow_amd/csrc/nfcs_fib.h (no HIP, no GPU):
// compiles random forwarding tables and checks every decision of fib_decide against a direct walk of
// the inputs in the reference's order (first matching route, ARP of the gateway or of the destination,
// then the interface MAC; the last duplicate of an ARP entry or interface MAC wins). Built and run by
// tests/test_route_fib.py under -fsanitize=address,undefined. Exit status 0 = every decision agrees.
#include <stdio.h>
#include <stdlib.h>

#include "nfcs_fib.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

struct Want { uint32_t verdict; const uint8_t* dst_mac; const uint8_t* src_mac; uint32_t egress_if; };

Want direct(const nfcs::FibInputs& in, uint32_t dst, uint32_t ttl) {
    Want w{NFCS_RT_NO_ROUTE, nullptr, nullptr, NFCS_IF_NONE};
    for (uint32_t a : in.local_ips)
        if (a == dst) return w.verdict = NFCS_RT_LOCAL, w;
    if (ttl <= 1) return w.verdict = NFCS_RT_TTL_EXPIRED, w;
    for (const nfcs_fib_route& r : in.routes) {
        if ((dst & r.mask) != r.network) continue;
        const uint32_t target = r.next_hop_ip ? r.next_hop_ip : dst;
        for (const nfcs_fib_arp& a : in.arp)
            if (a.ip == target) w.dst_mac = a.mac;  // the last one wins
        for (const nfcs_fib_if_mac& m : in.if_macs)
            if (m.egress_if == r.egress_if) w.src_mac = m.mac;
        w.verdict = !w.dst_mac ? NFCS_RT_ARP_MISS : !w.src_mac ? NFCS_RT_NO_IF_MAC : NFCS_RT_FORWARD;
        if (w.verdict == NFCS_RT_FORWARD) w.egress_if = r.egress_if;
        return w;
    }
    return w;
}

}  // namespace

int main() {
    int bad = 0;
    for (int round = 0; round < 40 && !bad; ++round) {
        nfcs::FibInputs in;
        // addresses from a small space, so routes, ARP entries, gateways and locals collide
        auto addr = [] { return 0x0Au | ((rnd() % 4u) << 8) | ((rnd() % 4u) << 16) | ((rnd() % 16u) << 24); };
        const uint32_t nr = round == 0 ? 0 : rnd() % 40u, na = round == 1 ? 0 : rnd() % 60u;
        for (uint32_t i = 0; i < nr; ++i) {
            static const uint32_t masks[] = {0u, 0xFFu, 0xFFFFu, 0xFFFFFFu, 0xFFFFFFFFu, 0xFF00FFFFu, 0xF0FFFFFFu};
            const uint32_t mask = masks[rnd() % 7u];
            in.routes.push_back(nfcs_fib_route{addr() & mask, mask, rnd() % 3u ? 0u : addr(), rnd() % 6u});
        }
        for (uint32_t i = 0; i < na; ++i) {
            nfcs_fib_arp a{};
            a.ip = addr();
            for (uint8_t& b : a.mac) b = (uint8_t)rnd();
            in.arp.push_back(a);
        }
        for (uint32_t i = 0, n = rnd() % 8u; i < n; ++i) {
            nfcs_fib_if_mac m{};
            m.egress_if = rnd() % 6u;
            for (uint8_t& b : m.mac) b = (uint8_t)rnd();
            in.if_macs.push_back(m);
        }
        for (uint32_t i = 0, n = rnd() % 4u; i < n; ++i) in.local_ips.push_back(addr());
        nfcs::FibTables t;
        nfcs::fib_compile(in, t);
        for (int k = 0; k < 2000; ++k) {
            const uint32_t dst = addr(), ttl = rnd() % 4u;
            uint32_t v, nh, eif;
            nfcs::fib_decide(t, dst, ttl, &v, &nh, &eif);
            const Want w = direct(in, dst, ttl);
            bool ok = v == w.verdict && eif == w.egress_if && (v == NFCS_RT_FORWARD) == (nh != NFCS_NH_NONE);
            if (ok && v == NFCS_RT_FORWARD)
                ok = nh < t.table.size() && !memcmp(t.table[nh].dst_mac, w.dst_mac, 6) &&
                     !memcmp(t.table[nh].src_mac, w.src_mac, 6);
            if (!ok) {
                printf("round %d dst %08x ttl %u: verdict %u want %u, nh %u, if %u want %u\n", round, dst, ttl, v,
                       w.verdict, nh, eif, w.egress_if);
                ++bad;
                break;
            }
        }
    }
    printf(bad ? "FAIL\n" : "fib compile OK\n");
    return bad ? 1 : 0;
}

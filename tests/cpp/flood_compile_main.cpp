// flood_compile_main.cpp — stand-alone host program over netflow_amd/csrc/nfcs_fdb.h (no HIP, no GPU):
// compiles random port tables and checks (1) every flood mask of the per-VLAN port bitmap (fdb_flood_word)
// against fdb_flood_ports, the scan of the ports that nfcs_fdb_flood_ports_host serves, and (2) the host walk
// flood_expand against a direct walk of the burst over those port lists, with the item arrays in heap
// blocks of exactly `cap` entries and cap and the copy region cut short, so that a store past the emitted
// prefix or past cap is reported. Built and run by tests/test_flood.py under -fsanitize=address,undefined.
// Exit status 0 = everything agrees.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "nfcs_fdb.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

const uint16_t kVlans[] = {0, 1, 10, 31, 32, 4095};
constexpr uint32_t kNumVlans = sizeof kVlans / sizeof kVlans[0];
const uint32_t kLens[] = {0, 14, 16, 17, 64, 1500};

struct Item { nfcs_desc d; uint32_t port, src; bool copy; };

int check(uint32_t ports_n, uint32_t n) {
    nfcs::FdbInputs in;
    in.ports.resize(ports_n);
    for (uint32_t p = 0; p < ports_n; ++p) {
        nfcs::FdbPortIn& pi = in.ports[p];
        pi.set = rnd() % 8u != 0;
        pi.port.port_id = p;
        pi.port.link_up = rnd() % 8u != 0;
        pi.port.stp_forwarding = rnd() % 8u != 0;
        pi.port.has_vlan_config = rnd() % 8u != 0;
        pi.port.type = (uint8_t)(rnd() % 3u);
        pi.port.native_vlan = kVlans[rnd() % kNumVlans];
        for (uint32_t k = 0; k < kNumVlans; ++k)
            if (rnd() % 2u) pi.allowed.push_back(kVlans[k]);
    }
    nfcs::FdbTables t;
    nfcs::fdb_compile(in, t);
    if (t.port_words != (ports_n + 31u) / 32u || t.vlan_ports.size() != (size_t)nfcs::kL2Vlans * t.port_words) return 1;

    // (1) the mask against the scan
    const uint32_t ingresses[] = {0, 1, 31, 32, 33, ports_n ? ports_n - 1u : 0u, ports_n, ports_n + 40u};
    const uint32_t counts[] = {0, 1, 31, 32, 33, ports_n ? ports_n - 1u : 0u, ports_n, ports_n + 1u, 5000};
    for (uint32_t ingress : ingresses)
        for (uint32_t num_ports : counts)
            for (uint32_t k = 0; k <= kNumVlans; ++k) {
                const uint32_t vlan = k < kNumVlans ? kVlans[k] : 77u;
                std::vector<uint32_t> want(ports_n + 1u), got;
                want.resize(nfcs::fdb_flood_ports(t, ingress, vlan, num_ports, want.data(), (uint32_t)want.size()));
                const bool in_ok = nfcs::fdb_vlan_bit(t, ingress, vlan);
                const uint32_t* row = t.vlan_ports.data() + (size_t)vlan * t.port_words;
                for (uint32_t w = 0; w < t.port_words; ++w)
                    for (uint32_t m = nfcs::fdb_flood_word(row, w, ingress, num_ports, in_ok); m; m &= m - 1u)
                        got.push_back(w * 32u + (uint32_t)__builtin_ctz(m));
                if (got != want) {
                    printf("mask differs: ports %u ingress %u num_ports %u vlan %u\n", ports_n, ingress, num_ports, vlan);
                    return 1;
                }
            }

    // (2) the walk
    for (int round = 0; round < 6; ++round) {
        const uint32_t ingress = ingresses[rnd() % 8u], num_ports = counts[1u + rnd() % 8u], align = 16u << (rnd() % 4u);
        std::unique_ptr<nfcs_desc[]> desc(new nfcs_desc[n]);
        std::unique_ptr<uint32_t[]> l3(new uint32_t[n]), l2(new uint32_t[n]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[n]), verdict(new uint8_t[n]);
        std::unique_ptr<uint16_t[]> vlan(new uint16_t[n]);
        uint64_t pos = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t len = kLens[rnd() % 6u];
            desc[i] = nfcs_desc{(uint32_t)(pos / 16u), len};
            pos += (len + 15u) / 16u * 16u;
            l3[i] = rnd() % 4u ? NFCS_IF_NONE : rnd() % 70u;
            l2[i] = rnd() % 3u ? NFCS_IF_NONE : rnd() % 70u;
            st[i] = (uint8_t)(rnd() % 2u ? NFCS_ST_FLAG_FWD | 1u : 1u);
            verdict[i] = (uint8_t)(rnd() % 4u ? NFCS_L2_FLOOD : NFCS_L2_DROP_VLAN);
            vlan[i] = rnd() % 16u ? kVlans[rnd() % kNumVlans] : (uint16_t)(4096u + rnd() % 100u);
        }
        if (n > 3) desc[3].off16 = 0xFFFFFFFFu;  // dead
        const uint64_t copy_base = nfcs::flood_round_up(pos, 128u) - (round % 2 && pos >= 256u ? 128u : 0u);
        const bool use_l3 = round % 3 != 0, use_st = use_l3 && round % 2, use_verdict = round != 4;
        // the direct walk
        std::vector<Item> full;
        std::vector<uint64_t> end;  // the copy region's end after each item
        uint64_t used = 0;
        uint32_t flooded = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if ((uint64_t)desc[i].off16 * 16u + (desc[i].len + 15ull) / 16u * 16u > copy_base) continue;
            uint32_t port = NFCS_IF_NONE;
            if (use_l3 && l3[i] != NFCS_IF_NONE && (!use_st || (st[i] & NFCS_ST_FLAG_FWD))) port = l3[i];
            else port = l2[i];
            if (port != NFCS_IF_NONE) {
                full.push_back(Item{desc[i], port, i, false});
                end.push_back(copy_base + used);
            } else if (use_verdict && verdict[i] == NFCS_L2_FLOOD) {
                ++flooded;
                std::vector<uint32_t> ports(ports_n + 1u);
                ports.resize(nfcs::fdb_flood_ports(t, ingress, vlan[i], num_ports, ports.data(), (uint32_t)ports.size()));
                for (uint32_t p : ports) {
                    full.push_back(Item{nfcs_desc{(uint32_t)((copy_base + used) / 16u), desc[i].len}, p, i, true});
                    used += nfcs::flood_round_up(desc[i].len, align);
                    end.push_back(copy_base + used);
                }
            }
        }
        const uint32_t caps[] = {(uint32_t)full.size() + 3u, (uint32_t)full.size(), (uint32_t)full.size() / 2u, 0u};
        const uint64_t rooms[] = {used + 64u, used, used / 2u, 0u};
        for (uint32_t cap : caps)
            for (uint64_t room : rooms) {
                std::unique_ptr<nfcs_desc[]> item_desc(new nfcs_desc[cap]);
                std::unique_ptr<uint32_t[]> item_port(new uint32_t[cap]), item_src(new uint32_t[cap]);
                nfcs_flood_totals tot;
                if (!nfcs::flood_args_ok(num_ports, copy_base + room, copy_base, align, n, use_l3, use_st, true, use_verdict, true))
                    return 1;
                nfcs::flood_expand(t, ingress, num_ports, copy_base + room, copy_base, align, desc.get(), n,
                                   use_l3 ? l3.get() : nullptr, use_st ? st.get() : nullptr, l2.get(),
                                   use_verdict ? verdict.get() : nullptr, vlan.get(), cap, item_desc.get(), item_port.get(),
                                   item_src.get(), &tot);
                uint32_t m = 0;
                while (m < full.size() && m < cap && end[m] <= copy_base + room) ++m;
                bool ok = tot.items == m && tot.items_needed == full.size() && tot.flooded == flooded &&
                          tot.copy_bytes_needed == used;
                uint32_t copies = 0;
                for (uint32_t k = 0; k < m && ok; ++k) {
                    ok = item_desc[k].off16 == full[k].d.off16 && item_desc[k].len == full[k].d.len &&
                         item_port[k] == full[k].port && item_src[k] == full[k].src;
                    copies += full[k].copy;
                }
                for (uint32_t k = m; k < cap && ok; ++k)
                    ok = item_desc[k].off16 == 0 && item_desc[k].len == 0 && item_port[k] == NFCS_IF_NONE &&
                         item_src[k] == NFCS_ITEM_NONE;
                ok = ok && tot.copies == copies && tot.copy_bytes == (m ? end[m - 1] - copy_base : 0u);
                if (!ok) {
                    printf("walk differs: ports %u n %u round %d cap %u room %llu\n", ports_n, n, round, cap,
                           (unsigned long long)room);
                    return 1;
                }
            }
    }
    return 0;
}

}  // namespace

int main() {
    const uint32_t sizes[] = {0, 1, 5, 31, 32, 33, 64, 65, 200};
    for (uint32_t ports_n : sizes)
        for (uint32_t n : {0u, 1u, 7u, 120u})
            if (check(ports_n, n)) return 1;
    // a VLAN above 4095 and an empty table read no row
    nfcs::FdbTables t;
    nfcs::fdb_compile(nfcs::FdbInputs{}, t);
    if (t.port_words != 0 || !t.vlan_ports.empty()) return 1;
    printf("flood compile OK\n");
    return 0;
}

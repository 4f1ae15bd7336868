// fdb_compile_main.cpp — stand-alone host program over netflow_amd/csrc/nfcs_fdb.h (no HIP, no GPU):
// compiles random forwarding databases and port states and checks every decision of fdb_decide (hash
// probes, state bytes, VLAN bitmaps) and every list of fdb_flood_ports against a direct walk of the
// inputs written the way the switch's L2 block is (switch.hpp:305-326: a linear find_if over the entries,
// the port checks by id, should_forward from the configs). Built and run by tests/test_l2_fdb.py under
// -fsanitize=address,undefined; every frame lives in a heap block of exactly its length, so a read past
// it is reported. Exit status 0 = every decision agrees.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>

#include "nfcs_fdb.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

const uint16_t kVlans[] = {0, 1, 10, 20, 30, 99, 4095};
constexpr uint32_t kNumVlans = sizeof kVlans / sizeof kVlans[0];

const nfcs::FdbPortIn* port_of(const nfcs::FdbInputs& in, uint32_t p) {
    return p < in.ports.size() && in.ports[p].set ? &in.ports[p] : nullptr;
}
bool allows(const nfcs::FdbInputs& in, uint32_t p, uint32_t vlan) {
    const nfcs::FdbPortIn* pi = port_of(in, p);
    if (!pi || !pi->port.has_vlan_config) return false;
    if (pi->port.type == 0) return vlan == pi->port.native_vlan;
    return std::find(pi->allowed.begin(), pi->allowed.end(), (uint16_t)vlan) != pi->allowed.end();
}
const nfcs_fdb_entry* direct_find(const nfcs::FdbInputs& in, const uint8_t* mac, uint32_t vlan) {
    for (const nfcs_fdb_entry& e : in.entries)
        if (!memcmp(e.mac, mac, 6) && e.vlan_id == vlan) return &e;  // find_if: the first
    return nullptr;
}

void direct_decide(const nfcs::FdbInputs& in, uint32_t ingress, const uint8_t* f, uint32_t len, uint32_t out[4]) {
    out[0] = NFCS_L2_NO_ETH, out[1] = NFCS_IF_NONE, out[2] = 0, out[3] = NFCS_L2_LEARN_NONE;
    if (len < 14) return;
    const nfcs::FdbPortIn* ing = port_of(in, ingress);
    uint32_t vlan = ing && ing->port.has_vlan_config ? ing->port.native_vlan : 1u;
    if (f[12] == 0x81 && f[13] == 0x00 && len >= 18) vlan = (((uint32_t)f[14] << 8) | f[15]) & 0x0FFFu;
    out[2] = vlan;
    const nfcs_fdb_entry* d = direct_find(in, f, vlan);
    if (!d) out[0] = NFCS_L2_FLOOD;
    else {
        const nfcs::FdbPortIn* eg = port_of(in, d->port);
        if (d->port == ingress) out[0] = NFCS_L2_DROP_SAME_PORT;
        else if (!eg || !eg->port.link_up) out[0] = NFCS_L2_DROP_LINK_DOWN;
        else if (!eg->port.stp_forwarding) out[0] = NFCS_L2_DROP_STP;
        else if (!allows(in, ingress, vlan) || !allows(in, d->port, vlan)) out[0] = NFCS_L2_DROP_VLAN;
        else out[0] = NFCS_L2_FORWARD, out[1] = d->port;
    }
    const nfcs_fdb_entry* s = direct_find(in, f + 6, vlan);
    out[3] = !s ? NFCS_L2_LEARN_NEW : s->is_static ? NFCS_L2_LEARN_NONE
           : s->port == ingress ? NFCS_L2_LEARN_REFRESH : NFCS_L2_LEARN_MOVED;
}

int check(uint32_t entries_n, uint32_t mac_pool, uint32_t ports_n) {
    nfcs::FdbInputs in;
    std::vector<nfcs_fdb_entry> pool(mac_pool);
    for (nfcs_fdb_entry& e : pool) {
        memset(&e, 0, sizeof e);
        for (int j = 0; j < 6; ++j) e.mac[j] = (uint8_t)(rnd() % (mac_pool < 8 ? 2u : 256u));  // small pools collide
    }
    for (uint32_t i = 0; i < entries_n; ++i) {  // keys may repeat: the first one wins
        nfcs_fdb_entry e = pool[rnd() % mac_pool];
        e.vlan_id = kVlans[rnd() % kNumVlans];
        e.port = rnd() % (ports_n + 3u);
        e.is_static = (uint8_t)(rnd() & 1u);
        in.entries.push_back(e);
    }
    in.ports.resize(ports_n);
    for (uint32_t p = 0; p < ports_n; ++p) {
        nfcs::FdbPortIn& pi = in.ports[p];
        if (rnd() % 8u == 0) continue;  // never set
        pi.set = true;
        pi.port.port_id = p;
        pi.port.link_up = rnd() % 6u != 0;
        pi.port.stp_forwarding = rnd() % 6u != 0;
        pi.port.has_vlan_config = rnd() % 6u != 0;
        pi.port.type = (uint8_t)(rnd() % 3u);
        pi.port.native_vlan = kVlans[rnd() % kNumVlans];
        for (uint32_t k = rnd() % 5u; k > 0; --k) pi.allowed.push_back(kVlans[rnd() % kNumVlans]);
    }
    nfcs::FdbTables t;
    nfcs::fdb_compile(in, t);
    const size_t ns = t.slots.size();
    if (ns < 16 || (ns & (ns - 1)) || ns < 2u * entries_n || t.entries > entries_n || t.max_probe > t.entries) {
        printf("table shape: %zu slots for %u entries, max_probe %u\n", ns, entries_n, t.max_probe);
        return 1;
    }
    int bad = 0;
    const uint32_t lens[] = {0, 13, 14, 15, 16, 17, 18, 19, 60};
    for (uint32_t i = 0; i < 3000 && bad < 5; ++i) {
        const uint32_t len = lens[rnd() % 9u];
        std::unique_ptr<uint8_t[]> f(new uint8_t[len ? len : 1]);  // exactly len bytes: a read past it is reported
        for (uint32_t j = 0; j < len; ++j) f[j] = (uint8_t)rnd();
        uint8_t hdr[18];
        memcpy(hdr, pool[rnd() % mac_pool].mac, 6);
        memcpy(hdr + 6, pool[rnd() % mac_pool].mac, 6);
        const bool tag = rnd() & 1u;
        const uint16_t vlan = kVlans[rnd() % kNumVlans];
        hdr[12] = tag ? 0x81 : 0x88, hdr[13] = tag ? 0x00 : 0xB5;
        hdr[14] = (uint8_t)(((rnd() & 0xF0u) | (vlan >> 8)) & 0xFFu), hdr[15] = (uint8_t)vlan;
        hdr[16] = hdr[17] = 0;
        memcpy(f.get(), hdr, len < 18 ? len : 18);
        const uint32_t ingress = rnd() % (ports_n + 2u);
        uint32_t got[4], want[4];
        nfcs::fdb_decide(t, ingress, f.get(), len, &got[0], &got[1], &got[2], &got[3]);
        direct_decide(in, ingress, f.get(), len, want);
        if (memcmp(got, want, sizeof got)) {
            printf("frame %u (len %u, ingress %u): got %u %u %u %u, want %u %u %u %u\n", i, len, ingress, got[0], got[1],
                   got[2], got[3], want[0], want[1], want[2], want[3]);
            ++bad;
        }
    }
    for (uint32_t i = 0; i < 200 && bad < 5; ++i) {
        const uint32_t ingress = rnd() % (ports_n + 2u), vlan = kVlans[rnd() % kNumVlans], num = rnd() % (ports_n + 4u);
        std::vector<uint32_t> want;
        for (uint32_t p = 0; p < num; ++p) {
            const nfcs::FdbPortIn* pi = port_of(in, p);
            if (p == ingress || !pi || !pi->port.link_up || !pi->port.stp_forwarding) continue;
            if (allows(in, ingress, vlan) && allows(in, p, vlan)) want.push_back(p);
        }
        const uint32_t cap = rnd() % (num + 1u);
        std::unique_ptr<uint32_t[]> out(new uint32_t[cap ? cap : 1]);  // exactly cap entries
        const uint32_t n = nfcs::fdb_flood_ports(t, ingress, vlan, num, out.get(), cap);
        bool ok = n == want.size();
        for (uint32_t k = 0; ok && k < std::min<uint32_t>(cap, n); ++k) ok = out[k] == want[k];
        if (!ok) {
            printf("flood list %u (ingress %u, vlan %u, %u ports): %u ports, want %zu\n", i, ingress, vlan, num, n, want.size());
            ++bad;
        }
    }
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    bad += check(0, 4, 0);
    bad += check(1, 4, 1);
    bad += check(40, 6, 5);      // a pool of few, similar MACs: repeated keys
    bad += check(8, 40, 12);     // 16 slots, half full
    bad += check(300, 200, 20);
    bad += check(5000, 3000, 64);
    printf(bad ? "FAIL\n" : "fdb compile OK\n");
    return bad ? 1 : 0;
}

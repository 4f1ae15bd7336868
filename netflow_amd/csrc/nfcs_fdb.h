// nfcs_fdb.h — the L2 forwarding database's host side: inputs, the compile step of nfcs_fdb_commit
// (an open-addressing hash table over (MAC, VLAN) and the per-port state the L2 block reads), the
// one-frame decision of nfcs_fdb_lookup_host, the flood list, the per-VLAN port bitmap behind the flood mask
// and the sequential walk of nfcs_flood_expand_host. Pure C++ (no HIP), so it also builds into a
// stand-alone host program (tests/cpp/fdb_compile_main.cpp and flood_compile_main.cpp, run under the host
// sanitizers). The
// device side (upload, launch) is in nfcs_api.hip / nfcs_kernels.hip; nfcs_internal.h includes this
// file, so the hash and the slot layout below are the kernel's as well: one definition each.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "nfcs.h"

#if defined(__HIPCC__)
#define NFCS_HD __host__ __device__
#else
#define NFCS_HD
#endif

namespace nfcs {

// One slot of the table, 16 bytes: one probe is one 16-byte load.
//   k0    MAC bytes 0..3 as they lie in the frame, read as one little-endian u32
//   k1    MAC bytes 4..5 in bits 0-15, the VLAN id in bits 16-31
//   port  the entry's port
//   flags kFdbOccupied | kFdbStatic. An empty slot is all zero; 00:00:00:00:00:00 on VLAN 0 is a
//         legal key, so only the flag says whether a slot holds an entry.
struct alignas(16) FdbSlot {
    uint32_t k0, k1, port, flags;
};
static_assert(sizeof(FdbSlot) == 16, "one probe is one 16-byte load");
constexpr uint32_t kFdbOccupied = 1u, kFdbStatic = 2u;
constexpr uint32_t kFdbMinSlots = 16;

// Per-port state byte (FdbTables::port_state).
constexpr uint32_t kL2LinkUp = 1u, kL2StpFwd = 2u, kL2HasCfg = 4u;
constexpr uint32_t kL2Vlans = 4096u;
constexpr uint32_t kL2VlanWords = kL2Vlans / 32u;  // one 4096-bit VLAN bitmap per port
constexpr uint32_t kL2DefaultVlan = 1;          // VlanManager::PortConfig().native_vlan

// The home slot of a key, before masking with slots - 1. Host and device, this one definition.
NFCS_HD inline uint32_t fdb_hash(uint32_t k0, uint32_t k1) {
    uint32_t h = k0 * 0x9E3779B1u;
    h ^= h >> 15;
    h = (h ^ k1) * 0x85EBCA77u;
    h ^= h >> 13;
    h *= 0xC2B2AE3Du;
    return h ^ (h >> 16);
}

inline uint32_t fdb_k0(const uint8_t* mac) {
    return (uint32_t)mac[0] | ((uint32_t)mac[1] << 8) | ((uint32_t)mac[2] << 16) | ((uint32_t)mac[3] << 24);
}
inline uint32_t fdb_k1(const uint8_t* mac, uint32_t vlan) {
    return (uint32_t)mac[4] | ((uint32_t)mac[5] << 8) | (vlan << 16);
}

struct FdbPortIn {
    bool set = false;
    nfcs_l2_port port{};
    std::vector<uint16_t> allowed;
};

struct FdbInputs {
    std::vector<nfcs_fdb_entry> entries;
    std::vector<FdbPortIn> ports;  // indexed by port id, as long as the highest id set + 1
};

// What the lookup reads (host copies; the kernel reads the same arrays from device memory).
struct FdbTables {
    std::vector<FdbSlot> slots;        // a power of two, >= 2 x entries, >= kFdbMinSlots
    uint32_t entries = 0;              // distinct keys in the table
    uint32_t max_probe = 0;            // the longest displacement of any entry, plus one (0: empty table)
    uint32_t wrapped = 0;              // entries whose probe sequence crossed from the last slot to slot 0
    uint32_t ports = 0;                // the highest port id set, plus one
    std::vector<uint8_t> port_state;   // per port: kL2LinkUp | kL2StpFwd | kL2HasCfg
    std::vector<uint16_t> port_native; // per port: native_vlan (kL2DefaultVlan without a config)
    std::vector<uint32_t> port_vlans;  // per port: kL2VlanWords words, bit v set = VLAN v passes
    // per VLAN one row of port_words words: bit p set = port p is link-up, STP-forwarding and has the VLAN's
    // bit. The transpose of port_vlans restricted to the ports a flood may leave through (fdb_flood_word).
    uint32_t port_words = 0;           // ceil(ports / 32)
    std::vector<uint32_t> vlan_ports;  // kL2Vlans x port_words
};

inline void fdb_compile(const FdbInputs& in, FdbTables& t) {
    t = FdbTables{};
    uint32_t ns = kFdbMinSlots;
    while ((uint64_t)ns < 2ull * in.entries.size()) ns *= 2u;
    t.slots.assign(ns, FdbSlot{0, 0, 0, 0});
    const uint32_t mask = ns - 1u;
    for (const nfcs_fdb_entry& e : in.entries) {
        const uint32_t k0 = fdb_k0(e.mac), k1 = fdb_k1(e.mac, e.vlan_id);
        const uint32_t home = fdb_hash(k0, k1) & mask;
        for (uint32_t d = 0; d < ns; ++d) {  // the table is at most half full: an empty slot comes
            FdbSlot& s = t.slots[(home + d) & mask];
            if (s.flags & kFdbOccupied) {
                if (s.k0 == k0 && s.k1 == k1) break;  // a key given twice: the first one stays
                continue;
            }
            s = FdbSlot{k0, k1, e.port, kFdbOccupied | (e.is_static ? kFdbStatic : 0u)};
            ++t.entries;
            if (d + 1u > t.max_probe) t.max_probe = d + 1u;
            if (home + d >= ns) ++t.wrapped;
            break;
        }
    }
    t.ports = (uint32_t)in.ports.size();
    t.port_state.assign(t.ports, 0);
    t.port_native.assign(t.ports, (uint16_t)kL2DefaultVlan);
    t.port_vlans.assign((size_t)t.ports * kL2VlanWords, 0u);
    for (uint32_t p = 0; p < t.ports; ++p) {
        const FdbPortIn& pi = in.ports[p];
        if (!pi.set) continue;  // never set: link down, STP unknown, no VLAN config
        t.port_state[p] = (uint8_t)((pi.port.link_up ? kL2LinkUp : 0u) | (pi.port.stp_forwarding ? kL2StpFwd : 0u) |
                                    (pi.port.has_vlan_config ? kL2HasCfg : 0u));
        if (!pi.port.has_vlan_config) continue;
        t.port_native[p] = pi.port.native_vlan;
        uint32_t* bm = t.port_vlans.data() + (size_t)p * kL2VlanWords;
        if (pi.port.type == 0) {  // ACCESS: should_forward compares with native_vlan, the set is ignored
            bm[pi.port.native_vlan >> 5] |= 1u << (pi.port.native_vlan & 31u);
        } else {
            for (uint16_t v : pi.allowed) bm[v >> 5] |= 1u << (v & 31u);
        }
    }
    // the per-VLAN port bitmap: 4096 x ports / 8 bytes, at most 512 KiB at 1,024 ports
    t.port_words = (t.ports + 31u) / 32u;
    t.vlan_ports.assign((size_t)kL2Vlans * t.port_words, 0u);
    for (uint32_t p = 0; p < t.ports; ++p) {
        if ((t.port_state[p] & (kL2LinkUp | kL2StpFwd)) != (kL2LinkUp | kL2StpFwd)) continue;
        const uint32_t* bm = t.port_vlans.data() + (size_t)p * kL2VlanWords;
        for (uint32_t w = 0; w < kL2VlanWords; ++w)
            for (uint32_t m = bm[w]; m; m &= m - 1u) {
                const uint32_t v = w * 32u + (uint32_t)__builtin_ctz(m);
                t.vlan_ports[(size_t)v * t.port_words + (p >> 5)] |= 1u << (p & 31u);
            }
    }
}

// ForwardingDatabase::lookup_port / the find_if of learn_mac: the slot of (mac, vlan), or nullptr. At
// most max_probe probes; a miss also ends at the first empty slot. The kernel's loop is this one.
inline const FdbSlot* fdb_find(const FdbTables& t, const uint8_t* mac, uint32_t vlan) {
    const uint32_t k0 = fdb_k0(mac), k1 = fdb_k1(mac, vlan);
    const uint32_t mask = (uint32_t)t.slots.size() - 1u, home = fdb_hash(k0, k1) & mask;
    for (uint32_t d = 0; d < t.max_probe; ++d) {
        const FdbSlot& s = t.slots[(home + d) & mask];
        if (!(s.flags & kFdbOccupied)) return nullptr;
        if (s.k0 == k0 && s.k1 == k1) return &s;
    }
    return nullptr;
}

inline uint32_t fdb_port_state(const FdbTables& t, uint32_t port) { return port < t.ports ? t.port_state[port] : 0u; }
inline bool fdb_vlan_bit(const FdbTables& t, uint32_t port, uint32_t vlan) {
    if (port >= t.ports || vlan > 4095u) return false;
    return (t.port_vlans[(size_t)port * kL2VlanWords + (vlan >> 5)] >> (vlan & 31u)) & 1u;
}
// VlanManager::should_forward (vlan_manager.cpp:33-64): a port without a config has an all-zero bitmap.
inline bool fdb_should_forward(const FdbTables& t, uint32_t ingress, uint32_t egress, uint32_t vlan) {
    return fdb_vlan_bit(t, ingress, vlan) && fdb_vlan_bit(t, egress, vlan);
}

// The L2 block (switch.hpp:305-326) for one frame, and what learn_mac(src_mac, ingress, vlan) would do.
inline void fdb_decide(const FdbTables& t, uint32_t ingress, const uint8_t* f, uint32_t len, uint32_t* verdict,
                       uint32_t* egress_port, uint32_t* vlan_out, uint32_t* learn_out) {
    uint32_t v = NFCS_L2_NO_ETH, eg = NFCS_IF_NONE, vlan = 0, learn = NFCS_L2_LEARN_NONE;
    if (len >= 14) {
        const bool tagged = f[12] == 0x81 && f[13] == 0x00;
        if (tagged && len >= 18) vlan = (((uint32_t)f[14] << 8) | f[15]) & 0x0FFFu;  // Packet::vlan_id()
        else vlan = ingress < t.ports ? t.port_native[ingress] : kL2DefaultVlan;
        const FdbSlot* d = fdb_find(t, f, vlan);
        if (!d) v = NFCS_L2_FLOOD;
        else {
            const uint32_t port = d->port, st = fdb_port_state(t, port);
            if (port == ingress) v = NFCS_L2_DROP_SAME_PORT;
            else if (!(st & kL2LinkUp)) v = NFCS_L2_DROP_LINK_DOWN;
            else if (!(st & kL2StpFwd)) v = NFCS_L2_DROP_STP;
            else if (!fdb_should_forward(t, ingress, port, vlan)) v = NFCS_L2_DROP_VLAN;
            else { v = NFCS_L2_FORWARD; eg = port; }
        }
        const FdbSlot* s = fdb_find(t, f + 6, vlan);
        if (!s) learn = NFCS_L2_LEARN_NEW;
        else if (s->flags & kFdbStatic) learn = NFCS_L2_LEARN_NONE;
        else learn = s->port == ingress ? NFCS_L2_LEARN_REFRESH : NFCS_L2_LEARN_MOVED;
    }
    if (verdict) *verdict = v;
    if (egress_port) *egress_port = eg;
    if (vlan_out) *vlan_out = vlan;
    if (learn_out) *learn_out = learn;
}

// flood_packet's port loop (switch.hpp:180-186): the ports i < num_ports with i != ingress, link up, STP
// forwarding and should_forward(ingress, i, vlan), ascending. Returns how many there are; the first
// `cap` of them go to `out` (may be NULL when cap is 0).
inline uint32_t fdb_flood_ports(const FdbTables& t, uint32_t ingress, uint32_t vlan, uint32_t num_ports, uint32_t* out,
                                uint32_t cap) {
    uint32_t n = 0;
    const uint32_t hi = num_ports < t.ports ? num_ports : t.ports;  // a port never set has its link down
    for (uint32_t i = 0; i < hi; ++i) {
        if (i == ingress) continue;
        const uint32_t st = t.port_state[i];
        if (!(st & kL2LinkUp) || !(st & kL2StpFwd) || !fdb_should_forward(t, ingress, i, vlan)) continue;
        if (n < cap && out) out[n] = i;
        ++n;
    }
    return n;
}

// ---- flood replication: the flood mask and the sequential walk of nfcs_flood_expand_host ---------------

// Word w (w < port_words) of the flood mask of (ingress, vlan, num_ports): the VLAN's row of vlan_ports
// with the ingress bit and the ports >= num_ports cleared, or empty when the ingress port lacks the VLAN's
// bit (in_ok false; should_forward needs both). Bit b of word w is port 32 w + b; ascending bits are
// fdb_flood_ports' order. Host and device, this one definition.
NFCS_HD inline uint32_t fdb_flood_word(const uint32_t* row, uint32_t w, uint32_t ingress, uint32_t num_ports, bool in_ok) {
    uint32_t m = in_ok ? row[w] : 0u;
    if ((ingress >> 5) == w) m &= ~(1u << (ingress & 31u));
    const uint32_t lo = w * 32u;
    if (num_ports <= lo) m = 0u;
    else if (num_ports - lo < 32u) m &= (1u << (num_ports - lo)) - 1u;
    return m;
}
NFCS_HD inline uint64_t flood_sat_add(uint64_t a, uint64_t b) {  // associative: any scan order gives one answer
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}
NFCS_HD inline uint64_t flood_round_up(uint64_t x, uint64_t pow2) { return (x + pow2 - 1u) & ~(pow2 - 1u); }
// The unicast port of a packet: nfcs_egress_plan_device's rule.
NFCS_HD inline uint32_t flood_unicast_port(uint32_t l3, bool have_l3, uint32_t st, bool have_st, uint32_t l2, bool have_l2) {
    uint32_t p = have_l3 ? l3 : NFCS_IF_NONE;
    if (have_st && !(st & NFCS_ST_FLAG_FWD)) p = NFCS_IF_NONE;
    return p != NFCS_IF_NONE ? p : have_l2 ? l2 : NFCS_IF_NONE;
}
// A burst's item count must fit 32 bits whatever floods: n x max(1, min(num_ports, NFCS_L2_MAX_PORTS)).
inline bool flood_args_ok(uint32_t num_ports, uint64_t arena_bytes, uint64_t copy_base, uint32_t copy_align, uint32_t n,
                          bool l3, bool st, bool l2, bool verdict, bool vlan) {
    if ((!l3 && !l2) || (st && !l3) || (verdict && !vlan)) return false;
    if (copy_align < 16u || (copy_align & (copy_align - 1u)) || (copy_base & (copy_align - 1u)) || copy_base > arena_bytes)
        return false;
    const uint64_t fan = num_ports < NFCS_L2_MAX_PORTS ? (num_ports ? num_ports : 1u) : NFCS_L2_MAX_PORTS;
    return (uint64_t)n * fan <= 0xFFFFFFFFull;
}

// flood_packet over the burst, one packet after another (nfcs.h, nfcs_flood_expand_device: the rules). The
// item arrays have `cap` entries; entries [items, cap) are written inert.
inline void flood_expand(const FdbTables& t, uint32_t ingress, uint32_t num_ports, uint64_t arena_bytes,
                         uint64_t copy_base, uint32_t copy_align, const nfcs_desc* desc, uint32_t n,
                         const uint32_t* l3_port, const uint8_t* fwd_status, const uint32_t* l2_port,
                         const uint8_t* l2_verdict, const uint16_t* l2_vlan, uint32_t cap, nfcs_desc* item_desc,
                         uint32_t* item_port, uint32_t* item_src, nfcs_flood_totals* tot) {
    nfcs_flood_totals r{};
    uint64_t k = 0, used = 0;  // items called for so far; slot bytes called for so far
    bool open = true;          // every item so far was emitted
    auto item = [&](nfcs_desc d, uint32_t port, uint32_t src, uint64_t slot, bool copy) {
        used = flood_sat_add(used, slot);
        open = open && k < cap && flood_sat_add(copy_base, used) <= arena_bytes;
        if (open) {
            item_desc[k] = d;
            item_port[k] = port;
            item_src[k] = src;
            ++r.items;
            if (copy) {
                ++r.copies;
                r.copy_bytes += slot;
            }
        }
        ++k;
    };
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t off = (uint64_t)desc[i].off16 * 16u, len = desc[i].len;
        if (off + flood_round_up(len, 16u) > copy_base) continue;  // not live
        const uint32_t uni = flood_unicast_port(l3_port ? l3_port[i] : 0u, l3_port != nullptr, fwd_status ? fwd_status[i] : 0u,
                                                fwd_status != nullptr, l2_port ? l2_port[i] : 0u, l2_port != nullptr);
        if (uni != NFCS_IF_NONE) {
            item(desc[i], uni, i, 0u, false);
            continue;
        }
        if (!l2_verdict || l2_verdict[i] != NFCS_L2_FLOOD) continue;
        ++r.flooded;
        const uint32_t vlan = l2_vlan[i];
        const bool in_ok = vlan < kL2Vlans && fdb_vlan_bit(t, ingress, vlan);
        const uint32_t* row = in_ok ? t.vlan_ports.data() + (size_t)vlan * t.port_words : nullptr;
        const uint64_t slot = flood_round_up(len, copy_align);
        for (uint32_t w = 0; w < t.port_words; ++w)
            for (uint32_t m = fdb_flood_word(row, w, ingress, num_ports, in_ok); m; m &= m - 1u) {
                const uint64_t at = flood_sat_add(copy_base, used);  // this copy's slot, when it is emitted
                item(nfcs_desc{(uint32_t)(at / 16u), desc[i].len}, w * 32u + (uint32_t)__builtin_ctz(m), i, slot, true);
            }
    }
    r.items_needed = (uint32_t)k;
    r.copy_bytes_needed = used;
    for (uint64_t j = r.items; j < cap; ++j) {
        item_desc[j] = nfcs_desc{0u, 0u};
        item_port[j] = NFCS_IF_NONE;
        item_src[j] = NFCS_ITEM_NONE;
    }
    *tot = r;
}

}  // namespace nfcs

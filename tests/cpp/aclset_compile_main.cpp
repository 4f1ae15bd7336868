// aclset_compile_main.cpp — stand-alone host program over netflow_amd/csrc/nfcs_aclset.h (no HIP, no GPU):
// builds random sets of rule lists with port bindings (shared, empty, removed and never-set lists, unbound
// ports), commits them and checks the layout and every decision of aclset_decide and of the burst walk
// aclset_egress against a direct walk of each port's own rule vector, written the way
// AclManager::check_match is (as tests/cpp/acl_compile_main.cpp does for one list). Built and run by
// tests/test_egress_acl.py under -fsanitize=address,undefined; every frame lives in a heap block of exactly
// its length, so a read past it is reported. Exit status 0 = everything agrees.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "nfcs_aclset.h"

namespace {

uint64_t g_state = 0x2545F4914F6CDD1Dull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

uint32_t be16(const uint8_t* b, uint32_t o) { return ((uint32_t)b[o] << 8) | b[o + 1]; }
uint32_t be32(const uint8_t* b, uint32_t o) { return (be16(b, o) << 16) | be16(b, o + 2); }

bool direct_match(const nfcs_acl_rule& r, const uint8_t* b, uint32_t len) {
    const bool eth = len >= 14;
    const bool tagged = eth && be16(b, 12) == 0x8100u;
    if (r.fields & NFCS_ACL_F_SRC_MAC)
        if (!eth || memcmp(b + 6, r.src_mac, 6)) return false;
    if (r.fields & NFCS_ACL_F_DST_MAC)
        if (!eth || memcmp(b, r.dst_mac, 6)) return false;
    if (r.fields & NFCS_ACL_F_VLAN_ID)
        if (!tagged || len < 18 || (be16(b, 14) & 0x0FFFu) != r.vlan_id) return false;
    const uint32_t upper = NFCS_ACL_F_ETHERTYPE | NFCS_ACL_F_SRC_IP | NFCS_ACL_F_DST_IP | NFCS_ACL_F_PROTOCOL |
                           NFCS_ACL_F_SRC_PORT | NFCS_ACL_F_DST_PORT;
    uint32_t et = 0;
    if (!eth) {
        if (r.fields & upper) return false;
    } else {
        if (tagged) {
            if (len >= 18) et = be16(b, 16);
            else if (r.fields & upper) return false;
        } else {
            et = be16(b, 12);
        }
        if ((r.fields & NFCS_ACL_F_ETHERTYPE) && et != r.ethertype) return false;
    }
    if (!(r.fields & (upper & ~NFCS_ACL_F_ETHERTYPE))) return true;
    const uint32_t l2 = tagged ? 18u : 14u;
    if (et != 0x0800u || l2 + 20u > len) return false;
    if ((r.fields & NFCS_ACL_F_SRC_IP) && (be32(b, l2 + 12) & r.src_ip_mask) != (r.src_ip & r.src_ip_mask)) return false;
    if ((r.fields & NFCS_ACL_F_DST_IP) && (be32(b, l2 + 16) & r.dst_ip_mask) != (r.dst_ip & r.dst_ip_mask)) return false;
    const uint32_t proto = b[l2 + 9];
    if ((r.fields & NFCS_ACL_F_PROTOCOL) && proto != r.protocol) return false;
    if (r.fields & (NFCS_ACL_F_SRC_PORT | NFCS_ACL_F_DST_PORT)) {
        const uint32_t l4 = l2 + (b[l2] & 15u) * 4u;
        if (proto == 6) {
            if (l4 + 19u > len) return false;
        } else if (proto == 17) {
            if (l4 + 8u > len) return false;
        } else {
            return false;
        }
        if ((r.fields & NFCS_ACL_F_SRC_PORT) && be16(b, l4) != r.src_port) return false;
        if ((r.fields & NFCS_ACL_F_DST_PORT) && be16(b, l4 + 2) != r.dst_port) return false;
    }
    return true;
}

void pool_mac(uint8_t* m) {
    static const uint8_t init[6] = {0x02, 0xAC, 0, 0, 0, 0};
    memcpy(m, init, 6);
    m[5] = (uint8_t)(rnd() % 4u);
}
uint32_t pool_ip() { return 0x0A000000u | ((rnd() % 3u) << 8) | (rnd() % 3u); }
uint16_t pool_port() {
    static const uint16_t p[] = {22, 53, 80, 443};
    return p[rnd() % 4u];
}

nfcs_acl_rule random_rule() {
    nfcs_acl_rule r{};
    for (int k = 0, nf = (int)(rnd() % 16u ? 1u + rnd() % 2u : 0u); k < nf; ++k) r.fields |= 1u << (rnd() % 9u);
    r.rule_id = rnd();
    pool_mac(r.src_mac);
    pool_mac(r.dst_mac);
    r.vlan_id = (uint16_t)(10u * (rnd() % 3u));
    static const uint16_t ets[] = {0x0800, 0x86DD, 0x0806, 0};
    r.ethertype = ets[rnd() % 4u];
    r.src_ip = pool_ip();
    r.dst_ip = pool_ip();
    static const uint32_t masks[] = {0xFFFFFFFFu, 0xFFFFFF00u, 0xFFFF0000u, 0u, 0xFF00FF0Fu};
    r.src_ip_mask = masks[rnd() % 5u];
    r.dst_ip_mask = masks[rnd() % 5u];
    r.src_port = pool_port();
    r.dst_port = pool_port();
    static const uint8_t protos[] = {6, 17, 1};
    r.protocol = protos[rnd() % 3u];
    r.action = (uint8_t)(rnd() % 3u);
    r.redirect_port = rnd() % 2u ? NFCS_IF_NONE : rnd() % 64u;
    return r;
}

// a frame of exactly `len` heap bytes
std::unique_ptr<uint8_t[]> random_frame(uint32_t* len_out) {
    uint8_t f[128];
    for (uint8_t& x : f) x = (uint8_t)rnd();
    pool_mac(f);
    pool_mac(f + 6);
    const bool tagged = rnd() % 3u == 0;
    const uint32_t l2 = tagged ? 18u : 14u;
    static const uint16_t ets[] = {0x0800, 0x0800, 0x0800, 0x86DD, 0x0806, 0};
    const uint16_t et = ets[rnd() % 6u];
    if (tagged) {
        f[12] = 0x81, f[13] = 0x00;
        const uint32_t tci = ((rnd() % 8u) << 13) | (10u * (rnd() % 3u));
        f[14] = (uint8_t)(tci >> 8), f[15] = (uint8_t)tci;
    }
    f[l2 - 2] = (uint8_t)(et >> 8), f[l2 - 1] = (uint8_t)et;
    static const uint8_t ihls[] = {5, 5, 5, 0, 4, 6, 15};
    const uint32_t ihl = ihls[rnd() % 7u], l4 = l2 + 4u * ihl;
    f[l2] = (uint8_t)(0x40u | ihl);
    static const uint8_t protos[] = {6, 17, 1};
    f[l2 + 9] = protos[rnd() % 3u];
    const uint32_t s = pool_ip(), d = pool_ip();
    for (int j = 0; j < 4; ++j) f[l2 + 12 + j] = (uint8_t)(s >> (24 - 8 * j)), f[l2 + 16 + j] = (uint8_t)(d >> (24 - 8 * j));
    if (ihl >= 5) {
        const uint16_t sp = pool_port(), dp = pool_port();
        f[l4] = (uint8_t)(sp >> 8), f[l4 + 1] = (uint8_t)sp, f[l4 + 2] = (uint8_t)(dp >> 8), f[l4 + 3] = (uint8_t)dp;
    }
    const uint32_t bounds[] = {0, 10, 13, 14, 17, 18, l2 + 19, l2 + 20, l4 + 7, l4 + 8, l4 + 18, l4 + 19, 128};
    const uint32_t len = rnd() % 2u ? bounds[rnd() % 13u] : rnd() % 129u;
    std::unique_ptr<uint8_t[]> frame(new uint8_t[len ? len : 1]);
    memcpy(frame.get(), f, len);
    *len_out = len;
    return frame;
}

struct Want { uint32_t action, rule, port; };
Want walk(const std::vector<nfcs_acl_rule>* rules, const uint8_t* b, uint32_t len) {
    Want w{NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE};
    if (!rules) return w;
    for (uint32_t i = 0; i < rules->size(); ++i) {
        if (!direct_match((*rules)[i], b, len)) continue;
        w.rule = i;
        w.action = (*rules)[i].action;
        if (w.action == NFCS_ACL_REDIRECT) {
            if ((*rules)[i].redirect_port == NFCS_IF_NONE) w.action = NFCS_ACL_DENY;
            else w.port = (*rules)[i].redirect_port;
        }
        break;
    }
    return w;
}

}  // namespace

int main() {
    int bad = 0;
    long matched = 0, total = 0, no_list = 0;
    for (int round = 0; round < 40 && !bad; ++round) {
        nfcs::AclSetInputs in;
        const uint32_t n_lists = 1u + rnd() % 9u, n_ports = 1u + rnd() % 24u;
        std::vector<uint32_t> ids;
        uint32_t padded = 0, laid = 0;
        for (uint32_t l = 0; l < n_lists; ++l) {
            const uint32_t id = rnd() % NFCS_ACLSET_MAX_LISTS;
            std::vector<nfcs_acl_rule> rules(rnd() % 5u ? rnd() % 30u : 0u);
            for (nfcs_acl_rule& r : rules) r = random_rule();
            if (nfcs::aclset_set_list(in, id, rules.data(), (uint32_t)rules.size()) != NFCS_OK) ++bad;
            ids.push_back(id);
        }
        if (rnd() % 2u) nfcs::aclset_remove_list(in, ids[rnd() % ids.size()]);
        ids.push_back(rnd() % NFCS_ACLSET_MAX_LISTS);  // perhaps never set
        for (uint32_t id = 0; id < NFCS_ACLSET_MAX_LISTS; ++id)
            if (in.have[id] && !in.list[id].empty()) padded += ((uint32_t)in.list[id].size() + 3u) & ~3u, ++laid;
        uint32_t top = 0;
        for (uint32_t p = 0; p < n_ports; ++p) {
            if (rnd() % 4u == 0) continue;  // unbound
            if (nfcs::aclset_bind_port(in, p, ids[rnd() % ids.size()]) != NFCS_OK) ++bad;
            top = p + 1u;
        }
        if (nfcs::aclset_set_list(in, NFCS_ACLSET_MAX_LISTS, nullptr, 0) != NFCS_EINVAL) ++bad;
        if (nfcs::aclset_bind_port(in, NFCS_L2_MAX_PORTS, 0) != NFCS_EINVAL) ++bad;
        nfcs::AclSetTables t;
        if (nfcs::aclset_compile(in, t) != NFCS_OK) ++bad;
        if (t.ports != top || t.bind.size() != top || t.rec.size() != padded || t.act.size() != padded || t.lists != laid) {
            printf("round %d: layout ports %u/%u rules %zu/%u lists %u/%u\n", round, t.ports, top, t.rec.size(), padded,
                   t.lists, laid);
            ++bad;
        }
        // the burst: frames in an arena of 16-byte slots for aclset_egress, and alone in exact heap blocks
        const uint32_t n = 600;
        std::vector<uint8_t> arena((size_t)n * 128u, 0);
        std::vector<nfcs_desc> desc(n);
        std::vector<uint32_t> port(n), port_io;
        std::vector<Want> want(n);
        std::vector<uint32_t> pk(top, 0), pk_want(top, 0);
        std::vector<uint64_t> by(top, 0), by_want(top, 0);
        for (uint32_t i = 0; i < n && !bad; ++i) {
            uint32_t len = 0;
            std::unique_ptr<uint8_t[]> frame = random_frame(&len);
            memcpy(arena.data() + (size_t)i * 128u, frame.get(), len);
            desc[i].off16 = i * 8u;
            desc[i].len = len;
            port[i] = rnd() % 8u == 0 ? NFCS_IF_NONE : rnd() % (n_ports + 4u);
            const std::vector<nfcs_acl_rule>* rules = nullptr;
            if (port[i] != NFCS_IF_NONE && port[i] < in.port_list.size() && in.port_list[port[i]] != NFCS_ACL_LIST_NONE &&
                in.have[in.port_list[port[i]]] && !in.list[in.port_list[port[i]]].empty())
                rules = &in.list[in.port_list[port[i]]];
            want[i] = walk(rules, frame.get(), len);
            if (port[i] == NFCS_IF_NONE) {
                want[i].action = NFCS_ACL_NO_PORT;
                continue;
            }
            uint32_t action = 99, rule = 99, rp = 99;
            nfcs::aclset_decide(t, port[i], frame.get(), len, &action, &rule, &rp);
            ++total;
            if (!rules) ++no_list;
            if (want[i].rule != NFCS_ACL_NO_MATCH) ++matched;
            if (action != want[i].action || rule != want[i].rule || rp != want[i].port) {
                printf("round %d packet %u port %u len %u: action %u want %u, rule %u want %u, port %u want %u\n", round, i,
                       port[i], len, action, want[i].action, rule, want[i].rule, rp, want[i].port);
                ++bad;
            }
            if (want[i].action == NFCS_ACL_DENY) pk_want[port[i]] += 1u, by_want[port[i]] += len;
        }
        port_io = port;
        std::vector<uint8_t> action(n);
        std::vector<uint32_t> rule(n), rp(n);
        nfcs::aclset_egress(t, arena.data(), arena.size(), desc.data(), n, port_io.data(), action.data(), rule.data(),
                            rp.data(), pk.data(), by.data());
        for (uint32_t i = 0; i < n && !bad; ++i) {
            const uint32_t keep = want[i].action == NFCS_ACL_DENY ? NFCS_IF_NONE : port[i];
            if (action[i] != want[i].action || rule[i] != want[i].rule || rp[i] != want[i].port || port_io[i] != keep) {
                printf("round %d burst packet %u differs\n", round, i);
                ++bad;
            }
        }
        if (pk != pk_want || by != by_want) ++bad, printf("round %d: counters differ\n", round);
    }
    // the limit: 512 padded rules fit, one list more does not, and the last list is reachable
    {
        nfcs::AclSetInputs in;
        std::vector<nfcs_acl_rule> never(505);
        for (nfcs_acl_rule& r : never) r.fields = NFCS_ACL_F_VLAN_ID, r.vlan_id = 0x1000, r.action = NFCS_ACL_DENY;
        nfcs_acl_rule all{};
        all.action = NFCS_ACL_DENY;
        nfcs::aclset_set_list(in, 3, never.data(), 505);
        nfcs::aclset_set_list(in, 9, &all, 1);
        nfcs::aclset_bind_port(in, 0, 3);
        nfcs::aclset_bind_port(in, 1, 9);
        nfcs::AclSetTables t;
        uint32_t a = 9, r = 9;
        if (nfcs::aclset_compile(in, t) != NFCS_OK || t.rec.size() != NFCS_ACL_MAX_RULES) ++bad;
        std::unique_ptr<uint8_t[]> f(new uint8_t[20]());
        nfcs::aclset_decide(t, 1, f.get(), 20, &a, &r, nullptr);
        if (a != NFCS_ACL_DENY || r != 0) ++bad, printf("last list: action %u rule %u\n", a, r);
        nfcs::aclset_decide(t, 0, f.get(), 20, &a, &r, nullptr);
        if (a != NFCS_ACL_PERMIT || r != NFCS_ACL_NO_MATCH) ++bad;
        nfcs::aclset_set_list(in, 10, &all, 1);
        if (nfcs::aclset_compile(in, t) != NFCS_EINVAL || !t.rec.empty()) ++bad, printf("516 padded rules accepted\n");
    }
    printf("matched %ld of %ld, %ld without a list\n", matched, total, no_list);
    if (matched * 10 < total || (total - matched) * 50 < total || no_list * 50 < total) ++bad;
    printf(bad ? "FAIL\n" : "aclset compile OK\n");
    return bad ? 1 : 0;
}

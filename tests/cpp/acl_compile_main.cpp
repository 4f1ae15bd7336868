// acl_compile_main.cpp — stand-alone host program over netflow_amd/csrc/nfcs_acl.h (no HIP, no GPU):
// compiles random rule lists and checks every decision of acl_decide (key + masked compares) against a
// direct walk of the rules written the way AclManager::check_match is (acl_manager.cpp:198-278: one
// test per engaged field against what the Packet accessors return for the frame), plus the address
// masks. Built and run by tests/test_acl.py under -fsanitize=address,undefined; every frame lives in
// a heap block of exactly its length, so a read past it is reported. Exit status 0 = every decision agrees.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "nfcs_acl.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
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

// values from small pools, so rules hit
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

}  // namespace

int main() {
    int bad = 0;
    long matched = 0, total = 0;
    for (int round = 0; round < 60 && !bad; ++round) {
        std::vector<nfcs_acl_rule> rules;
        const uint32_t nr = round == 0 ? 0u : round == 1 ? NFCS_ACL_MAX_RULES : rnd() % 40u;
        for (uint32_t i = 0; i < nr; ++i) {
            nfcs_acl_rule r{};
            // few fields per rule, or nothing would ever match
            for (int k = 0, nf = (int)(rnd() % 16u ? 1u + rnd() % 3u : 0u); k < nf; ++k) r.fields |= 1u << (rnd() % 9u);
            if (round == 1 && i + 1 < nr) r.fields |= NFCS_ACL_F_VLAN_ID, r.vlan_id = 0x1000;  // never matches
            r.rule_id = rnd();
            pool_mac(r.src_mac);
            pool_mac(r.dst_mac);
            if (!(round == 1 && i + 1 < nr)) r.vlan_id = (uint16_t)(10u * (rnd() % 3u));
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
            rules.push_back(r);
        }
        nfcs::AclTables t;
        nfcs::acl_compile(rules, t);
        if (t.rec.size() % nfcs::kAclGroup || t.rec.size() < rules.size() || t.act.size() != rules.size()) ++bad;
        for (int k = 0; k < 1500 && !bad; ++k) {
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
            // a length at one of the bounds, or anything up to 128
            const uint32_t bounds[] = {0, 10, 13, 14, 17, 18, l2 + 19, l2 + 20, l4 + 7, l4 + 8, l4 + 18, l4 + 19, 128};
            const uint32_t len = rnd() % 2u ? bounds[rnd() % 13u] : rnd() % 129u;
            std::unique_ptr<uint8_t[]> frame(new uint8_t[len ? len : 1]);  // exactly len bytes: ASan sees a read past them
            memcpy(frame.get(), f, len);
            uint32_t action = 99, rule = 99, port = 99;
            nfcs::acl_decide(t, frame.get(), len, &action, &rule, &port);
            uint32_t want_rule = NFCS_ACL_NO_MATCH, want_action = NFCS_ACL_PERMIT, want_port = NFCS_IF_NONE;
            for (uint32_t i = 0; i < rules.size(); ++i) {
                if (!direct_match(rules[i], frame.get(), len)) continue;
                want_rule = i;
                want_action = rules[i].action;
                if (want_action == NFCS_ACL_REDIRECT) {
                    if (rules[i].redirect_port == NFCS_IF_NONE) want_action = NFCS_ACL_DENY;
                    else want_port = rules[i].redirect_port;
                }
                break;
            }
            ++total;
            if (want_rule != NFCS_ACL_NO_MATCH) ++matched;
            if (action != want_action || rule != want_rule || port != want_port) {
                printf("round %d frame %d len %u: action %u want %u, rule %u want %u, port %u want %u\n", round, k, len,
                       action, want_action, rule, want_rule, port, want_port);
                ++bad;
            }
        }
        if (round == 1 && !bad) {  // 512 rules: only the last one can match, and it must be reachable
            uint8_t f[64] = {0};
            nfcs_acl_rule last = rules.back();
            last.fields = 0;
            rules.back() = last;
            nfcs::acl_compile(rules, t);
            uint32_t rule = 0;
            nfcs::acl_decide(t, f, 64, nullptr, &rule, nullptr);
            if (rule != NFCS_ACL_MAX_RULES - 1u) ++bad, printf("512 rules: rule %u\n", rule);
        }
    }
    // the walk above proves nothing if no rule ever matches, or every frame does
    printf("matched %ld of %ld\n", matched, total);
    if (matched * 10 < total || (total - matched) * 50 < total) ++bad;
    printf(bad ? "FAIL\n" : "acl compile OK\n");
    return bad ? 1 : 0;
}

// make_acl_test.cpp — host-only check of netflow_amd::make_acl_from (include/netflow_amd/packet.hpp),
// the work behind netflow_adapter.hpp's make_acl(const std::vector<netflow::AclRule>&, ...): a stand-in
// rule struct with AclRule's member names (std::optional match fields, an enum action, an optional
// redirect_port_id) and a MAC type with bytes[6], then the decisions of the list it builds. No GPU: the
// list is host code until it is uploaded. Built and run by tests/test_acl.py. Prints "make_acl OK" and
// exits 0 when every check holds.
#include <cstdio>
#include <optional>
#include <vector>

#include "netflow_amd/packet.hpp"

namespace {

struct Mac { uint8_t bytes[6]; };
enum class Action { PERMIT, DENY, REDIRECT };
struct Rule {
    uint32_t rule_id = 0;
    int priority = 0;
    std::optional<Mac> src_mac, dst_mac;
    std::optional<uint16_t> vlan_id, ethertype;
    std::optional<uint32_t> src_ip, dst_ip;
    std::optional<uint8_t> protocol;
    std::optional<uint16_t> src_port, dst_port;
    Action action = Action::DENY;
    std::optional<uint32_t> redirect_port_id;
};

std::vector<uint8_t> udp_frame(uint32_t src, uint32_t dst, uint16_t sport, uint16_t dport, uint8_t smac_last) {
    std::vector<uint8_t> f(64, 0);
    f[11] = smac_last;
    f[12] = 0x08;
    f[14] = 0x45;
    f[23] = 17;
    for (int j = 0; j < 4; ++j) f[26 + j] = (uint8_t)(src >> (24 - 8 * j)), f[30 + j] = (uint8_t)(dst >> (24 - 8 * j));
    f[34] = (uint8_t)(sport >> 8), f[35] = (uint8_t)sport, f[36] = (uint8_t)(dport >> 8), f[37] = (uint8_t)dport;
    return f;
}

int g_bad = 0;
void expect(const nfcs_acl* acl, const std::vector<uint8_t>& f, uint32_t action, uint32_t rule, uint32_t port) {
    uint32_t a = 99, r = 99, p = 99;
    const int rc = nfcs_acl_eval_host(acl, f.data(), (uint32_t)f.size(), &a, &r, &p);
    if (rc != 0 || a != action || r != rule || p != port) {
        std::printf("rc %d action %u (want %u) rule %u (want %u) port %u (want %u)\n", rc, a, action, r, rule, p, port);
        ++g_bad;
    }
}

}  // namespace

int main() {
    std::vector<Rule> rules(4);
    rules[0].rule_id = 40;  // host-order addresses, as AclRule holds them: 10.1.2.3 -> UDP port 53
    rules[0].src_ip = 0x0A010203u;
    rules[0].protocol = 17;
    rules[0].dst_port = 53;
    rules[0].action = Action::PERMIT;
    rules[1].rule_id = 30;  // REDIRECT without a port: DENY at this rule
    rules[1].dst_ip = 0x0A0000FEu;
    rules[1].action = Action::REDIRECT;
    rules[2].rule_id = 20;
    rules[2].src_mac = Mac{{0, 0, 0, 0, 0, 7}};
    rules[2].action = Action::REDIRECT;
    rules[2].redirect_port_id = 12;
    rules[3].rule_id = 10;  // would match what rule 1 matches, but stands behind it
    rules[3].dst_ip = 0x0A0000FEu;
    rules[3].action = Action::PERMIT;
    nfcs_acl* acl = nullptr;
    if (netflow_amd::make_acl_from(rules, &acl) != NFCS_OK || !acl) return 2;
    if (netflow_amd::make_acl_from(rules, (nfcs_acl**)nullptr) != NFCS_EINVAL) return 3;
    expect(acl, udp_frame(0x0A010203u, 0x0A000001u, 999, 53, 0), NFCS_ACL_PERMIT, 0, NFCS_IF_NONE);
    expect(acl, udp_frame(0x0A010203u, 0x0A0000FEu, 999, 53, 7), NFCS_ACL_PERMIT, 0, NFCS_IF_NONE);  // the first of three
    expect(acl, udp_frame(0x0A010204u, 0x0A0000FEu, 999, 53, 7), NFCS_ACL_DENY, 1, NFCS_IF_NONE);
    expect(acl, udp_frame(0x0A010204u, 0x0A000001u, 999, 53, 7), NFCS_ACL_REDIRECT, 2, 12);
    expect(acl, udp_frame(0x03020100u | 0x0Au, 0x0A000001u, 999, 53, 0), NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);  // network order does not match
    expect(acl, std::vector<uint8_t>(10, 0), NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);
    nfcs_acl_destroy(acl);
    // an empty vector is a valid list, and too many rules are an error that leaves no list behind
    if (netflow_amd::make_acl_from(std::vector<Rule>{}, &acl) != NFCS_OK || !acl) return 4;
    expect(acl, udp_frame(1, 2, 3, 4, 5), NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);
    nfcs_acl_destroy(acl);
    if (netflow_amd::make_acl_from(std::vector<Rule>(NFCS_ACL_MAX_RULES + 1), &acl) != NFCS_EINVAL || acl) return 5;
    std::printf(g_bad ? "FAIL\n" : "make_acl OK\n");
    return g_bad ? 1 : 0;
}

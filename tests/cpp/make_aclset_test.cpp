// make_aclset_test.cpp — host-only check of netflow_amd::make_acl_set_from (include/netflow_amd/packet.hpp),
// the work behind netflow_adapter.hpp's make_acl_set: named rule vectors (a stand-in rule struct with
// AclRule's member names, as tests/cpp/make_acl_test.cpp has) and (port, applied name) pairs, then the
// decisions of the set it builds. No GPU: the set is host code until it is uploaded. Built and run by
// tests/test_egress_acl.py. Prints "make_acl_set OK" and exits 0 when every check holds.
#include <cstdio>
#include <map>
#include <optional>
#include <string>
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

std::vector<uint8_t> udp_frame(uint32_t src, uint16_t dport) {
    std::vector<uint8_t> f(64, 0);
    f[12] = 0x08;
    f[14] = 0x45;
    f[23] = 17;
    for (int j = 0; j < 4; ++j) f[26 + j] = (uint8_t)(src >> (24 - 8 * j));
    f[36] = (uint8_t)(dport >> 8), f[37] = (uint8_t)dport;
    return f;
}

int g_bad = 0;
void expect(const nfcs_aclset* set, uint32_t port, const std::vector<uint8_t>& f, uint32_t action, uint32_t rule,
            uint32_t redirect) {
    uint32_t a = 99, r = 99, p = 99;
    const int rc = nfcs_aclset_eval_host(set, port, f.data(), (uint32_t)f.size(), &a, &r, &p);
    if (rc != 0 || a != action || r != rule || p != redirect) {
        std::printf("port %u: rc %d action %u (want %u) rule %u (want %u) redirect %u (want %u)\n", port, rc, a, action, r,
                    rule, p, redirect);
        ++g_bad;
    }
}

}  // namespace

int main() {
    std::map<std::string, std::vector<Rule>> lists;
    std::vector<Rule>& web = lists["web"];
    web.resize(2);
    web[0].src_ip = 0x0A010203u;  // host order, as AclRule holds it
    web[0].action = Action::PERMIT;
    web[1].protocol = 17;
    web[1].dst_port = 80;
    web[1].action = Action::DENY;
    std::vector<Rule>& mirror = lists["mirror"];
    mirror.resize(1);
    mirror[0].dst_port = 80;
    mirror[0].action = Action::REDIRECT;
    mirror[0].redirect_port_id = 12;
    lists["empty"];
    const std::vector<std::pair<uint32_t, std::string>> bound = {
        {0, "web"}, {1, "mirror"}, {2, "web"}, {4, "gone"}, {5, "empty"}, {7, "also gone"}};
    nfcs_aclset* set = nullptr;
    if (netflow_amd::make_acl_set_from(lists, bound, &set) != NFCS_OK || !set) return 2;
    if (netflow_amd::make_acl_set_from(lists, bound, (nfcs_aclset**)nullptr) != NFCS_EINVAL) return 3;
    uint32_t ports = 0, laid = 0, padded = 0;
    if (nfcs_aclset_info(set, &ports, &laid, &padded) != NFCS_OK || ports != 8 || laid != 2 || padded != 8) {
        std::printf("info: ports %u lists %u rules %u\n", ports, laid, padded);
        ++g_bad;
    }
    const std::vector<uint8_t> a = udp_frame(0x0A010203u, 80), b = udp_frame(0x0A010204u, 80), c = udp_frame(0x0A010204u, 81);
    for (uint32_t port : {0u, 2u}) {  // the shared list
        expect(set, port, a, NFCS_ACL_PERMIT, 0, NFCS_IF_NONE);
        expect(set, port, b, NFCS_ACL_DENY, 1, NFCS_IF_NONE);
        expect(set, port, c, NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);
    }
    expect(set, 1, b, NFCS_ACL_REDIRECT, 0, 12);
    expect(set, 1, c, NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);
    for (uint32_t port : {3u, 4u, 5u, 6u, 7u, 8u, 900u})  // unbound, a name without a list, the empty list, past the last
        expect(set, port, b, NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);
    nfcs_aclset_destroy(set);
    // errors leave no set behind: a port out of range, lists that pad to more than NFCS_ACL_MAX_RULES rules
    if (netflow_amd::make_acl_set_from(lists, {{NFCS_L2_MAX_PORTS, "web"}}, &set) != NFCS_EINVAL || set) return 4;
    lists["big"].resize(NFCS_ACL_MAX_RULES - 7);
    if (netflow_amd::make_acl_set_from(lists, bound, &set) != NFCS_EINVAL || set) return 5;
    lists["big"].resize(NFCS_ACL_MAX_RULES - 8);
    if (netflow_amd::make_acl_set_from(lists, bound, &set) != NFCS_OK || !set) return 6;
    nfcs_aclset_destroy(set);
    // no list and no binding is a valid set
    if (netflow_amd::make_acl_set_from(std::map<std::string, std::vector<Rule>>{}, {}, &set) != NFCS_OK || !set) return 7;
    expect(set, 0, b, NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH, NFCS_IF_NONE);
    nfcs_aclset_destroy(set);
    std::printf(g_bad ? "FAIL\n" : "make_acl_set OK\n");
    return g_bad ? 1 : 0;
}

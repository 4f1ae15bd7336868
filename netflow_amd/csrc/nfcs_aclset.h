// nfcs_aclset.h — the egress ACLs' host side: rule lists by id, port -> list bindings, the commit that lays
// every list out in one array, and the per-port decision of nfcs_aclset_eval_host / nfcs_egress_acl_host.
// Pure C++ (no HIP), so it also builds into a stand-alone host program (tests/cpp/aclset_compile_main.cpp,
// run under the host sanitizers). The rule form, the key and the match are nfcs_acl.h's, unchanged; the
// device side (upload, launch) is in nfcs_api.hip / nfcs_kernels.hip.
//
// InterfaceManager::get_applied_acl_name(port, EGRESS) names a list per port and AclManager::evaluate
// (acl_manager.cpp:161-190) answers PERMIT for a name it does not know, so a port that was never bound, a
// port bound to a list that was never set or was removed, and a port bound to an empty list all read
// "no list": PERMIT, NFCS_ACL_NO_MATCH, and no frame byte looked at.
#pragma once

#include <stdint.h>

#include <vector>

#include "nfcs.h"
#include "nfcs_acl.h"

namespace nfcs {

struct AclBind {     // per port: where its list lies in the one array
    uint32_t first;  // index of the list's first rule
    uint32_t count;  // rules to scan, padded to kAclGroup; 0 = no list (first is 0 then)
};
static_assert(sizeof(AclBind) == 8, "a port's binding is an 8-byte record");

struct AclSetInputs {
    std::vector<nfcs_acl_rule> list[NFCS_ACLSET_MAX_LISTS];
    bool have[NFCS_ACLSET_MAX_LISTS] = {};  // set (possibly empty) and not removed
    std::vector<uint32_t> port_list;        // per port id: the list id, or NFCS_ACL_LIST_NONE
};

// What the evaluation reads (host copies; the kernel reads the same arrays from device memory).
struct AclSetTables {
    std::vector<AclRec> rec;    // every non-empty list, in list-id order, each padded to kAclGroup
    std::vector<AclAct> act;    // indexed like rec (a padding rule's entry is never read)
    std::vector<AclBind> bind;  // `ports` records
    uint32_t ports = 0;         // highest bound port id + 1
    uint32_t lists = 0;         // lists laid out (the non-empty ones)
};

inline bool acl_rule_ok(const nfcs_acl_rule& r) {  // the test of nfcs_acl_set_rules
    return !(r.fields & ~NFCS_ACL_F_ALL) && r.action <= NFCS_ACL_REDIRECT;
}

inline int aclset_set_list(AclSetInputs& in, uint32_t id, const nfcs_acl_rule* rules, uint32_t n) {
    if (id >= NFCS_ACLSET_MAX_LISTS || (n > 0 && !rules) || n > NFCS_ACL_MAX_RULES) return NFCS_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (!acl_rule_ok(rules[i])) return NFCS_EINVAL;
    in.list[id].assign(rules, rules + n);
    in.have[id] = true;
    return NFCS_OK;
}

inline int aclset_remove_list(AclSetInputs& in, uint32_t id) {  // AclManager::delete_acl: bindings to it stay
    if (id >= NFCS_ACLSET_MAX_LISTS) return NFCS_EINVAL;
    in.list[id].clear();
    in.have[id] = false;
    return NFCS_OK;
}

inline int aclset_bind_port(AclSetInputs& in, uint32_t port, uint32_t id) {
    if (port >= NFCS_L2_MAX_PORTS || (id != NFCS_ACL_LIST_NONE && id >= NFCS_ACLSET_MAX_LISTS)) return NFCS_EINVAL;
    if (port >= in.port_list.size()) {
        if (id == NFCS_ACL_LIST_NONE) return NFCS_OK;
        in.port_list.resize(port + 1u, NFCS_ACL_LIST_NONE);
    }
    in.port_list[port] = id;
    return NFCS_OK;
}

inline void aclset_clear(AclSetInputs& in) {
    for (uint32_t i = 0; i < NFCS_ACLSET_MAX_LISTS; ++i) {
        in.list[i].clear();
        in.have[i] = false;
    }
    in.port_list.clear();
}

// NFCS_EINVAL when the lists, each padded, come to more than NFCS_ACL_MAX_RULES rules (t is then empty).
inline int aclset_compile(const AclSetInputs& in, AclSetTables& t) {
    t = AclSetTables{};
    AclBind where[NFCS_ACLSET_MAX_LISTS] = {};
    AclTables one;
    for (uint32_t id = 0; id < NFCS_ACLSET_MAX_LISTS; ++id) {
        if (!in.have[id] || in.list[id].empty()) continue;
        acl_compile(in.list[id], one);
        if (t.rec.size() + one.rec.size() > NFCS_ACL_MAX_RULES) {
            t = AclSetTables{};
            return NFCS_EINVAL;
        }
        where[id] = AclBind{(uint32_t)t.rec.size(), (uint32_t)one.rec.size()};
        t.rec.insert(t.rec.end(), one.rec.begin(), one.rec.end());
        t.act.insert(t.act.end(), one.act.begin(), one.act.end());
        t.act.resize(t.rec.size(), AclAct{NFCS_ACL_PERMIT, NFCS_IF_NONE});
        ++t.lists;
    }
    uint32_t ports = 0;
    for (uint32_t p = 0; p < in.port_list.size(); ++p)
        if (in.port_list[p] != NFCS_ACL_LIST_NONE) ports = p + 1u;
    t.ports = ports;
    t.bind.assign(ports, AclBind{0u, 0u});
    for (uint32_t p = 0; p < ports; ++p)
        if (in.port_list[p] != NFCS_ACL_LIST_NONE) t.bind[p] = where[in.port_list[p]];
    return NFCS_OK;
}

// The first rule of the port's list that matches, as an index into t.rec, or NFCS_ACL_NO_MATCH.
inline uint32_t aclset_first_match(const AclSetTables& t, AclBind b, const uint32_t k[8]) {
    for (uint32_t r = b.first; r < b.first + b.count; ++r) {
        const AclRec& c = t.rec[r];
        uint32_t d = 0;
        for (uint32_t i = 0; i < 8; ++i) d |= (k[i] ^ c.value[i]) & c.mask[i];
        if (d == 0) return r;
    }
    return NFCS_ACL_NO_MATCH;
}

// One frame leaving through `port`. rule_index counts inside the port's list.
inline void aclset_decide(const AclSetTables& t, uint32_t port, const uint8_t* frame, uint32_t len, uint32_t* action,
                          uint32_t* rule_index, uint32_t* redirect_port) {
    const AclBind b = port < t.ports ? t.bind[port] : AclBind{0u, 0u};
    uint32_t r = NFCS_ACL_NO_MATCH;
    if (b.count) {  // without a list the frame is not looked at
        uint32_t k[8];
        acl_key(frame, len, k);
        r = aclset_first_match(t, b, k);
    }
    if (action) *action = r == NFCS_ACL_NO_MATCH ? NFCS_ACL_PERMIT : t.act[r].action;
    if (rule_index) *rule_index = r == NFCS_ACL_NO_MATCH ? NFCS_ACL_NO_MATCH : r - b.first;
    if (redirect_port) *redirect_port = r == NFCS_ACL_NO_MATCH ? NFCS_IF_NONE : t.act[r].redirect;
}

// nfcs_egress_acl_host: the burst in order (the order matters to nothing: the counters are sums). With item_src
// and bypass (n_src bytes) it is nfcs_egress_acl_items_host: an item of a redirected frame keeps its port unread
// and uncounted (switch.hpp:238-240).
inline void aclset_egress(const AclSetTables& t, const uint8_t* arena, uint64_t arena_bytes, const nfcs_desc* desc,
                          uint32_t n, uint32_t* port, uint8_t* action, uint32_t* rule, uint32_t* redirect,
                          uint32_t* denied_pkts, uint64_t* denied_bytes, const uint32_t* item_src = nullptr,
                          const uint8_t* bypass = nullptr, uint32_t n_src = 0) {
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t a = NFCS_ACL_NO_PORT, r = NFCS_ACL_NO_MATCH, rp = NFCS_IF_NONE;
        const uint32_t pt = port[i];
        if (pt != NFCS_IF_NONE && item_src && bypass && item_src[i] < n_src && bypass[item_src[i]]) {
            a = NFCS_ACL_BYPASS;
        } else if (pt != NFCS_IF_NONE) {
            const uint64_t off = (uint64_t)desc[i].off16 * 16u, len = desc[i].len;
            if (off + ((len + 15u) & ~15ull) > arena_bytes) {
                a = NFCS_ACL_BAD_DESC;
                port[i] = NFCS_IF_NONE;
            } else {
                aclset_decide(t, pt, arena + off, (uint32_t)len, &a, &r, &rp);
                if (a == NFCS_ACL_DENY) {
                    port[i] = NFCS_IF_NONE;
                    if (denied_pkts) {  // a denied packet had a list, so pt < t.ports
                        denied_pkts[pt] += 1u;
                        denied_bytes[pt] += len;
                    }
                }
            }
        }
        action[i] = (uint8_t)a;
        if (rule) rule[i] = r;
        if (redirect) redirect[i] = rp;
    }
}

}  // namespace nfcs

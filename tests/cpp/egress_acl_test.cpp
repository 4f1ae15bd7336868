// egress_acl_test.cpp — the egress ACLs through the C ABI from C++ on the GPU: an nfcs_aclset built from the
// rule lists and bindings on stdin, uploaded, nfcs_egress_acl_device over the packets on stdin, and the
// result printed for tests/test_gpu_egress_acl_cpp.py, which holds it against the reference's answers on the
// fixture. The same burst also goes through nfcs_egress_acl_host; exit status 1 when the two differ.
//
// stdin, one item per line:
//   L <list id> <hex of n x 52-byte nfcs_acl_rule, possibly empty>   nfcs_aclset_set_list
//   R <list id>                                                      nfcs_aclset_remove_list
//   B <port> <list id>                                               nfcs_aclset_bind_port
//   F <port> <hex frame>                                             a packet, in burst order
// stdout:
//   per packet  "F <action> <rule> <redirect> <port after>"
//   "I <ports> <lists> <rules_padded>", "P <denied_pkts per port>", "Y <denied_bytes per port>"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nfcs.h"

namespace {

std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return v;
}

#define CHECK(call)                                                   \
    do {                                                              \
        const int rc_ = (call);                                       \
        if (rc_ != NFCS_OK) {                                         \
            std::fprintf(stderr, "%s: %s\n", #call, nfcs_strerror(rc_)); \
            return 2;                                                 \
        }                                                             \
    } while (0)

}  // namespace

int main() {
    nfcs_aclset* set = nullptr;
    CHECK(nfcs_aclset_create(&set));
    std::vector<std::vector<uint8_t>> frames;
    std::vector<uint32_t> port;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string tag, hex;
        uint32_t a = 0, b = 0;
        in >> tag;
        if (tag == "L") {
            in >> a >> hex;
            const std::vector<uint8_t> raw = unhex(hex);
            std::vector<nfcs_acl_rule> rules(raw.size() / sizeof(nfcs_acl_rule));
            if (!raw.empty()) std::memcpy(rules.data(), raw.data(), rules.size() * sizeof(nfcs_acl_rule));
            CHECK(nfcs_aclset_set_list(set, a, rules.data(), (uint32_t)rules.size()));
        } else if (tag == "R") {
            in >> a;
            CHECK(nfcs_aclset_remove_list(set, a));
        } else if (tag == "B") {
            in >> a >> b;
            CHECK(nfcs_aclset_bind_port(set, a, b));
        } else if (tag == "F") {
            in >> a >> hex;
            port.push_back(a);
            frames.push_back(unhex(hex));
        }
    }
    CHECK(nfcs_aclset_commit(set));
    uint32_t ports = 0, lists = 0, padded = 0;
    CHECK(nfcs_aclset_info(set, &ports, &lists, &padded));
    const uint32_t n = (uint32_t)frames.size();
    std::vector<nfcs_desc> desc(n);
    std::vector<uint8_t> arena;
    for (uint32_t i = 0; i < n; ++i) {
        desc[i].off16 = (uint32_t)(arena.size() / 16);
        desc[i].len = (uint32_t)frames[i].size();
        arena.insert(arena.end(), frames[i].begin(), frames[i].end());
        arena.resize((arena.size() + 15) / 16 * 16 + (frames[i].empty() ? 16 : 0), 0xEE);
    }
    // the host walk
    std::vector<uint32_t> h_port = port, h_rule(n), h_red(n), h_pk(ports, 0);
    std::vector<uint8_t> h_action(n);
    std::vector<uint64_t> h_by(ports, 0);
    CHECK(nfcs_egress_acl_host(set, arena.data(), arena.size(), desc.data(), n, h_port.data(), h_action.data(), h_rule.data(),
                               h_red.data(), h_pk.data(), h_by.data()));
    // the device
    nfcs_ctx* ctx = nullptr;
    CHECK(nfcs_ctx_create(0, &ctx));
    CHECK(nfcs_aclset_upload(ctx, set));
    void *d_arena, *d_desc, *d_port, *d_action, *d_rule, *d_red, *d_pk, *d_by;
    CHECK(nfcs_device_alloc(ctx, arena.size(), &d_arena));
    CHECK(nfcs_device_alloc(ctx, n * sizeof(nfcs_desc), &d_desc));
    CHECK(nfcs_device_alloc(ctx, n * 4, &d_port));
    CHECK(nfcs_device_alloc(ctx, n, &d_action));
    CHECK(nfcs_device_alloc(ctx, n * 4, &d_rule));
    CHECK(nfcs_device_alloc(ctx, n * 4, &d_red));
    CHECK(nfcs_device_alloc(ctx, (ports + 1) * 4, &d_pk));
    CHECK(nfcs_device_alloc(ctx, (ports + 1) * 8, &d_by));
    std::vector<uint32_t> pk(ports + 1, 0);
    std::vector<uint64_t> by(ports + 1, 0);
    CHECK(nfcs_memcpy_h2d(ctx, d_arena, arena.data(), arena.size()));
    CHECK(nfcs_memcpy_h2d(ctx, d_desc, desc.data(), n * sizeof(nfcs_desc)));
    CHECK(nfcs_memcpy_h2d(ctx, d_port, port.data(), n * 4));
    CHECK(nfcs_memcpy_h2d(ctx, d_pk, pk.data(), pk.size() * 4));
    CHECK(nfcs_memcpy_h2d(ctx, d_by, by.data(), by.size() * 8));
    CHECK(nfcs_egress_acl_device(ctx, set, (const uint8_t*)d_arena, arena.size(), (const nfcs_desc*)d_desc, n, (uint32_t*)d_port,
                                 (uint8_t*)d_action, (uint32_t*)d_rule, (uint32_t*)d_red, (uint32_t*)d_pk, (uint64_t*)d_by,
                                 nullptr));
    CHECK(nfcs_stream_sync(ctx, nullptr));
    std::vector<uint32_t> g_port(n), g_rule(n), g_red(n);
    std::vector<uint8_t> g_action(n), g_arena(arena.size());
    CHECK(nfcs_memcpy_d2h(ctx, g_port.data(), d_port, n * 4));
    CHECK(nfcs_memcpy_d2h(ctx, g_action.data(), d_action, n));
    CHECK(nfcs_memcpy_d2h(ctx, g_rule.data(), d_rule, n * 4));
    CHECK(nfcs_memcpy_d2h(ctx, g_red.data(), d_red, n * 4));
    CHECK(nfcs_memcpy_d2h(ctx, pk.data(), d_pk, pk.size() * 4));
    CHECK(nfcs_memcpy_d2h(ctx, by.data(), d_by, by.size() * 8));
    CHECK(nfcs_memcpy_d2h(ctx, g_arena.data(), d_arena, arena.size()));
    for (void* p : {d_arena, d_desc, d_port, d_action, d_rule, d_red, d_pk, d_by}) nfcs_device_free(ctx, p);
    nfcs_aclset_destroy(set);  // before the ctx
    nfcs_ctx_destroy(ctx);
    pk.pop_back();
    by.pop_back();
    if (g_port != h_port || g_action != h_action || g_rule != h_rule || g_red != h_red || pk != h_pk || by != h_by ||
        g_arena != arena) {
        std::fprintf(stderr, "device and host differ\n");
        return 1;
    }
    for (uint32_t i = 0; i < n; ++i) std::printf("F %u %u %u %u\n", g_action[i], g_rule[i], g_red[i], g_port[i]);
    std::printf("I %u %u %u\nP", ports, lists, padded);
    for (uint32_t v : pk) std::printf(" %u", v);
    std::printf("\nY");
    for (uint64_t v : by) std::printf(" %llu", (unsigned long long)v);
    std::printf("\n");
    return 0;
}

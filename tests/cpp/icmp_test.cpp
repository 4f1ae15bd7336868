// icmp_test.cpp — stand-alone host program over netflow_amd/csrc/nfcs_icmp.h (no HIP, no GPU): compiles random
// tables, builds bursts of random frames (truncated headers, IHL 0-15, tags, lengths around every bound the
// plan tests) and runs the host walk icmp_respond over them with every array — the arena included — in a heap
// block of exactly its size, cap and the message region cut short at random, so that a read past a frame or a
// store past the emitted prefix, past cap or past the arena is reported. Every emitted message is then checked
// on its own bytes: the fixed header fields, both checksums recomputed by the reference's rule (big-endian
// words, an odd last byte as the low byte), the slot layout and the inert entries. Built and run by
// tests/test_icmp.py under -fsanitize=address,undefined. Exit status 0 = everything agrees.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "nfcs_icmp.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

uint32_t ip_of(uint32_t net, uint32_t host) { return 10u | (net << 16) | (host << 24); }  // 10.0.net.host, network order

uint32_t sum_be(const uint8_t* d, uint32_t len) {
    uint32_t s = 0, i = 0;
    for (; i + 1u < len; i += 2u) s += ((uint32_t)d[i] << 8) | d[i + 1u];
    if (i < len) s += d[i];
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);   \
            return 1;                                         \
        }                                                     \
    } while (0)

int burst(uint32_t n) {
    nfcs::FibInputs fin;
    nfcs::IcmpInputs iin;
    for (uint32_t k = 0; k < 6; ++k) {  // interface k: 10.0.k.1, network 10.0.k.0/24; some lack pieces
        if (rnd() % 5u) fin.routes.push_back(nfcs_fib_route{ip_of(k, 0), 0x00FFFFFFu, (rnd() % 3u) ? 0u : ip_of(k, 2), k});
        nfcs_fib_if_mac m{k, {2, 0, 0, 0, 0, (uint8_t)k}, {0, 0}};
        if (rnd() % 5u) fin.if_macs.push_back(m);
        nfcs_icmp_local l{ip_of(k, 1), {2, 0, 0, 0, 1, (uint8_t)k}, {0, 0}};
        if (rnd() % 5u) iin.local.push_back(l);
        if (rnd() % 5u) iin.if_ips.push_back(nfcs_icmp_if_ip{k, ip_of(k, 1)});
        if (rnd() % 5u) iin.up.push_back(k);
        fin.local_ips.push_back(ip_of(k, 1));
        for (uint32_t h = 2; h < 6; ++h) {
            nfcs_fib_arp a{ip_of(k, h), {2, 0, 0, 1, (uint8_t)k, (uint8_t)h}, {0, 0}};
            if (rnd() % 4u) fin.arp.push_back(a);
        }
    }
    iin.up.push_back(77);
    iin.num_ports = 5;  // interface 5 is never a port
    nfcs::FibTables ft;
    nfcs::IcmpTables it;
    nfcs::fib_compile(fin, ft);
    nfcs::icmp_compile(iin, it);

    // frames
    std::vector<std::vector<uint8_t>> frames(n);
    std::vector<uint8_t> verdict(n);
    std::vector<uint16_t> ids(n);
    const uint32_t kPay[] = {0, 1, 2, 5, 6, 7, 8, 9, 21, 22, 23, 37, 38, 100, 1000, 1499, 1535, 1536, 1537, 3100};
    for (uint32_t i = 0; i < n; ++i) {
        const bool tagged = rnd() % 3u == 0;
        const uint32_t ihl = (rnd() % 4u) ? 5u : rnd() % 16u, l2 = tagged ? 18u : 14u;
        const uint32_t pay = kPay[rnd() % (sizeof kPay / sizeof kPay[0])];
        std::vector<uint8_t> f(l2 + 20u + (ihl > 5u ? (ihl - 5u) * 4u : 0u) + 8u + pay);
        for (uint8_t& b : f) b = (uint8_t)rnd();
        f[12] = tagged ? 0x81 : 0x08;
        f[13] = 0x00;
        if (tagged) { f[16] = 0x08; f[17] = 0x00; }
        uint8_t* ip = f.data() + l2;
        ip[0] = (uint8_t)(0x40u | ihl);
        uint32_t tl = ihl * 4u + 8u + pay;
        if (rnd() % 8u == 0) tl = rnd() % 70000u;
        ip[2] = (uint8_t)(tl >> 8);
        ip[3] = (uint8_t)tl;
        ip[8] = (uint8_t)(rnd() % 3u);
        ip[9] = (rnd() % 6u) ? 1 : 17;
        const uint32_t src = (rnd() % 8u) ? ip_of(rnd() % 7u, 2u + rnd() % 5u) : rnd();
        const uint32_t dst = (rnd() % 2u) ? ip_of(rnd() % 7u, 1) : rnd();
        memcpy(ip + 12, &src, 4);
        memcpy(ip + 16, &dst, 4);
        if (l2 + ihl * 4u + 2u <= f.size() && rnd() % 6u) { f[l2 + ihl * 4u] = 8; f[l2 + ihl * 4u + 1u] = 0; }
        if (rnd() % 6u == 0) f.resize(rnd() % (f.size() + 1u));  // truncated anywhere
        frames[i] = f;
        const uint8_t kinds[] = {NFCS_RT_LOCAL, NFCS_RT_TTL_EXPIRED, NFCS_RT_NO_ROUTE, NFCS_RT_FORWARD, NFCS_RT_NOT_IPV4, 99};
        verdict[i] = kinds[rnd() % ((rnd() % 4u) ? 3u : 6u)];
        ids[i] = (uint16_t)rnd();
    }
    const uint32_t aligns[] = {16, 32, 64, 128, 4096};
    const uint32_t align = aligns[rnd() % 5u];
    std::unique_ptr<nfcs_desc[]> desc(new nfcs_desc[n]);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        desc[i] = nfcs_desc{(uint32_t)(pos / 16u), (uint32_t)frames[i].size()};
        pos += (frames[i].size() + 15u) & ~(size_t)15u;
        if (rnd() % 4u == 0) pos += 16u * (rnd() % 9u);
    }
    const uint64_t msg_base = nfcs::flood_round_up(pos, align);

    // what the burst calls for, with room for everything
    auto run = [&](uint64_t region, uint32_t cap, std::vector<uint8_t>& arena, std::vector<nfcs_desc>& md,
                   std::vector<uint32_t>& mp, std::vector<uint32_t>& ms, std::vector<uint8_t>& st, nfcs_icmp_totals& tot) {
        // exact-size heap blocks; the last frame's padding to 16 bytes exists (a descriptor's contract)
        std::unique_ptr<uint8_t[]> a(new uint8_t[msg_base + region]);
        memset(a.get(), 0xEE, msg_base + region);
        for (uint32_t i = 0; i < n; ++i)
            if (!frames[i].empty()) memcpy(a.get() + (uint64_t)desc[i].off16 * 16u, frames[i].data(), frames[i].size());
        std::unique_ptr<nfcs_desc[]> d(new nfcs_desc[cap]);
        std::unique_ptr<uint32_t[]> p(new uint32_t[cap]), s(new uint32_t[cap]);
        std::unique_ptr<uint8_t[]> status(new uint8_t[n]);
        nfcs::icmp_respond(it, ft, 1, a.get(), msg_base + region, msg_base, align, desc.get(), n, verdict.data(), ids.data(),
                           cap, d.get(), p.get(), s.get(), status.get(), &tot);
        arena.assign(a.get(), a.get() + msg_base + region);
        md.assign(d.get(), d.get() + cap);
        mp.assign(p.get(), p.get() + cap);
        ms.assign(s.get(), s.get() + cap);
        st.assign(status.get(), status.get() + n);
    };
    std::vector<uint8_t> arena, st, arena2, st2;
    std::vector<nfcs_desc> md, md2;
    std::vector<uint32_t> mp, ms, mp2, ms2;
    nfcs_icmp_totals full, cut;
    // first with room for everything: a dry run sizes it
    run(0, 0, arena, md, mp, ms, st, full);
    CHECK(full.messages == 0 && full.msg_bytes == 0);
    const uint32_t need = full.messages_needed;
    const uint64_t need_bytes = full.msg_bytes_needed;
    run(need_bytes, need, arena, md, mp, ms, st, full);
    CHECK(full.messages == need && full.messages_needed == need && full.msg_bytes == need_bytes);
    CHECK(full.echo_replies + full.errors == need);
    uint64_t at = msg_base;
    uint32_t echoes = 0;
    for (uint32_t k = 0; k < need; ++k) {
        const uint8_t* m = arena.data() + (uint64_t)md[k].off16 * 16u;
        const uint32_t len = md[k].len, src = ms[k];
        CHECK((uint64_t)md[k].off16 * 16u == at && len >= 42u && len <= 65549u && src < n && (k == 0 || ms[k - 1] < src));
        at += nfcs::flood_round_up(len, align);
        CHECK(m[12] == 0x08 && m[13] == 0x00 && m[14] == 0x45 && m[15] == 0 && m[20] == 0 && m[21] == 0 && m[22] == 64 && m[23] == 1);
        CHECK((((uint32_t)m[16] << 8) | m[17]) == len - 14u);
        CHECK(sum_be(m + 14, 20) == 0xFFFFu && sum_be(m + 34, len - 34u) == 0xFFFFu);
        for (uint32_t b = len; b < ((len + 15u) & ~15u); ++b) CHECK(m[b] == 0);
        const std::vector<uint8_t>& f = frames[src];
        const uint32_t l2 = f[12] == 0x81 ? 18u : 14u, ihl4 = (f[l2] & 15u) * 4u;
        if (st[src] == NFCS_ICMP_ST_ECHO_REPLY) {
            ++echoes;
            CHECK(verdict[src] == NFCS_RT_LOCAL && mp[k] == 1u && m[34] == 0 && m[35] == 0 && m[18] == 0 && m[19] == 0);
            CHECK(!memcmp(m, f.data() + 6, 6) && !memcmp(m + 26, f.data() + l2 + 16, 4) && !memcmp(m + 30, f.data() + l2 + 12, 4));
            CHECK(!memcmp(m + 38, f.data() + l2 + ihl4 + 4u, len - 38u));
        } else {
            const bool ttl = st[src] == NFCS_ICMP_ST_TIME_EXCEEDED;
            CHECK(ttl || st[src] == NFCS_ICMP_ST_UNREACHABLE);
            CHECK(verdict[src] == (ttl ? NFCS_RT_TTL_EXPIRED : NFCS_RT_NO_ROUTE) && m[34] == (ttl ? 11 : 3) && m[35] == 0);
            CHECK(m[18] == (uint8_t)(ids[src] >> 8) && m[19] == (uint8_t)ids[src] && !memcmp(m + 30, f.data() + l2 + 12, 4));
            CHECK(m[38] == 0 && m[39] == 0 && m[40] == 0 && m[41] == 0 && !memcmp(m + 42, f.data() + l2, len - 42u));
            CHECK(len - 42u == ihl4 + (f.size() - l2 - ihl4 < 8u ? f.size() - l2 - ihl4 : 8u));
            CHECK(mp[k] < 5u);
        }
    }
    CHECK(echoes == full.echo_replies);
    for (uint32_t i = 0; i < n; ++i)  // no byte of the frames changed
        CHECK(frames[i].empty() || !memcmp(arena.data() + (uint64_t)desc[i].off16 * 16u, frames[i].data(), frames[i].size()));
    // then with cap and the region cut short: the same prefix
    for (uint32_t rep = 0; rep < 4; ++rep) {
        const uint32_t cap = need ? rnd() % (need + 2u) : rnd() % 3u;
        const uint64_t region = need_bytes ? rnd() % (need_bytes + 64u) : 0u;
        run(region, cap, arena2, md2, mp2, ms2, st2, cut);
        CHECK(cut.messages_needed == need && cut.msg_bytes_needed == need_bytes && cut.messages <= cap && cut.messages <= need);
        uint64_t used = 0;
        uint32_t want = 0;
        while (want < need && want < cap && used + nfcs::flood_round_up(md[want].len, align) <= region)
            used += nfcs::flood_round_up(md[want++].len, align);
        CHECK(cut.messages == want && cut.msg_bytes == used);
        for (uint32_t k = 0; k < cap; ++k) {
            if (k < want) CHECK(md2[k].off16 == md[k].off16 && md2[k].len == md[k].len && mp2[k] == mp[k] && ms2[k] == ms[k]);
            else CHECK(md2[k].off16 == 0 && md2[k].len == 0 && mp2[k] == NFCS_IF_NONE && ms2[k] == NFCS_ITEM_NONE);
        }
        CHECK(msg_base == 0 || !memcmp(arena2.data(), arena.data(), msg_base));
        for (uint32_t k = 0; k < want; ++k)
            CHECK(!memcmp(arena2.data() + (uint64_t)md[k].off16 * 16u, arena.data() + (uint64_t)md[k].off16 * 16u,
                          (md[k].len + 15u) & ~15u));
        for (uint64_t b = msg_base + used; b < msg_base + region; ++b) CHECK(arena2[b] == 0xEE);
        uint32_t k = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const bool msg = st[i] >= NFCS_ICMP_ST_ECHO_REPLY && st[i] <= NFCS_ICMP_ST_UNREACHABLE;
            CHECK(st2[i] == ((msg && k >= want) ? (uint8_t)NFCS_ICMP_ST_OVERFLOW : st[i]));
            k += msg;
        }
    }
    return 0;
}

}  // namespace

int main() {
    uint32_t total = 0;
    for (uint32_t rep = 0; rep < 60; ++rep) {
        const uint32_t n = rep < 4 ? rep : 1u + rnd() % 200u;
        const int rc = burst(n);
        if (rc) {
            fprintf(stderr, "burst %u (n = %u) failed\n", rep, n);
            return rc;
        }
        total += n;
    }
    printf("icmp host walk OK: %u packets\n", total);
    return 0;
}

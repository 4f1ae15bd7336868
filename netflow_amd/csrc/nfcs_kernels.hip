// nfcs_kernels.hip — CDNA4 (gfx950) kernels of the batched Internet-checksum engine.
//
// The hot path is NetFlow++'s Packet::update_checksums() (include/netflow++/packet.hpp:722-890)
// with its fold Packet::calculate_checksum() (packet.hpp:894-912), applied to a batch of
// frames in HBM. Design (every choice below was A/B-measured, profiles/):
//
//  * One 16-lane DPP row per packet, four packets per wave64, 16 packets per 256-thread
//    workgroup, one workgroup per 16 packets (no grid-stride loop). Lane rl of a row loads
//    chunks rl, rl+16, ... of its frame as 16-byte global_load_dwordx4 (a row reads 256
//    contiguous bytes per instruction); K = 6 slots cover a 1536-byte frame in one batch,
//    longer (jumbo) frames continue in further batches of K slots.
//  * The descriptors of a wave's four packets are consecutive: one scalar s_load_dwordx8.
//  * All per-packet decisions run on the VALU, so one instruction serves four packets. (A
//    wave-per-packet kernel with the parse on SGPRs measured 364 SALU + 194 VALU instructions
//    per 1500-byte packet and was bound by the CU's single scalar unit at 1.9 TB/s.)
//  * Header fields reach the whole row by DPP row_newbcast at compile-time offsets: an
//    802.1Q tag is removed once per lane (one row_shl:1 + 4 selects), and the common headers
//    (untagged/tagged x IPv4 IHL 5 / IPv6 / non-IP) are planned at constant offsets. Anything
//    else (IP options, IHL < 5, headers past the frame) is parsed by the row's lane 0 from
//    memory; IHL < 5 overlaps run an exact sequential emulation of the reference.
//  * The L4 region is summed as little-endian dwords into an exact 64-bit per-lane sum. The
//    one's-complement sum is byte-order independent (RFC 1071 §2(B)): the LE-domain fold is
//    bswap16 of the reference's big-endian fold, so one swap at the end replaces the
//    reference's per-word ntohs. Full chunks are added unmasked; at most two boundary chunks
//    per packet are masked. The checksum field bytes (which the reference zeroes) and the 2
//    bytes before a region starting at 2 mod 4 are subtracted exactly; the odd trailing byte,
//    which the reference adds as the LOW byte (packet.hpp:903-905), gets +255*b.
//  * Row sum: four DPP steps. Final fold, complement, UDP 0 -> 0xFFFF (packet.hpp:867-871),
//    then the 2+2 checksum bytes are stored from lanes 0..3 of the row.
//  * Cache policy: the header slot is loaded with the default policy and the payload slots
//    with non-temporal (evict-first) loads (measured best for the 1500-byte config).
//  * No MFMA and no LDS staging: this is an HBM-read-bound integer fold.
#include "nfcs_internal.h"

namespace nfcs {

#define DEV __device__ __forceinline__

DEV uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// XCD-aware block order: workgroups are dealt to the 8 XCDs round-robin; this bijection on
// [0, gridDim.x) gives each XCD one contiguous eighth of the blocks (the tail beyond a
// multiple of 8 keeps its order).
DEV uint32_t xcd_block_n(uint32_t nblocks) {
    const uint32_t b = blockIdx.x, g8 = nblocks / 8u;
    return b < 8u * g8 ? (b % 8u) * g8 + b / 8u : b;
}
DEV uint32_t xcd_block() { return xcd_block_n(gridDim.x); }
DEV uint32_t bswap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }

// The target of every load of a lane past its frame (or, in a line-aligned window, before it): every
// load is issued by every lane, so a wave's compiler-counted vmcnt waits stay static. One zero line,
// aligned to 4 KB, so its page offset never depends on what the linker places before it (round 4's
// 16-byte g_zero16 sat wherever the linker put it). Round 5 measured the alternatives on one box,
// alternating builds (profiles/r05_zero_target_ab.jsonl): one chunk per slot of a pool,
// the same instruction's first in-frame chunk (no extra request, but ~12 more instructions per slot
// ahead of the loads: C1 -2.5%, the C4 shard -2%), the wave's row-0 frame start — none faster; and the
// forward's C3 mix moves by +-3% from run to run in every form, round 4's as well.
__device__ __attribute__((aligned(4096))) uint4 g_zero_line[8];

// Component j of a uint4 by mask arithmetic (no indexable temporary, so no scratch).
DEV uint32_t comp(const uint4& v, uint32_t j) {
    const uint32_t m0 = 0u - (uint32_t)(j == 0), m1 = 0u - (uint32_t)(j == 1);
    const uint32_t m2 = 0u - (uint32_t)(j == 2), m3 = 0u - (uint32_t)(j == 3);
    return (v.x & m0) | (v.y & m1) | (v.z & m2) | (v.w & m3);
}


DEV uint4 put_byte(const uint4& v, uint32_t i, uint32_t b) {
    uint32_t r[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t sh = 8u * (i & 3u);
        const uint32_t m = ((i >> 2) == j) ? (0xFFu << sh) : 0u;
        r[j] = (comp(v, j) & ~m) | ((b << sh) & m);
    }
    return make_uint4(r[0], r[1], r[2], r[3]);
}

// Lane rl's chunk register v (frame bytes 16*rl .. 16*rl+15) with the 2-byte field w patched in
// (w: frame offset in the low half, the byte for that offset in bits 16-23, the next in 24-31;
// offset 0xFFFF = none). A field inside one dword — every fast-path header's — is one masked
// 16-bit insert; one that straddles two dwords goes byte by byte. In the fused L3 forward's
// segment store it took the forward on the C3 mix from 0.511 to 0.536 (its short waves are
// latency-bound and this VALU sits on their path).
DEV uint4 put_field(const uint4& v, uint32_t w, uint32_t rl) {
    const uint32_t pos = w & 0xFFFFu;
    if (pos == NFCS_PATCH_NONE || (pos & 3u) != 3u) {
        const bool mine = pos != NFCS_PATCH_NONE && (pos >> 4) == rl;
        const uint32_t sh = 8u * (pos & 3u), j = (pos >> 2) & 3u;
        const uint32_t m = mine ? (0xFFFFu << sh) : 0u, b = ((w >> 16) << sh) & m;
        return make_uint4(j == 0 ? ((v.x & ~m) | b) : v.x, j == 1 ? ((v.y & ~m) | b) : v.y,
                          j == 2 ? ((v.z & ~m) | b) : v.z, j == 3 ? ((v.w & ~m) | b) : v.w);
    }
    uint4 r = v;
    if ((pos >> 4) == rl) r = put_byte(r, pos & 15u, (w >> 16) & 0xFFu);
    if (((pos + 1u) >> 4) == rl) r = put_byte(r, (pos + 1u) & 15u, (w >> 24) & 0xFFu);
    return r;
}


// ---- exact sequential path (IHL < 5 overlap cases), one lane --------------------------------
// Mirrors packet.hpp:722-890 byte by byte on global memory, in the reference's write order.
struct SeqOut { uint32_t st, ip_off, ip_val, l4_off, l4_val; };

__device__ uint32_t g_be16(const uint8_t* f, uint32_t o) { return ((uint32_t)f[o] << 8) | f[o + 1]; }
__device__ uint32_t g_sum(const uint8_t* d, uint32_t len) {  // 898-905, raw sum
    uint32_t s = 0, i = 0;
    for (; len > 1; len -= 2, i += 2) s += g_be16(d, i);
    if (len) s += d[i];
    return s;
}
__device__ uint32_t g_fin(uint32_t s) {  // 907-911: value stored big-endian
    while (s >> 16) s = (s & 0xFFFF) + (s >> 16);
    return (~s) & 0xFFFFu;
}

__device__ __noinline__ SeqOut seq_update(uint8_t* f, uint32_t len) {
    SeqOut o = {NFCS_ST_NONE, NFCS_PATCH_NONE, 0, NFCS_PATCH_NONE, 0};
    uint32_t l2 = 14;
    if (len >= 14) l2 = (g_be16(f, 12) == 0x8100u) ? 18u : 14u;
    uint32_t v4 = 0, proto, ihl4 = 0, l4;
    if (l2 + 20 <= len && (f[l2] >> 4) == 4) {
        v4 = 1;
        proto = f[l2 + 9];
        ihl4 = (f[l2] & 15u) * 4u;
        l4 = l2 + ihl4;
        if (l2 + ihl4 > len) { o.st = NFCS_ST_OOB; return o; }
        f[l2 + 10] = 0;
        f[l2 + 11] = 0;
        uint32_t c = g_fin(g_sum(f + l2, ihl4));
        f[l2 + 10] = (uint8_t)(c >> 8);
        f[l2 + 11] = (uint8_t)c;
        o.ip_off = l2 + 10;
        o.ip_val = bswap16(c);
        o.st = NFCS_ST_V4;
    } else {
        uint32_t et = (len >= 14) ? g_be16(f, 12) : 0;
        if (et == 0x8100u) et = (len >= 18) ? g_be16(f, 16) : 0;
        if (et != 0x86DDu || !(l2 + 40 <= len && (f[l2] >> 4) == 6)) return o;
        proto = f[l2 + 6];
        l4 = l2 + 40;
        o.st = NFCS_ST_V6;
    }
    const uint32_t skip = v4 ? NFCS_ST_V4_L4SKIP : NFCS_ST_V6_L4SKIP;
    uint32_t fs, L, st;
    uint32_t sum = 0;
    if (proto == 6) {
        if (l4 + 19 > len) { o.st = skip; return o; }
        uint32_t hl = (f[l4 + 12] >> 4) * 4u;
        if (v4) {
            uint32_t tl = g_be16(f, l2 + 2);
            if (tl < ihl4) { o.st = skip; return o; }
            L = (tl - ihl4) & 0xFFFFu;
        } else {
            L = g_be16(f, l2 + 4);
        }
        if (L < hl || l4 + L > len) { o.st = skip; return o; }
        fs = l4 + 15;
        st = v4 ? NFCS_ST_V4_TCP : NFCS_ST_V6_TCP;
    } else if (proto == 17) {
        if (l4 + 8 > len) { o.st = skip; return o; }
        L = g_be16(f, l4 + 4);
        if (L < 8 || l4 + L > len) { o.st = skip; return o; }
        fs = l4 + 6;
        st = v4 ? NFCS_ST_V4_UDP : NFCS_ST_V6_UDP;
    } else if (proto == 1 && v4) {
        if (l4 + 8 > len) { o.st = skip; return o; }
        uint32_t tl = g_be16(f, l2 + 2);
        if (tl < ihl4) { o.st = skip; return o; }
        L = tl - ihl4;
        if (l4 + L > len || L < 8) { o.st = skip; return o; }
        fs = l4 + 2;
        st = NFCS_ST_V4_ICMP;
    } else {
        return o;
    }
    f[fs] = 0;  // zero the field, then read pseudo-header and segment (reference order)
    f[fs + 1] = 0;
    if (proto != 1) {
        if (v4) sum = g_sum(f + l2 + 12, 8) + proto + L;
        else sum = g_sum(f + l2 + 8, 32) + (L >> 16) + (L & 0xFFFF) + proto;
    }
    sum += g_sum(f + l4, L);
    uint32_t c = g_fin(sum);
    if (proto == 17 && c == 0) c = 0xFFFF;
    f[fs] = (uint8_t)(c >> 8);
    f[fs + 1] = (uint8_t)c;
    o.l4_off = fs;
    o.l4_val = bswap16(c);
    o.st = st;
    return o;
}

// ---- region accumulation ---------------------------------------------------------------------
// The L4 region is summed as 16-bit little-endian words: v_sad_u16(d, 0, acc) adds both
// halves of a dword to a u32 accumulator in one instruction, with no carry chain. The word
// sum is congruent to the dword sum mod 0xFFFF (65536 = 1 mod 0xFFFF) and both are zero
// exactly when every byte is, so they fold to the same checksum; it cannot overflow 32 bits
// (a region ends before l4 + 65,536 < 65,614 bytes: 16,404 dwords x 131,070 < 2^32).
DEV uint32_t wsum(uint32_t d, uint32_t acc) { return __builtin_amdgcn_sad_u16(d, 0u, acc); }

DEV uint32_t add_chunk(const uint4& v, uint32_t acc) {
    return wsum(v.w, wsum(v.z, wsum(v.y, wsum(v.x, acc))));
}

// End-around-carry fold of an exact sum to 16 bits (packet.hpp:907-909), branch-free: two
// steps take any u32 below 0x10000 (a further step on such a value is the identity, so this
// equals the reference's while loop). Zero stays zero; a nonzero multiple of 0xFFFF folds to
// 0xFFFF, as in the reference.
DEV uint32_t fold32(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);  // <= 0x1FFFE
    return (s & 0xFFFFu) + (s >> 16);
}

// =============================================================================================
// v3: one 16-lane DPP row per packet, four packets per wave, all per-packet logic on the VALU.
//
// v2 (one wave per packet, parse on SGPRs) measured 364 SALU + 194 VALU instructions per
// 1500 B packet: the CU's single scalar unit, not HBM, set the rate (profiles/). Here every
// per-packet decision runs once per 16-lane row, so one VALU instruction serves four packets
// and the scalar unit only runs the loop. Lane rl of a row holds chunks rl, rl+16, ... of its
// packet; header dwords reach the whole row by DPP row_newbcast (compile-time offsets) or
// ds_bpermute (runtime offsets: IP options, IPv6); the row sum is four DPP steps.
// =============================================================================================

// Lane L of this lane's packet row. R = 16: one DPP row_newbcast. R = 8 (two packets per DPP
// row): row_newbcast L into banks 0-1 (lanes 0-7), row_newbcast 8+L into banks 2-3 (8-15).
template <int L, int R = 16>
DEV uint32_t row_bcast(uint32_t x) {
    static_assert(R == 16 || R == 8, "row width");
    if (R == 16) return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x150 + L, 0xF, 0xF, false);
    const int lo = __builtin_amdgcn_mov_dpp((int)x, 0x150 + (L & 7), 0xF, 0x3, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(lo, (int)x, 0x158 + (L & 7), 0xF, 0xC, false);
}

// Per-lane view of the header bytes [0, 16R) of the row's packet: lane rl of the row holds
// chunk rl (frame bytes 16rl .. 16rl+15) of slot 0. Every header field the plan reads lies
// below byte 128, so R = 8 rows see all of them.
template <int R>
struct RowHdr {
    uint4 c0;
    uint32_t rowbase4;  // byte address of lane 0 of this row, for ds_bpermute
    DEV uint32_t dw(uint32_t q) const {
        const uint32_t x = comp(c0, q & 3u);
        if (__builtin_constant_p(q)) {
            switch ((q >> 2) & (R - 1)) {
            case 0: return row_bcast<0, R>(x);   case 1: return row_bcast<1, R>(x);
            case 2: return row_bcast<2, R>(x);   case 3: return row_bcast<3, R>(x);
            case 4: return row_bcast<4, R>(x);   case 5: return row_bcast<5, R>(x);
            case 6: return row_bcast<6, R>(x);   case 7: return row_bcast<7, R>(x);
            case 8: return row_bcast<8, R>(x);   case 9: return row_bcast<9, R>(x);
            case 10: return row_bcast<10, R>(x); case 11: return row_bcast<11, R>(x);
            case 12: return row_bcast<12, R>(x); case 13: return row_bcast<13, R>(x);
            case 14: return row_bcast<14, R>(x); default: return row_bcast<15, R>(x);
            }
        }
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(rowbase4 + ((q >> 2) & (R - 1)) * 4u), (int)x);
    }
    DEV uint32_t b(uint32_t o) const { return (dw(o >> 2) >> (8 * (o & 3u))) & 0xFFu; }
    DEV uint32_t le16(uint32_t o) const { return (dw(o >> 2) >> (8 * (o & 2u))) & 0xFFFFu; }
    DEV uint32_t be16(uint32_t o) const { return bswap16(le16(o)); }
};

// Compact per-lane plan (row-uniform values).
enum : uint32_t { F_IP = 1, F_L4 = 2, F_UDP = 4, F_TAIL = 8, F_SEQ = 16 };
struct RPlan {
    uint32_t st;     // status byte
    uint32_t flags;  // F_*
    uint32_t ipw;    // ip_off | ip_val << 16
    uint32_t rs, re, fs;
    uint32_t corr;   // pseudo-header words minus over-counted bytes (two's complement)
    uint32_t old;    // fast path: the frame's IPv4 field bytes as read (LE16) | its L4 field bytes << 16
};

DEV RPlan rplan_none(uint32_t st) {
    RPlan P;
    P.st = st; P.flags = 0; P.ipw = 0; P.rs = 0; P.re = 0; P.fs = 0; P.corr = 0; P.old = 0;
    return P;
}

// Header bytes with an 802.1Q tag removed: view byte o (o >= 12) is frame byte o + 4*tagged.
// The reference's offsets are all relative to l2 = 14 or 18 (ethernet(), packet.hpp:405-418),
// so one plan written at l2 = 14 serves both framings. Each lane shifts its own chunk by one
// dword (the 4th dword comes from the next lane of the row via DPP row_shl:1), so every
// header access afterwards is a single row broadcast at a compile-time offset.
DEV uint4 strip_tag(const uint4& c, bool tagged) {
    const uint32_t nx = (uint32_t)__builtin_amdgcn_mov_dpp((int)c.x, 0x101, 0xF, 0xF, true);
    const uint32_t m = 0u - (uint32_t)tagged;
    return make_uint4((c.x & ~m) | (c.y & m), (c.y & ~m) | (c.z & m),
                      (c.z & ~m) | (c.w & m), (c.w & ~m) | (nx & m));
}


// L4 branch of packet.hpp:773-889 in view coordinates with compile-time l2 = 14 and l4
// (34 for IPv4 with IHL 5, 54 for IPv6); sh = 4 for tagged frames shifts the frame offsets.
// OLD (here and in the two plans below): also return the checksum fields' bytes as they are (RPlan::old);
// the fused forward does not ask for them and compiles as before.
template <int R, bool OLD>
DEV RPlan fast_l4(const RowHdr<R>& V, RPlan P, uint32_t lenv, uint32_t v4, uint32_t l4, uint32_t proto,
                  uint32_t sh) {
    const uint32_t l2 = 14, ihl4 = 20;
    const uint32_t skip = v4 ? NFCS_ST_V4_L4SKIP : NFCS_ST_V6_L4SKIP;
    uint32_t L, fs, st, fl = F_L4;
    if (proto == 6) {
        if (l4 + 19 > lenv) { P.st = skip; return P; }  // sizeof(TcpHeader) == 19
        const uint32_t hl = (V.b(l4 + 12) >> 4) * 4u;
        if (v4) {
            const uint32_t tl = V.be16(l2 + 2);
            if (tl < ihl4) { P.st = skip; return P; }
            L = (tl - ihl4) & 0xFFFFu;
        } else {
            L = V.be16(l2 + 4);
        }
        if (L < hl || l4 + L > lenv) { P.st = skip; return P; }
        fs = l4 + 15;  // TcpHeader::checksum at offset 15 (19-byte packed struct)
        st = v4 ? NFCS_ST_V4_TCP : NFCS_ST_V6_TCP;
    } else if (proto == 17) {
        if (l4 + 8 > lenv) { P.st = skip; return P; }
        L = V.be16(l4 + 4);
        if (L < 8 || l4 + L > lenv) { P.st = skip; return P; }
        fs = l4 + 6;
        fl |= F_UDP;
        st = v4 ? NFCS_ST_V4_UDP : NFCS_ST_V6_UDP;
    } else if (proto == 1 && v4) {
        if (l4 + 8 > lenv) { P.st = skip; return P; }
        const uint32_t tl = V.be16(l2 + 2);
        if (tl < ihl4) { P.st = skip; return P; }
        L = tl - ihl4;
        if (l4 + L > lenv || L < 8) { P.st = skip; return P; }
        fs = l4 + 2;
        st = NFCS_ST_V4_ICMP;
    } else {
        return P;
    }
    uint32_t add = 0;
    if (proto != 1) {  // pseudo-header in the LE domain (797-816 / 840-859)
        add = bswap16(proto) + bswap16(L);
        if (v4) {
#pragma unroll
            for (uint32_t w = 0; w < 8; w += 2) add += V.le16(l2 + 12 + w);
        } else {
#pragma unroll
            for (uint32_t w = 0; w < 32; w += 2) add += V.le16(l2 + 8 + w);
        }
    }
    // over-counted bytes: the LE word before l4 when l4 = 2 mod 4 (sh keeps the parity), and
    // the raw checksum field bytes the reference zeroes first (795 / 838 / 885)
    const uint32_t re = l4 + L;
    uint32_t sub = ((l4 + sh) & 2u) ? V.le16(l4 - 2) : 0u;
    if (fs < re) sub += V.b(fs) << (((fs + sh) & 1u) ? 8 : 0);
    if (fs + 1 < re) sub += V.b(fs + 1) << (((fs + 1 + sh) & 1u) ? 8 : 0);
    const uint32_t t = re - 1;
    if ((L & 1u) && !(t >= fs && t < fs + 2)) fl |= F_TAIL;
    if (OLD) P.old |= (V.b(fs) | (V.b(fs + 1) << 8)) << 16;  // both in the frame: fs + 2 <= lenv in every branch
    P.st = st;
    P.flags |= fl;
    P.rs = l4 + sh;
    P.re = re + sh;
    P.fs = fs + sh;
    P.corr = add - sub;
    return P;
}

// fast_l4 for IPv4 with IHL 5 (l4 = 34 in view coordinates), its three protocol branches evaluated
// side by side and merged by selects: every field sits at a compile-time offset (one row_newbcast per
// dword), so a wave whose rows carry different protocols (C3 mixes TCP and UDP in most waves) runs one
// pass instead of one per protocol, and the checksum field's bytes are read at their constant offsets
// instead of through two runtime-indexed ds_bpermute round trips. Same conditions and values as
// fast_l4 (packet.hpp:773-889).
template <int R, bool OLD>
DEV RPlan fast_l4_v4(const RowHdr<R>& V, RPlan P, uint32_t lenv, uint32_t proto, uint32_t sh) {
    const bool isT = proto == 6, isU = proto == 17, isI = proto == 1;
    const uint32_t d4 = V.dw(4), d6 = V.dw(6), d7 = V.dw(7), d8 = V.dw(8);
    const uint32_t d9 = V.dw(9), d10 = V.dw(10), d11 = V.dw(11), d12 = V.dw(12);
    const uint32_t tl = bswap16(d4 & 0xFFFFu);  // total length (bytes 16-17)
    const uint32_t lu = bswap16(d9 >> 16);      // udp.length (bytes 38-39)
    const uint32_t hl = (d11 >> 18) & 0x3Cu;    // TCP data offset * 4 (byte 46, high nibble)
    const uint32_t L = isU ? lu : ((tl - 20u) & 0xFFFFu);
    // the conditions combined with non-short-circuit & so they stay selects, not branches
    const bool inl = (34u + L <= lenv) & (42u <= lenv);
    const bool ok = (isT & (53u <= lenv) & (tl >= 20u) & (L >= hl) & inl) |  // sizeof(TcpHeader) == 19
                    (isU & (lu >= 8u) & inl) | (isI & (tl >= 20u) & (L >= 8u) & inl);
    const uint32_t fs = isT ? 49u : (isU ? 40u : 36u), re = 34u + L;
    // the raw field bytes the reference zeroes (LE weights): TCP 49 (high byte of word 48) and 50
    // (low byte of word 50), each only inside the region; UDP 40-41, ICMP 36-37 (always inside: L >= 8)
    const uint32_t ft = (d12 & ((49u < re) ? 0xFF00u : 0u)) + ((d12 >> 16) & ((50u < re) ? 0xFFu : 0u));
    const uint32_t fsub = isT ? ft : ((isU ? d10 : d9) & 0xFFFFu);
    // pseudo-header (src, dst, proto, length) in the LE domain; ICMP has none
    const uint32_t ph = bswap16(proto) + bswap16(L) + (d6 >> 16) + (d7 & 0xFFFFu) + (d7 >> 16) + (d8 & 0xFFFFu);
    const uint32_t add = isI ? 0u : ph;
    // over-counted: the LE word at 32 (l4 = 2 mod 4, sh keeps the parity) and the field bytes
    const uint32_t sub = (d8 & 0xFFFFu) + fsub;
    const uint32_t t = re - 1u;
    const bool tail = (L & 1u) & ((t < fs) | (t >= fs + 2u));
    const uint32_t st = ok ? (isT ? NFCS_ST_V4_TCP : (isU ? NFCS_ST_V4_UDP : NFCS_ST_V4_ICMP)) : NFCS_ST_V4_L4SKIP;
    P.st = (isT | isU | isI) ? st : P.st;
    P.flags |= ok ? (F_L4 | (isU ? F_UDP : 0u) | (tail ? F_TAIL : 0u)) : 0u;
    P.rs = ok ? 34u + sh : P.rs;
    P.re = ok ? re + sh : P.re;
    P.fs = ok ? fs + sh : P.fs;
    P.corr = ok ? add - sub : P.corr;
    // the field's two bytes as they are (TCP: 49-50, bits 8-23 of dword 12; UDP 40-41; ICMP 36-37)
    if (OLD) P.old |= (isT ? (d12 >> 8) : (isU ? d10 : d9)) << 16;
    return P;
}

// Common headers with compile-time offsets: untagged / 802.1Q; IPv4 with IHL 5; IPv6; non-IP.
// Returns F_SEQ in flags for everything else (IHL != 5: options, IHL < 5, past the frame).
template <int R, bool OLD>
DEV RPlan fast_plan(const uint4& c0, uint32_t rowbase4, uint32_t len) {
    const RowHdr<R> h{c0, rowbase4};
    const bool tagged = (len >= 14) && h.be16(12) == 0x8100u;  // ethernet(): l2 = 18
    const uint32_t sh = tagged ? 4u : 0u;
    const RowHdr<R> V{strip_tag(c0, tagged), rowbase4};
    const uint32_t lenv = len - sh;  // len >= 14 whenever tagged
    const uint32_t b0 = V.b(14);
    if (len >= 14 + sh && lenv >= 34 && (b0 >> 4) == 4) {  // 728-734: IPv4 by nibble
        if ((b0 & 15u) != 5) return rplan_none(NFCS_ST_NONE | (F_SEQ << 8));
        uint32_t s = 0;  // 739-740: header checksum, field zeroed
#pragma unroll
        for (uint32_t w = 0; w < 20; w += 2)
            if (w != 10) s += V.le16(14 + w);
        RPlan P = rplan_none(NFCS_ST_V4);
        P.flags = F_IP;
        P.ipw = (24u + sh) | (((~fold32(s)) & 0xFFFFu) << 16);
        if (OLD) P.old = V.le16(24);
        return fast_l4_v4<R, OLD>(V, P, lenv, V.b(23), sh);
    }
    // 741-765: effective EtherType (after one tag) must be IPv6 and the nibble 6
    const uint32_t et = (len >= 14 + sh) ? V.be16(12) : 0u;
    if (et != 0x86DDu || !(len >= 14 + sh && lenv >= 54 && (b0 >> 4) == 6))
        return rplan_none(NFCS_ST_NONE);
    return fast_l4<R, OLD>(V, rplan_none(NFCS_ST_V6), lenv, 0u, 54u, V.b(20), sh);
}

// Any header, parsed by one lane from global memory (IP options, IHL < 5, past the frame).
__device__ __noinline__ RPlan slow_plan(const uint8_t* f, uint32_t len) {
    uint32_t l2 = 14;
    if (len >= 14) l2 = (g_be16(f, 12) == 0x8100u) ? 18u : 14u;
    RPlan P = rplan_none(NFCS_ST_NONE);
    uint32_t v4 = 0, proto, ihl4 = 0, l4;
    if (l2 + 20 <= len && (f[l2] >> 4) == 4) {
        v4 = 1;
        proto = f[l2 + 9];
        ihl4 = (f[l2] & 15u) * 4u;
        l4 = l2 + ihl4;
        if (l2 + ihl4 > len) return rplan_none(NFCS_ST_OOB);
        if (ihl4 < 20 && (proto == 6 || proto == 17 || proto == 1)) {
            P.flags = F_SEQ;  // overlapping headers: full sequential emulation
            return P;
        }
        uint32_t s = 0;
        for (uint32_t w = 0; w < ihl4; w += 2)
            if (w != 10) s += g_be16(f, l2 + w);
        P.st = NFCS_ST_V4;
        P.flags = F_IP;
        P.ipw = (l2 + 10) | (bswap16(g_fin(s)) << 16);
    } else {
        uint32_t et = (len >= 14) ? g_be16(f, 12) : 0;
        if (et == 0x8100u) et = (len >= 18) ? g_be16(f, 16) : 0;
        if (et != 0x86DDu || !(l2 + 40 <= len && (f[l2] >> 4) == 6)) return P;
        proto = f[l2 + 6];
        l4 = l2 + 40;
        P.st = NFCS_ST_V6;
    }
    const uint32_t skip = v4 ? NFCS_ST_V4_L4SKIP : NFCS_ST_V6_L4SKIP;
    uint32_t L, fs, st, fl = F_L4;
    if (proto == 6) {
        if (l4 + 19 > len) { P.st = skip; return P; }
        const uint32_t hl = (f[l4 + 12] >> 4) * 4u;
        if (v4) {
            const uint32_t tl = g_be16(f, l2 + 2);
            if (tl < ihl4) { P.st = skip; return P; }
            L = (tl - ihl4) & 0xFFFFu;
        } else {
            L = g_be16(f, l2 + 4);
        }
        if (L < hl || l4 + L > len) { P.st = skip; return P; }
        fs = l4 + 15;
        st = v4 ? NFCS_ST_V4_TCP : NFCS_ST_V6_TCP;
    } else if (proto == 17) {
        if (l4 + 8 > len) { P.st = skip; return P; }
        L = g_be16(f, l4 + 4);
        if (L < 8 || l4 + L > len) { P.st = skip; return P; }
        fs = l4 + 6;
        fl |= F_UDP;
        st = v4 ? NFCS_ST_V4_UDP : NFCS_ST_V6_UDP;
    } else if (proto == 1 && v4) {
        if (l4 + 8 > len) { P.st = skip; return P; }
        const uint32_t tl = g_be16(f, l2 + 2);
        if (tl < ihl4) { P.st = skip; return P; }
        L = tl - ihl4;
        if (l4 + L > len || L < 8) { P.st = skip; return P; }
        fs = l4 + 2;
        st = NFCS_ST_V4_ICMP;
    } else {
        return P;
    }
    uint32_t add = 0;
    if (proto != 1) {
        add = bswap16(proto) + bswap16(L);
        const uint32_t a0 = v4 ? l2 + 12 : l2 + 8, an = v4 ? 8u : 32u;
        for (uint32_t w = 0; w < an; w += 2) add += bswap16(g_be16(f, a0 + w));
    }
    const uint32_t re = l4 + L;
    uint32_t sub = (l4 & 2u) ? bswap16(g_be16(f, l4 - 2)) : 0u;
    if (fs < re) sub += (uint32_t)f[fs] << ((fs & 1u) ? 8 : 0);
    if (fs + 1 < re) sub += (uint32_t)f[fs + 1] << (((fs + 1) & 1u) ? 8 : 0);
    const uint32_t t = re - 1;
    if ((L & 1u) && !(t >= fs && t < fs + 2)) fl |= F_TAIL;
    P.st = st;
    P.flags |= fl;
    P.rs = l4;
    P.re = re;
    P.fs = fs;
    P.corr = add - sub;
    return P;
}

// Masked add of one boundary chunk at frame offset o: dwords from lo4 up to byte re, plus the
// odd-tail fix.
DEV uint32_t masked_chunk(const uint4& v, uint32_t o, uint32_t lo4, uint32_t re, uint32_t tailfix,
                          uint32_t acc) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t od = o + 4u * j;
        const int nb = (int)re - (int)od;
        uint32_t m = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
        m = (od >= lo4) ? m : 0u;
        acc = wsum(comp(v, j) & m, acc);
    }
    const uint32_t t = re - 1;
    if (tailfix && t >= o && t < o + 16) acc += 255u * ((comp(v, (t - o) >> 2) >> (8 * (t & 3u))) & 0xFFu);
    return acc;
}

DEV void acc_slot(uint32_t& acc, const uint4& v, uint32_t c, uint32_t lo4, uint32_t re, uint32_t tailfix) {
    const uint32_t o = c * 16u;
    const bool full = (o >= lo4) && (o + 16u <= re);
    const bool part = !full && (o + 16u > lo4) && (o < re);
    if (full) acc = add_chunk(v, acc);
    if (part) acc = masked_chunk(v, o, lo4, re, tailfix, acc);
}

template <int R>
DEV uint32_t row_sum(uint32_t x) {  // every lane of an R-lane row gets the row's sum
    x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true);   // quad_perm 1,0,3,2
    x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true);   // quad_perm 2,3,0,1
    x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xF, 0xF, true);  // row_half_mirror
    if (R == 16) x += (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xF, 0xF, true);  // row_mirror
    return x;
}

template <int R>
DEV uint32_t wave_max_rows(uint32_t x) {  // x row-uniform
    uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)x, 0);
#pragma unroll
    for (int l = R; l < 64; l += R) m = max(m, (uint32_t)__builtin_amdgcn_readlane((int)x, l));
    return m;
}

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
constexpr int kCpolNt = 2;  // buffer-load cache policy bits: nt (the global loads' non-temporal hint)

template <int NT>
DEV uint4 ld16(const uint4* p) {
    if (NT) {
        const u32x4_t t = __builtin_nontemporal_load((const u32x4_t*)p);
        return make_uint4(t.x, t.y, t.z, t.w);
    }
    return *p;
}

// Frame stores. WT: write-through at agent scope (`sc1`): the L2 keeps no dirty copy of the
// frame's line, so the line leaves as a clean eviction and the write goes to memory at once
// instead of as a later write-back in the middle of the read stream (session 3: C1 +2.5%,
// C3 +5% over plain stores; `sc0 sc1` measured the same, `sc0 sc1 nt` 5% worse).

template <bool WT>
DEV void st8(uint8_t* p, uint32_t b) {
    if (WT) __hip_atomic_store(p, (uint8_t)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = (uint8_t)b;
}
// A byte store that goes to memory past the caches (`sc0 sc1 nt`: system scope, non-temporal).
DEV void st8_nt(uint8_t* p, uint32_t b) {
    asm volatile("global_store_byte %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(b) : "memory");
}
// The same for 16 bytes (the s_nop: see st16 below).
DEV void st16_nt(uint4* p, const uint4& v) {
    const u32x4_t t = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt\n\ts_nop 1" ::"v"(p), "v"(t) : "memory");
}
template <bool WT>
DEV void st16(uint4* p, const uint4& v) {
    if (WT) {
        // One dwordx4 sc1 store. The s_nop covers the gfx9 hazard of a VALU write to the data
        // VGPRs of a store wider than 8 bytes right after it, which hipcc's hazard recognizer
        // does not see inside inline asm (without it the VLAN kernel stored clobbered dwords).
        // Two 8-byte atomic sc1 stores instead cost 37% on VLAN C1.
        const u32x4_t t = {v.x, v.y, v.z, v.w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(t) : "memory");
    } else {
        *p = v;
    }
}

// Descriptors of the wave's four rows: packets w, w+1, w+2, w+3 are consecutive in the
// descriptor array, so one wave-uniform scalar load (s_load_dwordx8) fetches all four; each
// lane picks its row's pair. Counted on lgkmcnt, so prefetching them never holds up a vmcnt
// wait for chunk data.
template <int P>  // packets per wave
struct DescW { uint32_t w[2 * P]; };

template <int P>
DEV DescW<P> load_descw(const nfcs_desc* __restrict__ desc, uint64_t pw, uint32_t n) {
    DescW<P> D;
    if (pw + P <= n) {
        const uint32_t* q = (const uint32_t*)(desc + pw);
#pragma unroll
        for (int i = 0; i < 2 * P; ++i) D.w[i] = q[i];
    } else {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const bool ok = pw + i < n;
            D.w[2 * i] = ok ? desc[pw + i].off16 : 0u;
            D.w[2 * i + 1] = ok ? desc[pw + i].len : 0u;
        }
    }
    return D;
}

template <int P>
DEV nfcs_desc pick_desc(const DescW<P>& D, uint32_t row) {  // mask selects: no indexable temp
    nfcs_desc d;
    d.off16 = 0;
    d.len = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const uint32_t m = 0u - (uint32_t)(row == (uint32_t)i);
        d.off16 |= D.w[2 * i] & m;
        d.len |= D.w[2 * i + 1] & m;
    }
    return d;
}

// The wave's frames as one raw buffer resource (round 4): based at the lowest frame of the wave's
// rows (wave-uniform, from the descriptors in SGPRs), so a lane past its frame (or, in a line-aligned
// window, before it) gives an out-of-range offset and its load returns zeros with no memory request.
// With every such lane aimed at one shared zero chunk instead, up to half the load requests of a
// short-frame batch went to a single 16-byte address, and C3 moved by 3% with the link-time address
// of that chunk (profiles/r04_s2_zero_target_ab.jsonl). Used where it measured faster (rows_body's
// BUF: the plain update's short shape). ok = every row's frame starts within
// kBufSpan16 16-byte units of the base (32-bit offsets, a 64 KB frame on top); else row_stage loads
// through global addresses, lanes past the frame from the wave's zero chunk.
struct WaveBuf {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t lo16;
    bool ok;
};
constexpr uint32_t kBufSpan16 = (1u << 28) - (1u << 13);
constexpr uint32_t kBufOob = 0xFFFFFFF0u;  // num_records, and the offset of a lane past its frame

template <int P>
DEV WaveBuf wave_buf(const DescW<P>& D, uint64_t pw, uint32_t n, uint8_t* arena, uint32_t base16) {
    uint32_t lo = D.w[0], hi = D.w[0];  // row 0 is always a packet (the wave exits when pw >= n)
#pragma unroll
    for (int i = 1; i < P; ++i) {
        const uint32_t o = (pw + (uint64_t)i < n) ? D.w[2 * i] : D.w[0];
        lo = min(lo, o);
        hi = max(hi, o);
    }
    lo = rfl(lo);  // wave-uniform: a scalar branch in row_stage, not an exec-masked one
    hi = rfl(hi);
    WaveBuf b;
    b.lo16 = lo;
    b.ok = hi - lo < kBufSpan16;
    b.rs = __builtin_amdgcn_make_buffer_rsrc(arena + ((int64_t)lo - (int64_t)base16) * 16, (short)0, kBufOob,
                                             0x00020000);
    return b;
}

// One row's packet, staged: frame window and its first K slots of chunks in flight.
template <int K>
struct RowStage {
    uint4 v[K];
    uint8_t* frame;
    uint32_t len;   // 0 unless live
    uint32_t p;
    uint32_t valid, bad;
    uint32_t nh;    // fused L3 forward: next-hop index (row-uniform)
    uint32_t mis;   // 16-byte chunks between the frame start and the 128-byte line below it
};

// Per-launch extras of update_rows_kernel: the fused L3 forward's inputs (unused by the plain
// update) and the footprint observation slot (sample_footprint; null = none).
struct FwdArgs {
    const uint32_t* nh;
    const nfcs_nexthop* table;
    uint32_t table_n;
    ObsReq obs;
    DoneReq done = {};
    DemandReq dem = {};
};

// DoneReq (nfcs_internal.h): every wave releases its own frame / record / status stores at system scope
// (each wave's fence waits for that wave's stores; one lane's fence would not cover the other waves'
// stores still in flight), the barrier then has them all; one lane counts the workgroup (a vector
// atomic), and the workgroup that completes the count publishes it with a system-scope release store
// (a vector store), which the host's acquire load of the flag pairs with. Waves that had no packets reach
// the barrier too (update_rows_kernel returns early only without a DoneReq).
DEV void signal_done(const DoneReq& d, uint32_t nblocks) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t now = __hip_atomic_fetch_add(d.ctr, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1ull;
        if (now == d.base + nblocks) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            __hip_atomic_store(d.flag, now, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The footprint of a call's frames — 256 descriptors spread evenly over the call's tag & 0xFFFFFFFF
// packets from desc (the whole call, also when it runs as sub-batches: the first sub-batch samples):
// the mean of their lengths rounded up to 128 bytes, how many of the 256 are longer than one 8-lane row
// pass (kTinyRowBytes), whether many start off a 128-byte line (kObsUnaligned), whether their rounded
// lengths vary (kObsMixed) and how many lie between minimum and full size (kObsMidShift) — written to
// *obs (host-mapped, system scope) by one wave of the launch, in one 64-bit store together with the
// burst's generation (tag >> 32), so the host can tell a late sample of an earlier burst from this
// one's: kObsPresent | bits | longs << kObsLongShift | mean (nfcs_internal.h). The
// next call over the same burst (descriptor array, n and arena_bytes) picks its launch shape from it
// when arena_bytes / n cannot tell (a burst inside a larger ring; a densely packed mix whose mean
// alone says 8-lane rows; nfcs_api.hip launch_shape). Speed only.
DEV void sample_footprint(const nfcs_desc* __restrict__ desc, uint64_t tag, uint32_t lane, uint64_t* obs) {
    const uint32_t n = (uint32_t)tag;
    uint32_t s = 0, c = 0, u = 0, md = 0, lo = 0xFFFFFFFFu, hi = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const nfcs_desc d = desc[(uint32_t)(((uint64_t)(4u * lane + k) * n) >> 8)];
        const uint32_t r = ((d.len < 0xFFFFu ? d.len : 0xFFFFu) + 127u) & ~127u;
        s += r;
        c += d.len > kTinyRowBytes ? 1u : 0u;
        u += (d.off16 & 7u) ? 1u : 0u;
        md += (r > 128u && r <= 1408u) ? 1u : 0u;
        lo = min(lo, r);
        hi = max(hi, r);
    }
    s = row_sum<16>(s);
    c = row_sum<16>(c);
    u = row_sum<16>(u);
    md = row_sum<16>(md);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {  // wave min / max of the rounded lengths (one wave, once per launch)
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, m));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, m));
    }
    auto wave_total = [](uint32_t v) {
        return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
               (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    };
    const uint32_t t = wave_total(s), l = wave_total(c), un = wave_total(u), mid = wave_total(md) >> 5;
    const uint32_t bits = (un > kObsUnalignedMax ? kObsUnaligned : 0u) | (hi - lo > 128u ? kObsMixed : 0u) |
                          ((mid < 7u ? mid : 7u) << kObsMidShift);
    if (lane == 0)
        __hip_atomic_store(obs, (tag & 0xFFFFFFFF00000000ull) | kObsPresent | bits | (l << kObsLongShift) | (t >> 8),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The previous call's store demand, forwarded by one wave of this call (DemandReq): each lane reads and
// clears one of the 64 words (that call has finished: calls on one stream run in order), and lane 0
// writes their total with that call's generation to the host-mapped word in one 64-bit store, as
// sample_footprint does. Speed only (the next calls' form, nfcs_store_policy.h).
DEV void forward_demand(const DemandReq& d, uint32_t lane) {
    static_assert(kDemandWords == 64, "one word per lane");
    uint32_t* w = d.prev + lane * kDemandStrideWords;
    uint32_t v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = row_sum<16>(v);
    v = (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
        (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    if (lane == 0)
        __hip_atomic_store(d.host, ((uint64_t)d.prev_gen << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Issue the row's K chunk loads: the header slot with the default cache policy (its lines are
// parsed and, with inline stores, written back while still in L2), payload slots non-temporal
// (evict-first). Every load is always issued — lanes past the frame read zeros: from g_zero_line, or
// in the BUF shape (the update's short shape) through an out-of-range buffer offset with no memory
// request (WaveBuf; g_zero_line again where a wave's frames span more than 4 GB) — so the waits are
// counted vmcnt waits. Line-aligned windows (LA, round 3): lane rl of slot k holds the chunk
// R*k + rl past the 128-byte line in which the frame starts, i.e. frame chunk R*k + rl - mis, so
// each load instruction covers whole lines (2 for 16-lane rows, 1 for 8-lane rows) whatever the
// frame's alignment; lanes before the frame start or past its end read zeros. Frame-relative
// windows on a frame that starts mid-line make every instruction touch one line more (densely
// packed frames: C1 -4.5%, C2 -8%, C3 -15%; 64-byte-aligned starts C1 -5%;
// profiles/r03_s3_ab_align*.jsonl). Without LA, mis = 0 and the windows are frame-relative.
template <int K, int R = 16, bool FWD = false, bool LA = false, bool BUF = false>
DEV void row_stage(RowStage<K>& S, uint8_t* arena, uint64_t arena_bytes, const nfcs_desc& d,
                   uint64_t p64, uint32_t n, uint32_t base16, uint32_t rl, const WaveBuf& wb, uint32_t nh = 0) {
    const bool valid = p64 < n;
    const uint64_t off = ((uint64_t)d.off16 - base16) * 16u;
    const bool bad = valid && ((d.off16 < base16) ||
                               (off + (((uint64_t)d.len + 15u) & ~15ull) > arena_bytes));
    const bool live = valid && !bad;
    S.valid = valid;
    S.bad = bad;
    S.p = (uint32_t)p64;
    S.len = live ? d.len : 0u;
    S.frame = arena + (live ? off : 0);
    S.mis = LA && live ? (uint32_t)(((uintptr_t)S.frame >> 4) & 7u) : 0u;
    const uint32_t nch = (S.len + 15u) >> 4;
    const uint4* src = (const uint4*)S.frame;
    if (FWD) S.nh = nh;  // its MACs arrive as wave-uniform scalars (update_rows_kernel)
    if (BUF && wb.ok) {  // wave-uniform
        const uint32_t rel = (d.off16 - wb.lo16) * 16u;  // the row's frame in the wave's buffer
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t c = rl + (uint32_t)R * k - S.mis;  // frame chunk (wraps below the frame start)
            const uint32_t vo = (c < nch) ? rel + 16u * c : kBufOob;
            const u32x4_t t = k == 0 ? __builtin_amdgcn_raw_buffer_load_b128(wb.rs, vo, 0, 0)
                                     : __builtin_amdgcn_raw_buffer_load_b128(wb.rs, vo, 0, kCpolNt);
            S.v[k] = make_uint4(t.x, t.y, t.z, t.w);
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t c = rl + (uint32_t)R * k - S.mis;
            const uint4* a = (c < nch) ? src + c : g_zero_line;
            S.v[k] = k == 0 ? ld16<0>(a) : ld16<1>(a);
        }
    }
    // all K loads issue before any use of the header slot: without this fence the scheduler
    // hoists the forward decision's first DPP read above the last loads of the FWD kernel and
    // waits for the header line (vmcnt) with half the row's loads not yet issued
    if (FWD) __builtin_amdgcn_sched_barrier(0);
}

// How update_rows_kernel's checksum bytes reach the frames:
//   SF_INLINE   the row's lanes 0-3 store the 2+2 bytes as soon as they are known, write-through
//               (sc1) or, in the short-frame shape, past the caches (sc0 sc1 nt): one 64-byte
//               write request per packet inside the read stream;
//   SF_DEFER    per wave, from its four descriptor lengths (SGPRs): a wave whose frames average
//               at least kDeferMeanBytes writes 8-byte patch records instead, and
//               apply_bytes_kernel writes them after the read pass with non-temporal stores (the
//               writes then reach HBM in a write-only pass instead of interleaving with, or being
//               evicted from the memory-side cache into, the read stream); other waves as SF_INLINE;
//   SF_RECORDS  patch records only, frames untouched (nfcs_update_host: only the records cross
//               PCIe back).
// In the plain update's fast path a field whose bytes already equal the computed value is not stored
// (SF_INLINE) and is recorded as "none" in the engine's own workspace (SF_DEFER, so the write pass issues
// nothing for it); a caller's records (SF_RECORDS, SF_DEFER into d_patch) hold every field (row_process).
// Round 4 measured, under rotating batches, forms storing each frame's first 64 bytes whole (from
// the read pass, or from 64-byte records through a write pass) and write passes of write-back /
// write-through stores: all slower than SF_DEFER's masked `nt` stores (their code is
// in git 2288ac5, tools/r04/fresh_exp.hip variants 4-8, 11-13, 30-34).
enum : int { SF_INLINE = 0, SF_DEFER = 1, SF_RECORDS = 2 };
// The fused forward's deferred record (large bursts, SF_DEFER; the write pass apply_fwd_kernel is
// its only reader), 8 bytes for a forwarded frame with a common header, all offsets below 64:
//   x = ip_off | ttl' << 8 | proto << 16 | l4_off << 24, y = ip checksum bytes | l4 checksum bytes << 16
// ip_off 0xFE: forwarded without an IPv4 checksum field (EtherType IPv4, version nibble != 4:
// update_checksums() is a no-op), the TTL offset then in y's low byte; l4_off 0xFF: no L4 field;
// x = 0xFFFFFFFF: nothing for the write pass (not forwarded, or written by the read pass's cold path).
constexpr uint32_t kFwdNoIp = 0xFEu, kFwdNone = 0xFFu;
DEV uint2 fwd_record(uint32_t ipw, uint32_t l4w, uint32_t ttl_new, uint32_t proto, bool tagged) {
    const bool ip = (ipw & 0xFFFFu) != NFCS_PATCH_NONE, l4 = (l4w & 0xFFFFu) != NFCS_PATCH_NONE;
    const uint32_t ipo = ip ? (ipw & 0xFFu) : kFwdNoIp, l4o = l4 ? (l4w & 0xFFu) : kFwdNone;
    const uint32_t y = (ip ? (ipw >> 16) : (tagged ? 26u : 22u)) | (l4w & 0xFFFF0000u);
    return make_uint2(ipo | ((ttl_new & 0xFFu) << 8) | ((proto & 0xFFu) << 16) | (l4o << 24), y);
}

// SF_DEFER's decision for the P packets pw .. pw+P-1 (lengths 0 past n), shared by the read pass
// and apply_bytes_kernel so both pick the same waves.
DEV bool defer_group(uint32_t lensum, uint32_t P) { return lensum >= P * (uint32_t)kDeferMeanBytes; }
DEV uint32_t defer_len(uint32_t len) { return len < 0xFFFFu ? len : 0xFFFFu; }

// Frame chunk rl (rl < R) of the row's packet from its line-aligned slots 0 and 1: the header
// view the plan, the forward's rewrite and its segment stores work on (lane rl + mis of the row).
template <int K, int R>
DEV uint4 hdr_view(const RowStage<K>& S, uint32_t rowbase4, uint32_t rl) {
    const uint32_t a = rl + S.mis;
    const int sl = (int)(rowbase4 + (a & (R - 1)) * 4u);
    const uint4 v0 = S.v[0], v1 = S.v[1];
    const uint4 r0 = make_uint4((uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v0.x),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v0.y),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v0.z),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v0.w));
    const uint4 r1 = make_uint4((uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v1.x),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v1.y),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v1.z),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v1.w));
    return a < (uint32_t)R ? r0 : r1;
}

// (Round 4's measurement-only knobs — uncommon-header rows deferred to a later pass, fewer
// continuation slots — were measured, not adopted, and dropped from the product; tools/r04/fresh_exp.hip
// builds against the round-4 sources, git 00f5686.)
template <int K, int R = 16, bool FWD = false, bool NT = false, bool DFR = false, bool LA = false>
DEV void row_process(const RowStage<K>& S, uint32_t rl, uint32_t rowbase4, uint8_t* status,
                     nfcs_patch* rec, bool rec_full, bool frame_stores, uint32_t table_n = 0,
                     const uint32_t* wmac = nullptr, const nfcs_nexthop* table = nullptr,
                     uint32_t* demand = nullptr) {
    const uint32_t len = S.len;
    uint8_t* frame = S.frame;
    const uint4* src = (const uint4*)frame;
    const bool live = S.valid && !S.bad;
    static_assert(K >= 2, "the header view reads slots 0 and 1");
    // frame chunk rl in lane rl: slot 0 itself when every row of the wave starts on a line
    uint4 h0 = S.v[0];
    if (LA && __builtin_amdgcn_ballot_w64(S.mis != 0) != 0) h0 = hdr_view<K, R>(S, rowbase4, rl);
    // Fused L3 forward (switch.hpp:247-294): the decision, then the TTL decrement and MAC
    // rewrite applied to the header registers, so the checksums below see the new header.
    bool fwd = false, tagged = false;
    uint32_t fst = NFCS_ST_NONE, ttl = 0, proto = 0;
    if (FWD) {
        const RowHdr<R> h{h0, rowbase4};
        const uint32_t e12 = h.be16(12);
        tagged = e12 == 0x8100u;  // ethernet() l2 = 18 (packet.hpp:410)
        const uint32_t l3t = len < 14 ? 0u : (tagged ? (len >= 18 ? h.be16(16) : e12) : e12);
        const bool v4 = l3t == 0x0800u && (tagged ? 38u : 34u) <= len;  // ipv4() present
        ttl = tagged ? h.b(26) : h.b(22);
        if (DFR) proto = tagged ? h.b(27) : h.b(23);  // the byte beside the TTL (the write pass's TTL short)
        fst = !v4 ? (uint32_t)NFCS_ST_NOT_IPV4
                  : (ttl <= 1 ? (uint32_t)NFCS_ST_TTL_EXPIRED
                              : (S.nh >= table_n ? (uint32_t)NFCS_ST_NO_ROUTE : 0u));
        fwd = live && fst == 0;
        if (fwd && rl == 0 && (!DFR || frame_stores)) {  // dst_mac, src_mac (286-289): the row's pick of the wave's MACs
            constexpr uint32_t PW = 64 / R;
            const uint32_t row = rowbase4 / (4u * R);
            uint32_t m0 = 0, m1 = 0, m2 = 0;
#pragma unroll
            for (uint32_t i = 0; i < PW; ++i) {
                m0 = (row == i) ? wmac[3 * i] : m0;
                m1 = (row == i) ? wmac[3 * i + 1] : m1;
                m2 = (row == i) ? wmac[3 * i + 2] : m2;
            }
            h0.x = m0;
            h0.y = m1;
            h0.z = m2;
        }
        if (fwd && rl == 1) {  // ttl-- (279): byte 22 (dword 1) or 26 (dword 2), never borrows
            if (tagged) h0.z -= 1u << 16;
            else h0.y -= 1u << 16;
        }
    }
    RPlan P = fast_plan<R, !FWD>(h0, rowbase4, len);
    const bool act = live && (!FWD || fwd);  // rows whose checksums are updated
    // uncommon headers (IP options, IHL < 5, IHL past the frame) take the cold path below,
    // after the chunk registers are dead, so it adds nothing to the kernel's register peak
    const bool slow = act && (P.st >> 8) != 0;
    if (!act || slow)
        P = rplan_none(S.bad ? (uint32_t)NFCS_ST_BAD_DESC
                             : (FWD && live && !fwd) ? fst : (uint32_t)NFCS_ST_NONE);
    const uint32_t st = P.st | ((FWD && fwd) ? (uint32_t)NFCS_ST_FLAG_FWD : 0u);
    const uint32_t ipw = (P.flags & F_IP) ? P.ipw : NFCS_PATCH_NONE;
    uint32_t l4w = NFCS_PATCH_NONE;
    // Region sums without per-slot boundary branches (rows without an L4 region add nothing):
    // chunks below nre are added whole (the region starts below byte 80, in the header view h0,
    // where dwords under lo4 are masked); the last chunk's bytes past re and the odd trailing byte
    // are corrected once per row by the lane that holds it. The header view stands for slot 0:
    // it holds frame chunks 0..R-1 in lanes 0..R-1, so slot 0's own lanes (frame chunks below
    // R - mis) are never summed and slot 1 adds only its chunks from R on; lane rl of slot k >= 1
    // holds frame chunk R*k + rl - mis (row_stage). Frames longer than one batch leave
    // their end to the masked continuation below. rlv is opaque so the per-slot offsets are
    // recomputed rather than hoisted into ~35 long-lived VGPRs.
    const uint32_t re = (P.flags & F_L4) ? P.re : 0u, lo4 = P.rs & ~3u;
    const uint32_t tailfix = P.flags & F_TAIL;
    uint32_t rlv = rl;
    asm volatile("" : "+v"(rlv));
    uint32_t acc = 0;
    const uint32_t nre = (re + 15u) >> 4;
    {
        // la: the last chunk's place in the slots (lane la % R of slot la / R; slot 0 = h0)
        const uint32_t last = nre - 1u, la = (!LA || last < (uint32_t)R) ? last : last + S.mis;
        const uint32_t own = (re != 0) && (la < (uint32_t)R * K) && ((la & (R - 1)) == rl);
        uint4 lc = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint4 v = k == 0 ? h0 : S.v[k];
            const uint32_t c = k == 0 ? rlv : rlv + (uint32_t)R * k - S.mis;
            const uint32_t m = (c < nre && (!LA || k != 1 || c >= (uint32_t)R)) ? 0xFFFFFFFFu : 0u;
            if (k == 0) {
                const uint32_t o = 16u * c;
                acc = wsum(v.x & m & ((o >= lo4) ? 0xFFFFFFFFu : 0u), acc);
                acc = wsum(v.y & m & ((o + 4u >= lo4) ? 0xFFFFFFFFu : 0u), acc);
                acc = wsum(v.z & m & ((o + 8u >= lo4) ? 0xFFFFFFFFu : 0u), acc);
                acc = wsum(v.w & m & ((o + 12u >= lo4) ? 0xFFFFFFFFu : 0u), acc);
            } else {
                acc = wsum(v.w & m, wsum(v.z & m, wsum(v.y & m, wsum(v.x & m, acc))));
            }
            const bool sel = (la >> (R == 16 ? 4 : 3)) == (uint32_t)k;
            lc.x = sel ? v.x : lc.x;
            lc.y = sel ? v.y : lc.y;
            lc.z = sel ? v.z : lc.z;
            lc.w = sel ? v.w : lc.w;
        }
        if (own) {
            // the chunk's bytes at or past re come off again: dword j keeps its low
            // clamp(8 (re - o) - 32 j, 0, 32) bits (one 64-bit shift each). Bytes under lo4 of a one-chunk
            // region were never added, and none of them lies at or past re (re >= rs >= lo4).
            const uint32_t o = 16u * last, kb8 = 8u * (re - o);
            uint32_t ex = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const int s = min(max((int)kb8 - 32 * (int)j, 0), 32);
                ex = wsum(comp(lc, j) & (uint32_t)(~0ull << s), ex);
            }
            acc -= ex;
            const uint32_t t = re - 1u - o, q = t >> 2;
            const uint32_t dt = q == 0 ? lc.x : (q == 1 ? lc.y : (q == 2 ? lc.z : lc.w));
            if (tailfix) acc += 255u * ((dt >> (8 * (t & 3u))) & 0xFFu);
        }
    }
    // continuation batches for frames longer than R*K chunks (jumbo)
    const uint32_t cmax = wave_max_rows<R>(LA ? nre + S.mis : nre);
    for (uint32_t cb = (uint32_t)R * K; cb < cmax; cb += (uint32_t)R * K) {
        uint4 w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t c = cb + rlv + (uint32_t)R * k - S.mis;
            w[k] = ld16<1>((c < nre) ? src + c : g_zero_line);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc_slot(acc, w[k], cb + rlv + (uint32_t)R * k - S.mis, lo4, re, tailfix);
    }
    const uint32_t z = row_sum<R>(acc) + P.corr;
    if (P.flags & F_L4) {
        uint32_t c = (~fold32(z)) & 0xFFFFu;  // LE-domain complement = bswap of ref value
        if ((P.flags & F_UDP) && c == 0) c = 0xFFFFu;  // 867-871
        l4w = P.fs | (c << 16);
    }
    // Store skipping (the plain update's fast path): a field whose two bytes in the frame already equal
    // the computed value is not written — memory is the same either way, and received traffic or an
    // L2-only edit leaves most fields so. The plan read the old bytes with the header (P.old, in the
    // same view), so the comparison is two VALU instructions per field and exact: 0x0000 and 0xFFFF
    // differ. sipw / sl4w are what the frame still needs (an unchanged field becomes "none"): the inline
    // stores and the engine's own deferred records follow these; a caller's records keep every field.
    const bool ip_new = FWD || (P.old & 0xFFFFu) != (ipw >> 16), l4_new = FWD || (P.old >> 16) != (l4w >> 16);
    const uint32_t sipw = ip_new ? ipw : (uint32_t)NFCS_PATCH_NONE;
    const uint32_t sl4w = l4_new ? l4w : (uint32_t)NFCS_PATCH_NONE;
    // The (at most 4) checksum bytes from lanes 0..3 of the row, write-through (sc1: the L2
    // keeps no dirty copy of the header line; session 3, C1 +2.5% / C3 +5% over write-back
    // stores; byte stores measured fastest against chunk, dword, whole-line and re-load-then-
    // store forms) or, with NT (the short-frame shape), past the caches (`sc0 sc1 nt`: round 2
    // session 3, C3 +2%, uniform 1024-byte frames +2.7%; in the long shape it cost 64K-packet
    // bursts of 9000-byte frames 3%, in 8-lane rows IMIX ±1%), then the status byte / patch
    // record from lane 0.
    // ipw_ / l4w_: the fields as computed; sip_ / sl4_: those of them the frame still needs
    auto emit = [&](bool on, uint32_t st_, uint32_t ipw_, uint32_t l4w_, uint32_t sip_, uint32_t sl4_, bool stores,
                    bool recw = true) {
        if (stores && on && rl < 4) {
            const uint32_t w = (rl & 2u) ? sl4_ : sip_;
            const uint32_t pos = (w & 0xFFFFu) + (rl & 1u);
            if ((w & 0xFFFFu) != NFCS_PATCH_NONE) {
                if (NT) st8_nt(frame + pos, w >> (16 + 8 * (rl & 1u)));
                else st8<true>(frame + pos, w >> (16 + 8 * (rl & 1u)));
            }
        }
        if (on && rl == 0) {
            if (status) status[S.p] = (uint8_t)st_;
            if (rec && recw) {
                const uint32_t ri = rec_full ? ipw_ : sip_, rl4 = rec_full ? l4w_ : sl4_;
                uint2 r;
                r.x = (ri & 0xFFFFu) | (rl4 << 16);
                r.y = (ri >> 16) | (rl4 & 0xFFFF0000u);
                ((uint2*)rec)[S.p] = r;
            }
        }
    };
    if (FWD) {
        // The fused forward's segment store: one write-through segment per forwarded packet.
        // Lanes 0..c store chunks 0..c of the header (c = the last chunk holding a byte to
        // write) from the header registers with the checksum bytes and the forward's rewrite
        // patched in; unchanged bytes are rewritten with the values just read from them (a frame
        // never shares a 16-byte chunk with another frame). +1.5% over a 16-byte store + byte
        // stores (session 3).
        if (S.valid && !slow && fwd) {
            // IPv4 field first, then L4, as the reference writes them
            const uint4 v = put_field(put_field(h0, ipw, rl), l4w, rl);
            uint32_t last = 1u;
            if ((ipw & 0xFFFFu) != NFCS_PATCH_NONE) last = max(last, ((ipw & 0xFFFFu) + 1u) >> 4);
            if ((l4w & 0xFFFFu) != NFCS_PATCH_NONE) last = max(last, ((l4w & 0xFFFFu) + 1u) >> 4);
            // the short-mix shape (8-lane rows, line-aligned windows) stores past the caches (`sc0 sc1
            // nt`, as the update's short shape does), the others write-through (`sc1`): round 5, calls
            // rotating over fresh C3-mix batches, 0.690-0.710 against 0.719-0.735 ms per call
            // (profiles/r05_fwd_var.jsonl, r05_fwd_store_ab.jsonl; the replayed measurements of rounds
            // 2-3 had seen no gain); 1M x 64-byte frames (the tiny shape) 1% slower with them
            if ((!DFR || frame_stores) && rl <= last && 16u * rl < len) {
                if (R == 8 && LA) st16_nt((uint4*)frame + rl, v);
                else st16<true>((uint4*)frame + rl, v);
            }
        }
        // a deferred wave (large bursts, SF_DEFER) leaves the frame alone here: its forward record
        // (fwd_record) goes to apply_fwd_kernel, which writes the rewritten bytes without reading
        // the frame again
        emit(S.valid && !slow, st, ipw, l4w, ipw, l4w, false, !DFR);
        if (DFR && rec && S.valid && !slow && rl == 0)
            ((uint2*)rec)[S.p] = (fwd && live) ? fwd_record(ipw, l4w, ttl - 1u, proto, tagged) : make_uint2(0xFFFFFFFFu, 0u);
    } else {
        emit(S.valid && !slow, st, ipw, l4w, sipw, sl4w, frame_stores);
        // Store demand (DemandReq; a sampled workgroup of the long shape, wave-uniform): the wave's
        // packets whose frame still needs a store, one ballot and one count, and one returnless atomic
        // from one lane only when there are any: a wave of frames that are already right issues nothing.
        if (demand) {
            const bool need = slow || (sipw & 0xFFFFu) != NFCS_PATCH_NONE || (sl4w & 0xFFFFu) != NFCS_PATCH_NONE;
            const uint32_t cnt = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(need && rl == 0));
            if (cnt != 0 && rl == 0 && rowbase4 == 0)
                (void)__hip_atomic_fetch_add(demand, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (__builtin_amdgcn_ballot_w64(slow) != 0) {  // cold path, wave-uniform branch
        // Uncommon headers, handled last so that only the frame address and length are live
        // across the calls: the row's lane 0 parses from memory (IHL < 5 overlaps run the
        // exact sequential emulation, which writes its own bytes) and the region is re-summed
        // from memory.
        if (FWD && slow && fwd) {
            // segment stores skip uncommon headers: their forward rewrite goes out here, from
            // the next-hop MACs (SGPRs) and the TTL byte in memory (the header registers are
            // dead by now, which keeps the fast path free of spills)
            if (rl == 0) {
                constexpr uint32_t PW = 64 / R;
                const uint32_t row = rowbase4 / (4u * R);
                uint32_t m[3] = {0, 0, 0};
                if (DFR && !frame_stores) {  // a deferring wave loaded no MACs: this row's, from the table
#pragma unroll
                    for (uint32_t j = 0; j < 3; ++j) m[j] = ((const uint32_t*)(table + S.nh))[j];
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < PW; ++i) {
#pragma unroll
                        for (uint32_t j = 0; j < 3; ++j) m[j] = (row == i) ? wmac[3 * i + j] : m[j];
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < 3; ++j)
                    __hip_atomic_store((uint32_t*)frame + j, m[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (rl == 1) {
                const uint32_t o = tagged ? 26u : 22u;
                st8<true>(frame + o, frame[o] - 1u);
            }
        }
        if (FWD) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // see the header stores
        RPlan Q = rplan_none(0);
        SeqOut o = {0, 0, 0, 0, 0};
        if (slow && rl == 0) {
            Q = slow_plan(frame, len);
            if (Q.flags & F_SEQ) o = seq_update(frame, len);
        }
        Q.st = row_bcast<0, R>(Q.st);
        Q.flags = row_bcast<0, R>(Q.flags);
        Q.ipw = row_bcast<0, R>(Q.ipw);
        Q.rs = row_bcast<0, R>(Q.rs);
        Q.re = row_bcast<0, R>(Q.re);
        Q.fs = row_bcast<0, R>(Q.fs);
        Q.corr = row_bcast<0, R>(Q.corr);
        const uint32_t ost = row_bcast<0, R>(o.st);
        const uint32_t oip = row_bcast<0, R>((o.ip_off & 0xFFFFu) | (o.ip_val << 16));
        const uint32_t ol4 = row_bcast<0, R>((o.l4_off & 0xFFFFu) | (o.l4_val << 16));
        const bool seq = slow && (Q.flags & F_SEQ);
        const uint32_t re2 = (slow && !seq && (Q.flags & F_L4)) ? Q.re : 0u;
        const uint32_t lo42 = Q.rs & ~3u, tf2 = Q.flags & F_TAIL;
        uint32_t acc2 = 0;
        for (uint32_t c = rl; c < ((re2 + 15u) >> 4); c += R) acc_slot(acc2, src[c], c, lo42, re2, tf2);
        const uint32_t z2 = row_sum<R>(acc2) + Q.corr;
        uint32_t st2 = Q.st, ipw2 = (Q.flags & F_IP) ? Q.ipw : NFCS_PATCH_NONE, l4w2 = NFCS_PATCH_NONE;
        if (Q.flags & F_L4) {
            uint32_t c = (~fold32(z2)) & 0xFFFFu;
            if ((Q.flags & F_UDP) && c == 0) c = 0xFFFFu;
            l4w2 = Q.fs | (c << 16);
        }
        if (seq) {
            st2 = ost | NFCS_ST_FLAG_OVERLAP;
            ipw2 = oip;
            l4w2 = ol4;
        }
        if (FWD) st2 |= NFCS_ST_FLAG_FWD;
        // the forward always stores (its header rewrite went out above)
        emit(slow, st2, ipw2, l4w2, ipw2, l4w2, !seq && (FWD || frame_stores), !(FWD && DFR));
        // the forward stored everything of an uncommon header here: nothing left for the write pass
        if (FWD && DFR && rec && slow && rl == 0) ((uint2*)rec)[S.p] = make_uint2(0xFFFFFFFFu, 0u);
    }
}

// One wave = 64/R packet rows; one workgroup per BS/R packets, as many workgroups as the batch
// needs (a grid that strides over resident workgroups measured 10-15% slower).
// XCD-aware block order (session 3): workgroups are dealt to the 8 XCDs round-robin; remapped,
// the workgroups one XCD runs take one contiguous eighth of the batch, so each XCD streams its
// own region of HBM and the descriptor lines its workgroups share stay in its L2 (a bijection on
// [0, gridDim.x); the tail beyond a multiple of 8 keeps its order). C1 +1.3%, C3 +0.5%.
// Arguments in the order a wave needs them: the first eight (14 dwords: what every wave reads
// before its frame loads, plus the footprint slot) are preloaded into SGPRs at dispatch
// (-amdgpu-kernarg-preload-count=8, netflow_amd/__init__.py), so a wave's first memory access is
// its descriptor load, with no kernel-argument round trip ahead of it; `nblocks` (= gridDim.x) is
// passed explicitly for the same reason (the grid size is a hidden argument, loaded from memory).
// The rows of one wave from their frame loads on: line-aligned windows of KL slots (LA) or
// frame-relative ones of K slots.
template <int K, int R, int BS, bool FWD, int SF, bool LA, int PW>
DEV void rows_body(const DescW<PW>& D, uint64_t pw, uint32_t n, uint8_t* arena, uint64_t arena_bytes, uint32_t base16,
                   uint32_t rl, uint32_t row, uint32_t rowbase4, bool defer, const uint32_t (&q)[PW],
                   uint8_t* status, nfcs_patch* patch, nfcs_patch* ws, const nfcs_nexthop* table, uint32_t table_n,
                   uint32_t* demand) {
    typedef const __attribute__((address_space(4))) uint32_t cu32;
    const bool frame_stores = SF == SF_INLINE || (SF == SF_DEFER && !defer);
    nfcs_patch* rec = patch ? patch : (defer ? ws : nullptr);
    RowStage<K> S;
    // buffer loads in the plain update's short shape (16-lane rows, frame-relative windows), where
    // most lanes of a wave's later slots are past their frames: C3 0.689-0.692 -> 0.664-0.669 ms per
    // call; the long shape (+0.5%), the C4 shard (+0.8%), the 8-lane tiny shape (+1.2%) and the
    // fused forward's short-mix shape (+4-10%) measured slower with them and keep global loads
    // (profiles/r04_s2_wave_buf_ab.jsonl). (The long shape's frame-relative body is never launched:
    // it runs line-aligned windows, LAM 1.)
    constexpr bool BUF = !FWD && R == 16 && !LA;
    row_stage<K, R, FWD, LA, BUF>(S, arena, arena_bytes, pick_desc<PW>(D, row), pw + row, n, base16, rl,
                                  wave_buf<PW>(D, pw, n, arena, base16), 0u);
    uint32_t wmac[3 * PW];  // the wave's next-hop MACs: scalar loads, selected per row at use
    if (FWD) {
#pragma unroll
        for (uint32_t i = 0; i < PW; ++i) S.nh |= (row == i) ? q[i] : 0u;
        // a deferring wave's MACs are written by apply_fwd_kernel (the checksums do not cover
        // them): only waves that store inline load them
        if (!(SF == SF_DEFER && defer)) {
#pragma unroll
            for (uint32_t i = 0; i < PW; ++i) {
                const cu32* m = (q[i] < table_n) ? (const cu32*)(table + q[i]) : (const cu32*)g_zero_line;
                wmac[3 * i] = m[0];
                wmac[3 * i + 1] = m[1];
                wmac[3 * i + 2] = m[2];
            }
        }
    }
    // inline checksum stores past the caches in the short-frame shape (16-lane rows, frame-relative
    // windows), write-through elsewhere (see row_process)
    row_process<K, R, FWD, !FWD && R == 16 && !LA, FWD && SF == SF_DEFER, LA>(S, rl, rowbase4, status, rec,
                                                                                 patch != nullptr, frame_stores, table_n,
                                                                                 wmac, table, demand);
}

// One wave of update_rows_kernel: its PW packets from the descriptor load on.
template <int K, int R, int BS, bool FWD, int SF, int LAM, int KL>
DEV void rows_wave(const nfcs_desc* __restrict__ desc, uint32_t n, uint8_t* __restrict__ arena, uint64_t arena_bytes,
                   uint32_t base16, const uint32_t* __restrict__ nh, uint64_t* __restrict__ obs,
                   uint8_t* __restrict__ status, nfcs_patch* __restrict__ patch, nfcs_patch* __restrict__ ws,
                   const nfcs_nexthop* __restrict__ table, uint32_t table_n, uint64_t obs_tag, uint32_t lane,
                   uint32_t rl, uint32_t row, uint32_t rowbase4, uint64_t pw, uint32_t* demand) {
    constexpr uint32_t PW = 64 / R;  // packets per wave
    if (blockIdx.x == 0 && threadIdx.x < 64 && obs) sample_footprint(desc, obs_tag, lane, obs);
    // the wave's PW descriptors: one scalar load (s_load_dwordx8 for PW = 4)
    const DescW<PW> D = load_descw<PW>(desc, pw, n);
    // the store form of each aligned group of 4 packets, from their own frame lengths (scalar
    // arithmetic on the descriptors): the whole wave with 16-lane rows, each half of the wave with
    // 8-lane rows; apply_bytes_kernel recomputes the same groups
    bool defer = false;
    if (SF == SF_DEFER) {
        static_assert(PW == 4 || PW == 8, "deferral groups of 4 packets");
        uint32_t s0 = 0, s1 = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) s0 += defer_len(D.w[2 * i + 1]);
#pragma unroll
        for (uint32_t i = 4; i < PW; ++i) s1 += defer_len(D.w[2 * i + 1]);
        defer = (PW == 8 && row >= 4) ? defer_group(s1, 4) : defer_group(s0, 4);
    }
    // Fused L3 forward: the wave's PW next-hop indexes and their table rows are wave-uniform.
    // Read through the constant address space they are scalar loads on lgkmcnt: the indexes are
    // issued with the descriptors, and everything that depends on them (the row's pick, the MAC
    // loads) comes after the frame loads are issued (row_stage's sched_barrier), so no frame load
    // waits for a next-hop round trip (as generic loads the compiler made each index a vector load
    // drained by vmcnt(0) ahead of the frame loads: four serial memory round trips per wave).
    typedef const __attribute__((address_space(4))) uint32_t cu32;
    uint32_t q[PW];
    if (FWD) {
        const cu32* nhp = (const cu32*)nh + pw;
        if (pw + PW <= n) {
#pragma unroll
            for (uint32_t i = 0; i < PW; ++i) q[i] = nhp[i];
        } else {
#pragma unroll
            for (uint32_t i = 0; i < PW; ++i) q[i] = (pw + i < n) ? nhp[i] : NFCS_NH_NONE;
        }
    }
    bool la = LAM == 1;
    if (LAM == 2) {  // any row of the wave starting mid-line (its frame address, as row_stage computes it)
        const nfcs_desc d = pick_desc<PW>(D, row);
        const uint64_t a = (uint64_t)(uintptr_t)arena + ((uint64_t)d.off16 - base16) * 16u;
        la = __builtin_amdgcn_ballot_w64(pw + row < n && d.len != 0 && ((a >> 4) & 7u) != 0) != 0;
    }
    if (la)
        rows_body<KL, R, BS, FWD, SF, true, PW>(D, pw, n, arena, arena_bytes, base16, rl, row, rowbase4, defer, q,
                                                status, patch, ws, table, table_n, demand);
    else
        rows_body<K, R, BS, FWD, SF, false, PW>(D, pw, n, arena, arena_bytes, base16, rl, row, rowbase4, defer, q,
                                                status, patch, ws, table, table_n, demand);
}

// LAM: 0 frame-relative windows of K slots; 1 line-aligned windows of KL slots; 2 per wave, line-
// aligned (KL slots) when a row of the wave starts mid-line, else frame-relative (K slots), so
// line-aligned batches run the frame-relative code unchanged.
template <int K, int R, int OCC, int BS, bool FWD, int SF, int LAM = 0, int KL = K>
__global__ __launch_bounds__(BS, OCC) void update_rows_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                              uint32_t nblocks, uint8_t* __restrict__ arena,
                                                              uint64_t arena_bytes, uint32_t base16,
                                                              const uint32_t* __restrict__ nh,
                                                              uint64_t* __restrict__ obs,
                                                              uint8_t* __restrict__ status,
                                                              nfcs_patch* __restrict__ patch,
                                                              nfcs_patch* __restrict__ ws,
                                                              const nfcs_nexthop* __restrict__ table,
                                                              uint32_t table_n, uint64_t obs_tag, DoneReq done,
                                                              DemandReq dem) {
    constexpr uint32_t PW = 64 / R;  // packets per wave
    const uint32_t lane = threadIdx.x & 63u, rl = lane & (R - 1), row = lane / R;
    const uint32_t rowbase4 = (lane & ~(uint32_t)(R - 1)) * 4u;
    const uint32_t lb = xcd_block_n(nblocks);
    const uint64_t pw = (uint64_t)lb * (BS / R) + rfl(threadIdx.x >> 6) * PW;
    // with a DoneReq (a kernel argument: uniform) waves without packets stay for signal_done's barrier
    if (pw >= n && !done.flag) return;
    // Store demand: the plain update's long shape only (its workgroups hold kDemandBlockPackets packets)
    constexpr bool DEM = !FWD && R == 16 && LAM == 1 && BS == kBlock && SF != SF_RECORDS;
    uint32_t* demand = nullptr;
    if (DEM && dem.cur) {
        static_assert(!DEM || BS / R == (int)kDemandBlockPackets, "demand_sampled_one counts 16-packet workgroups");
        if ((lb & (kDemandSampleEvery - 1u)) == 0)
            demand = dem.cur + ((lb / kDemandSampleEvery) & (kDemandWords - 1u)) * kDemandStrideWords;
        if (blockIdx.x == 0 && threadIdx.x < 64 && dem.host) forward_demand(dem, lane);
    }
    if (pw < n)
        rows_wave<K, R, BS, FWD, SF, LAM, KL>(desc, n, arena, arena_bytes, base16, nh, obs, status, patch, ws, table,
                                              table_n, obs_tag, lane, rl, row, rowbase4, pw, demand);
    if (done.flag) signal_done(done, nblocks);
}

// SF_DEFER's write pass: the patch records of the waves that deferred, written into the frames
// with ONE store request per packet, non-temporal at system scope (`sc0 sc1 nt`): the writes go to
// HBM during this write-only pass instead of lingering dirty in the memory-side cache and being
// evicted into the next read stream (4M x 1500 B shard: read pass + this pass 0.715-0.718 of 8 TB/s
// against 0.658 for the fused kernel with write-back stores; tools/wr_probe.hip).
// One thread per packet: lane l of a wave loads descriptor p0 + l (one coalesced 512-byte load)
// and, from the lengths of its aligned quad of lanes, recomputes the read pass's decision for that
// group of 4 packets, and loads its record (with the descriptor when EARLY). The stores go out in 4
// rounds of 16 packets: in round k lane l writes byte l % 4 of (ip[0], ip[1], l4[0], l4[1]) of packet 16k + l/4
// (its record and frame offset by ds_bpermute), so the packet's 4 bytes leave in one store
// instruction as one write request with a byte mask. An IPv4 byte that the L4 field overlaps
// (IHL < 5) is left to the L4 lane: the reference writes the L4 field last.
__global__ __launch_bounds__(kBlock) void apply_bytes_kernel(uint8_t* __restrict__ arena,
                                                             const nfcs_desc* __restrict__ desc,
                                                             uint32_t n, uint32_t base16,
                                                             const nfcs_patch* __restrict__ rec) {
    const uint32_t lane = threadIdx.x & 63u;
    // the read pass's XCD-aware order: each XCD writes the eighth of the sub-batch its own read pass
    // covered, whose records and descriptors its L2 still holds (round 5, calls rotating over fresh
    // batches: C1 -0.5%, the C4 shard -0.4% per call; profiles/r05_block_order_ab.jsonl)
    const uint64_t i = (uint64_t)xcd_block() * kBlock + threadIdx.x;
    const nfcs_desc d = i < n ? desc[i] : nfcs_desc{0u, 0u};
    // The record is loaded with the descriptor, before the decision — one memory round trip ahead
    // of the stores instead of two (C1 +1.5%, the 4M shard +0.5%; records of waves that stored
    // inline are stale and ignored). Only the long shape runs this pass (launch_update_one).
    uint2 r0 = make_uint2(0u, 0u);
    if (i < n) r0 = ((const uint2*)rec)[i];
    uint32_t s = defer_len(d.len);
    s += (uint32_t)__builtin_amdgcn_mov_dpp((int)s, 0xB1, 0xF, 0xF, true);  // quad_perm 1,0,3,2
    s += (uint32_t)__builtin_amdgcn_mov_dpp((int)s, 0x4E, 0xF, 0xF, true);  // quad_perm 2,3,0,1
    const bool dfr = i < n && defer_group(s, 4);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(dfr);
    if (!mask) return;
    const uint2 r = dfr ? r0 : make_uint2(NFCS_PATCH_NONE | (NFCS_PATCH_NONE << 16), 0u);
    const uint32_t j = lane & 3u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (((mask >> (16u * k)) & 0xFFFFu) == 0) continue;  // wave-uniform
        const int q4 = (int)((16u * k + (lane >> 2)) * 4u);  // source lane, in bytes
        const uint32_t rx = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)r.x);
        const uint32_t ry = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)r.y);
        const uint32_t o16 = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)d.off16);
        const uint32_t ipo = rx & 0xFFFFu, l4o = rx >> 16;
        const uint32_t off = j < 2 ? ipo : l4o;
        const uint32_t a = off + (j & 1u);
        const bool overlap = j < 2 && l4o != NFCS_PATCH_NONE && (a == l4o || a == l4o + 1u);
        if (off != NFCS_PATCH_NONE && !overlap) {
            const uint32_t b = (j < 2 ? (ry >> (8 * j)) : (ry >> (16 + 8 * (j - 2)))) & 0xFFu;
            uint8_t* p = arena + ((uint64_t)o16 - base16) * 16u + a;
            asm volatile("global_store_byte %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(b) : "memory");
        }
    }
}

// A 2-byte store past the caches (`sc0 sc1 nt`), as st8_nt.
DEV void st16b_nt(uint8_t* p, uint32_t v) {
    asm volatile("global_store_short %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(v) : "memory");
}

// The fused L3 forward's write pass (large bursts, SF_DEFER), from the records alone — no frame
// byte is read again. One thread per packet loads its descriptor, record and next hop (coalesced)
// and, for a forwarded packet of a deferring group of 4 (the decision recomputed from the four
// lengths, as in apply_bytes_kernel), its next hop's MACs. Then 16 rounds of 4 packets: in round k
// the 16 lanes of row r write packet 4k + r (its values by ds_bpermute) as ONE instruction of 2-byte
// stores — lanes 0-5 the MACs (switch.hpp:286-289), lane 6 the TTL with the protocol byte beside it
// (279), lane 7 the IPv4 checksum, lane 8 an even-offset L4 checksum — so each packet's bytes leave
// as one write request with a byte mask, past the caches (`sc0 sc1 nt`); an L4 field at an odd
// offset (TCP: l4 + 15, the 19-byte TcpHeader) goes out as two byte stores after it.
__global__ __launch_bounds__(kBlock) void apply_fwd_kernel(uint8_t* __restrict__ arena,
                                                           const nfcs_desc* __restrict__ desc, uint32_t n,
                                                           const uint32_t* __restrict__ nh,
                                                           const nfcs_nexthop* __restrict__ table,
                                                           const nfcs_patch* __restrict__ rec) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)xcd_block() * kBlock + threadIdx.x;  // as apply_bytes_kernel
    const bool in = i < n;
    const nfcs_desc d = in ? desc[i] : nfcs_desc{0u, 0u};
    const uint2 r0 = in ? ((const uint2*)rec)[i] : make_uint2(0xFFFFFFFFu, 0u);
    const uint32_t h = in ? nh[i] : 0u;
    uint32_t s = defer_len(d.len);
    s += (uint32_t)__builtin_amdgcn_mov_dpp((int)s, 0xB1, 0xF, 0xF, true);  // quad_perm 1,0,3,2
    s += (uint32_t)__builtin_amdgcn_mov_dpp((int)s, 0x4E, 0xF, 0xF, true);  // quad_perm 2,3,0,1
    // records of groups that stored inline are stale: ignored
    const bool go = in && defer_group(s, 4) && (r0.x & 0xFFu) != kFwdNone;
    const uint64_t mask = __builtin_amdgcn_ballot_w64(go);
    if (!mask) return;
    uint32_t m0 = 0, m1 = 0, m2 = 0;
    if (go) {  // a forwarded packet's next hop is in the table (the read pass checked it)
        const uint32_t* m = (const uint32_t*)(table + h);
        m0 = m[0];
        m1 = m[1];
        m2 = m[2];
    }
    const uint32_t rx = go ? r0.x : 0xFFFFFFFFu, ry = r0.y;
    const uint32_t j = lane & 15u;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (((mask >> (4u * k)) & 0xFu) == 0) continue;  // wave-uniform
        const int q4 = (int)((4u * k + (lane >> 4)) * 4u);  // source lane, in bytes
        const uint32_t x = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)rx);
        const uint32_t y = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)ry);
        const uint32_t o16 = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)d.off16);
        const uint32_t a0 = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)m0);
        const uint32_t a1 = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)m1);
        const uint32_t a2 = (uint32_t)__builtin_amdgcn_ds_bpermute(q4, (int)m2);
        const uint32_t ipo = x & 0xFFu, l4o = x >> 24;
        if (ipo == kFwdNone) continue;
        uint8_t* f = arena + (uint64_t)o16 * 16u;
        const uint32_t mw = j < 2 ? a0 : (j < 4 ? a1 : a2);
        uint32_t off = 0xFFFFu, v = 0;
        if (j < 6) {
            off = 2u * j;
            v = mw >> (16u * (j & 1u));
        } else if (j == 6) {  // TTL and protocol (l2 + 8, l2 + 9)
            off = ipo == kFwdNoIp ? (y & 0xFFu) : ipo - 2u;
            v = ((x >> 8) & 0xFFu) | (((x >> 16) & 0xFFu) << 8);
        } else if (j == 7 && ipo != kFwdNoIp) {
            off = ipo;
            v = y;
        } else if (j == 8 && l4o != kFwdNone && !(l4o & 1u)) {
            off = l4o;
            v = y >> 16;
        }
        if (off != 0xFFFFu) st16b_nt(f + off, v & 0xFFFFu);
        if ((j == 8 || j == 9) && l4o != kFwdNone && (l4o & 1u))
            st8_nt(f + l4o + (j - 8u), (y >> (16u + 8u * (j - 8u))) & 0xFFu);
    }
}

// Workgroup shapes of the checksum read pass, chosen per call from the mean arena footprint per
// packet (speed only: results and store forms never depend on it):
//   kShapeTiny   (< kTinyMeanBytes)  8-lane rows of 6 slots (768 B per row pass), 8 packets per
//                one-wave workgroup: frames this short are packet-rate bound, and twice the packets
//                per wave doubles it (64-256 B frames 1.8-1.9x, IMIX 1.47x, 768 B 1.2x);
//   kShapeShort  (< kSmallMeanBytes) 16-lane rows in 256-thread workgroups at 7 waves/SIMD: mixes of
//                short and long frames (C3), where 8-lane rows would need a second row pass for
//                most waves (C3 -7.5%);
//   kShapeLong   16-lane rows in 256-thread workgroups held at 5 waves/SIMD.
enum : int { kShapeTiny = 0, kShapeShort = 1, kShapeLong = 2 };

// One launch of update_rows_kernel (the grid size passed as `nblocks` too).
template <int K, int R, int OCC, int BS, bool FWD, int SF, int LAM = 0, int KL = K>
static void launch_rows(uint32_t grid, unsigned lds, hipStream_t stream, uint8_t* arena, uint64_t arena_bytes,
                        const nfcs_desc* desc, uint32_t n, uint32_t base16, uint8_t* status, nfcs_patch* patch,
                        nfcs_patch* ws, const FwdArgs& fa) {
    hipLaunchKernelGGL((update_rows_kernel<K, R, OCC, BS, FWD, SF, LAM, KL>), dim3(grid), dim3(BS), lds, stream, desc, n, grid,
                       arena, arena_bytes, base16, fa.nh, fa.obs.slot, status, patch, ws, fa.table, fa.table_n,
                       fa.obs.tag, fa.done, fa.dem);
}

// One launch of the checksum path (its read pass and, for kUpdateAuto, its write pass) over n
// packets, in the shape chosen for the whole call.
static hipError_t launch_update_one(uint8_t* arena, uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n,
                                    uint32_t base16, uint8_t* status, nfcs_patch* patch, nfcs_patch* ws,
                                    int form, int shape, hipStream_t stream, ObsReq obs, DoneReq done = {},
                                    DemandReq dem = {}) {
    const FwdArgs nofwd = {nullptr, nullptr, 0, obs, done, dem};
    // a burst of at most kInlineMaxPackets packets: one kernel, every wave inline (the write pass's
    // launch would cost more than deferral saves on so few packets)
    if (form == kUpdateAuto && n <= kInlineMaxPackets) form = kUpdateInline;
    const uint32_t g8 = (n + 7u) / 8u, g4 = (n + 15u) / 16u;
#define NFCS_ROWS(OCC, BS, G, SF)                                                                  \
    launch_rows<6, 16, OCC, BS, false, SF, BS == kBlock ? 1 : 0, BS == kBlock ? 7 : 6>(                          \
        G, BS == kBlock ? kRowsLdsPad : 0u, stream, arena, arena_bytes, desc,                                 \
                                           n, base16, status, patch, ws, nofwd)
#define NFCS_ROWS8(SF) \
    launch_rows<6, 8, 8, 64, false, SF>(g8, 0u, stream, arena, arena_bytes, desc, n, base16, status, patch, ws, nofwd)
#define NFCS_SHORT(SF) \
    launch_rows<6, 16, 7, kBlock, false, SF, 0, 6>(g4, 0u, stream, arena, arena_bytes, desc, n, base16, status, patch, ws, nofwd)
#define NFCS_SHAPED(SF)                                                                            \
    do {                                                                                           \
        if (shape == kShapeTiny) NFCS_ROWS8(SF);                                                   \
        else if (shape == kShapeShort) NFCS_SHORT(SF);                                             \
        else NFCS_ROWS(1, kBlock, g4, SF);                                                         \
    } while (0)
    if (form == kUpdateRecords) {
        NFCS_ROWS(1, kBlock, g4, SF_RECORDS);
    } else if (form == kUpdateInline) {
        NFCS_SHAPED(SF_INLINE);
    } else if (shape != kShapeLong) {
        // short and tiny shapes: every wave stores inline and no write pass is launched. The few
        // groups of 4 that average >= kDeferMeanBytes in such batches gain less from deferral than
        // the write pass costs to find them among all the descriptors (round 3, same box: C3 +1.5-2.4%,
        // 1M x 64 B +5.5%, 4M mixes of 64/1500-byte frames with 25/50/75% long frames +2/+1.3/+3.7%;
        // profiles/r03_s3_ab_c3_inline.jsonl, r03_s3_ab_bimodal.jsonl)
        NFCS_SHAPED(SF_INLINE);
    } else {
        NFCS_ROWS(1, kBlock, g4, SF_DEFER);
        hipLaunchKernelGGL(apply_bytes_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                           arena, desc, n, base16, patch ? patch : ws);
    }
#undef NFCS_SHAPED
#undef NFCS_SHORT
#undef NFCS_ROWS8
#undef NFCS_ROWS
    return hipGetLastError();
}

hipError_t launch_update(const DevInfo& di, uint8_t* arena, uint64_t arena_bytes,
                         const nfcs_desc* desc, uint32_t n, uint32_t base16, uint8_t* status,
                         nfcs_patch* patch, nfcs_patch* ws, int form, hipStream_t stream,
                         uint64_t slot_bytes, ObsReq obs, DoneReq done, DemandReq dem, bool sparse) {
    (void)di;
    if (n == 0) return hipSuccess;
    if (form == kUpdateRecords && !patch) return hipErrorInvalidValue;
    if (done.flag && form == kUpdateAuto) return hipErrorInvalidValue;  // one kernel per call only
    if (form == kUpdateAuto && !patch && !ws) return hipErrorInvalidValue;
    // The short shape at 7 waves/SIMD: __launch_bounds__ 7 caps the kernel at 94 SGPRs (at the
    // compiler's 106 the SGPR file admits only 6 waves/SIMD: C3 +2%). Its workgroups were one wave
    // (round 3, a replayed batch: short-lived waves retire and relaunch with less granularity loss,
    // C3 +2-3%); in the steady state 256-thread workgroups, whose 4 waves on one CU share the
    // descriptor line of their 16 packets, measured 0.3-0.5% faster (round 5, C3 0.662-0.663
    // against 0.665 ms per call; profiles/r05_c3_rows_ab.jsonl). 256-thread workgroups are held at 5 waves/SIMD by kRowsLdsPad
    // bytes of (unused) LDS: at the 8 their 54 VGPRs allow, the read stream runs slower (round 1,
    // one replayed batch: C1 0.768 vs 0.777 at 6). Round 4, calls rotating over fresh batches with
    // 512K-packet sub-batches: 5 waves beat 6 by 1.2-1.5% on C1, 1.6% on the C4 shard, 0.3% on C2
    // (profiles/r04_s2_long_occupancy5_ab.jsonl).
    const uint64_t mean = shape_mean(arena_bytes, n, slot_bytes);
    const int shape = mean < kTinyMeanBytes ? kShapeTiny : (mean < kSmallMeanBytes ? kShapeShort : kShapeLong);
    // Long frames in a batch of more than kSubBatchAbovePackets: read pass and write pass alternate
    // per sub-batch of kSubBatchPackets, so the write pass finds its header lines still in the
    // 256 MB memory-side cache that the read pass just brought them into (the 4M
    // shard 0.683-0.714 -> 0.749-0.755). Sub-batches are multiples of 4 packets, so every wave's
    // deferral group is the same as in one launch; they run in order on the stream and share the
    // workspace.
    // The sparse form (nfcs_store_policy.h: the context's recent calls found next to nothing to store): the
    // whole call as one inline launch, as a burst of at most kInlineMaxPackets runs; never with a caller's
    // records, which keep every field.
    // One launch whatever the size: as 512K sub-batches the sparse form measured 1-2% slower on C1 and 3-4%
    // on the 4M shard (profiles/store_policy_sub_batches.jsonl).
    if (form == kUpdateAuto && shape == kShapeLong && sparse && !patch) form = kUpdateInline;
    if (form == kUpdateAuto && shape == kShapeLong && n > kSubBatchAbovePackets) {
        for (uint32_t i = 0; i < n; i += kSubBatchPackets) {
            // every sub-batch counts its store demand into the call's words; the first forwards the
            // previous call's
            const DemandReq ds = {dem.cur, dem.prev, i == 0 ? dem.host : nullptr, dem.prev_gen};
            const hipError_t e = launch_update_one(arena, arena_bytes, desc + i, std::min(kSubBatchPackets, n - i),
                                                   base16, status ? status + i : nullptr,
                                                   patch ? patch + i : nullptr, ws, form, shape, stream,
                                                   i == 0 ? obs : ObsReq{}, DoneReq{}, ds);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    return launch_update_one(arena, arena_bytes, desc, n, base16, status, patch, ws, form, shape, stream, obs, done,
                             dem);
}

uint32_t update_demand_sampled(uint64_t arena_bytes, uint32_t n, uint64_t slot_bytes, bool sparse) {
    if (n <= kInlineMaxPackets || shape_mean(arena_bytes, n, slot_bytes) < kSmallMeanBytes) return 0;
    if (sparse || n <= kSubBatchAbovePackets) return demand_sampled_one(n);
    uint32_t s = 0;
    for (uint32_t i = 0; i < n; i += kSubBatchPackets) s += demand_sampled_one(std::min(kSubBatchPackets, n - i));
    return s;
}

hipError_t launch_l3_forward(const DevInfo& di, uint8_t* arena, uint64_t arena_bytes,
                             const nfcs_desc* desc, const uint32_t* nh, uint32_t n,
                             const nfcs_nexthop* table, uint32_t table_n, uint8_t* status,
                             nfcs_patch* ws, hipStream_t stream, uint64_t slot_bytes, ObsReq obs) {
    (void)di;
    if (n == 0) return hipSuccess;
    const FwdArgs fa = {nh, table, table_n, obs};
    const uint64_t mean = shape_mean(arena_bytes, n, slot_bytes);
    if (mean < kTinyMeanBytes) {
        // short frames: 8-lane rows, 8 packets per one-wave workgroup (packet-rate bound, §5g)
        launch_rows<6, 8, 8, 64, true, SF_INLINE>((n + 7u) / 8u, 0u, stream, arena, arena_bytes, desc, n, 0u, status,
                                                  nullptr, nullptr, fa);
        return hipGetLastError();
    }
    if (mean < kSmallMeanBytes) {
        // mixes of short and long frames (the C3 mix): 8-lane rows of 12 slots (1536 bytes per row
        // pass, so a 1500-byte frame needs no second pass), 8 packets per wave at 6 waves/SIMD (80
        // VGPRs). The forward's header work (decision, MAC pick, segment) then serves 8 packets per
        // instruction instead of 4; its short waves are latency-bound and every instruction is on
        // their path: C3 mix 0.519 -> 0.587 (round 3, profiles/r03_s1_ab_fwd_c3_rows.jsonl). The plain
        // update keeps 16-lane rows there (8-lane rows of 12 slots: C3 0.569 vs 0.594). 256-thread
        // workgroups (32 packets) since round 5: in the steady state, median 0.6915 against 0.6935 ms
        // per call over 9 alternating processes each (profiles/r05_fwd_wg256_ab.jsonl)
        launch_rows<12, 8, 6, kBlock, true, SF_INLINE, 1, 12>((n + 31u) / 32u, 0u, stream, arena, arena_bytes, desc, n, 0u, status,
                                                   nullptr, nullptr, fa);
        return hipGetLastError();
    }
    if (ws && n > kFwdDeferAbovePackets) {
        // bursts of long frames: per 512K-packet sub-batch, a read pass whose long-frame waves write
        // forward records instead of segments, then apply_fwd_kernel while the header lines are
        // still in the memory-side cache (4M x 1500 B 0.681 -> 0.705; round 4, calls
        // rotating over fresh batches: 1M C1 bursts too; mixes like C3, whose waves rarely defer,
        // lose 10% to the sub-batch launches and take the short-mix shape above). The read pass is
        // held at 6 waves/SIMD by kRowsLdsPad6 (round 4, calls rotating over fresh batches: 4M -0.9%,
        // C1 -0.2% per call against 7; 5 waves, the update's long shape, +1.5-3.5% here;
        // profiles/r04_s2_fwd_occupancy_ab.jsonl)
        for (uint32_t i = 0; i < n; i += kSubBatchPackets) {
            const uint32_t m = std::min(kSubBatchPackets, n - i);
            const FwdArgs fs = {nh + i, table, table_n, i == 0 ? obs : ObsReq{}};
            launch_rows<6, 16, 7, kBlock, true, SF_DEFER, 2, 7>((m + 15u) / 16u, kRowsLdsPad6, stream, arena, arena_bytes, desc + i, m,
                                                          0u, status ? status + i : nullptr, nullptr, ws, fs);
            hipLaunchKernelGGL(apply_fwd_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, arena,
                               desc + i, m, nh + i, table, (const nfcs_patch*)ws);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // 7 waves per SIMD (72 VGPRs and 94 SGPRs, no scratch; the compiler alone picks 81 VGPRs
    // and 106 SGPRs = 6 waves and the kernel runs 4-5% slower)
    launch_rows<6, 16, 7, kBlock, true, SF_INLINE, 2, 7>((n + 15u) / 16u, 0u, stream, arena, arena_bytes, desc, n, 0u, status,
                                                   nullptr, nullptr, fa);
    return hipGetLastError();
}

// ---- VLAN push / pop + checksum ----------------------------------------------
// Packet::push_vlan(vid, prio) / pop_vlan() (packet.hpp:655-720) and the update_checksums() they
// end with, in one pass per frame. One 16-lane row per packet as in update_rows_kernel: the row
// loads the frame's chunks (K slots of 16 lanes), builds the EDITED frame's chunks in registers
// (a 4-byte shift is one DPP row_shr:1 / row_shl:1 of a dword plus three register moves per
// chunk; the chunk that crosses a slot boundary takes a row_newbcast from the neighbouring
// slot), plans update_checksums() on the edited header, sums the edited chunks, patches the
// checksum bytes into the chunk registers and stores the edited frame with 16-byte stores. So
// the memmove, the tag and the checksums cost one read and one write of the frame.
//   * frames longer than one batch (K*16 chunks) are processed batch by batch, in ascending
//     order: a push carries the last dword of the previous batch's old chunks in a register
//     (the store of batch b overwrites it), a pop loads the first dword of the next batch;
//     batch 0 is then stored before the loop and the checksum bytes are stored at the end by
//     the lanes that stored their chunks;
//   * bytes of a frame's last chunk past the bytes the reference writes keep their old values
//     (the slot's tail is rewritten with what it held), so the arena matches the reference's
//     memmove byte for byte;
//   * uncommon headers take the same cold path as update_rows_kernel, after the edited frame is
//     in memory.
enum : uint32_t { VM_NONE = 0, VM_FAIL = 1, VM_RETAG = 2, VM_PUSH = 3, VM_POP = 4 };

// Chunk bytes at frame offsets >= wend keep their old values.
DEV uint4 keep_tail(const uint4& nv, const uint4& ov, uint32_t o, uint32_t wend) {
    uint32_t r[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const int nb = (int)wend - (int)(o + 4u * j);
        const uint32_t m = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
        r[j] = (comp(nv, j) & m) | (comp(ov, j) & ~m);
    }
    return make_uint4(r[0], r[1], r[2], r[3]);
}

// Byte i (0..15) of a chunk register := b.

DEV uint32_t dpp_prev(uint32_t x) {  // lane rl gets lane rl-1 of its row (0 for rl = 0)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x111, 0xF, 0xF, true);
}
DEV uint32_t dpp_next(uint32_t x) {  // lane rl gets lane rl+1 of its row (0 for rl = 15)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x101, 0xF, 0xF, true);
}

// Edited chunks of one batch. v: old chunks rl + 16k (+ cb) of the row's window, i.e. frame chunks
// rl + 16k + cb - mis (line-aligned windows: the frame's chunk 0 sits in lane mis of slot 0);
// prevw: for a push, the old dword just before this batch (the row's lane 15 of the previous
// batch); nextx: for a pop, the old dword just after it. Batch 0 (first = true) builds the new
// bytes 12-15 in chunk 0. Lanes before the frame start get values that are never stored or summed.
template <int K, int R = 16>
DEV void vlan_edit(uint4 (&nv)[K], const uint4 (&v)[K], uint32_t mode, uint32_t rl, bool first,
                   uint32_t prevw, uint32_t nextx, uint32_t tag_dw, uint32_t cb, uint32_t wend,
                   uint32_t mis = 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint4 e = v[k];
        if (mode == VM_PUSH) {  // new[o] = old[o - 4] for o >= 16
            uint32_t pw = dpp_prev(v[k].w);  // across an 8-lane row's start: replaced below
            const uint32_t lw = (k > 0) ? row_bcast<R - 1, R>(v[k - 1].w) : prevw;
            if (rl == 0) pw = lw;
            e = make_uint4(pw, v[k].x, v[k].y, v[k].z);
            if (first && k == 0 && rl == mis) e = make_uint4(v[0].x, v[0].y, v[0].z, tag_dw);
        } else if (mode == VM_POP) {  // new[o] = old[o + 4] for o >= 12
            uint32_t nx = dpp_next(v[k].x);  // across an 8-lane row's end: replaced below
            const uint32_t fx = (k + 1 < K) ? row_bcast<0, R>(v[k + 1 < K ? k + 1 : k].x) : nextx;
            if (rl == (uint32_t)R - 1u) nx = fx;
            e = make_uint4(v[k].y, v[k].z, v[k].w, nx);
            if (first && k == 0 && rl == mis) e = make_uint4(v[0].x, v[0].y, v[0].z, nx);
        } else if (mode == VM_RETAG) {
            if (first && k == 0 && rl == mis) e.w = tag_dw;
        }
        const uint32_t c = cb + rl + (uint32_t)R * (uint32_t)k - mis;
        nv[k] = (int)c < 0 ? v[k] : keep_tail(e, v[k], 16u * c, wend);
    }
}

// Store policy of the VLAN kernel's frame writes: every write of a frame (its rewritten chunks and,
// after them, its checksum bytes) takes the same path, so same-address writes stay in program order.
enum : int { VST_PLAIN = 0, VST_WT = 1, VST_NT = 2 };
template <int POL>
DEV void vst16(uint4* p, const uint4& v) {
    if (POL == VST_NT) st16_nt(p, v);
    else st16<POL == VST_WT>(p, v);
}
template <int POL>
DEV void vst8(uint8_t* p, uint32_t b) {
    if (POL == VST_NT) st8_nt(p, b);
    else st8<POL == VST_WT>(p, b);
}

// Frame chunk rl (rl < R) of a row whose window is line-aligned (slot 0 lane rl + mis, or slot 1).
template <int K, int R>
DEV uint4 vlan_view(const uint4 (&v)[K], uint32_t rowbase4, uint32_t rl, uint32_t mis) {
    const uint32_t a = rl + mis;
    const int sl = (int)(rowbase4 + (a & (R - 1)) * 4u);
    const uint4 r0 = make_uint4((uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[0].x),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[0].y),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[0].z),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[0].w));
    const uint4 r1 = make_uint4((uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[1].x),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[1].y),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[1].z),
                                (uint32_t)__builtin_amdgcn_ds_bpermute(sl, (int)v[1].w));
    return a < (uint32_t)R ? r0 : r1;
}

// LA: line-aligned windows as in the checksum kernel (row_stage): lane rl of slot k holds frame
// chunk 16k + rl - mis, so every load and store instruction covers whole lines whatever the frame's
// line offset; the 4-byte moves are the same lane shifts in these coordinates, and the header views
// the edit and the plan read are rotated into frame order (vlan_view) in waves with a row starting
// mid-line.
template <int K, int K2 = 2, int POL = VST_PLAIN, int R = 16, bool LA = false>
__global__ __launch_bounds__(kBlock) void vlan_rows_kernel(uint8_t* __restrict__ arena,
                                                           uint64_t arena_bytes,
                                                           nfcs_desc* __restrict__ desc, uint32_t n,
                                                           const uint32_t* __restrict__ ops,
                                                           uint32_t op_all,
                                                           const uint32_t* __restrict__ caps,
                                                           uint32_t cap_all,
                                                           uint8_t* __restrict__ status,
                                                           uint64_t* __restrict__ obs, uint64_t obs_tag) {
    static_assert(R == 16 || R == 8, "16- or 8-lane rows");
    constexpr uint32_t PW = 64 / R, KR = (uint32_t)(K * R);
    const uint32_t lane = threadIdx.x & 63u, rl = lane & (R - 1), row = lane / R;
    const uint32_t rowbase4 = (lane & ~(uint32_t)(R - 1)) * 4u;
    const uint64_t pw = (uint64_t)blockIdx.x * (kBlock / R) + rfl(threadIdx.x >> 6) * PW;
    if (pw >= n) return;
    // the footprint sample for the next call's shape (lengths other waves are editing may be read
    // old or new: speed only)
    if (blockIdx.x == 0 && threadIdx.x < 64 && obs) sample_footprint(desc, obs_tag, lane, obs);
    const nfcs_desc d = pick_desc<PW>(load_descw<PW>(desc, pw, n), row);
    uint32_t op = op_all, cap = cap_all;
    {  // the wave's edit words / capacities: scalar loads, like the descriptors
        uint32_t q[PW], r[PW];
#pragma unroll
        for (uint32_t i = 0; i < PW; ++i) {
            q[i] = (ops && pw + i < n) ? ops[pw + i] : op_all;
            r[i] = (caps && pw + i < n) ? caps[pw + i] : cap_all;
        }
        if (ops) { op = 0; for (uint32_t i = 0; i < PW; ++i) op |= (row == i) ? q[i] : 0u; }
        if (caps) { cap = 0; for (uint32_t i = 0; i < PW; ++i) cap |= (row == i) ? r[i] : 0u; }
    }
    const uint64_t p = pw + row;
    const bool valid = p < n;
    const uint32_t kind = op & NFCS_VLAN_OP_MASK;
    const uint64_t off = (uint64_t)d.off16 * 16u;
    const uint64_t need = (uint64_t)d.len + (kind == NFCS_VLAN_PUSH ? 4u : 0u);
    const bool bad = valid && (off + ((need + 15u) & ~15ull) > arena_bytes);
    const bool live = valid && !bad;
    const uint32_t len = live ? d.len : 0u;
    uint8_t* frame = arena + (live ? off : 0);
    const uint4* src = (const uint4*)frame;
    const uint32_t nl = live ? (uint32_t)((need + 15u) >> 4) : 0u;  // old chunks to load
    // a row takes line-aligned windows only where they need no more row passes than frame-relative
    // ones (a 1500-byte frame 48+ bytes into a line would spill into a second pass: 64-byte starts
    // measured 0.47 against 0.71 with it)
    const uint32_t lm = LA && live ? (uint32_t)(((uintptr_t)frame >> 4) & 7u) : 0u;
    const uint32_t mis = (nl + lm <= KR || nl > KR) ? lm : 0u;
    const bool rot = LA && __builtin_amdgcn_ballot_w64(mis != 0) != 0;  // wave-uniform

    const uint4* zl = g_zero_line;
    uint4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t c = rl + (uint32_t)R * k - mis;  // frame chunk (wraps below the frame start)
        v[k] = ld16<0>((c < nl) ? src + c : zl);
    }
    // pop: the old dword after batch 0 (first dword of the window's chunk KR)
    const uint32_t nx0 = *(const uint32_t*)((KR - mis < nl) ? src + (KR - mis) : zl);

    // the edit the reference makes (packet.hpp:655-720), decided on the old header
    const RowHdr<R> h{rot ? vlan_view<K, R>(v, rowbase4, rl, mis) : v[0], rowbase4};
    const bool tagged = len >= 14 && h.be16(12) == 0x8100u;  // has_vlan() (603-606)
    uint32_t mode = VM_NONE;
    if (live && kind == NFCS_VLAN_PUSH)
        mode = len < 14 ? VM_FAIL : tagged ? VM_RETAG : (len + 4u > cap ? VM_FAIL : VM_PUSH);
    else if (live && kind == NFCS_VLAN_POP)
        mode = (!tagged || len < 18) ? VM_FAIL : VM_POP;
    const bool act = mode >= VM_RETAG;
    const uint32_t vid = op & 0x0FFFu, prio = (op >> 13) & 7u;
    const uint32_t tci_old = h.be16(14);
    const uint32_t tci = ((mode == VM_RETAG ? tci_old : 0u) & 0x1000u) | (prio << 13) | vid;  // 185-190
    const uint32_t tag_dw = (mode == VM_RETAG) ? ((comp(v[0], 3) & 0xFFFFu) | (bswap16(tci) << 16))
                                               : (0x81u | (bswap16(tci) << 16));
    const uint32_t nlen = mode == VM_PUSH ? len + 4u : mode == VM_POP ? len - 4u : len;
    // bytes the reference writes end at wend: the moved frame, or bytes 14-15 of the tag
    const uint32_t wend = mode == VM_RETAG ? (len > 16u ? len : 16u) : nlen;
    const uint32_t nst = !act ? 0u : mode == VM_RETAG ? 1u : (wend + 15u) >> 4;  // chunks stored

    uint4 nv[K];
    vlan_edit<K, R>(nv, v, mode, rl, true, 0u, nx0, tag_dw, 0u, wend, mis);
    uint32_t carry = row_bcast<R - 1, R>(v[K - 1].w);  // push: old dword before batch 1

    // update_checksums() on the edited frame (690 / 718)
    RPlan P = fast_plan<R, false>(rot ? vlan_view<K, R>(nv, rowbase4, rl, mis) : nv[0], rowbase4, nlen);
    const bool slow = act && (P.st >> 8) != 0;
    if (!act || slow) P = rplan_none(0);
    const uint32_t re = (P.flags & F_L4) ? P.re : 0u, lo4 = P.rs & ~3u;
    const uint32_t tailfix = P.flags & F_TAIL;
    uint32_t rlv = rl;
    asm volatile("" : "+v"(rlv));
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t c = rlv + (uint32_t)R * k - mis;
        if ((int)c >= 0) acc_slot(acc, nv[k], c, lo4, re, tailfix);
    }

    // rows whose frame continues past batch 0 (moved chunks or summed chunks)
    const uint32_t nre = (re + 15u) >> 4;
    const uint32_t cm = ((nst > nre) ? nst : nre) + mis;  // window chunks
    const bool multi = __builtin_amdgcn_ballot_w64(cm > KR) != 0;  // wave-uniform
    auto finish = [&](uint32_t a) -> uint32_t {  // l4 field word
        const uint32_t z = row_sum<R>(a) + P.corr;
        uint32_t c = (~fold32(z)) & 0xFFFFu;
        if ((P.flags & F_UDP) && c == 0) c = 0xFFFFu;
        return (P.flags & F_L4) ? (P.fs | (c << 16)) : NFCS_PATCH_NONE;
    };
    const uint32_t ipw = (P.flags & F_IP) ? P.ipw : NFCS_PATCH_NONE;
    uint32_t l4w = NFCS_PATCH_NONE;
    if (!multi) {
        l4w = finish(acc);
        // checksum bytes into the chunk registers (fast-path fields lie below byte 80: slot 0);
        // a re-tag stores chunk 0 and the chunks holding checksum bytes
        // (byte by byte: put_field measured 1.2% slower here, 0.723 against 0.732 on C1)
        // (with line-aligned windows the chunk of byte pos sits in lane (pos/16 + mis) % R of slot
        // (pos/16 + mis) / R: slot 0, or slot 1 of an 8-lane row)
        bool patched0 = false, patched1 = false;
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint32_t w = (t < 2) ? ipw : l4w;
            const uint32_t pos = (w & 0xFFFFu) + (t & 1u);
            const uint32_t a = (pos >> 4) + mis, b = (w >> (16 + 8 * (t & 1u))) & 0xFFu;
            if ((w & 0xFFFFu) != NFCS_PATCH_NONE && (a & (R - 1)) == rl) {
                if (a < (uint32_t)R) {
                    nv[0] = put_byte(nv[0], pos & 15u, b);
                    patched0 = true;
                } else {
                    nv[1] = put_byte(nv[1], pos & 15u, b);
                    patched1 = true;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t c = rl + (uint32_t)R * k - mis;
            if (c < nst || (k == 0 && patched0) || (k == 1 && patched1)) vst16<POL>((uint4*)frame + c, nv[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t c = rl + (uint32_t)R * k - mis;
            if (c < nst) vst16<POL>((uint4*)frame + c, nv[k]);
        }
        const uint32_t cmax = wave_max_rows<R>(cm);
        // the rest of a long frame in batches of K2 slots (K2 < K saves VGPRs: w and e live
        // together here)
        constexpr uint32_t KR2 = (uint32_t)(K2 * R);
        for (uint32_t cb = KR; cb < cmax; cb += KR2) {
            uint4 w[K2], e[K2];
#pragma unroll
            for (int k = 0; k < K2; ++k) {
                const uint32_t c = cb + rlv + (uint32_t)R * k - mis;
                w[k] = ld16<1>((c < nl) ? src + c : zl);
            }
            const uint32_t nx = *(const uint32_t*)((cb + KR2 - mis < nl) ? src + (cb + KR2 - mis) : zl);
            vlan_edit<K2, R>(e, w, mode, rl, false, carry, nx, 0u, cb, wend, mis);
            carry = row_bcast<R - 1, R>(w[K2 - 1].w);
#pragma unroll
            for (int k = 0; k < K2; ++k) {
                const uint32_t c = cb + rlv + (uint32_t)R * k - mis;
                acc_slot(acc, e[k], c, lo4, re, tailfix);
                if (c < nst) vst16<POL>((uint4*)frame + c, e[k]);
            }
        }
        l4w = finish(acc);
        // the lanes that stored chunk pos/16 store the checksum bytes (program order)
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint32_t w = (t < 2) ? ipw : l4w;
            const uint32_t pos = (w & 0xFFFFu) + (t & 1u);
            if ((w & 0xFFFFu) != NFCS_PATCH_NONE && (((pos >> 4) + mis) & (R - 1)) == rl)
                vst8<POL>(frame + pos, w >> (16 + 8 * (t & 1u)));
        }
    }
    const uint32_t st0 = bad ? (uint32_t)NFCS_ST_BAD_DESC
                       : mode == VM_FAIL ? (uint32_t)NFCS_ST_VLAN_FAIL
                       : act ? (P.st | NFCS_ST_FLAG_VLAN) : (uint32_t)NFCS_ST_NONE;
    if (valid && rl == 0) {
        if (!slow && status) status[p] = (uint8_t)st0;
        if (act) desc[p].len = nlen;
    }
    if (__builtin_amdgcn_ballot_w64(slow) != 0) {  // cold path on the edited frame in memory
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        RPlan Q = rplan_none(0);
        SeqOut o = {0, 0, 0, 0, 0};
        if (slow && rl == 0) {
            Q = slow_plan(frame, nlen);
            if (Q.flags & F_SEQ) o = seq_update(frame, nlen);
        }
        Q.st = row_bcast<0, R>(Q.st);
        Q.flags = row_bcast<0, R>(Q.flags);
        Q.ipw = row_bcast<0, R>(Q.ipw);
        Q.rs = row_bcast<0, R>(Q.rs);
        Q.re = row_bcast<0, R>(Q.re);
        Q.fs = row_bcast<0, R>(Q.fs);
        Q.corr = row_bcast<0, R>(Q.corr);
        const uint32_t ost = row_bcast<0, R>(o.st);
        const bool seq = slow && (Q.flags & F_SEQ);
        const uint32_t re2 = (slow && !seq && (Q.flags & F_L4)) ? Q.re : 0u;
        const uint32_t lo42 = Q.rs & ~3u, tf2 = Q.flags & F_TAIL;
        uint32_t acc2 = 0;
        for (uint32_t c = rl; c < ((re2 + 15u) >> 4); c += R) acc_slot(acc2, src[c], c, lo42, re2, tf2);
        const uint32_t z2 = row_sum<R>(acc2) + Q.corr;
        const uint32_t ipw2 = (Q.flags & F_IP) ? Q.ipw : NFCS_PATCH_NONE;
        uint32_t l4w2 = NFCS_PATCH_NONE;
        if (Q.flags & F_L4) {
            uint32_t c = (~fold32(z2)) & 0xFFFFu;
            if ((Q.flags & F_UDP) && c == 0) c = 0xFFFFu;
            l4w2 = Q.fs | (c << 16);
        }
        if (slow && !seq && rl < 4) {
            const uint32_t w = (rl & 2u) ? l4w2 : ipw2;
            const uint32_t pos = (w & 0xFFFFu) + (rl & 1u);
            if ((w & 0xFFFFu) != NFCS_PATCH_NONE) vst8<POL>(frame + pos, w >> (16 + 8 * (rl & 1u)));
        }
        if (slow && rl == 0 && status)
            status[p] = (uint8_t)((seq ? (ost | NFCS_ST_FLAG_OVERLAP) : Q.st) | NFCS_ST_FLAG_VLAN);
    }
}

hipError_t launch_vlan(const DevInfo& di, uint8_t* arena, uint64_t arena_bytes, nfcs_desc* desc,
                       uint32_t n, const uint32_t* ops, uint32_t op_all, const uint32_t* caps,
                       uint32_t cap_all, uint8_t* status, hipStream_t stream, uint64_t slot_bytes,
                       ObsReq obs, uint32_t sample_bits) {
    (void)di;
    if (n == 0) return hipSuccess;
    // Long frames continue in batches of 6 slots (128 VGPRs, 4 waves/SIMD); batches of 2 slots
    // (94 VGPRs, 5 waves/SIMD) measured 6% slower on C1 push/pop, capping the occupancy lower
    // slower still (profiles/r01_s2_occupancy.md); dispatch order (the XCD-aware order measured 2%
    // slower here). Frame stores past the caches (`sc0 sc1 nt`, round 2 session 3): C1 push/pop
    // +4.5%, 1M 256 / 512-byte frames +2-5% against write-through `sc1` (itself +1.2% over plain
    // stores); frames in slots under 256 B keep `sc1` (64-byte frames: 177 vs 181 µs per 1M).
    // Short frames (mean footprint < kTinyMeanBytes): 8-lane rows, 8 packets per wave (§5g), their
    // stores write-through also when the burst's sample found frames off their lines or of varying
    // lengths (sample_bits; nfcs_internal.h kVlanWtMeanBytes).
    const uint64_t mean = shape_mean(arena_bytes, n, slot_bytes);
    const dim3 g8((n + 31u) / 32u), g16((n + 15u) / 16u);
    if (mean < kVlanWtMeanBytes || (mean < kTinyMeanBytes && (sample_bits & (kObsUnaligned | kObsMixed))))
        hipLaunchKernelGGL((vlan_rows_kernel<6, 6, VST_WT, 8>), g8, dim3(kBlock), 0, stream, arena, arena_bytes,
                           desc, n, ops, op_all, caps, cap_all, status, obs.slot, obs.tag);
    else if (mean < kTinyMeanBytes)
        hipLaunchKernelGGL((vlan_rows_kernel<6, 6, VST_NT, 8>), g8, dim3(kBlock), 0, stream, arena, arena_bytes,
                           desc, n, ops, op_all, caps, cap_all, status, obs.slot, obs.tag);
    else  // 4 rows per wave, 4 waves per workgroup
        hipLaunchKernelGGL((vlan_rows_kernel<6, 6, VST_NT, 16, true>), g16, dim3(kBlock), 0, stream, arena, arena_bytes,
                           desc, n, ops, op_all, caps, cap_all, status, obs.slot, obs.tag);
    return hipGetLastError();
}

// ---- the lane-per-packet stage shape -------------------------------------------
// What the read-only stage kernels below share: a wave takes 64 consecutive packets in XCD-aware block
// order and lane l decides packet l. A kernel states its own decision and calls these for the rest.
inline uint32_t lane_blocks(uint32_t n) { return (n + 255u) / 256u; }  // kBlock lanes, one packet each

// Lane l's packet. d is zero past n; a dead packet (past n, or with a chunk outside the arena) reads as
// length 0, so nothing of its frame is requested. A kernel's further conditions are `&&` on live, and
// where a wave past n returns (before a barrier, after it, or not at all) is the kernel's choice.
struct LanePkt {
    uint64_t p0, p;  // the wave's first packet, this lane's packet
    uint2 d;         // the descriptor {off16, len}
    uint64_t off;    // the frame's byte offset in the arena
    bool live;
    uint32_t len;
};
DEV LanePkt lane_pkt(const nfcs_desc* __restrict__ desc, uint32_t n, uint32_t nblocks, uint64_t arena_bytes) {
    LanePkt k;
    k.p0 = ((uint64_t)xcd_block_n(nblocks) * kWavesPerBlock + rfl(threadIdx.x >> 6)) * 64u;
    k.p = k.p0 + (threadIdx.x & 63u);
    k.d = make_uint2(0u, 0u);
    if (k.p < n) k.d = ((const uint2*)desc)[k.p];  // one coalesced load
    k.off = (uint64_t)k.d.x * 16u;
    k.live = k.p < n && sw_desc_live(k.d.x, k.d.y, arena_bytes);
    k.len = k.live ? k.d.y : 0u;
    return k;
}

// Header chunks 0..2 (bytes 0..47) of the wave's 64 packets in 8-lane rows: instruction k, row r ->
// packet 8k + r, lane rl -> chunk rl, so one instruction reads one line of each of 8 packets and 8 are in
// flight. off16 / len are the lane's own packet's; chunks at or past len read the zero line. Non-temporal:
// the frames are read once. The loads stay in flight until hdr_rows_store, so a kernel that stages a table
// issues them first and stores the rows after its barrier.
DEV void hdr_rows_load(const uint8_t* __restrict__ arena, uint32_t off16, uint32_t len, uint32_t lane, uint4 (&c)[8]) {
    const uint32_t rl = lane & 7u, r = lane >> 3;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t q = 8u * k + r;
        const uint32_t qo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(q * 4u), (int)off16);
        const uint32_t ql = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(q * 4u), (int)len);
        const uint4* src = (const uint4*)(arena + (uint64_t)qo * 16u);
        c[k] = ld16<1>((rl < 3u && rl * 16u < ql) ? src + rl : g_zero_line);
    }
}
// The rows into the wave's LDS, ROW bytes per packet; on return every lane may read its packet's row.
template <uint32_t ROW>
DEV void hdr_rows_store(uint8_t* rows, uint32_t lane, const uint4 (&c)[8]) {
    const uint32_t rl = lane & 7u, r = lane >> 3;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (rl < 3u) *(uint4*)(rows + (8u * k + r) * ROW + 16u * rl) = c[k];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes are done
    __builtin_amdgcn_wave_barrier();
}
// Headers past byte 47 (IPv6, IPv4 options): the lanes with `more` load chunks 3..5 of their own frame
// into their row b (96 bytes). Every lane of the wave calls it.
DEV void hdr_late_chunks(uint8_t* b, const uint8_t* __restrict__ arena, uint64_t off, uint32_t len, bool more) {
    if (__builtin_amdgcn_ballot_w64(more) == 0) return;
    if (more) {
        const uint4* src = (const uint4*)(arena + off);
#pragma unroll
        for (uint32_t j = 3; j < 6; ++j) *(uint4*)(b + 16u * j) = ld16<0>(16u * j < len ? src + j : g_zero_line);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
}

// A table of n4 16-byte pieces into LDS, once per workgroup: every thread takes part and the caller's
// __syncthreads() follows. Four loads in flight per lane (the index clamped, not branched).
DEV void stage_to_lds(uint4* dst, const uint4* src, uint32_t n4) {
    for (uint32_t i0 = 0; i0 < n4; i0 += 4u * kBlock) {
        uint4 t[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = i0 + j * kBlock + threadIdx.x;
            t[j] = src[i < n4 ? i : n4 - 1u];
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = i0 + j * kBlock + threadIdx.x;
            if (i < n4) dst[i] = t[j];
        }
    }
}

// ---- flow-key extract + hash -----------------------------------------------
// PacketClassifier::extract_flow_key + hash_flow (packet_classifier.cpp:12-108) on the first 96
// bytes of each frame (every field the key reads lies below byte 82: l2 18 + IHL 60 + 4 port bytes).
// hash_flow's byte-wise XOR at shift (i % 4) * 8 is the XOR of little-endian dwords.
static_assert(sizeof(nfcs_flow_key) == 64, "nfcs_flow_key is a 64-byte record");

// A wave takes 64 packets. Their header bytes 0..95 are loaded in 8-lane rows — one coalesced
// 128-byte line per packet, 8 packets per instruction, 8 instructions in flight — and written to
// LDS (96 bytes per packet); then lane l parses packet l on its own, reading the fields at their
// (802.1Q- and IHL-dependent) byte offsets from LDS, so one VALU instruction serves 64 packets and
// no DPP broadcast is needed (round 2's form parsed in 8-lane rows: 909 VALU + 539 SALU per 32
// packets, 0.77 against 0.82 now); the 64-byte records go back through LDS so each global store
// writes 1 KB of consecutive records.
DEV uint32_t lds_u8(const uint8_t* b, uint32_t o) { return b[o]; }
DEV uint32_t lds_be16(const uint8_t* b, uint32_t o) { return ((uint32_t)b[o] << 8) | b[o + 1]; }
DEV uint32_t lds_le32(const uint8_t* b, uint32_t o) {  // any alignment, 2-byte pieces where it can
    if ((o & 1u) == 0) return (uint32_t)*(const uint16_t*)(b + o) | ((uint32_t)*(const uint16_t*)(b + o + 2) << 16);
    return (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24);
}

constexpr uint32_t kFkRow = 96;  // LDS bytes per packet: header bytes 0..95

__global__ __launch_bounds__(kBlock) void flow_keys_lanes_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                                 uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                                 uint64_t arena_bytes, nfcs_flow_key* __restrict__ keys,
                                                                 uint32_t* __restrict__ hashes) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * 64 * kFkRow];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const LanePkt lp = lane_pkt(desc, n, nblocks, arena_bytes);
    const uint64_t p0 = lp.p0, p = lp.p;
    if (p0 >= n) return;
    uint8_t* rows = lds + wave * 64u * kFkRow;
    const bool live = lp.live;
    const uint32_t len = lp.len;
    // Header bytes 0..47 hold every field of an IPv4 header without options, tagged or not, and its
    // ports. A frame starting up to 80 bytes into a 128-byte line reads that one line (64-byte starts:
    // one line instead of two; round 3). Headers reaching past byte 47 (IPv6, IPv4 options) load chunks
    // 3..5 afterwards, lane by lane. The header lines load non-temporally (round 5, calls rotating
    // over fresh batches, same box: 0.0385-0.0390 against 0.0411-0.0414 ms per 1M C1 frames; `sc1` /
    // `sc0 sc1` loads measured as the default; profiles/r05_flowkey_load_policy_ab.jsonl).
    uint4 c[8];
    hdr_rows_load(arena, lp.d.x, len, lane, c);
    hdr_rows_store<kFkRow>(rows, lane, c);
    // lane l parses packet l (extract_flow_key + hash_flow, packet_classifier.cpp:12-108)
    uint8_t* b = rows + lane * kFkRow;
    {  // the bytes the key reads end at the ports (IPv4: l2 + IHL*4 + 4; IPv6: l2 + 44)
        const uint32_t f12 = lds_be16(b, 12), ft = f12 == 0x8100u ? 4u : 0u;
        const uint32_t fet = (f12 == 0x8100u && len >= 18) ? lds_be16(b, 16) : f12;
        const uint32_t need = (fet == 0x0800u && 34u + ft <= len) ? 18u + ft + (lds_u8(b, 14u + ft) & 15u) * 4u
                            : (fet == 0x86DDu && 54u + ft <= len) ? 58u + ft : 0u;
        hdr_late_chunks(b, arena, lp.off, len, len >= 14 && need > 48u && len > 48u);
    }
    const bool eth = len >= 14;
    const uint32_t m0 = eth ? *(const uint32_t*)b : 0u, m1 = eth ? *(const uint32_t*)(b + 4) : 0u;
    const uint32_t m2 = eth ? *(const uint32_t*)(b + 8) : 0u;
    const uint32_t e12 = lds_be16(b, 12);
    const bool tagged = e12 == 0x8100u;
    uint32_t et = eth ? e12 : 0u, vlan = 0;
    if (eth && tagged && len >= 18) {  // has_vlan / vlan_id / vlan() (packet.hpp:603-618)
        vlan = lds_be16(b, 14) & 0x0FFFu;
        et = lds_be16(b, 16);
    }
    const uint32_t sh = tagged ? 4u : 0u;  // l2 = 18 after a tag (ethernet(), packet.hpp:410)
    const bool v4 = et == 0x0800u, v6 = et == 0x86DDu;
    uint32_t proto = 0, sp = 0, dp = 0, s4 = 0, d4 = 0, l4 = 0;
    uint32_t s6[4] = {0, 0, 0, 0}, d6[4] = {0, 0, 0, 0};
    bool hdr = false;
    if (v4 && 34u + sh <= len) {  // ipv4() present
        s4 = __builtin_bswap32(lds_le32(b, 26u + sh));
        d4 = __builtin_bswap32(lds_le32(b, 30u + sh));
        proto = lds_u8(b, 23u + sh);
        l4 = 14u + (lds_u8(b, 14u + sh) & 15u) * 4u;
        hdr = true;
    } else if (v6 && 54u + sh <= len) {  // ipv6() present
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            s6[j] = lds_le32(b, 22u + sh + 4u * j);
            d6[j] = lds_le32(b, 38u + sh + 4u * j);
        }
        proto = lds_u8(b, 20u + sh);
        l4 = 54u;
        hdr = true;
    }
    // tcp() needs l4 + 19 <= len (19-byte TcpHeader), udp() l4 + 8 (packet.hpp:473-535)
    if (hdr && ((proto == 6 && l4 + sh + 19u <= len) || (proto == 17 && l4 + sh + 8u <= len))) {
        sp = lds_be16(b, l4 + sh);
        dp = lds_be16(b, l4 + sh + 2u);
    }
    uint32_t hv = m0 ^ (m1 & 0xFFFFu) ^ ((m1 >> 16) | (m2 << 16)) ^ (m2 >> 16);
    hv ^= vlan ^ (et << 16);
    if (v6) hv ^= s6[0] ^ s6[1] ^ s6[2] ^ s6[3] ^ d6[0] ^ d6[1] ^ d6[2] ^ d6[3];
    else hv ^= s4 ^ d4;
    hv ^= proto ^ (sp << 16) ^ dp;
    if (!live) hv = 0;
    if (hashes && p < n) hashes[p] = hv;
    if (!keys) return;
    // the record (nfcs_flow_key: hash, vlan, ethertype, MACs, ports, addresses) into this lane's LDS row, then 1 KB of
    // consecutive records per store instruction
    uint4* rec = (uint4*)(rows + lane * kFkRow);
    __builtin_amdgcn_wave_barrier();
    rec[0] = make_uint4(hv, vlan | (et << 16), (m1 >> 16) | (m2 << 16), (m2 >> 16) | (m0 << 16));
    rec[1] = make_uint4((m0 >> 16) | (m1 << 16), proto | ((v6 ? 1u : 0u) << 8) | (sp << 16), dp, 0u);
    rec[2] = v6 ? make_uint4(s6[0], s6[1], s6[2], s6[3]) : make_uint4(s4, 0u, 0u, 0u);
    rec[3] = v6 ? make_uint4(d6[0], d6[1], d6[2], d6[3]) : make_uint4(d4, 0u, 0u, 0u);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t q = 16u * j + (lane >> 2);  // packet of this 16-byte piece
        const uint4 v = *(const uint4*)(rows + q * kFkRow + 16u * (lane & 3u));
        // plain (write-back) stores: the L2 merges each 1 KB into whole lines (round 5, calls
        // rotating over fresh batches, same box: 0.0352-0.0355 against 0.0387-0.0392 ms per 1M C1
        // frames with non-temporal ones; profiles/r05_store_policy_ab.jsonl)
        if (p0 + q < n) *((uint4*)(keys + p0 + q) + (lane & 3u)) = v;
    }
}

hipError_t launch_flow_keys(const DevInfo& di, const uint8_t* arena, uint64_t arena_bytes,
                            const nfcs_desc* desc, uint32_t n, nfcs_flow_key* keys,
                            uint32_t* hashes, hipStream_t stream) {
    (void)di;
    if (n == 0) return hipSuccess;
    // 64 packets per wave, one lane each (round 3: C1 0.77 -> 0.82 against round 2's 8-lane rows of
    // 4 slots; profiles/r03_s2_ab_flowkey_lanes.jsonl); write-back record stores, XCD-aware order
    const uint32_t g = lane_blocks(n);
    hipLaunchKernelGGL(flow_keys_lanes_kernel, dim3(g), dim3(kBlock), 0, stream, desc, n, g, arena, arena_bytes, keys,
                       hashes);
    return hipGetLastError();
}

// ---- route + ARP lookup in front of the fused forward -------------------------
// The switch's L3 decision (switch.hpp:259-301) per packet: lane_pkt, header bytes 0..47 (every byte the
// decision reads lies below 38) by hdr_rows_load / hdr_rows_store, and lane l decides packet l from LDS. The
// {network, mask} pairs of the routes are staged once per workgroup in LDS behind the header rows
// (stage_to_lds, issued between the rows' loads and their store) and scanned in lookup order by
// a wave-uniform loop: every lane reads the same pair (an LDS broadcast, no bank conflict), kRtGroup
// pairs per trip, and the wave leaves the loop once each of its lanes has its first match
// (RoutingManager::lookup_route, routing_manager.cpp:80-92). ARP entries and the switch's own
// addresses are ascending u32 arrays in global memory, searched per lane.
constexpr uint32_t kRtRow = 48;  // LDS bytes per packet: header bytes 0..47
constexpr uint32_t kRtRowsBytes = kWavesPerBlock * 64u * kRtRow;

DEV uint32_t dev_find(const uint32_t* __restrict__ a, uint32_t n, uint32_t key) {  // nfcs_fib.h fib_find
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return (lo < n && a[lo] == key) ? lo : NFCS_NH_NONE;
}

__global__ __launch_bounds__(kBlock) void route_lookup_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                              uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                              uint64_t arena_bytes, const FibDev fib,
                                                              uint32_t* __restrict__ nh_out,
                                                              uint32_t* __restrict__ if_out,
                                                              uint8_t* __restrict__ verdict_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rt_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const LanePkt lp = lane_pkt(desc, n, nblocks, arena_bytes);
    const uint64_t p0 = lp.p0, p = lp.p;
    uint8_t* rows = rt_lds + wave * 64u * kRtRow;
    const bool live = lp.live;
    const uint32_t len = lp.len;
    uint4 c[8];
    if (p0 < n) hdr_rows_load(arena, lp.d.x, len, lane, c);
    // the routes' {network, mask} pairs, two per 16-byte piece, once per workgroup (every wave of the
    // workgroup takes part, also one past n: it leaves after the barrier)
    stage_to_lds((uint4*)(rt_lds + kRtRowsBytes), (const uint4*)fib.rt_nm, fib.routes_padded / 2u);
    __syncthreads();
    if (p0 >= n) return;
    hdr_rows_store<kRtRow>(rows, lane, c);
    // lane l decides packet l. The forward's predicate (row_process above): L3 EtherType after at
    // most one tag, ipv4() present
    const uint8_t* b = rows + lane * kRtRow;
    const uint32_t e12 = lds_be16(b, 12);
    const bool tagged = e12 == 0x8100u;
    const uint32_t l3t = len < 14 ? 0u : (tagged ? (len >= 18 ? lds_be16(b, 16) : e12) : e12);
    const bool v4 = live && l3t == 0x0800u && (tagged ? 38u : 34u) <= len;
    const uint32_t sh = tagged ? 4u : 0u;
    const uint32_t ttl = lds_u8(b, 22u + sh);
    const uint32_t dst = lds_le32(b, 30u + sh);  // network byte order as a u32: the reference's IpAddress
    const bool local = v4 && dev_find(fib.local_ip, fib.locals, dst) != NFCS_NH_NONE;  // is_my_ip (270)
    const bool need = v4 && !local && ttl > 1;  // lookup_route runs (282)
    const uint2* rt = (const uint2*)(rt_lds + kRtRowsBytes);
    uint32_t match = NFCS_NH_NONE;
    for (uint32_t i = 0; i < fib.routes_padded; i += kRtGroup) {
        if (__builtin_amdgcn_ballot_w64(need && match == NFCS_NH_NONE) == 0) break;
        uint32_t m = NFCS_NH_NONE;
#pragma unroll
        for (uint32_t j = kRtGroup; j-- > 0;) {  // descending, so the first pair in order wins
            const uint2 e = rt[i + j];
            m = ((dst & e.y) == e.x) ? i + j : m;
        }
        match = match == NFCS_NH_NONE ? m : match;
    }
    uint32_t v = !live ? (uint32_t)NFCS_RT_BAD_DESC
               : !v4   ? (uint32_t)NFCS_RT_NOT_IPV4
               : local ? (uint32_t)NFCS_RT_LOCAL
                       : (uint32_t)NFCS_RT_TTL_EXPIRED;
    uint32_t nh = NFCS_NH_NONE, eif = NFCS_IF_NONE;
    if (need) {
        v = NFCS_RT_NO_ROUTE;
        if (match != NFCS_NH_NONE) {  // match < fib.routes: the padding pairs match nothing
            const uint2 info = fib.rt_info[match];  // the gateway, or ARP for the destination itself (285-292)
            v = fib_route_word(info.x, fib.arp_ip, fib.arp_nh, fib.arps, dst, &nh);
            if (v == NFCS_RT_FORWARD) eif = info.y;
        }
    }
    if (p < n) {  // one packet per lane: each store instruction writes consecutive elements
        nh_out[p] = nh;
        if (if_out) if_out[p] = eif;
        if (verdict_out) verdict_out[p] = (uint8_t)v;
    }
}

hipError_t launch_route_lookup(const DevInfo& di, const FibDev& fib, const uint8_t* arena, uint64_t arena_bytes,
                               const nfcs_desc* desc, uint32_t n, uint32_t* nh, uint32_t* egress_if,
                               uint8_t* verdict, hipStream_t stream) {
    (void)di;
    if (n == 0) return hipSuccess;
    // 64 packets per wave, one lane each, XCD-aware order; LDS: the header rows, then the pairs
    const uint32_t g = lane_blocks(n);
    const unsigned lds = kRtRowsBytes + fib.routes_padded * 8u;
    hipLaunchKernelGGL(route_lookup_kernel, dim3(g), dim3(kBlock), lds, stream, desc, n, g, arena, arena_bytes, fib,
                       nh, egress_if, verdict);
    return hipGetLastError();
}

// ---- ACL evaluation in front of the lookup and the forward --------------------
// AclManager::evaluate (acl_manager.cpp:161-278) per packet: lane_pkt, header bytes 0..47 by hdr_rows_load /
// hdr_rows_store (96 bytes of LDS per packet; headers whose ports lie past byte 47 — IPv4 options — take
// hdr_late_chunks), and lane l folds every field check_match can read into a key of eight dwords
// (acl_key_lds). The compiled rules {value[8], mask[8]} are staged once per workgroup in LDS behind the
// header rows (stage_to_lds) and scanned in the given order by a wave-uniform loop of acl_scan_trip:
// kAclGroup rules per trip folded last to first so the first in order wins, one ballot per trip, and the
// wave leaves the loop once each of its live lanes has its match. A trip reads the rules' address / port /
// protocol halves first and their MAC / VLAN / EtherType halves only when one of its rules tests those
// (half the LDS traffic for a list of address and port rules).
constexpr uint32_t kAclRowsBytes = kWavesPerBlock * 64u * kFkRow;
static_assert(kAclRowsBytes + NFCS_ACL_MAX_RULES * sizeof(AclRec) < 64u * 1024u,
              "header rows + rules stay under 64 KiB of dynamic LDS (no opt-in needed)");

// Lane l's key from its packet's LDS row b (kFkRow bytes, chunks 0..2 present): nfcs_acl.h acl_key with the
// same bounds, read in 2-byte pieces. Loads the late chunks where the ports need them, so every lane of the
// wave calls it; len is 0 for a packet that is not read.
DEV void acl_key_lds(uint8_t* b, const uint8_t* __restrict__ arena, uint64_t off, uint32_t len, uint32_t (&key)[8]) {
    const uint32_t e12 = lds_be16(b, 12);
    const bool eth = len >= 14, tagged = e12 == 0x8100u;
    const uint32_t sh = tagged ? 4u : 0u;  // l2 = 18 behind a tag
    const bool known = eth && (!tagged || len >= 18);
    const uint32_t et = !known ? 0u : tagged ? lds_be16(b, 16) : e12;
    const bool v4 = known && et == 0x0800u && 34u + sh <= len;  // ipv4() present
    const uint32_t l4 = 14u + sh + (lds_u8(b, 14u + sh) & 15u) * 4u;
    // the ports end at l4 + 4: past byte 47 only with IPv4 options (IHL >= 8; 7 behind a tag)
    hdr_late_chunks(b, arena, off, len, v4 && l4 + 4u > 48u && len > 48u);
    key[kAkMac0] = eth ? *(const uint32_t*)b : 0u;
    key[kAkMac1] = eth ? *(const uint32_t*)(b + 4) : 0u;
    key[kAkMac2] = eth ? *(const uint32_t*)(b + 8) : 0u;
    const bool has_vid = eth && tagged && len >= 18;
    key[kAkL2] = (has_vid ? lds_be16(b, 14) & 0x0FFFu : 0u) | (et << 16);
    uint32_t meta = (eth ? kApEth : 0u) | (has_vid ? kApVlan : 0u) | (known ? kApEtype : 0u);
    uint32_t sip = 0, dip = 0, ports = 0;
    if (v4) {
        sip = __builtin_bswap32(lds_le32(b, 26u + sh));  // ntohl: AclRule holds host order
        dip = __builtin_bswap32(lds_le32(b, 30u + sh));
        const uint32_t proto = lds_u8(b, 23u + sh);
        meta |= kApIpv4 | proto;
        // tcp() needs l4 + 19 <= len (19-byte TcpHeader), udp() l4 + 8 (packet.hpp:473-541)
        if ((proto == 6 && l4 + 19u <= len) || (proto == 17 && l4 + 8u <= len)) {
            meta |= kApPorts;
            ports = lds_be16(b, l4) | (lds_be16(b, l4 + 2u) << 16);
        }
    }
    key[kAkSrcIp] = sip;
    key[kAkDstIp] = dip;
    key[kAkPorts] = ports;
    key[kAkMeta] = meta;
}

// One trip of the scan over rules i .. i + kAclGroup - 1 of rec (LDS; the same rules for every lane, so the
// reads are broadcasts and the branch is uniform): the first of them in order that the key matches —
// ((key ^ value) & mask) == 0 over the eight dwords — or NFCS_ACL_NO_MATCH. Dwords 4..7 (addresses, ports,
// protocol and presence bits) of the trip's rules first; dwords 0..3 (MACs, VLAN id, EtherType) only when
// one of these rules tests them, which its mask says in a bit no key has (kApNeedL2).
DEV uint32_t acl_scan_trip(const uint4* rec, uint32_t i, const uint32_t (&key)[8]) {
    uint32_t d[kAclGroup], l2 = 0;
#pragma unroll
    for (uint32_t j = 0; j < kAclGroup; ++j) {
        const uint4* e = rec + (i + j) * 4u;
        const uint4 v1 = e[1], m1 = e[3];
        d[j] = (key[4] ^ v1.x) & m1.x;
        d[j] |= (key[5] ^ v1.y) & m1.y;
        d[j] |= (key[6] ^ v1.z) & m1.z;
        d[j] |= (key[7] ^ v1.w) & m1.w;
        l2 |= m1.w;
    }
    if (rfl(l2) & kApNeedL2) {
#pragma unroll
        for (uint32_t j = 0; j < kAclGroup; ++j) {
            const uint4* e = rec + (i + j) * 4u;
            const uint4 v0 = e[0], m0 = e[2];
            d[j] |= (key[0] ^ v0.x) & m0.x;
            d[j] |= (key[1] ^ v0.y) & m0.y;
            d[j] |= (key[2] ^ v0.z) & m0.z;
            d[j] |= (key[3] ^ v0.w) & m0.w;
        }
    }
    uint32_t m = NFCS_ACL_NO_MATCH;
#pragma unroll
    for (uint32_t j = kAclGroup; j-- > 0;) m = d[j] == 0 ? i + j : m;  // descending: the first rule in order wins
    return m;
}

__global__ __launch_bounds__(kBlock) void acl_eval_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                          uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                          uint64_t arena_bytes, const AclDev acl,
                                                          uint8_t* __restrict__ action_out,
                                                          uint32_t* __restrict__ rule_out,
                                                          uint32_t* __restrict__ redirect_out,
                                                          uint32_t* __restrict__ nh_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t acl_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const LanePkt lp = lane_pkt(desc, n, nblocks, arena_bytes);
    const uint64_t p0 = lp.p0, p = lp.p;
    uint8_t* rows = acl_lds + wave * 64u * kFkRow;
    const bool live = lp.live;
    uint4 c[8];
    if (p0 < n) hdr_rows_load(arena, lp.d.x, lp.len, lane, c);
    // the compiled rules, four 16-byte pieces each, once per workgroup (every wave of the workgroup
    // takes part, also one past n: it leaves after the barrier)
    stage_to_lds((uint4*)(acl_lds + kAclRowsBytes), acl.rec, acl.rules_padded * 4u);
    __syncthreads();
    if (p0 >= n) return;
    hdr_rows_store<kFkRow>(rows, lane, c);
    uint32_t key[8];
    acl_key_lds(rows + lane * kFkRow, arena, lp.off, lp.len, key);
    const uint4* rec = (const uint4*)(acl_lds + kAclRowsBytes);
    uint32_t match = NFCS_ACL_NO_MATCH;
    for (uint32_t i = 0; i < acl.rules_padded; i += kAclGroup) {
        if (__builtin_amdgcn_ballot_w64(live && match == NFCS_ACL_NO_MATCH) == 0) break;
        const uint32_t m = acl_scan_trip(rec, i, key);
        match = match == NFCS_ACL_NO_MATCH ? m : match;
    }
    uint32_t action = live ? NFCS_ACL_PERMIT : NFCS_ACL_BAD_DESC, redirect = NFCS_IF_NONE;
    if (live && match != NFCS_ACL_NO_MATCH) {  // match < acl.rules: the padding rules match nothing
        const uint2 a = acl.act[match];
        action = a.x;
        redirect = a.y;
    }
    if (!live) match = NFCS_ACL_NO_MATCH;
    if (p < n) {  // one packet per lane: each store instruction writes consecutive elements
        action_out[p] = (uint8_t)action;
        if (rule_out) rule_out[p] = match;
        if (redirect_out) redirect_out[p] = redirect;
        if (nh_out && action != NFCS_ACL_PERMIT) nh_out[p] = NFCS_NH_NONE;  // a predicated store, no read
    }
}

hipError_t launch_acl_eval(const DevInfo& di, const AclDev& acl, const uint8_t* arena, uint64_t arena_bytes,
                           const nfcs_desc* desc, uint32_t n, uint8_t* action, uint32_t* rule, uint32_t* redirect,
                           uint32_t* nh, hipStream_t stream) {
    (void)di;
    if (n == 0) return hipSuccess;
    // 64 packets per wave, one lane each, XCD-aware order; LDS: the header rows, then the rules
    const uint32_t g = lane_blocks(n);
    const unsigned lds = kAclRowsBytes + acl.rules_padded * (unsigned)sizeof(AclRec);
    hipLaunchKernelGGL(acl_eval_kernel, dim3(g), dim3(kBlock), lds, stream, desc, n, g, arena, arena_bytes, acl, action,
                       rule, redirect, nh);
    return hipGetLastError();
}

// ---- Egress ACLs: the list chosen per packet by its egress port -----------------
// The ACL stage's functions (lane_pkt; hdr_rows_load / hdr_rows_store; acl_key_lds; every rule staged once
// per workgroup behind the header rows by stage_to_lds), with the rule list taken from the packet's egress
// port: lane l gathers its port's binding {first rule, padded count} (the binding array is
// small and reused: default cache policy). A lane whose packet needs no scan — no port, a descriptor
// outside the arena, a port without a list — requests no frame bytes (its row loads read the zero line), and
// a wave without any scan skips rows, keys and scan. The scan is a waterfall over the lists present in the
// wave: take the binding of the first pending lane (readfirstlane), run the wave-uniform scan (acl_scan_trip)
// over that list's range for the lanes bound to it, retire them, repeat. Every list is scanned at most once
// per wave, and a wave whose packets all leave by one port runs exactly the single-list loop.
// Deny counters: the denied lanes of a wave are grouped by port (the same waterfall), each group's lengths
// are summed in a 64-bit LDS slot of its first lane. The four waves' groups then meet in a table of kBlock
// entries {port, packets, bytes} in LDS (in the header rows, which no wave needs any more behind a barrier;
// open addressing, at most kBlock distinct ports, so every port finds an entry within kBlock probes), and
// one thread per occupied entry adds it to the port's two slots of the workgroup's stripe of the counter
// scratch (nfcs_internal.h): one pair of global atomics per distinct denied port per workgroup, spread over
// kCtAclStripes addresses per counter; counter_fold_kernel behind the launch moves the sums to the caller's
// arrays. A workgroup without a denied packet leaves at the first of these barriers.
constexpr uint32_t kEaSlotsBytes = kWavesPerBlock * 64u * 8u + 16u;  // one u64 per lane, and the workgroup's flag
constexpr uint32_t kEaTableBytes = kBlock * 16u;                     // u32 port, u32 packets, u64 bytes per entry
static_assert(kEaTableBytes <= kAclRowsBytes, "the table lies in the header rows");
static_assert(kAclRowsBytes + kEaSlotsBytes + NFCS_ACL_MAX_RULES * sizeof(AclRec) < 64u * 1024u,
              "header rows + sum slots + rules stay under 64 KiB of dynamic LDS (no opt-in needed)");

// The fold behind a counting kernel (nfcs_internal.h): thread j sums slot j of the S stripes (`stride` slots
// apart), stores zero where it read something else, and adds a non-zero sum to the caller's counter with one
// atomic: out64[j], or with out32 (the egress ACL's pairs) out32[j / 2] for an even j and out64[j / 2] for an
// odd one. The loads and stores are 8-byte agent-scope accesses, as the adds into the stripes are.
template <uint32_t S>
__global__ __launch_bounds__(kBlock) void counter_fold_kernel(unsigned long long* __restrict__ stripes, uint32_t stride,
                                                              uint32_t slots, unsigned long long* __restrict__ out64,
                                                              uint32_t* __restrict__ out32) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= slots) return;
    unsigned long long v[S], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < S; ++k)
        v[k] = __hip_atomic_load(stripes + (uint64_t)k * stride + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (uint32_t k = 0; k < S; ++k) {
        if (v[k]) __hip_atomic_store(stripes + (uint64_t)k * stride + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sum += v[k];
    }
    if (!sum) return;
    if (!out32)
        atomicAdd(out64 + j, sum);
    else if (j & 1u)
        atomicAdd(out64 + (j >> 1), sum);
    else
        atomicAdd(out32 + (j >> 1), (uint32_t)sum);  // a stripe's packets fit 32 bits, and the counter wraps as before
}

template <uint32_t S>
void launch_counter_fold(uint64_t* stripes, uint32_t stride, uint32_t slots, uint64_t* out64, uint32_t* out32,
                         hipStream_t stream) {
    hipLaunchKernelGGL(counter_fold_kernel<S>, dim3((slots + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream,
                       (unsigned long long*)stripes, stride, slots, (unsigned long long*)out64, out32);
}

__global__ __launch_bounds__(kBlock) void egress_acl_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                            uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                            uint64_t arena_bytes, uint32_t* __restrict__ port_io,
                                                            const AclSetDev set, uint8_t* __restrict__ action_out,
                                                            uint32_t* __restrict__ rule_out,
                                                            uint32_t* __restrict__ redirect_out,
                                                            unsigned long long* __restrict__ ct, uint32_t ct_stride,
                                                            const uint32_t* __restrict__ item_src,
                                                            const uint8_t* __restrict__ bypass, uint32_t n_src) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ea_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const LanePkt lp = lane_pkt(desc, n, nblocks, arena_bytes);
    const uint64_t p0 = lp.p0, p = lp.p;
    const uint2 dl = lp.d;
    uint8_t* rows = ea_lds + wave * 64u * kFkRow;
    // lane l: the port of packet p0 + l (a coalesced load), then its port's binding
    uint32_t port = NFCS_IF_NONE;
    if (p < n) port = port_io[p];
    const bool has_port = port != NFCS_IF_NONE;  // false past n; without a port the descriptor means nothing
    // an item of a redirected frame bypasses the ACL (switch.hpp:238-240): it keeps its port unread and uncounted
    bool byp = false;
    if (item_src && has_port) {
        const uint32_t src = item_src[p];
        if (src < n_src) byp = bypass[src] != 0;
    }
    const bool live = lp.live && has_port && !byp;
    uint2 bind = make_uint2(0u, 0u);
    if (live && port < set.ports) bind = set.bind[port];
    const bool scan = bind.y != 0u;  // the frame is read only for these
    const uint32_t len = scan ? dl.y : 0u;
    const bool any = __builtin_amdgcn_ballot_w64(scan) != 0;  // wave-uniform
    uint4 c[8];
    if (any) hdr_rows_load(arena, dl.x, len, lane, c);
    // every list's compiled rules, four 16-byte pieces each, once per workgroup (every wave of the
    // workgroup takes part, also one past n or without a scan: it reaches the barrier)
    stage_to_lds((uint4*)(ea_lds + kAclRowsBytes + kEaSlotsBytes), set.rec, set.rules_padded * 4u);
    uint32_t* wg_denied = (uint32_t*)(ea_lds + kAclRowsBytes + kEaSlotsBytes - 16u);
    if (ct && threadIdx.x == 0) *wg_denied = 0u;
    __syncthreads();
    if (!ct && p0 >= n) return;  // a counting wave past n has no scan and no denied lane, and reaches the barriers
    uint32_t match = NFCS_ACL_NO_MATCH;  // an index into the one array
    if (any) {
        hdr_rows_store<kFkRow>(rows, lane, c);
        uint32_t key[8];
        acl_key_lds(rows + lane * kFkRow, arena, lp.off, len, key);  // len is 0 without a scan
        // the waterfall: one wave-uniform scan per list present in the wave
        const uint4* rec = (const uint4*)(ea_lds + kAclRowsBytes + kEaSlotsBytes);
        bool pending = scan;
        while (__builtin_amdgcn_ballot_w64(pending) != 0) {
            if (pending) {  // among the pending lanes, the first one's list (lists are disjoint, non-empty ranges)
                const uint32_t first = rfl(bind.x), end = first + rfl(bind.y);
                const bool mine = bind.x == first;
                for (uint32_t i = first; i < end; i += kAclGroup) {
                    if (__builtin_amdgcn_ballot_w64(mine && match == NFCS_ACL_NO_MATCH) == 0) break;
                    const uint32_t m = acl_scan_trip(rec, i, key);
                    match = (mine && match == NFCS_ACL_NO_MATCH) ? m : match;
                }
                if (mine) pending = false;
            }
        }
    }
    uint32_t action = !has_port ? NFCS_ACL_NO_PORT : byp ? NFCS_ACL_BYPASS : live ? NFCS_ACL_PERMIT : NFCS_ACL_BAD_DESC;
    uint32_t redirect = NFCS_IF_NONE, rule = NFCS_ACL_NO_MATCH;
    if (match != NFCS_ACL_NO_MATCH) {  // a scanned lane; match < set.rules_padded and no padding rule matches
        const uint2 a = set.act[match];
        action = a.x;
        redirect = a.y;
        rule = match - bind.x;
    }
    const bool denied = action == NFCS_ACL_DENY;
    if (p < n) {  // one packet per lane: each store instruction writes consecutive elements
        action_out[p] = (uint8_t)action;
        if (rule_out) rule_out[p] = rule;
        if (redirect_out) redirect_out[p] = redirect;
        if (denied || action == NFCS_ACL_BAD_DESC) port_io[p] = NFCS_IF_NONE;  // a predicated store
    }
    if (!ct) return;
    unsigned long long* slot = (unsigned long long*)(ea_lds + kAclRowsBytes) + wave * 64u;
    uint32_t lead = lane, cnt = 0;
    bool leader = false;
    if (__builtin_amdgcn_ballot_w64(denied) != 0) {  // denied lanes had a list: port < set.ports
        bool dp = denied;
        while (__builtin_amdgcn_ballot_w64(dp) != 0) {
            if (dp) {
                const uint32_t lp = rfl(port);  // the first pending lane's port
                if (port == lp) {               // its group
                    const uint64_t grp = __builtin_amdgcn_ballot_w64(true);
                    lead = (uint32_t)__builtin_ctzll(grp);
                    cnt = (uint32_t)__builtin_popcountll(grp);
                    dp = false;
                }
            }
        }
        leader = denied && lead == lane;
        if (leader) slot[lane] = 0ull;
        __builtin_amdgcn_wave_barrier();  // one wave's LDS operations execute in order
        if (denied) atomicAdd(&slot[lead], (unsigned long long)dl.y);
        if (lane == 0) *wg_denied = 1u;
    }
    __syncthreads();  // every wave is done with its header rows
    if (*wg_denied == 0u) return;  // uniform over the workgroup
    uint32_t* t_port = (uint32_t*)ea_lds;
    uint32_t* t_cnt = t_port + kBlock;
    unsigned long long* t_bytes = (unsigned long long*)(t_cnt + kBlock);
    t_port[threadIdx.x] = NFCS_IF_NONE;  // no port: a denied lane's port is below set.ports
    t_cnt[threadIdx.x] = 0u;
    t_bytes[threadIdx.x] = 0ull;
    __syncthreads();
    if (leader) {
        uint32_t h = (port * 0x9E3779B1u) >> 24;  // kBlock = 256 entries
        static_assert(kBlock == 256, "the hash keeps 8 bits");
        for (uint32_t k = 0; k < kBlock; ++k, h = (h + 1u) & (kBlock - 1u)) {  // an entry is free or the port's within kBlock probes
            const uint32_t was = atomicCAS(&t_port[h], (uint32_t)NFCS_IF_NONE, port);
            if (was == NFCS_IF_NONE || was == port) {
                atomicAdd(&t_cnt[h], cnt);
                atomicAdd(&t_bytes[h], slot[lane]);
                break;
            }
        }
    }
    __syncthreads();
    const uint32_t tp = t_port[threadIdx.x];
    if (tp != NFCS_IF_NONE) {
        unsigned long long* to = ct + (uint64_t)(xcd_block_n(nblocks) % kCtAclStripes) * ct_stride + 2u * tp;
        atomicAdd(to, (unsigned long long)t_cnt[threadIdx.x]);
        atomicAdd(to + 1, t_bytes[threadIdx.x]);
    }
}

hipError_t launch_egress_acl(const DevInfo& di, const AclSetDev& set, const uint8_t* arena, uint64_t arena_bytes,
                             const nfcs_desc* desc, uint32_t n, uint32_t* port, uint8_t* action, uint32_t* rule,
                             uint32_t* redirect, uint32_t* denied_pkts, uint64_t* denied_bytes, uint64_t* ct,
                             hipStream_t stream, const uint32_t* item_src, const uint8_t* bypass, uint32_t n_src) {
    (void)di;
    if (n == 0) return hipSuccess;
    if (!item_src || !bypass) item_src = nullptr, bypass = nullptr, n_src = 0;
    if (denied_pkts && !ct) return hipErrorInvalidValue;
    // the stripes of the counter scratch: {packets, bytes} per port, all zero before and after
    uint64_t* stripes = denied_pkts ? ct + kCtAclAt : nullptr;
    const uint32_t stride = ct_acl_stride(set.ports);
    // 64 packets per wave, one lane each, XCD-aware order; LDS: the header rows, the sum slots, then the rules
    const uint32_t g = lane_blocks(n);
    const unsigned lds = kAclRowsBytes + kEaSlotsBytes + set.rules_padded * (unsigned)sizeof(AclRec);
    hipLaunchKernelGGL(egress_acl_kernel, dim3(g), dim3(kBlock), lds, stream, desc, n, g, arena, arena_bytes, port, set,
                       action, rule, redirect, (unsigned long long*)stripes, stride, item_src, bypass, n_src);
    if (stripes && set.ports) launch_counter_fold<kCtAclStripes>(stripes, stride, 2u * set.ports, denied_bytes, denied_pkts, stream);
    return hipGetLastError();
}

// ---- L2 forwarding: FDB lookup, port / VLAN checks, learning -------------------
// The L2 block of the switch (switch.hpp:305-326) per packet: a wave takes 64 packets, one lane each
// (lane_pkt's descriptor load, liveness test and XCD-aware block order, in its own text). Everything the
// block reads of a frame — both MACs, the EtherType and the TCI — lies in bytes 0..15, so lane l loads
// that one 16-byte chunk of packet l itself (non-temporal: the frames are streamed) and no LDS is
// used. The table (nfcs_fdb.h FdbSlot) is probed per lane from global memory with the default cache
// policy (it is the reused data): the destination's and the source's probe sequences advance together,
// two independent 16-byte loads per lane per trip issued from one block, so that both are in flight
// before the first is used. A lane that has finished both searches issues no loads (a wave makes as many
// trips as its slowest lane: with every lane loading on every trip the kernel took up to four times as
// long). The wave leaves the loop once no lane is still searching, after max_probe trips
// at the latest; a lane's search also ends at an empty slot (nfcs_fdb.h fdb_find is the same loop). Every
// slot index is masked into the table. LEARN = false (d_learn NULL) compiles the source probe out.

// One slot of a probe sequence: fdb_find's loop body.
DEV void fdb_step(const uint4& s, uint32_t k0, uint32_t k1, bool& search, bool& hit, uint32_t& port, uint32_t& flags) {
    const bool occ = (s.w & kFdbOccupied) != 0, m = search && occ && s.x == k0 && s.y == k1;
    port = m ? s.z : port;
    flags = m ? s.w : flags;
    hit = hit || m;
    search = search && !m && occ;
}

template <bool LEARN>
__global__ __launch_bounds__(kBlock) void l2_lookup_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                           uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                           uint64_t arena_bytes, const FdbDev fdb, uint32_t ingress,
                                                           const uint8_t* __restrict__ rt_verdict,
                                                           uint32_t* __restrict__ port_out,
                                                           uint8_t* __restrict__ verdict_out,
                                                           uint16_t* __restrict__ vlan_out,
                                                           uint8_t* __restrict__ learn_out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t p0 = ((uint64_t)xcd_block_n(nblocks) * kWavesPerBlock + rfl(wave)) * 64u;
    if (p0 >= n) return;
    // lane_pkt's text, kept here: the descriptor and the route verdict load from one block, so that both are
    // in flight together (through lane_pkt the verdict's load waits for the descriptor's: +0.5-1.5%, §26)
    const uint64_t p = p0 + lane;
    uint2 dl = make_uint2(0u, 0u);
    uint32_t rtv = NFCS_RT_NOT_IPV4;
    if (p < n) {
        dl = ((const uint2*)desc)[p];
        if (rt_verdict) rtv = rt_verdict[p];
    }
    const uint64_t off = (uint64_t)dl.x * 16u;
    const bool live = p < n && off + (((uint64_t)dl.y + 15u) & ~15ull) <= arena_bytes && rtv != NFCS_RT_BAD_DESC;
    const bool mine = live && rtv == NFCS_RT_NOT_IPV4;  // else the L3 block took the packet
    const uint32_t len = mine ? dl.y : 0u;
    const bool eth = len >= 14u;  // the frame's first chunk lies inside the arena: len > 0 and live
    const uint4 c = ld16<1>(eth ? (const uint4*)(arena + off) : g_zero_line);
    // the ingress port's state: wave-uniform
    const bool in_known = ingress < fdb.ports;
    const uint32_t native = in_known ? fdb.port_native[ingress] : kL2DefaultVlan;
    const uint32_t* in_vlans = fdb.port_vlans + (size_t)(in_known ? ingress : 0u) * kL2VlanWords;
    // bytes 12-13 = 0x8100 and len >= 18: TCI & 0x0FFF (Packet::vlan_id), else the native VLAN
    const bool tagged = (c.w & 0xFFFFu) == 0x0081u && len >= 18u;
    const uint32_t vlan = !eth ? 0u : tagged ? (bswap16(c.w >> 16) & 0x0FFFu) : native;
    const uint32_t dk0 = c.x, dk1 = (c.y & 0xFFFFu) | (vlan << 16);
    const uint32_t sk0 = (c.y >> 16) | (c.z << 16), sk1 = (c.z >> 16) | (vlan << 16);
    const uint32_t mask = fdb.slot_mask;
    const uint32_t dh = fdb_hash(dk0, dk1), sh = fdb_hash(sk0, sk1);
    bool dsearch = eth, ssearch = LEARN && eth, dhit = false, shit = false;
    uint32_t dport = 0, dflags = 0, sport = 0, sflags = 0;
    for (uint32_t i = 0; i < fdb.max_probe; ++i) {
        if (__builtin_amdgcn_ballot_w64(dsearch || ssearch) == 0) break;
        uint4 ds = make_uint4(0u, 0u, 0u, 0u), ss = ds;
        if (dsearch || ssearch) {  // one block: both loads are in flight before the first use
            ds = fdb.slots[(dh + i) & mask];
            if (LEARN) ss = fdb.slots[(sh + i) & mask];
        }
        fdb_step(ds, dk0, dk1, dsearch, dhit, dport, dflags);
        if (LEARN) fdb_step(ss, sk0, sk1, ssearch, shit, sport, sflags);
    }
    // on a hit, the || chain of switch.hpp:314-316 in its order
    uint32_t v = !live ? (uint32_t)NFCS_L2_BAD_DESC
               : !mine ? (uint32_t)NFCS_L2_SKIP
               : !eth  ? (uint32_t)NFCS_L2_NO_ETH
                       : (uint32_t)NFCS_L2_FLOOD;
    uint32_t eg = NFCS_IF_NONE;
    if (dhit) {
        const bool known = dport < fdb.ports;  // a port never set: link down
        const uint32_t st = known ? fdb.port_state[dport] : 0u;
        const uint32_t w = vlan >> 5, bit = 1u << (vlan & 31u);  // vlan <= 4095: w < kL2VlanWords
        const uint32_t in_w = in_known ? in_vlans[w] : 0u;
        const uint32_t eg_w = known ? fdb.port_vlans[(size_t)dport * kL2VlanWords + w] : 0u;
        if (dport == ingress) v = NFCS_L2_DROP_SAME_PORT;
        else if (!(st & kL2LinkUp)) v = NFCS_L2_DROP_LINK_DOWN;
        else if (!(st & kL2StpFwd)) v = NFCS_L2_DROP_STP;
        else if (!(in_w & eg_w & bit)) v = NFCS_L2_DROP_VLAN;
        else {
            v = NFCS_L2_FORWARD;
            eg = dport;
        }
    }
    if (p < n) {  // one packet per lane: each store instruction writes consecutive elements
        port_out[p] = eg;
        if (verdict_out) verdict_out[p] = (uint8_t)v;
        if (vlan_out) vlan_out[p] = (uint16_t)vlan;
        if (LEARN) {
            const uint32_t learn = !eth                  ? (uint32_t)NFCS_L2_LEARN_NONE
                                 : !shit                 ? (uint32_t)NFCS_L2_LEARN_NEW
                                 : (sflags & kFdbStatic) ? (uint32_t)NFCS_L2_LEARN_NONE
                                 : sport == ingress      ? (uint32_t)NFCS_L2_LEARN_REFRESH
                                                         : (uint32_t)NFCS_L2_LEARN_MOVED;
            learn_out[p] = (uint8_t)learn;
        }
    }
}

hipError_t launch_l2_lookup(const DevInfo& di, const FdbDev& fdb, uint32_t ingress, const uint8_t* arena,
                            uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n, const uint8_t* rt_verdict,
                            uint32_t* egress_port, uint8_t* verdict, uint16_t* vlan, uint8_t* learn,
                            hipStream_t stream) {
    (void)di;
    if (n == 0) return hipSuccess;
    // 64 packets per wave, one lane each, XCD-aware order; no LDS
    const uint32_t g = lane_blocks(n);
    if (learn)
        hipLaunchKernelGGL(l2_lookup_kernel<true>, dim3(g), dim3(kBlock), 0, stream, desc, n, g, arena, arena_bytes, fdb,
                           ingress, rt_verdict, egress_port, verdict, vlan, learn);
    else
        hipLaunchKernelGGL(l2_lookup_kernel<false>, dim3(g), dim3(kBlock), 0, stream, desc, n, g, arena, arena_bytes, fdb,
                           ingress, rt_verdict, egress_port, verdict, vlan, learn);
    return hipGetLastError();
}

// ---- Egress stage: VLAN egress plan, QoS classify, enqueue ---------------------
// The plan: process_egress and classify_packet_to_queue per packet: a wave takes 64 packets, one lane each
// (lane_pkt). The decision reads frame bytes 12..19, which straddle chunks 0 and 1: the packet's own lane loads
// them with ONE 8-byte load at byte 12 (4-byte aligned, as every frame starts on a 16-byte boundary;
// non-temporal: the frames are streamed), or the 4 bytes 12..15 alone when the frame ends inside chunk 0
// (chunk 1 may then lie outside the arena). Two 16-byte chunk loads, the first form, touched every frame's
// line in two instructions and took 1.77 times the yardstick's time on C1. The port's
// 16-byte record is read with the default cache policy (it is the reused data). No LDS, no loop.
typedef uint32_t u32x2_a4_t __attribute__((ext_vector_type(2), aligned(4)));
DEV EgressRec eg_rec(const EgressDev& eg, uint32_t port, bool want) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);  // a port never set: no VLAN config, no QoS config
    if (want && port < eg.ports) r = eg.recs[port];
    return EgressRec{r.x, r.y, r.z, r.w};
}

__global__ __launch_bounds__(kBlock) void egress_plan_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                             uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                             uint64_t arena_bytes, const EgressDev eg,
                                                             const uint32_t* __restrict__ l3_port,
                                                             const uint8_t* __restrict__ fwd_status,
                                                             const uint32_t* __restrict__ l2_port,
                                                             uint32_t* __restrict__ port_out,
                                                             uint32_t* __restrict__ ops_out,
                                                             uint8_t* __restrict__ queue_out) {
    const LanePkt lp = lane_pkt(desc, n, nblocks, arena_bytes);
    const uint64_t p = lp.p, off = lp.off;
    if (lp.p0 >= n) return;
    // lane l: the ports of packet p0 + l (coalesced loads)
    uint32_t port = NFCS_IF_NONE;
    if (p < n) {
        uint32_t l3 = l3_port ? l3_port[p] : NFCS_IF_NONE;
        if (fwd_status && !(fwd_status[p] & NFCS_ST_FLAG_FWD)) l3 = NFCS_IF_NONE;  // masked by the ACL, TTL expired
        port = l3 != NFCS_IF_NONE ? l3 : l2_port ? l2_port[p] : NFCS_IF_NONE;
    }
    const bool live = lp.live && port != NFCS_IF_NONE;
    const uint32_t len = live ? lp.d.y : 0u;
    const EgressRec r = eg_rec(eg, port, live);
    // bytes 12..15 lie in chunk 0 once the frame has an Ethernet header; chunk 1 lies inside the arena
    // when len > 16 (the descriptor test covers len rounded up to 16)
    uint32_t w3 = 0, w4 = 0;
    if (len > 16u) {
        const u32x2_a4_t t = __builtin_nontemporal_load((const u32x2_a4_t*)(arena + off + 12u));
        w3 = t.x;
        w4 = t.y;
    } else if (len >= 14u) {
        w3 = __builtin_nontemporal_load((const uint32_t*)(arena + off + 12u));
    }
    uint32_t op, q;
    egress_plan_rec(r, len, w3, w4, &op, &q);
    if (p < n) {  // one packet per lane: each store instruction writes consecutive elements
        port_out[p] = live ? port : NFCS_IF_NONE;
        ops_out[p] = live ? op : NFCS_VLAN_NOP;
        queue_out[p] = (uint8_t)(live ? q : NFCS_QUEUE_NONE);
    }
}

hipError_t launch_egress_plan(const DevInfo& di, const EgressDev& eg, const uint8_t* arena, uint64_t arena_bytes,
                              const nfcs_desc* desc, uint32_t n, const uint32_t* l3_port, const uint8_t* fwd_status,
                              const uint32_t* l2_port, uint32_t* port, uint32_t* ops, uint8_t* queue,
                              hipStream_t stream) {
    (void)di;
    if (n == 0) return hipSuccess;
    const uint32_t g = lane_blocks(n);
    hipLaunchKernelGGL(egress_plan_kernel, dim3(g), dim3(kBlock), 0, stream, desc, n, g, arena, arena_bytes, eg, l3_port,
                       fwd_status, l2_port, port, ops, queue);
    return hipGetLastError();
}

// ---- Ingress dispatch: what process_received_packet does between the stages ----------
// A wave takes 64 packets, one lane each (lane_pkt); no loop. The decision is nfcs_switch.h sw_classify, the host
// walk's own function.
// A frame is read only where the ingress link is up, the frame is permitted, its descriptor lies inside the
// arena and it has an Ethernet header: bytes 0..15 with one 16-byte load, and bytes 16..19 (the inner EtherType
// behind a tag, inside the arena once len > 16) with one 4-byte load where len >= 18. Both loads are issued
// together, before anything uses either (a lane that reads nothing loads the zero line), non-temporal: the
// frames are streamed. The redirect port's state byte is gathered by the redirecting lanes only.
// COUNT (d_rx_stats given): packets (one per frame, two per dropped frame) and drops are packed into one
// word, the bytes are 64-bit; both are summed across the wave by xor shuffles, the four wave sums meet in LDS,
// and thread 0 adds the workgroup's sums with at most one 64-bit vector atomic per counter, into the workgroup's
// stripe of the counter scratch (nfcs_internal.h); counter_fold_kernel behind the launch adds the stripes' sums
// to rx_stats[ingress]. With the ingress link down no stripe is touched and the fold adds nothing.
template <bool COUNT>
__global__ __launch_bounds__(kBlock) void ingress_dispatch_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                                  uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                                  uint64_t arena_bytes,
                                                                  const uint8_t* __restrict__ port_state, uint32_t ports,
                                                                  const DispatchArgs a,
                                                                  unsigned long long* __restrict__ ct) {
    __shared__ unsigned long long s_bytes[kWavesPerBlock];
    __shared__ uint32_t s_cnt[kWavesPerBlock];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const LanePkt lp = lane_pkt(desc, n, nblocks, arena_bytes);
    if (!COUNT && lp.p0 >= n) return;  // a counting wave past n reaches the barrier with zeros
    const uint64_t p = lp.p, off = lp.off;
    const bool in = p < n, live = lp.live;
    uint32_t act = NFCS_ACL_PERMIT, red = NFCS_IF_NONE, rt = NFCS_RT_NOT_IPV4, l2v = NFCS_L2_SKIP;
    if (in) {
        if (a.action) act = a.action[p];
        if (a.redirect) red = a.redirect[p];
        rt = a.rt_verdict[p];
        l2v = a.l2_verdict[p];
    }
    // is_port_link_up(ingress_port_id) (215): uniform over the launch
    const bool rx_up = a.ingress < ports && (port_state[a.ingress] & kSwLinkUp) != 0;
    const uint32_t len = lp.d.y;  // counted also where the frame is not read; 0 past n
    const bool rd0 = in && rx_up && sw_reads_head(act, rt, live, len);
    const bool rd1 = in && rx_up && sw_reads_inner(act, rt, live, len);
    const uint4 c = ld16<1>(rd0 ? (const uint4*)(arena + off) : g_zero_line);
    const uint32_t w4 =
        __builtin_nontemporal_load(rd1 ? (const uint32_t*)(arena + off + 16u) : (const uint32_t*)g_zero_line);
    bool red_up = false;  // is_port_link_up(redirect port) (233)
    if (in && act == NFCS_ACL_REDIRECT && red < a.num_ports && red < ports) red_up = (port_state[red] & kSwLinkUp) != 0;
    const uint32_t cls = !rx_up ? (uint32_t)NFCS_SW_RX_DOWN
                                : sw_classify(len, live, act, red, a.num_ports, red_up, rt, l2v, c.x, c.y, c.w, w4);
    if (in) {  // one packet per lane: each store instruction writes consecutive elements (predicated)
        if (sw_masked(cls) || cls == NFCS_SW_RED_OK) {
            a.nh[p] = NFCS_NH_NONE;
            a.l2_port[p] = cls == NFCS_SW_RED_OK ? red : NFCS_IF_NONE;
            a.l2_verdict[p] = (uint8_t)NFCS_L2_SKIP;
        }
        if (a.cls) a.cls[p] = (uint8_t)cls;
        if (a.bypass) a.bypass[p] = (uint8_t)(cls == NFCS_SW_RED_OK);
    }
    if (COUNT) {
        if (!rx_up) return;  // uniform over the launch: nothing is counted (215 returns before 216)
        const uint32_t drop = (in && sw_drop(cls)) ? 1u : 0u;
        const uint32_t pk = in ? 1u + drop : 0u;          // 216, and once more at 228 / 235
        uint32_t cnt = pk | (drop << 16);                 // at most 128 and 64 per wave
        unsigned long long by = (unsigned long long)len * pk;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            cnt += (uint32_t)__shfl_xor((int)cnt, m);
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)by, m);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(by >> 32), m);
            by += ((unsigned long long)hi << 32) | lo;
        }
        if (lane == 0) {
            s_bytes[wave] = by;
            s_cnt[wave] = cnt;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tc = 0;
            unsigned long long tb = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) {
                tc += s_cnt[w];
                tb += s_bytes[w];
            }
            unsigned long long* rx = ct + (xcd_block_n(nblocks) % kCtStripes) * kCtLineSlots;  // the workgroup's stripe
            if (tc & 0xFFFFu) atomicAdd(rx + 0, (unsigned long long)(tc & 0xFFFFu));
            if (tb) atomicAdd(rx + 1, tb);
            if (tc >> 16) atomicAdd(rx + 2, (unsigned long long)(tc >> 16));
        }
    }
}

hipError_t launch_ingress_dispatch(const DevInfo& di, const FdbDev& fdb, const DispatchArgs& a, uint64_t* ct,
                                   hipStream_t stream) {
    (void)di;
    if (a.n == 0) return hipSuccess;
    const uint32_t g = lane_blocks(a.n);
    if (a.rx_stats) {
        if (!ct) return hipErrorInvalidValue;
        static_assert(sizeof(nfcs_rx_stats) == 3u * sizeof(uint64_t), "rx_packets, rx_bytes, rx_drops: the three slots");
        uint64_t* stripes = ct + kCtDispatchAt;
        hipLaunchKernelGGL(ingress_dispatch_kernel<true>, dim3(g), dim3(kBlock), 0, stream, a.desc, a.n, g, a.arena,
                           a.arena_bytes, fdb.port_state, fdb.ports, a, (unsigned long long*)stripes);
        if (a.ingress < fdb.ports)  // else the link reads as down and no stripe was touched
            launch_counter_fold<kCtStripes>(stripes, kCtLineSlots, 3u, (uint64_t*)(a.rx_stats + a.ingress), nullptr, stream);
    } else {
        hipLaunchKernelGGL(ingress_dispatch_kernel<false>, dim3(g), dim3(kBlock), 0, stream, a.desc, a.n, g, a.arena,
                           a.arena_bytes, fdb.port_state, fdb.ports, a, (unsigned long long*)nullptr);
    }
    return hipGetLastError();
}

// The enqueue: a stable partition of the burst by key = port * NFCS_QOS_MAX_QUEUES + queue, clamped by
// each queue's room. Four kernels over tiles of kEgTile consecutive packets, one 64-lane workgroup (one
// wave) per tile, so nothing orders waves inside a tile:
//   1. egress_hist_kernel: the tile's packets per key, counted in LDS (keys words), to hist[tile][key].
//   2. egress_scan_tiles_kernel: per key down the tiles: hist[tile][key] becomes the arrival index of the
//      tile's first packet of that key, total[key] the key's packets. 64 keys x 16 tile segments per
//      workgroup: a segment sums its tiles, the 16 partial sums meet in LDS, the segment writes its prefix.
//   3. egress_scan_keys_kernel (one workgroup): room = max(0, max_depth - depth), enqueued = min(total,
//      room), the exclusive scan of `enqueued` across keys into key_start, depth += enqueued, the drops.
//   4. egress_scatter_kernel: the tile's running count per key in LDS, starting from hist[tile][key]. Per
//      round of 64 packets each lane finds the lanes that hold its key (one ballot per key bit: kbits
//      ballots, a count fixed by the table), its rank among them is a population count of the lower lanes,
//      every lane reads the key's count and the highest lane of each key then adds the key's lanes to it.
//      A packet's arrival index is count + rank; it is enqueued while that is below the key's room, at
//      order[key_start[key] + index]. No position comes from an atomic and no loop ends on data.
// Packets that are not counted (NFCS_EQ_SKIP / DROP_NO_CONFIG / BAD_QUEUE) take no part in a key.
constexpr uint32_t kEgRounds = kEgTile / 64u;  // rounds of 64 packets per tile
DEV uint32_t eg_class_at(const EgressDev& eg, const uint32_t* __restrict__ port, const uint8_t* __restrict__ queue,
                         uint64_t i, uint32_t n, uint32_t* key) {
    if (i >= n) return NFCS_EQ_SKIP;
    const uint32_t pt = port[i], q = queue[i];
    const bool has = pt < eg.ports;  // NFCS_IF_NONE is never below ports (at most NFCS_L2_MAX_PORTS)
    return egress_class(pt, q, has, eg_rec(eg, pt, has), key);
}

__global__ __launch_bounds__(64) void egress_hist_kernel(const uint32_t* __restrict__ port,
                                                         const uint8_t* __restrict__ queue, uint32_t n,
                                                         const EgressDev eg, uint32_t* __restrict__ hist) {
    extern __shared__ uint32_t eg_cnt[];  // eg.keys words
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < eg.keys; k += 64u) eg_cnt[k] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kEgTile;
#pragma unroll 4
    for (uint32_t r = 0; r < kEgRounds; ++r) {
        uint32_t key = 0;
        if (eg_class_at(eg, port, queue, base + r * 64u + lane, n, &key) == NFCS_EQ_ENQUEUED)
            atomicAdd(&eg_cnt[key], 1u);  // key < eg.keys: port < ports, queue < queues <= 8. A count, not a position.
    }
    __syncthreads();
    uint32_t* row = hist + (size_t)blockIdx.x * eg.keys;
    for (uint32_t k = lane; k < eg.keys; k += 64u) row[k] = eg_cnt[k];
}

constexpr uint32_t kEgSegs = 16;  // tile segments per workgroup of egress_scan_tiles_kernel
__global__ __launch_bounds__(64 * kEgSegs) void egress_scan_tiles_kernel(uint32_t* __restrict__ hist, uint32_t tiles,
                                                                         uint32_t keys, uint32_t* __restrict__ total) {
    __shared__ uint32_t part[kEgSegs][64];
    const uint32_t lane = threadIdx.x & 63u, seg = threadIdx.x >> 6;
    const uint32_t key = blockIdx.x * 64u + lane;
    const uint32_t per = (tiles + kEgSegs - 1u) / kEgSegs;
    const uint32_t t0 = min(seg * per, tiles), t1 = min(t0 + per, tiles);
    const bool mine = key < keys;
    uint32_t sum = 0;
    if (mine) {
#pragma unroll 8
        for (uint32_t t = t0; t < t1; ++t) sum += hist[(size_t)t * keys + key];
    }
    part[seg][lane] = sum;
    __syncthreads();
    uint32_t run = 0, all = 0;
#pragma unroll
    for (uint32_t s = 0; s < kEgSegs; ++s) {
        const uint32_t v = part[s][lane];
        run += s < seg ? v : 0u;
        all += v;
    }
    if (!mine) return;
    // eight tiles' counts are loaded before the first prefix is stored: a store to hist keeps the loads behind
    // it from being issued early, and one load per store made this kernel 13-15 us on 1,024 tiles (§16)
    for (uint32_t t = t0; t < t1; t += 8u) {
        uint32_t v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) v[j] = hist[(size_t)min(t + j, t1 - 1u) * keys + key];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            if (t + j < t1) {
                hist[(size_t)(t + j) * keys + key] = run;
                run += v[j];
            }
        }
    }
    if (seg == 0) total[key] = all;
}

constexpr uint32_t kEgScanThreads = 1024;
constexpr uint32_t kEgKeysPerThread = NFCS_L2_MAX_PORTS * NFCS_QOS_MAX_QUEUES / kEgScanThreads;  // 8: every key has a thread
static_assert(kEgKeysPerThread * kEgScanThreads == NFCS_L2_MAX_PORTS * NFCS_QOS_MAX_QUEUES, "one workgroup scans every key");
__global__ __launch_bounds__(kEgScanThreads) void egress_scan_keys_kernel(const EgressDev eg,
                                                                          const uint32_t* __restrict__ total,
                                                                          uint32_t* __restrict__ depth,
                                                                          uint32_t* __restrict__ room,
                                                                          uint32_t* __restrict__ key_start,
                                                                          uint32_t* __restrict__ key_dropped) {
    __shared__ uint32_t scan[kEgScanThreads];
    const uint32_t tid = threadIdx.x;
    // kEgKeysPerThread consecutive keys per thread, read once into registers (clamped loads, so that they are
    // all in flight together) and used again after the scan
    const uint32_t k0 = tid * kEgKeysPerThread, last = eg.keys ? eg.keys - 1u : 0u;
    uint32_t rm[kEgKeysPerThread], tot[kEgKeysPerThread], dep[kEgKeysPerThread];
    uint32_t sum = 0;
    if (eg.keys) {  // with no key at all depth and total may be null: nothing is loaded
#pragma unroll
        for (uint32_t j = 0; j < kEgKeysPerThread; ++j) {
            const uint32_t k = min(k0 + j, last);
            const bool mine = k0 + j < eg.keys;
            const uint32_t cap = eg.recs[k / NFCS_QOS_MAX_QUEUES].w;
            dep[j] = depth[k];
            tot[j] = total[k];
            if (!mine) tot[j] = 0u;
            rm[j] = cap > dep[j] ? cap - dep[j] : 0u;  // size() >= max_queue_depth: no room, no underflow
            sum += min(tot[j], rm[j]);
        }
    }
    scan[tid] = sum;
    __syncthreads();
    for (uint32_t s = 1; s < kEgScanThreads; s *= 2u) {  // inclusive scan over the threads' sums
        const uint32_t v = tid >= s ? scan[tid - s] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    uint32_t run = scan[tid] - sum;
#pragma unroll
    for (uint32_t j = 0; j < kEgKeysPerThread; ++j) {
        const uint32_t k = k0 + j;
        if (k < eg.keys) {
            const uint32_t e = min(tot[j], rm[j]);
            key_start[k] = run;
            run += e;
            depth[k] = dep[j] + e;
            room[k] = rm[j];
            if (key_dropped) key_dropped[k] = tot[j] - e;
        }
    }
    if (tid == kEgScanThreads - 1u) key_start[eg.keys] = scan[tid];
}

__global__ __launch_bounds__(64) void egress_scatter_kernel(const uint32_t* __restrict__ port,
                                                            const uint8_t* __restrict__ queue, uint32_t n,
                                                            const EgressDev eg, uint32_t kbits,
                                                            const uint32_t* __restrict__ hist,
                                                            const uint32_t* __restrict__ room,
                                                            const uint32_t* __restrict__ key_start,
                                                            uint8_t* __restrict__ result,
                                                            uint32_t* __restrict__ order) {
    extern __shared__ uint32_t eg_cnt[];  // eg.keys words: the arrival index of the key's next packet
    const uint32_t lane = threadIdx.x;
    const uint32_t* row = hist + (size_t)blockIdx.x * eg.keys;
    for (uint32_t k = lane; k < eg.keys; k += 64u) eg_cnt[k] = row[k];
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kEgTile, below = (1ull << lane) - 1ull;
    // One pass over the tile's rounds. Splitting it into three unrolled passes (classes and keys; arrival
    // indexes; rooms, starts and stores) with unconditional clamped loads, so that each pass's loads are in
    // flight together, measured 6-15% slower (102 VGPRs).
    for (uint32_t r = 0; r < kEgRounds; ++r) {
        const uint64_t i = base + r * 64u + lane;
        uint32_t key = 0;
        uint32_t c = eg_class_at(eg, port, queue, i, n, &key);
        const bool keyed = c == NFCS_EQ_ENQUEUED;
        // the lanes that hold this lane's key
        uint64_t peers = __builtin_amdgcn_ballot_w64(keyed);
        for (uint32_t b = 0; b < kbits; ++b) {
            const bool bit = (key >> b) & 1u;
            const uint64_t has = __builtin_amdgcn_ballot_w64(keyed && bit);
            peers &= bit ? has : ~has;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below), cnt = (uint32_t)__popcll(peers);
        uint32_t at = 0;
        if (keyed) at = eg_cnt[key];
        __syncthreads();  // one wave: every lane has read before the keys' highest lanes write
        if (keyed && rank + 1u == cnt) eg_cnt[key] = at + cnt;
        __syncthreads();
        if (keyed) {
            const uint32_t a = at + rank;
            if (a < room[key]) {
                const uint32_t pos = key_start[key] + a;
                if (pos < n) order[pos] = (uint32_t)i;  // always true: enqueued packets number at most n
            } else {
                c = NFCS_EQ_DROP_FULL;
            }
        }
        if (result && i < n) result[i] = (uint8_t)c;
    }
}

hipError_t launch_egress_enqueue(const DevInfo& di, const EgressDev& eg, const uint32_t* port, const uint8_t* queue,
                                 uint32_t n, uint32_t* depth, uint8_t* result, uint32_t* order, uint32_t* key_start,
                                 uint32_t* key_dropped, uint32_t* scratch, hipStream_t stream) {
    (void)di;
    if (n == 0) return hipSuccess;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kEgTile - 1u) / kEgTile), keys = eg.keys;
    uint32_t* hist = scratch;
    uint32_t* total = scratch + (size_t)tiles * keys;
    uint32_t* room = total + keys;
    const size_t lds = (size_t)keys * sizeof(uint32_t);  // at most 1024 ports x 8 queues x 4 bytes = 32 KiB
    uint32_t kbits = 0;
    while ((1u << kbits) < keys) ++kbits;
    if (keys) {
        hipLaunchKernelGGL(egress_hist_kernel, dim3(tiles), dim3(64), lds, stream, port, queue, n, eg, hist);
        hipLaunchKernelGGL(egress_scan_tiles_kernel, dim3((keys + 63u) / 64u), dim3(64 * kEgSegs), 0, stream, hist, tiles,
                           keys, total);
    }
    hipLaunchKernelGGL(egress_scan_keys_kernel, dim3(1), dim3(kEgScanThreads), 0, stream, eg, total, depth, room, key_start,
                       key_dropped);
    hipLaunchKernelGGL(egress_scatter_kernel, dim3(tiles), dim3(64), lds, stream, port, queue, n, eg, kbits, hist, room,
                       key_start, result, order);
    return hipGetLastError();
}

// ---- Flood replication: the egress item list and the frame copies ----------------
// nfcs_fdb.h flood_expand is the sequential definition; these kernels equal it bit for bit. Tiles of
// kFloodTile consecutive packets, one 1,024-thread workgroup each, one lane per packet, XCD-aware order:
//   1. flood_count_kernel: per packet (items, copies, flooded, slot bytes) by flood_classify — the
//      descriptor load, the liveness test (sw_desc_live) against copy_base, the plan's port rule, and for a
//      flooded packet the population count of its flood mask (fdb_flood_word over the VLAN's row of the per-VLAN port bitmap, the
//      host walk's function) — summed over the tile into scratch[tile].
//   2. flood_scan_kernel: ONE workgroup of kFloodScanThreads looping over the tile sums, kFloodScanThreads per
//      trip with a running carry (no second level): scratch[tile] becomes the tile's exclusive prefix,
//      scratch[tiles] the burst's totals. The trip count is a function of n alone.
//   3. flood_emit_kernel: flood_classify again, the tile's exclusive scan (shuffles within a wave, LDS across
//      the 16 waves), and from the tile's prefix each packet's first item index k0 and first slot offset b0.
//      Both overflow conditions are monotone in the item index, so a packet's emitted items number
//      e = min(items, cap - k0, room / slot) in closed form. A unicast packet's lane stores its one item. The
//      flooded packets of the tile are compacted into LDS (position: the scan of `flooded`), and 64 rows of 16
//      lanes take them in turn: a row loads up to 6 of its frame's 16-byte chunks per lane ONCE (non-temporal:
//      the frames are streamed; 1,536 bytes per pass, longer frames make further passes) and walks the set
//      bits of the mask — at most port_words words of at most 32 bits, a bound fixed by the table — storing
//      the chunks to each emitted slot, a row's stores to one copy contiguous, and its lane 0 the item record.
//      Every item store has j < e, so k0 + j < items <= cap; every chunk store is also guarded by its slot's
//      end <= arena_bytes. The one packet that holds the cut (or the last packet, when nothing is cut) writes
//      d_totals from its prefix and the scan's last element: no atomic, no accumulation.
//   4. flood_pad_kernel: entries [items, cap) inert.
// No position comes from an atomic and no loop ends on data alone.
#ifndef NFCS_FLOOD_STORE
#define NFCS_FLOOD_STORE VST_NT  // the copies' store policy (measurement builds: VST_PLAIN / VST_WT), §17
#endif
constexpr uint32_t kFloodWaves = kFloodTile / 64u;
constexpr uint32_t kFloodR = 16, kFloodK = 6;  // a copy row: 16 lanes x 6 chunks
constexpr uint32_t kFloodRows = kFloodTile / kFloodR;
constexpr uint32_t kFloodScanThreads = 256;

struct FloodAcc {
    uint32_t items, copies, flooded;
    uint64_t bytes;
};
DEV FloodAcc flood_zero() { return FloodAcc{0u, 0u, 0u, 0ull}; }
DEV FloodAcc flood_add(const FloodAcc& a, const FloodAcc& b) {
    return FloodAcc{a.items + b.items, a.copies + b.copies, a.flooded + b.flooded, flood_sat_add(a.bytes, b.bytes)};
}
DEV FloodAcc flood_shfl_up(const FloodAcc& v, uint32_t d) {
    return FloodAcc{__shfl_up(v.items, d, 64), __shfl_up(v.copies, d, 64), __shfl_up(v.flooded, d, 64),
                    (uint64_t)__shfl_up((unsigned long long)v.bytes, d, 64)};
}
// Inclusive scan across the wave (saturating addition is associative, so the tree's shape does not matter).
DEV FloodAcc flood_wave_scan(FloodAcc v, uint32_t lane) {
#pragma unroll
    for (uint32_t s = 1; s < 64u; s *= 2u) {
        const FloodAcc t = flood_shfl_up(v, s);
        if (lane >= s) v = flood_add(t, v);
    }
    return v;
}
// Exclusive scan across a workgroup of W waves; *total = the workgroup's sum. wsum: W entries of LDS. Every
// thread of the workgroup calls it.
template <uint32_t W>
DEV FloodAcc flood_block_scan(const FloodAcc& own, FloodAcc* wsum, FloodAcc* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const FloodAcc inc = flood_wave_scan(own, lane);
    FloodAcc exc = flood_shfl_up(inc, 1u);
    if (lane == 0) exc = flood_zero();
    __syncthreads();  // an earlier call's readers are done with wsum
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    FloodAcc before = flood_zero(), all = flood_zero();
#pragma unroll
    for (uint32_t w = 0; w < W; ++w) {
        const FloodAcc v = wsum[w];
        if (w < wave) before = flood_add(before, v);
        all = flood_add(all, v);
    }
    *total = all;
    return flood_add(before, exc);
}

struct FloodLane {
    uint2 d;        // the descriptor
    uint32_t port;  // the unicast port, or NFCS_IF_NONE
    uint32_t cnt;   // items the packet calls for
    uint32_t vlan;
    bool flood;     // taken as a flood (live, verdict FLOOD, no unicast port)
    uint64_t slot;  // round_up(len, copy_align) for a flooded packet, else 0
};
DEV FloodLane flood_classify(const FdbDev& fdb, const FloodArgs& a, uint64_t p) {
    FloodLane r{make_uint2(0u, 0u), NFCS_IF_NONE, 0u, 0u, false, 0ull};
    if (p >= a.n) return r;
    r.d = ((const uint2*)a.desc)[p];
    if (!sw_desc_live(r.d.x, r.d.y, a.copy_base)) return r;
    r.port = flood_unicast_port(a.l3_port ? a.l3_port[p] : 0u, a.l3_port != nullptr, a.fwd_status ? a.fwd_status[p] : 0u,
                                a.fwd_status != nullptr, a.l2_port ? a.l2_port[p] : 0u, a.l2_port != nullptr);
    if (r.port != NFCS_IF_NONE) {
        r.cnt = 1u;
        return r;
    }
    if (!a.l2_verdict || a.l2_verdict[p] != NFCS_L2_FLOOD) return r;
    r.flood = true;
    r.vlan = a.l2_vlan[p];
    r.slot = flood_round_up(r.d.y, a.copy_align);
    if (r.vlan >= kL2Vlans || a.ingress >= fdb.ports) return r;  // should_forward fails for every port
    const bool in_ok = (fdb.port_vlans[(size_t)a.ingress * kL2VlanWords + (r.vlan >> 5)] >> (r.vlan & 31u)) & 1u;
    const uint32_t* row = fdb.vlan_ports + (size_t)r.vlan * fdb.port_words;
    for (uint32_t w = 0; w < fdb.port_words; ++w)  // at most NFCS_L2_MAX_PORTS / 32 words
        r.cnt += (uint32_t)__popc(fdb_flood_word(row, w, a.ingress, a.num_ports, in_ok));
    return r;
}
DEV FloodAcc flood_acc_of(const FloodLane& l) {
    return FloodAcc{l.cnt, l.flood ? l.cnt : 0u, l.flood ? 1u : 0u, (uint64_t)l.cnt * l.slot};  // <= 1,023 x 2^33
}
DEV FloodAcc flood_load(const FloodSum* s) { return FloodAcc{s->items, s->copies, s->flooded, s->bytes}; }
DEV void flood_store(FloodSum* s, const FloodAcc& v) {
    s->items = v.items;
    s->copies = v.copies;
    s->flooded = v.flooded;
    s->pad = 0u;
    s->bytes = v.bytes;
}
// Where a packet stands in the list: what the packets before it call for (the tile's prefix plus the scan
// inside the tile), where its first entry's bytes begin, and whether the list is still open there. Entry k is
// emitted iff k < cap and base + (slot bytes up to and including k) <= arena_bytes, so the entry before this
// packet's first (region at.bytes) was emitted iff `open`.
struct ListAt : FloodAcc {
    uint64_t region;
    bool open;
};
DEV ListAt list_at(const FloodSum* tile_prefix, const FloodAcc& exc, uint64_t base, uint32_t cap,
                   uint64_t arena_bytes) {
    const FloodAcc at = flood_add(flood_load(tile_prefix), exc);
    const uint64_t region = flood_sat_add(base, at.bytes);
    return ListAt{at, region, at.items <= cap && region <= arena_bytes};
}

__global__ __launch_bounds__(kFloodTile) void flood_count_kernel(const FdbDev fdb, const FloodArgs a, uint32_t tiles,
                                                                 FloodSum* __restrict__ sums) {
    __shared__ FloodAcc wsum[kFloodWaves];
    const uint32_t tile = xcd_block_n(tiles);
    const FloodLane l = flood_classify(fdb, a, (uint64_t)tile * kFloodTile + threadIdx.x);
    FloodAcc total;
    (void)flood_block_scan<kFloodWaves>(flood_acc_of(l), wsum, &total);
    if (threadIdx.x == 0) flood_store(sums + tile, total);
}

__global__ __launch_bounds__(kFloodScanThreads) void flood_scan_kernel(FloodSum* __restrict__ sums, uint32_t tiles) {
    __shared__ FloodAcc wsum[kFloodScanThreads / 64u];
    FloodAcc carry = flood_zero();
    for (uint32_t base = 0; base < tiles; base += kFloodScanThreads) {  // trips: a function of n alone
        const uint32_t t = base + threadIdx.x;
        const FloodAcc own = t < tiles ? flood_load(sums + t) : flood_zero();
        FloodAcc total;
        const FloodAcc exc = flood_block_scan<kFloodScanThreads / 64u>(own, wsum, &total);
        if (t < tiles) flood_store(sums + t, flood_add(carry, exc));
        carry = flood_add(carry, total);
    }
    if (threadIdx.x == 0) flood_store(sums + tiles, carry);
}

__global__ __launch_bounds__(kFloodTile) void flood_emit_kernel(const FdbDev fdb, const FloodArgs a, uint32_t tiles,
                                                                const FloodSum* __restrict__ sums) {
    __shared__ FloodAcc wsum[kFloodWaves];
    __shared__ uint64_t f_b0[kFloodTile];
    __shared__ uint32_t f_off16[kFloodTile], f_len[kFloodTile], f_vlan[kFloodTile], f_k0[kFloodTile], f_e[kFloodTile],
        f_src[kFloodTile];
    const uint32_t tile = xcd_block_n(tiles);
    const uint64_t p = (uint64_t)tile * kFloodTile + threadIdx.x;
    const FloodLane l = flood_classify(fdb, a, p);
    FloodAcc total;
    const FloodAcc exc = flood_block_scan<kFloodWaves>(flood_acc_of(l), wsum, &total);
    const ListAt at = list_at(sums + tile, exc, a.copy_base, a.cap, a.arena_bytes);
    uint32_t e = 0;  // how many of this packet's items are emitted
    if (at.open && l.cnt) {
        e = min(l.cnt, a.cap - at.items);
        if (l.slot) e = (uint32_t)min((uint64_t)e, (a.arena_bytes - at.region) / l.slot);
    }
    if (p < a.n) {
        if (!l.flood && e) {  // e = 1: at.items < cap
            ((uint2*)a.item_desc)[at.items] = l.d;
            a.item_port[at.items] = l.port;
            a.item_src[at.items] = (uint32_t)p;
        }
        if (l.flood) {  // exc.flooded < kFloodTile: its place among the tile's flooded packets
            f_off16[exc.flooded] = l.d.x;
            f_len[exc.flooded] = l.d.y;
            f_vlan[exc.flooded] = l.vlan;
            f_k0[exc.flooded] = at.items;
            f_e[exc.flooded] = e;
            f_b0[exc.flooded] = at.bytes;
            f_src[exc.flooded] = (uint32_t)p;
        }
        // the totals: from the packet that holds the cut, or from the last packet when nothing is cut
        if (at.open && (e < l.cnt || p + 1u == a.n)) {
            const FloodAcc all = flood_load(sums + tiles);
            nfcs_flood_totals t;
            t.items = at.items + e;
            t.items_needed = all.items;
            t.copies = at.copies + (l.flood ? e : 0u);
            t.flooded = all.flooded;
            t.copy_bytes = at.bytes + (l.flood ? (uint64_t)e * l.slot : 0ull);
            t.copy_bytes_needed = all.bytes;
            *a.totals = t;
        }
    }
    __syncthreads();
    // the copies: row `row` takes the tile's flooded packets row, row + kFloodRows, ...
    const uint32_t nflood = total.flooded, row = threadIdx.x / kFloodR, rl = threadIdx.x % kFloodR;
    for (uint32_t f = row; f < nflood; f += kFloodRows) {
        const uint32_t fe = f_e[f];
        if (fe == 0) continue;  // nothing emitted (then also: every mask word may be empty, the VLAN out of range)
        const uint32_t len = f_len[f], k0 = f_k0[f], src_i = f_src[f];
        const uint32_t chunks = (uint32_t)(((uint64_t)len + 15u) >> 4);
        const uint64_t slot = flood_round_up(len, a.copy_align), first = a.copy_base + f_b0[f];
        const uint4* src = (const uint4*)(a.arena + (uint64_t)f_off16[f] * 16u);
        const uint32_t* mrow = fdb.vlan_ports + (size_t)f_vlan[f] * fdb.port_words;  // fe > 0: the VLAN is in range
        for (uint32_t c0 = 0; c0 == 0 || c0 < chunks; c0 += kFloodR * kFloodK) {  // one pass per 1,536 bytes
            uint4 v[kFloodK];
#pragma unroll
            for (uint32_t s = 0; s < kFloodK; ++s) {
                const uint32_t c = c0 + rl + kFloodR * s;
                v[s] = make_uint4(0u, 0u, 0u, 0u);
                if (c < chunks) v[s] = ld16<1>(src + c);  // live: the frame's chunks lie below copy_base
            }
            uint32_t j = 0;
            for (uint32_t w = 0; w < fdb.port_words && j < fe; ++w) {
                uint32_t m = fdb_flood_word(mrow, w, a.ingress, a.num_ports, true);
                for (uint32_t b = 0; b < 32u && m != 0u && j < fe; ++b, ++j) {
                    const uint32_t port = w * 32u + (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    const uint64_t dst = first + (uint64_t)j * slot;  // j < fe: the slot ends inside the arena
                    if (c0 == 0 && rl == 0) {                         // k0 + j < items <= cap
                        ((uint2*)a.item_desc)[k0 + j] = make_uint2((uint32_t)(dst >> 4), len);
                        a.item_port[k0 + j] = port;
                        a.item_src[k0 + j] = src_i;
                    }
                    if (dst + slot <= a.arena_bytes) {
                        uint4* out = (uint4*)(a.arena + dst);
#pragma unroll
                        for (uint32_t s = 0; s < kFloodK; ++s) {
                            const uint32_t c = c0 + rl + kFloodR * s;
                            if (c < chunks) vst16<NFCS_FLOOD_STORE>(out + c, v[s]);
                        }
                    }
                }
            }
        }
    }
}

// Entries [*emitted, cap) of a list inert. The flood's and the ICMP responder's emitted counts are the first
// word of their totals.
static_assert(offsetof(nfcs_flood_totals, items) == 0, "flood_pad_kernel reads items at the struct's address");
static_assert(offsetof(nfcs_icmp_totals, messages) == 0, "flood_pad_kernel reads messages at the struct's address");
// One struct argument, which the waves that get that far read from the kernarg segment (five separate arguments
// would be preloaded into SGPRs for every wave, and most waves of this kernel leave at the first comparison).
struct ListOut {
    nfcs_desc* desc;
    uint32_t* port;
    uint32_t* src;
    uint32_t cap;
    const uint32_t* emitted;
};
__global__ __launch_bounds__(kBlock) void flood_pad_kernel(const ListOut o) {
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= o.cap || k < *o.emitted) return;
    ((uint2*)o.desc)[k] = make_uint2(0u, 0u);
    o.port[k] = NFCS_IF_NONE;
    o.src[k] = NFCS_ITEM_NONE;
}

// A list stage over n packets: count / flood_scan_kernel / emit / pad. t...: the tables and the stage's
// arguments, as both of its kernels take them in front of (tiles, sums).
template <typename... T>
hipError_t launch_list_stage(void (*count)(T..., uint32_t, FloodSum*), void (*emit)(T..., uint32_t, const FloodSum*),
                             uint32_t n, const ListOut& out, uint32_t* scratch, hipStream_t stream, const T&... t) {
    if (n == 0) return hipSuccess;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kFloodTile - 1u) / kFloodTile);
    FloodSum* sums = (FloodSum*)scratch;  // tiles + 1 records (flood_scratch_words)
    hipLaunchKernelGGL(count, dim3(tiles), dim3(kFloodTile), 0, stream, t..., tiles, sums);
    hipLaunchKernelGGL(flood_scan_kernel, dim3(1), dim3(kFloodScanThreads), 0, stream, sums, tiles);
    hipLaunchKernelGGL(emit, dim3(tiles), dim3(kFloodTile), 0, stream, t..., tiles, sums);
    if (out.cap) {
        const uint32_t g = (uint32_t)(((uint64_t)out.cap + kBlock - 1u) / kBlock);
        hipLaunchKernelGGL(flood_pad_kernel, dim3(g), dim3(kBlock), 0, stream, out);
    }
    return hipGetLastError();
}

hipError_t launch_flood_expand(const DevInfo& di, const FdbDev& fdb, const FloodArgs& a, uint32_t* scratch,
                               hipStream_t stream) {
    (void)di;
    const ListOut out = {a.item_desc, a.item_port, a.item_src, a.cap, (const uint32_t*)a.totals};
    return launch_list_stage(flood_count_kernel, flood_emit_kernel, a.n, out, scratch, stream, fdb, a);
}

// ---- ICMP responder: echo replies and TTL / unreachable errors -------------------
// nfcs_icmp.h icmp_respond is the sequential definition; these kernels equal it bit for bit. The flood stage's
// shape, scan and scratch (FloodAcc: items = messages, copies = echo replies, bytes = slot bytes):
//   1. icmp_count_kernel: per packet icmp_plan (nfcs_icmp.h, the host walk's function, on the frame's header
//      bytes in device memory) -> (message?, echo?, slot bytes), summed over the tile into scratch[tile].
//   2. flood_scan_kernel, as it is.
//   3. icmp_emit_kernel: icmp_plan again, the tile's exclusive scan, and from the tile's prefix each packet's
//      message index and slot offset; a packet yields at most one message, so "emitted" is one comparison per
//      overflow condition. The packet's lane stores the list entry, the status byte and message chunks 0-1
//      (bytes 0..31: MACs, EtherType, the IPv4 header up to its destination address, header checksum
//      included: icmp_plan sums the header it built). The tile's messages are compacted into LDS and 64 rows
//      of 16 lanes take them in turn: lane rl builds message chunks rl, rl + 16, ..., 6 per pass. Message byte
//      b >= 44 is frame byte b + shift with shift a multiple of 4, so a chunk is ONE 16-byte load at a
//      dword-aligned address (the dword shift is in the address; a pass issues its loads back to back, then
//      repairs with dword loads the chunk whose load would leave the frame's 16-byte chunks), masked at the end, summed with v_sad_u16 as §3 does while it is in
//      registers, and stored. The first pass's chunks stay in registers until the row's sum is complete:
//      chunk 2 then takes the ICMP checksum and the pass is stored. Every message byte is written once and no
//      byte of the region is read.
//   4. flood_pad_kernel, as it is: entries [messages, cap) inert.
// No position comes from an atomic and no loop ends on data alone (a message has at most 4,097 chunks).
constexpr uint32_t kIcmpR = 16, kIcmpK = 6;  // a row pass: 16 lanes x 6 chunks = 1,536 message bytes
constexpr uint32_t kIcmpRows = kIcmpTile / kIcmpR;

typedef uint32_t u32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));

DEV IcmpPlan icmp_classify(const IcmpView& t, const FibView& fib, const IcmpArgs& a, uint64_t p, uint2* d) {
    *d = make_uint2(0u, 0u);
    if (p < a.n) {
        *d = ((const uint2*)a.desc)[p];
        if (sw_desc_live(d->x, d->y, a.msg_base))
            return icmp_plan(t, fib, a.ingress, a.arena + (uint64_t)d->x * 16u, d->y, a.rt_verdict[p],
                             a.ip_id ? a.ip_id[p] : 0u);
    }
    IcmpPlan r;
    r.status = NFCS_ICMP_ST_NONE;
    r.msg_len = 0u;
    r.port = NFCS_IF_NONE;
    r.shift = 0;
#pragma unroll
    for (uint32_t i = 0; i < kIcmpHdrDwords; ++i) r.hdr[i] = 0u;
    return r;
}
DEV FloodAcc icmp_acc_of(const IcmpPlan& pl, uint32_t align) {
    const uint32_t m = pl.msg_len ? 1u : 0u;
    return FloodAcc{m, pl.status == NFCS_ICMP_ST_ECHO_REPLY ? m : 0u, 0u, m ? flood_round_up(pl.msg_len, align) : 0ull};
}

__global__ __launch_bounds__(kIcmpTile) void icmp_count_kernel(const IcmpView t, const FibView fib, const IcmpArgs a,
                                                               uint32_t tiles, FloodSum* __restrict__ sums) {
    __shared__ FloodAcc wsum[kFloodWaves];
    const uint32_t tile = xcd_block_n(tiles);
    uint2 d;
    const IcmpPlan pl = icmp_classify(t, fib, a, (uint64_t)tile * kIcmpTile + threadIdx.x, &d);
    FloodAcc total;
    (void)flood_block_scan<kFloodWaves>(icmp_acc_of(pl, a.msg_align), wsum, &total);
    if (threadIdx.x == 0) flood_store(sums + tile, total);
}

// Message chunk c >= 2 (bytes 16c .. 16c + 15, zero at and past len) in two steps, so that a row pass issues its
// loads back to back: icmp_chunk_load, the one 16-byte load (from the zero line where the chunk does not exist or
// the load would leave the frame's own 16-byte chunks), and icmp_chunk_finish, which repairs the latter case with
// guarded dword loads, masks, puts the plan's bytes 32..43 into chunk 2 and adds the chunk's share of the ICMP sum
// (message bytes 34.., as little-endian 16-bit words; an odd last byte counts as the reference's low byte, §3).
DEV bool icmp_chunk_full(int32_t shift, uint32_t srcpad, uint32_t c, uint32_t chunks) {
    const int32_t so = (int32_t)(16u * c) + shift;  // >= 4: c >= 2, shift >= -28
    return c >= 2u && c < chunks && (uint32_t)so + 16u <= srcpad;  // inside the frame's chunks (live: below msg_base)
}
DEV uint4 icmp_chunk_load(const uint8_t* src, int32_t shift, uint32_t c, bool full) {
    const uint8_t* p = full ? src + ((int32_t)(16u * c) + shift) : (const uint8_t*)g_zero_line;
    const u32x4_a4_t x = __builtin_nontemporal_load((const u32x4_a4_t*)p);
    return make_uint4(x.x, x.y, x.z, x.w);
}
DEV uint4 icmp_chunk_finish(const uint4& x, bool full, const uint8_t* src, int32_t shift, uint32_t c, uint32_t len, uint32_t h8,
                            uint32_t h9, uint32_t h10, uint32_t& acc) {
    const int32_t so = (int32_t)(16u * c) + shift;
    uint32_t w[4] = {x.x, x.y, x.z, x.w};
    if (!full) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t b = 16u * c + 4u * j;  // a dword the message needs starts inside the frame
            w[j] = (b >= 44u && b < len) ? *(const uint32_t*)(src + so + (int32_t)(4u * j)) : 0u;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t b = 16u * c + 4u * j;
        const uint32_t keep = b >= len ? 0u : (len - b >= 4u ? 0xFFFFFFFFu : (1u << (8u * (len - b))) - 1u);
        w[j] &= keep;
    }
    if (c == 2u) {  // bytes 32..43 are the plan's (already zero at and past len)
        w[0] = h8;
        w[1] = h9;
        w[2] = h10;
    }
    acc = wsum(w[3], wsum(w[2], wsum(w[1], wsum(c == 2u ? w[0] & 0xFFFF0000u : w[0], acc))));
    const uint32_t last = len - 1u;
    const uint4 r = make_uint4(w[0], w[1], w[2], w[3]);
    if ((len & 1u) && (last >> 4) == c) acc += 255u * ((comp(r, (last >> 2) & 3u) >> (8u * (last & 3u))) & 0xFFu);
    return r;
}

__global__ __launch_bounds__(kIcmpTile) void icmp_emit_kernel(const IcmpView t, const FibView fib, const IcmpArgs a,
                                                              uint32_t tiles, const FloodSum* __restrict__ sums) {
    __shared__ FloodAcc wsum_lds[kFloodWaves];
    __shared__ uint64_t m_at[kIcmpTile];
    __shared__ uint32_t m_off16[kIcmpTile], m_srcpad[kIcmpTile], m_len[kIcmpTile], m_h8[kIcmpTile], m_h9[kIcmpTile],
        m_h10[kIcmpTile];
    __shared__ int32_t m_shift[kIcmpTile];
    const uint32_t tile = xcd_block_n(tiles);
    const uint64_t p = (uint64_t)tile * kIcmpTile + threadIdx.x;
    uint2 d;
    const IcmpPlan pl = icmp_classify(t, fib, a, p, &d);
    const FloodAcc own = icmp_acc_of(pl, a.msg_align);
    FloodAcc total;
    const FloodAcc exc = flood_block_scan<kFloodWaves>(own, wsum_lds, &total);
    const ListAt at = list_at(sums + tile, exc, a.msg_base, a.cap, a.arena_bytes);
    const uint64_t region = at.region;
    const uint32_t e = (at.open && own.items && at.items < a.cap && a.arena_bytes - region >= own.bytes) ? 1u : 0u;
    if (p < a.n) {
        if (a.status) a.status[p] = (uint8_t)((own.items && !e) ? (uint32_t)NFCS_ICMP_ST_OVERFLOW : pl.status);
        if (own.items) {  // exc.items < kIcmpTile: its place among the tile's messages
            m_len[exc.items] = e ? pl.msg_len : 0u;
            m_at[exc.items] = region;
            m_off16[exc.items] = d.x;
            m_srcpad[exc.items] = (d.y + 15u) & ~15u;  // wraps to 0 only above 2^32 - 16: dword loads then
            m_shift[exc.items] = pl.shift;
            m_h8[exc.items] = pl.hdr[8];
            m_h9[exc.items] = pl.hdr[9];
            m_h10[exc.items] = pl.hdr[10];
        }
        if (e) {  // at.items < cap; region + slot <= arena_bytes and the slot holds round_up(msg_len, 16)
            ((uint2*)a.msg_desc)[at.items] = make_uint2((uint32_t)(region >> 4), pl.msg_len);
            a.msg_port[at.items] = pl.port;
            a.msg_src[at.items] = (uint32_t)p;
            uint4* out = (uint4*)(a.arena + region);
            vst16<NFCS_FLOOD_STORE>(out, make_uint4(pl.hdr[0], pl.hdr[1], pl.hdr[2], pl.hdr[3]));
            vst16<NFCS_FLOOD_STORE>(out + 1, make_uint4(pl.hdr[4], pl.hdr[5], pl.hdr[6], pl.hdr[7]));
        }
        // the totals: from the packet that holds the cut, or from the last packet when nothing is cut
        if (at.open && (e < own.items || p + 1u == a.n)) {
            const FloodAcc all = flood_load(sums + tiles);
            nfcs_icmp_totals r;
            r.messages = at.items + e;
            r.messages_needed = all.items;
            r.echo_replies = at.copies + (e ? own.copies : 0u);
            r.errors = r.messages - r.echo_replies;
            r.msg_bytes = at.bytes + (e ? own.bytes : 0ull);
            r.msg_bytes_needed = all.bytes;
            *a.totals = r;
        }
    }
    __syncthreads();
    // the messages' chunks 2..: row `row` takes the tile's messages row, row + kIcmpRows, ...
    const uint32_t nmsg = total.items, row = threadIdx.x / kIcmpR, rl = threadIdx.x % kIcmpR;
    for (uint32_t f = row; f < nmsg; f += kIcmpRows) {
        const uint32_t len = m_len[f];  // row-uniform; 0: not emitted. 42 <= len <= 65,549
        if (len == 0u) continue;
        const uint32_t chunks = (len + 15u) >> 4, srcpad = m_srcpad[f], h8 = m_h8[f], h9 = m_h9[f], h10 = m_h10[f];
        const int32_t shift = m_shift[f];
        const uint8_t* src = a.arena + (uint64_t)m_off16[f] * 16u;
        uint4* out = (uint4*)(a.arena + m_at[f]);  // the slot ends inside the arena and holds `chunks` chunks
        uint32_t acc = 0u;
        uint4 v[kIcmpK];
        bool full[kIcmpK];
#pragma unroll
        for (uint32_t s = 0; s < kIcmpK; ++s) {  // every load of the pass first
            full[s] = icmp_chunk_full(shift, srcpad, rl + kIcmpR * s, chunks);
            v[s] = icmp_chunk_load(src, shift, rl + kIcmpR * s, full[s]);
        }
#pragma unroll
        for (uint32_t s = 0; s < kIcmpK; ++s) {
            const uint32_t c = rl + kIcmpR * s;
            if (c >= 2u && c < chunks) v[s] = icmp_chunk_finish(v[s], full[s], src, shift, c, len, h8, h9, h10, acc);
        }
        for (uint32_t c0 = kIcmpR * kIcmpK; c0 < chunks; c0 += kIcmpR * kIcmpK) {  // further passes: at most 42
            uint4 w[kIcmpK];
            bool wf[kIcmpK];
#pragma unroll
            for (uint32_t s = 0; s < kIcmpK; ++s) {
                wf[s] = icmp_chunk_full(shift, srcpad, c0 + rl + kIcmpR * s, chunks);
                w[s] = icmp_chunk_load(src, shift, c0 + rl + kIcmpR * s, wf[s]);
            }
#pragma unroll
            for (uint32_t s = 0; s < kIcmpK; ++s) {
                const uint32_t c = c0 + rl + kIcmpR * s;
                if (c < chunks) vst16<NFCS_FLOOD_STORE>(out + c, icmp_chunk_finish(w[s], wf[s], src, shift, c, len, h8, h9, h10, acc));
            }
        }
        const uint32_t csum = (~fold32(row_sum<16>(acc))) & 0xFFFFu;  // its two bytes in memory order, §3
#pragma unroll
        for (uint32_t s = 0; s < kIcmpK; ++s) {
            const uint32_t c = rl + kIcmpR * s;
            if (c == 2u) v[s].y |= csum;  // bytes 36-37 (zero in the plan)
            if (c >= 2u && c < chunks) vst16<NFCS_FLOOD_STORE>(out + c, v[s]);
        }
    }
}

hipError_t launch_icmp_respond(const DevInfo& di, const IcmpView& icmp, const FibView& fib, const IcmpArgs& a,
                               uint32_t* scratch, hipStream_t stream) {
    (void)di;
    const ListOut out = {a.msg_desc, a.msg_port, a.msg_src, a.cap, (const uint32_t*)a.totals};
    return launch_list_stage(icmp_count_kernel, icmp_emit_kernel, a.n, out, scratch, stream, icmp, fib, a);
}

// ---- synthetic config generator (same spec as oracle/nfcs_oracle.c) -----------
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t pkt_key(uint64_t seed, uint64_t i) { return mix64(seed ^ (i * kGolden)); }
__host__ __device__ inline uint64_t draw(uint64_t key, uint64_t k) { return mix64(key + k * kGolden); }

__host__ __device__ inline uint32_t cfg_len(int config, uint64_t seed, uint64_t index) {
    switch (config) {
    case 0: return 64;
    case 1: return 1500;
    case 2: return 9000;
    case 3: return 64u + (uint32_t)(draw(pkt_key(seed, index), 1) % 1437u);
    default: return 0;
    }
}

// ---- read-stream reference (bench support; SURVEY.md §8d "achieved fraction of a measured
// read-only stream kernel on the same box") -------------------------------------------------------
// Pure reads of `bytes` (16-byte multiple), summed into a value that is stored only if it equals an
// impossible constant (the loads stay live, nothing is written). The bench times every form over the
// batch's own arena and takes the fastest as the ceiling:
//   form 0  the checksum read pass's own shape: 256-thread workgroups in the XCD-aware order held at
//           6 waves/SIMD, each wave reading 6 KiB as 6 wave-wide 1 KiB loads in flight (lane l:
//           chunks l + 64k), the first with the default policy and the rest non-temporal;
//   form 2  the same, every load non-temporal;
//   form 3  8 loads per lane (8 KiB per wave), all non-temporal, no occupancy cap;
//   form 4  16 loads per lane (16 KiB per wave), all non-temporal, no occupancy cap;
//   form 5  4 loads per lane (4 KiB per wave), all non-temporal, no occupancy cap;
//   form 1  round 1's microbenchmark (tools/stream_read.hip): 512 workgroups striding over the
//           buffer, 4 non-temporal loads per lane in flight.
template <uint32_t K, bool MIX>  // MIX: the first load of each wave with the default policy
__global__ __launch_bounds__(kBlock) void stream_read_kernel(const uint4* __restrict__ p, uint64_t n16,
                                                             unsigned long long* __restrict__ sink) {
    const uint64_t w = (uint64_t)xcd_block() * kWavesPerBlock + (threadIdx.x >> 6);
    const uint64_t base = w * 64u * K + (threadIdx.x & 63u);
    uint4 v[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t i = base + 64u * k;
        const uint4* a = i < n16 ? p + i : g_zero_line;
        v[k] = (MIX && k == 0) ? ld16<0>(a) : ld16<1>(a);
    }
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) acc += v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    if (acc == 0x9E3779B9u && sink) *sink = acc;
}

__global__ __launch_bounds__(kBlock) void stream_read_strided_kernel(const uint4* __restrict__ p, uint64_t n16,
                                                                     unsigned long long* __restrict__ sink) {
    constexpr uint32_t U = 4;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t acc = 0;
    for (; i + (U - 1) * stride < n16; i += U * stride) {
        uint4 v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = ld16<1>(p + i + u * stride);
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) acc += v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    for (; i < n16; i += stride) {
        const uint4 v = ld16<1>(p + i);
        acc += v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9E3779B9u && sink) *sink = acc;
}

hipError_t launch_stream_read(const uint8_t* buf, uint64_t bytes, int form, unsigned long long* sink,
                              hipStream_t stream) {
    const uint64_t n16 = bytes / 16u;
    if (n16 == 0) return hipSuccess;
    const uint4* q = (const uint4*)buf;
    auto grid = [&](uint32_t k) { return dim3((uint32_t)((n16 + 64u * k * kWavesPerBlock - 1) / (64u * k * kWavesPerBlock))); };
    switch (form) {
    case 1: hipLaunchKernelGGL(stream_read_strided_kernel, dim3(512), dim3(kBlock), 0, stream, q, n16, sink); break;
    // forms 0 and 2 are held at 6 waves/SIMD (the round-1 read stream's best)
    case 0: hipLaunchKernelGGL((stream_read_kernel<6, true>), grid(6), dim3(kBlock), kRowsLdsPad6, stream, q, n16, sink); break;
    case 2: hipLaunchKernelGGL((stream_read_kernel<6, false>), grid(6), dim3(kBlock), kRowsLdsPad6, stream, q, n16, sink); break;
    case 3: hipLaunchKernelGGL((stream_read_kernel<8, false>), grid(8), dim3(kBlock), 0, stream, q, n16, sink); break;
    case 4: hipLaunchKernelGGL((stream_read_kernel<16, false>), grid(16), dim3(kBlock), 0, stream, q, n16, sink); break;
    default: hipLaunchKernelGGL((stream_read_kernel<4, false>), grid(4), dim3(kBlock), 0, stream, q, n16, sink); break;
    }
    return hipGetLastError();
}

// The read-only floor of the checksum read pass's own access pattern (bench `stream_ceiling`): the
// batch's frames read exactly as update_rows_kernel reads them — 16-lane rows, 6 slots, four packets
// per wave, 256-thread workgroups held at 5 waves/SIMD, XCD-aware order, the header slot with the
// default policy and the rest non-temporal, jumbo frames continued in batches of 6 slots — with
// nothing computed or written (the chunks are XOR-ed into a value stored only if it equals an
// impossible constant). A buffer stream reads the arena contiguously; this form reads what the
// product reads, in its order, so it bounds the product on every layout (C2's 9.5 GB arena: a
// contiguous stream measured below the product on some boxes).
__global__ __launch_bounds__(kBlock) void frames_read_kernel(const nfcs_desc* __restrict__ desc, uint32_t n,
                                                             uint32_t nblocks, const uint8_t* __restrict__ arena,
                                                             uint64_t arena_bytes, unsigned long long* __restrict__ sink) {
    constexpr int K = 6, R = 16, PW = 4;
    const uint32_t lane = threadIdx.x & 63u, rl = lane & (R - 1), row = lane / R;
    const uint64_t pw = (uint64_t)xcd_block_n(nblocks) * (kBlock / R) + rfl(threadIdx.x >> 6) * PW;
    if (pw >= n) return;
    const nfcs_desc d = pick_desc<PW>(load_descw<PW>(desc, pw, n), row);
    const uint64_t off = (uint64_t)d.off16 * 16u;
    const bool live = pw + row < n && sw_desc_live(d.off16, d.len, arena_bytes);
    const uint32_t nch = live ? (d.len + 15u) >> 4 : 0u;
    const uint4* src = (const uint4*)(arena + (live ? off : 0));
    uint4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t c = rl + (uint32_t)R * k;
        const uint4* a = (c < nch) ? src + c : g_zero_line;
        v[k] = k == 0 ? ld16<0>(a) : ld16<1>(a);
    }
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) acc ^= v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    const uint32_t cmax = wave_max_rows<R>(nch);
    for (uint32_t cb = (uint32_t)R * K; cb < cmax; cb += (uint32_t)R * K) {
        uint4 w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t c = cb + rl + (uint32_t)R * k;
            w[k] = ld16<1>((c < nch) ? src + c : g_zero_line);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc ^= w[k].x ^ w[k].y ^ w[k].z ^ w[k].w;
    }
    if (acc == 0x9E3779B9u && sink) *sink = acc;
}

hipError_t launch_frames_read(const uint8_t* arena, uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n,
                              unsigned long long* sink, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = (n + 15u) / 16u;
    hipLaunchKernelGGL(frames_read_kernel, dim3(grid), dim3(kBlock), kRowsLdsPad, stream, desc, n, grid, arena,
                       arena_bytes, sink);
    return hipGetLastError();
}

uint32_t config_len(int config, uint64_t seed, uint64_t index) { return cfg_len(config, seed, index); }

// header byte override at frame offset o (o < 64), or -1
DEV int hdr_byte(uint32_t o, uint32_t len, uint32_t proto, uint32_t old_ip, uint32_t old_l4) {
    switch (o) {
    case 12: return 0x08;
    case 13: return 0x00;
    case 14: return 0x45;
    case 15: return 0x00;
    case 16: return (int)(((len - 14) >> 8) & 0xFF);
    case 17: return (int)((len - 14) & 0xFF);
    case 22: return 64;
    case 23: return (int)proto;
    case 24: return (int)(old_ip >> 8);
    case 25: return (int)(old_ip & 0xFF);
    default: break;
    }
    if (proto == 17) {
        if (o == 38) return (int)(((len - 34) >> 8) & 0xFF);
        if (o == 39) return (int)((len - 34) & 0xFF);
        if (o == 40) return (int)(old_l4 >> 8);
        if (o == 41) return (int)(old_l4 & 0xFF);
    } else if (proto == 6) {
        if (o == 46) return 0x50;
        if (o == 49) return (int)(old_l4 >> 8);
        if (o == 50) return (int)(old_l4 & 0xFF);
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void gen_config_kernel(int config, uint64_t seed,
                                                            uint64_t first, uint32_t n,
                                                            uint8_t* __restrict__ arena,
                                                            uint64_t arena_bytes,
                                                            const nfcs_desc* __restrict__ desc) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    for (uint32_t p = blockIdx.x * kWavesPerBlock + rfl(threadIdx.x >> 6); p < n; p += nw) {
        const nfcs_desc d = desc[p];
        const uint64_t off = (uint64_t)d.off16 * 16u;
        const uint32_t len = d.len;
        if (off + (((uint64_t)len + 15) & ~15ull) > arena_bytes) continue;
        const uint64_t key = pkt_key(seed, first + p);
        const uint32_t proto = config == 0 ? 253u : config == 1 ? 17u : config == 2 ? 6u
                             : ((draw(key, 2) & 1u) ? 6u : 17u);
        const uint32_t old_ip = (uint32_t)((draw(key, 3) & 0xFFFFu) | 0x0101u);
        const uint32_t old_l4 = (uint32_t)((draw(key, 4) & 0xFFFFu) | 0x0101u);
        uint4* dst = (uint4*)(arena + off);
        const uint32_t nch = (len + 15u) >> 4;
        for (uint32_t c = lane; c < nch; c += 64u) {
            uint64_t q[2] = {draw(key, 16 + 2 * c), draw(key, 17 + 2 * c)};
            uint8_t* b = (uint8_t*)q;
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t o = c * 16u + j;
                if (o >= len) b[j] = 0;
                else if (o < 64) {
                    int hb = hdr_byte(o, len, proto, old_ip, old_l4);
                    if (hb >= 0) b[j] = (uint8_t)hb;
                }
            }
            uint4 v;
            v.x = (uint32_t)q[0]; v.y = (uint32_t)(q[0] >> 32);
            v.z = (uint32_t)q[1]; v.w = (uint32_t)(q[1] >> 32);
            dst[c] = v;
        }
    }
}

hipError_t launch_gen_config(const DevInfo& di, int config, uint64_t seed, uint64_t first,
                             uint32_t n, uint8_t* arena, uint64_t arena_bytes,
                             const nfcs_desc* desc, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    uint32_t grid = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    if (grid > (uint32_t)di.cus * 8u) grid = (uint32_t)di.cus * 8u;
    hipLaunchKernelGGL(gen_config_kernel, dim3(grid), dim3(kBlock), 0, stream, config, seed,
                       first, n, arena, arena_bytes, desc);
    return hipGetLastError();
}

// A measurement helper (tools/store_case_bench.py --stale-every): one thread per group of `every`
// consecutive packets of an updated batch of untagged IPv4 frames with the L4 checksum at byte 40 (C1's
// UDP) flips the high byte of both checksum fields of one packet of the group, so the next update finds
// exactly those packets in need of a store. The packet's place in its group is hashed: with a fixed place
// the stale frames of a uniform batch lie at one stride (every 256th C1 frame: 384 KB), their partial
// writes fall on a few memory channels, and the sweep measured that aliasing instead of the store form
// (DESIGN.md §12). Untimed.
__global__ __launch_bounds__(kBlock) void stale_every_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                             const nfcs_desc* __restrict__ desc, uint32_t n,
                                                             uint32_t every) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t h = (uint32_t)g * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA77u;
    h ^= h >> 13;
    const uint64_t p = g * every + h % every;
    if (p >= n) return;
    const nfcs_desc d = desc[p];
    const uint64_t off = (uint64_t)d.off16 * 16u;
    if (d.len < 42u || off + (((uint64_t)d.len + 15u) & ~15ull) > arena_bytes) return;
    arena[off + 24u] ^= 0xFFu;
    arena[off + 40u] ^= 0xFFu;
}

hipError_t launch_stale_every(uint8_t* arena, uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n,
                              uint32_t every, hipStream_t stream) {
    if (n == 0 || every == 0) return hipSuccess;
    const uint32_t m = (n + every - 1u) / every;
    hipLaunchKernelGGL(stale_every_kernel, dim3((m + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, arena,
                       arena_bytes, desc, n, every);
    return hipGetLastError();
}

DEV uint64_t wave_sum64(uint64_t x) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
#define NFCS_DPP_STEP(ctrl)                                                              \
    {                                                                                    \
        uint32_t l2_ = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, ctrl, 0xF, 0xF, true); \
        uint32_t h2_ = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, ctrl, 0xF, 0xF, true); \
        uint64_t s_ = ((uint64_t)hi << 32 | lo) + ((uint64_t)h2_ << 32 | l2_);           \
        lo = (uint32_t)s_;                                                               \
        hi = (uint32_t)(s_ >> 32);                                                       \
    }
    NFCS_DPP_STEP(0xB1)   // quad_perm [1,0,3,2]
    NFCS_DPP_STEP(0x4E)   // quad_perm [2,3,0,1]
    NFCS_DPP_STEP(0x141)  // row_half_mirror
    NFCS_DPP_STEP(0x140)  // row_mirror: every lane of a 16-lane row now holds the row sum
#undef NFCS_DPP_STEP
    uint64_t s = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        s += ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, 16 * r) << 32) |
             (uint32_t)__builtin_amdgcn_readlane((int)lo, 16 * r);
    return s;
}

// ---- order-independent frame digest (same as oracle nfo_digest) --------------
__global__ __launch_bounds__(kBlock) void digest_kernel(const uint8_t* __restrict__ arena,
                                                        uint64_t arena_bytes,
                                                        const nfcs_desc* __restrict__ desc,
                                                        uint32_t n, uint64_t first,
                                                        unsigned long long* __restrict__ ct) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    uint64_t wsum = 0;  // uniform
    for (uint32_t p = blockIdx.x * kWavesPerBlock + rfl(threadIdx.x >> 6); p < n; p += nw) {
        const nfcs_desc d = desc[p];
        const uint64_t off = (uint64_t)d.off16 * 16u;
        const uint32_t len = d.len;
        if (off + (((uint64_t)len + 15) & ~15ull) > arena_bytes) continue;
        const uint4* src = (const uint4*)(arena + off);
        const uint32_t nch = (len + 15u) >> 4;
        uint64_t acc = 0;
        for (uint32_t c = lane; c < nch; c += 64u) {
            uint4 v = src[c];
            uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
            const uint32_t o = c * 16u;
            if (o + 16 > len) {  // bytes >= len read as zero
                const uint32_t keep = len - o;  // 1..15
                if (keep < 8) { lo &= (1ull << (8 * keep)) - 1ull; hi = 0; }
                else if (keep == 8) { hi = 0; }
                else { hi &= (1ull << (8 * (keep - 8))) - 1ull; }
            }
            acc += mix64(lo ^ mix64(hi + (uint64_t)(c + 1) * kGolden));
        }
        const uint64_t h = mix64((uint64_t)len * 0xD6E8FEB86659FD93ull + wave_sum64(acc));
        wsum += mix64(h ^ ((first + p) * 0xA0761D6478BD642Full));
    }
    // the four waves' sums meet in LDS (every wave leaves its loop and reaches the barrier), and thread 0 adds the
    // workgroup's sum to its stripe of the counter scratch (nfcs_internal.h); counter_fold_kernel adds them to *out
    __shared__ unsigned long long s_sum[kWavesPerBlock];
    if (lane == 0) s_sum[threadIdx.x >> 6] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) t += s_sum[w];
        if (t) atomicAdd(ct + (blockIdx.x % kCtStripes) * kCtLineSlots, t);
    }
}

hipError_t launch_digest(const DevInfo& di, const uint8_t* arena, uint64_t arena_bytes,
                         const nfcs_desc* desc, uint32_t n, uint64_t first, uint64_t* d_out, uint64_t* ct,
                         hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!ct) return hipErrorInvalidValue;
    uint32_t grid = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    if (grid > (uint32_t)di.cus * 8u) grid = (uint32_t)di.cus * 8u;
    uint64_t* stripes = ct + kCtDigestAt;
    hipLaunchKernelGGL(digest_kernel, dim3(grid), dim3(kBlock), 0, stream, arena, arena_bytes,
                       desc, n, first, (unsigned long long*)stripes);
    launch_counter_fold<kCtStripes>(stripes, kCtLineSlots, 1u, d_out, nullptr, stream);
    return hipGetLastError();
}

// ---- TX queues: append, and the dequeue as plan / gather / commit ---------------------
// Every loop bound below is a launch parameter (`trips`) or a constant of at most 10; no atomics, no
// inline assembly, plain vector loads and stores.

DEV TxqPort txq_port(const TxqDev& t, uint32_t p) {
    const uint4 r = t.port[p];
    return TxqPort{r.x, r.y, r.z, r.w};
}

// The key whose range of `start` (keys + 1 ascending words, start[0] = 0) holds e: the last k with
// start[k] <= e, by an upper-bound search of `trips` >= bit_length(keys + 1) steps, so empty keys (equal
// neighbours) are stepped over. e >= start[keys] gives keys; the callers guard k < keys.
DEV uint32_t txq_find_key(const uint32_t* __restrict__ start, uint32_t keys, uint32_t trips, uint32_t e) {
    uint32_t lo = 0, hi = keys + 1u;  // the first index in [0, keys] with start[index] > e, or keys + 1
    for (uint32_t s = 0; s < trips; ++s) {
        if (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (start[mid] > e) hi = mid;
            else lo = mid + 1u;
        }
    }
    return lo - 1u;
}

// One lane per enqueued position j < key_start[keys]; the grid covers n. Consecutive lanes of one key
// store consecutive ring slots (up to the wrap); the handle is gathered at order[j].
__global__ __launch_bounds__(kBlock) void txq_append_kernel(const TxqDev t, const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ key_start,
                                                            const uint32_t* __restrict__ depth,
                                                            const uint64_t* __restrict__ handle,
                                                            const nfcs_desc* __restrict__ desc, uint32_t n,
                                                            uint32_t trips, uint64_t handle_base) {
    const uint64_t j64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j64 >= n) return;
    const uint32_t j = (uint32_t)j64, keys = t.keys;
    if (j >= key_start[keys]) return;
    const uint32_t k = txq_find_key(key_start, keys, trips, j);
    if (k >= keys) return;
    const uint32_t b = key_start[k], e = key_start[k + 1u];
    if (j < b || j >= e || e > n) return;
    const uint32_t cnt = e - b, d = depth[k];
    const TxqPort pr = txq_port(t, k / kTxqQ);
    const uint32_t cap = txq_cap(pr, k % kTxqQ), head = t.head[k];
    if (cap == 0u || d < cnt || d > cap || head >= cap) return;  // inconsistent input: nothing for this key
    const uint32_t i = order[j];
    if (i >= n) return;
    uint64_t pos = (uint64_t)head + (d - cnt) + (j - b);  // below 2 * cap
    if (pos >= cap) pos -= cap;
    const uint64_t slot = t.ring_base[k] + pos;
    if (pos >= cap || slot >= t.ring_slots) return;
    uint64_t h;
    if (handle) {
        h = handle[i];
    } else if (desc) {
        const uint2 dl = ((const uint2*)desc)[i];
        h = txq_desc_handle(dl.x, dl.y);
    } else {
        h = handle_base + i;
    }
    t.ring[slot] = h;
}

hipError_t launch_txq_append(const TxqDev& t, const uint32_t* order, const uint32_t* key_start, const uint32_t* depth,
                             const uint64_t* handle, const nfcs_desc* desc, uint32_t n, hipStream_t stream,
                             uint64_t handle_base) {
    if (n == 0 || t.keys == 0) return hipSuccess;
    const uint32_t trips = 32u - (uint32_t)__builtin_clz(t.keys + 1u);
    hipLaunchKernelGGL(txq_append_kernel, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, t, order, key_start,
                       depth, handle, desc, n, trips, handle_base);
    return hipGetLastError();
}

// The plan: one workgroup, one lane per port. want = min(budget, sum D), W = its exclusive prefix over the
// ports in 64 bits (an LDS scan), G by the tx_cap rule, take[q] by txq_take.
__global__ __launch_bounds__(kTxqPlanThreads) void txq_plan_kernel(const TxqDev t, const uint32_t* __restrict__ budget,
                                                                   uint32_t budget_all,
                                                                   const uint32_t* __restrict__ depth, uint32_t tx_cap,
                                                                   uint32_t* __restrict__ tx_start_out) {
    __shared__ uint64_t scan[kTxqPlanThreads];
    const uint32_t p = threadIdx.x;
    const bool live = p < t.ports;
    TxqPort pr{0u, 0u, 0u, 0u};
    uint32_t D[kTxqQ] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t want = 0;
    if (live) {
        pr = txq_port(t, p);
        uint32_t d8[kTxqQ];
        for (uint32_t q = 0; q < kTxqQ; ++q) d8[q] = depth[p * kTxqQ + q];
        const uint64_t sum = txq_depths(pr, d8, D);
        const uint32_t b = budget ? budget[p] : budget_all;
        want = (uint32_t)(sum < b ? sum : b);
    }
    scan[p] = want;
    __syncthreads();
    for (uint32_t off = 1; off < kTxqPlanThreads; off <<= 1) {  // inclusive scan, 10 steps
        const uint64_t v = p >= off ? scan[p - off] : 0ull;
        __syncthreads();
        scan[p] += v;
        __syncthreads();
    }
    const uint64_t incl = scan[p];
    if (t.ports == 0u) {
        if (p == 0u) {
            t.tx_start[0] = 0u;
            tx_start_out[0] = 0u;
            t.elem_start[0] = 0u;
        }
        return;
    }
    if (!live) return;
    uint32_t start, take[kTxqQ], new_last;
    const uint32_t last = t.last[p];
    const uint32_t G = txq_grant(incl - want, want, tx_cap, &start);
    txq_take(pr, last, D, G, take, &new_last);
    t.tx_start[p] = start;
    tx_start_out[p] = start;
    t.new_last[p] = new_last;
    uint32_t run = start;
    for (uint32_t q = 0; q < kTxqQ; ++q) {
        t.take[p * kTxqQ + q] = take[q];
        t.elem_start[p * kTxqQ + q] = run;
        run += take[q];
    }
    if (p == t.ports - 1u) {
        const uint32_t total = (uint32_t)(incl < tx_cap ? incl : tx_cap);
        t.tx_start[t.ports] = total;
        tx_start_out[t.ports] = total;
        t.elem_start[t.keys] = total;
    }
}

// The gather: one lane per dequeued element e < tx_start[ports], in key order, so consecutive lanes read
// consecutive ring slots; each stores its handle at its TX rank within the port's segment.
__global__ __launch_bounds__(kBlock) void txq_gather_kernel(const TxqDev t, const uint32_t* __restrict__ depth,
                                                            uint64_t* __restrict__ tx, uint32_t tx_cap,
                                                            uint8_t* __restrict__ tx_queue, uint32_t trips) {
    const uint64_t e64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t keys = t.keys;
    if (e64 >= tx_cap || e64 >= t.elem_start[keys]) return;
    const uint32_t e = (uint32_t)e64;
    const uint32_t k = txq_find_key(t.elem_start, keys, trips, e);
    if (k >= keys) return;
    const uint32_t r = e - t.elem_start[k];
    if (r >= t.take[k]) return;
    const uint32_t p = k / kTxqQ, q = k % kTxqQ;
    const TxqPort pr = txq_port(t, p);
    uint32_t d8[kTxqQ], D[kTxqQ];
    for (uint32_t o = 0; o < kTxqQ; ++o) d8[o] = depth[p * kTxqQ + o];
    txq_depths(pr, d8, D);
    const uint32_t cap = txq_cap(pr, q), head = t.head[k];
    if (cap == 0u || head >= cap || r >= cap) return;
    uint64_t pos = (uint64_t)head + r;  // below 2 * cap
    if (pos >= cap) pos -= cap;
    const uint64_t slot = t.ring_base[k] + pos;
    if (slot >= t.ring_slots) return;
    const uint64_t h = t.ring[slot];
    const uint64_t rank = txq_rank(pr, t.last[p], D, q, r);
    const uint32_t seg = t.tx_start[p], seg_end = t.tx_start[p + 1u];
    const uint64_t dst = seg + rank;
    if (dst >= seg_end || dst >= tx_cap) return;
    tx[dst] = h;
    if (tx_queue) tx_queue[dst] = (uint8_t)q;
}

// The commit: one lane per key, after the gather (which reads the old heads, depths and last).
__global__ __launch_bounds__(kBlock) void txq_commit_kernel(const TxqDev t, uint32_t* __restrict__ depth,
                                                            uint32_t* __restrict__ dequeued) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= t.keys) return;
    const uint32_t tk = t.take[k];
    if (dequeued) dequeued[k] = tk;
    if (k % kTxqQ == 0u) t.last[k / kTxqQ] = t.new_last[k / kTxqQ];
    if (tk == 0u) return;
    const uint32_t cap = txq_cap(txq_port(t, k / kTxqQ), k % kTxqQ);
    if (cap == 0u) return;
    depth[k] -= tk;  // tk <= min(depth, cap)
    uint64_t h = (uint64_t)t.head[k] + tk;
    if (h >= cap) h -= cap;
    t.head[k] = (uint32_t)h;
}

hipError_t launch_txq_dequeue(const TxqDev& t, const uint32_t* budget, uint32_t budget_all, uint32_t* depth,
                              uint64_t* tx, uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start, uint32_t* dequeued,
                              hipStream_t stream) {
    hipLaunchKernelGGL(txq_plan_kernel, dim3(1), dim3(kTxqPlanThreads), 0, stream, t, budget, budget_all, depth, tx_cap,
                       tx_start);
    const uint64_t most = t.ring_slots < tx_cap ? t.ring_slots : tx_cap;
    if (most > 0 && t.keys > 0) {
        const uint32_t trips = 32u - (uint32_t)__builtin_clz(t.keys + 1u);
        hipLaunchKernelGGL(txq_gather_kernel, dim3((uint32_t)((most + kBlock - 1u) / kBlock)), dim3(kBlock), 0, stream, t,
                           depth, tx, tx_cap, tx_queue, trips);
    }
    if (t.keys > 0)
        hipLaunchKernelGGL(txq_commit_kernel, dim3((t.keys + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, t, depth,
                           dequeued);
    return hipGetLastError();
}

}  // namespace nfcs

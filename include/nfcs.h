/*
 * nfcs.h — C ABI of the MI355X batched Internet-checksum engine.
 *
 * This is the drop-in boundary for NetFlow++'s checksum path:
 *
 *   netflow::Packet::update_checksums()      include/netflow++/packet.hpp:722-890
 *   netflow::Packet::calculate_checksum()    include/netflow++/packet.hpp:894-912
 *
 * The reference exposes the path as a non-virtual inline C++ member that works on ONE
 * packet in a PacketBuffer (packet_buffer.hpp:10-111). This ABI exposes the same
 * computation over a BATCH of frames laid out in one arena (device or pinned host memory)
 * and described by 8-byte descriptors. Every function returns an int status (0 = OK,
 * < 0 = error; see nfcs_strerror) and never throws across the ABI. Per-packet results are
 * written in place into the frames exactly as the reference writes them (bit-exact,
 * including its quirks — SURVEY.md Appendix A), plus an optional per-packet status byte
 * that records which branch of update_checksums() ran (the reference returns void and
 * silently skips malformed packets: packet.hpp:758,763,780,784,786,791-793,830,834-836).
 *
 * No torch / HIP types appear in the signatures: streams are passed as void* (a
 * hipStream_t, or NULL for the context's own stream).
 */
#ifndef NFCS_H
#define NFCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define NFCS_API __attribute__((visibility("default")))
#else
#define NFCS_API
#endif

/* ABI versions: 1 = rounds 1-4; 2 = round 5 on: nfcs_update_host_frames, and nfcs_update_host accepts
 * descriptors in any order (an ABI-1 library returns NFCS_EINVAL for a burst that is not one ascending
 * run). A caller that needs either checks nfcs_abi_version() >= 2. */
#define NFCS_ABI_VERSION 2

/* ---- data layout ------------------------------------------------------------------ */

/* One frame inside an arena: bytes arena[off16*16, off16*16 + len).
 * Replaces PacketBuffer's data window [get_data_start_ptr(), +get_data_length())
 * (packet_buffer.hpp:51-52). Frames start on 16-byte boundaries; the arena must cover
 * off16*16 + round_up(len, 16) bytes for every descriptor (the kernel reads whole 16-byte
 * chunks; a descriptor outside the arena is rejected per packet with NFCS_ST_BAD_DESC).
 * Frames of one batch must not overlap (as separate PacketBuffers never do): the kernels may
 * rewrite a frame's own 16-byte chunks whole, with the values they read from them. */
typedef struct nfcs_desc {
    uint32_t off16; /* frame start, in 16-byte units from the arena base */
    uint32_t len;   /* frame length in bytes (PacketBuffer::data_len_)     */
} nfcs_desc;

/* What update_checksums() wrote into one frame: at most two 2-byte fields. Applying
 * ip then l4 to the original frame reproduces the updated frame exactly (also when the two
 * fields overlap, IHL < 5). Offsets are frame offsets; 0xFFFF = field not written. */
typedef struct nfcs_patch {
    uint16_t ip_off;  /* IPv4 header checksum field: l2 + 10                         */
    uint16_t l4_off;  /* L4 checksum field: TCP l4+15 (sic), UDP l4+6, ICMP l4+2     */
    uint8_t ip[2];    /* bytes written at ip_off (big-endian checksum)               */
    uint8_t l4[2];    /* bytes written at l4_off                                     */
} nfcs_patch;

#define NFCS_PATCH_NONE 0xFFFFu

/* ---- per-packet status (which branch of update_checksums() ran) -------------------- */
enum {
    NFCS_ST_NONE = 0,       /* neither IPv4 (by version nibble) nor IPv6: untouched (packet.hpp:761-765) */
    NFCS_ST_V4 = 1,         /* IPv4 header checksum written; protocol not TCP/UDP/ICMP              */
    NFCS_ST_V4_TCP = 2,     /* IPv4 header + TCP checksum (TCP field at l4+15, packet.hpp:258-270)  */
    NFCS_ST_V4_UDP = 3,     /* IPv4 header + UDP checksum                                            */
    NFCS_ST_V4_ICMP = 4,    /* IPv4 header + ICMP checksum                                           */
    NFCS_ST_V4_L4SKIP = 5,  /* IPv4 header written; TCP/UDP/ICMP branch returned early (bounds)    */
    NFCS_ST_V6 = 6,         /* IPv6 detected, next header neither TCP nor UDP: untouched            */
    NFCS_ST_V6_TCP = 7,     /* IPv6 TCP checksum                                                     */
    NFCS_ST_V6_UDP = 8,     /* IPv6 UDP checksum                                                     */
    NFCS_ST_V6_L4SKIP = 9,  /* IPv6 TCP/UDP branch returned early (bounds): untouched                */
    /* nfcs_l3_forward_device only (switch.hpp:247-294); such frames are left untouched:    */
    NFCS_ST_NO_ROUTE = 11,  /* next-hop index >= table size: no route / ARP miss (282-294)       */
    NFCS_ST_NOT_IPV4 = 12,  /* L3 EtherType (after one tag) not IPv4, or ipv4() absent (265-267) */
    NFCS_ST_TTL_EXPIRED = 13, /* TTL <= 1: the switch sends ICMP time exceeded and drops (278)   */
    NFCS_ST_OOB = 14,       /* IPv4 with l2 + IHL*4 > len: the reference reads past the frame (UB);
                               outside the parity domain, frame left untouched                      */
    NFCS_ST_BAD_DESC = 15,  /* descriptor reaches past arena_bytes: frame not touched                */
    NFCS_ST_VLAN_FAIL = 16, /* nfcs_vlan_device: push_vlan / pop_vlan returned false (no tag to pop,
                               runt frame, no tailroom): frame and length untouched                 */
    NFCS_ST_FLAG_VLAN = 0x20, /* OR-ed in by nfcs_vlan_device: the tag was pushed / re-written /
                                 popped, then the update_checksums() status in the low bits      */
    NFCS_ST_FLAG_OVERLAP = 0x40, /* OR-ed in: IPv4 IHL < 5 with TCP/UDP/ICMP, so the L4 region
                                   overlaps the IPv4 header; handled by the exact sequential path */
    NFCS_ST_FLAG_FWD = 0x80     /* OR-ed in by nfcs_l3_forward_device: TTL decremented, MACs
                                   rewritten, then the update_checksums() status in the low bits */
};

/* ---- error codes -------------------------------------------------------------------- */
enum {
    NFCS_OK = 0,
    NFCS_EINVAL = -1,   /* bad argument (null pointer with n > 0, misaligned arena, ...) */
    NFCS_EHIP = -2,     /* a HIP runtime call failed; nfcs_last_hip_error() has the code  */
    NFCS_ENOMEM = -3,   /* allocation failed                                              */
    NFCS_ENODEV = -4    /* no such device / no gfx950 device                              */
};

/* Synthetic workload configurations (BASELINE.json "configs"). */
enum {
    NFCS_CFG_C0_64B_V4 = 0,   /* 64 B IPv4, protocol 253 (header checksum only)   */
    NFCS_CFG_C1_1500B_UDP = 1,/* 1500 B IPv4 + UDP                                 */
    NFCS_CFG_C2_9000B_TCP = 2,/* 9000 B IPv4 + TCP                                 */
    NFCS_CFG_C3_MIXED = 3     /* U{64..1500} B, 50/50 IPv4 TCP/UDP                 */
};

typedef struct nfcs_ctx nfcs_ctx;

/* ---- library / context ---------------------------------------------------------------- */
NFCS_API int nfcs_abi_version(void);
NFCS_API const char* nfcs_strerror(int err);
NFCS_API int nfcs_last_hip_error(void);

/* Threads: any entry point may be called from any host thread; it makes the context's device
 * current for its duration and restores the caller's device on return. Calls on ONE context are
 * serialised by the caller (or ordered by a stream); different contexts run concurrently
 * (netflow_amd::MultiGpu, include/netflow_amd/multi_gpu.hpp: one thread per GPU). */

/* One context per device: owns a stream, events and the pinned staging ring used by
 * nfcs_update_host. Calls on one context must be serialised by the caller. */
NFCS_API int nfcs_ctx_create(int device, nfcs_ctx** out);
NFCS_API int nfcs_ctx_destroy(nfcs_ctx* ctx);
NFCS_API void* nfcs_ctx_stream(nfcs_ctx* ctx); /* the context's own hipStream_t */
/* Launch shapes (speed only; the bytes written never depend on them) follow the mean footprint per
 * packet: 8-lane rows for short frames, 16-lane rows for long ones, long-frame sub-batches. Without
 * a hint it is arena_bytes / n, which is exact for a batch that fills its arena and otherwise only
 * over-estimates; when that estimate says "long" or "8-lane rows", the update, the L3 forward and
 * VLAN also sample the frames on the device (256 descriptors, one wave, no host sync: the mean of their
 * lengths rounded up to 128 and how many exceed one 8-lane row pass), and the next call over the same
 * burst (descriptor array, n and arena_bytes) launches in the shape the sample calls for — a burst
 * inside a larger ring (a NIC ring reusing its descriptor array) adapts after one call,
 * and so does a densely packed mix of short and long frames (§5e). A caller may
 * instead state its frames' mean slot size, e.g. 128 for 64-byte frames in 128-byte slots; 0 (the
 * default) restores the automatic choice. Applies to the device-path calls that follow on ctx
 * (update, L3 forward, VLAN; nfcs_update_host measures each staged chunk itself). */
NFCS_API int nfcs_ctx_set_slot_bytes(nfcs_ctx* ctx, uint32_t bytes);
/* The mean footprint per packet (bytes) that the next device-path call on ctx over this burst
 * (d_arena of arena_bytes, d_desc, n) picks its launch shape from: the slot-size hint, arena_bytes / n,
 * or the footprint the previous call over the same burst sampled (once that call has finished).
 * No side effect; speed only (the bytes written never depend on it). */
NFCS_API int nfcs_ctx_launch_footprint(nfcs_ctx* ctx, uint64_t arena_bytes, const nfcs_desc* d_desc,
                                       uint32_t n, uint64_t* mean);
/* The form of nfcs_update_device on more than 65,536 long frames without d_patch:
 * deferred (sub-batches of a read pass that writes patch records and a write pass that stores them: the
 * fastest when most frames need their checksum bytes stored) or sparse (one read pass that stores the few
 * differing fields inline: the fastest when hardly any frame does, as with received traffic). AUTO (the
 * default) starts deferred and follows the store demand that the context's last calls observed: sparse
 * once the two newest observations found nearly nothing to store, deferred again after one that did, and
 * after a call on another stream than the previous update call's. Speed only: frame bytes, status bytes and
 * records never depend on the form. A call with d_patch always runs deferred. These two symbols were added
 * without changing NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup. */
#define NFCS_STORE_AUTO 0
#define NFCS_STORE_DEFERRED 1
#define NFCS_STORE_SPARSE 2
NFCS_API int nfcs_ctx_set_store_policy(nfcs_ctx* ctx, int policy);
/* *form = the form the newest nfcs_update_device call on ctx ran in (NFCS_STORE_DEFERRED or
 * NFCS_STORE_SPARSE; 0: none yet, or a call the forms do not apply to); *sampled / *storing = the newest
 * store-demand observation a finished call has delivered: how many packets it sampled and how many of
 * them needed a store (both 0: none yet). A call's observation is delivered by the next such call on the
 * context once that has started. Any pointer may be null. For tests and tools. */
NFCS_API int nfcs_ctx_store_state(nfcs_ctx* ctx, int* form, uint32_t* sampled, uint32_t* storing);
/* The host staging ring of nfcs_update_host (allocated by this call if not yet): *node = the GPU's
 * NUMA node (-1 if unknown), *local = 1 when the ring's pinned memory is bound to that node (its
 * copy threads then run on that node's CPUs). SURVEY.md §8e: one GPU per host thread, staging
 * NUMA-local to each GPU. */
NFCS_API int nfcs_ctx_host_numa(nfcs_ctx* ctx, int* node, int* local);

/* ---- the hot path --------------------------------------------------------------------- */

/* Batched Packet::update_checksums() on device-resident frames (packet.hpp:722-890).
 *   d_arena      device pointer, 16-byte aligned, frames mutated in place
 *   arena_bytes  size of the arena in bytes (descriptors are checked against it)
 *   d_desc       n device-resident descriptors
 *   d_status     optional (NULL) n status bytes, NFCS_ST_*
 *   d_patch      optional (NULL) n nfcs_patch records describing the bytes written
 *   stream       hipStream_t or NULL (context stream). Asynchronous: completion is
 *                observed by synchronising the stream.
 * Launches (speed only; the bytes written never depend on them): a call of at most 65,536
 * packets is one kernel; waves of long frames write their checksum bytes in a second, write-only
 * pass; a long-frame call of more than 1M packets runs as consecutive 512K-packet sub-batches. */
NFCS_API int nfcs_update_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                                const nfcs_desc* d_desc, uint32_t n, uint8_t* d_status,
                                nfcs_patch* d_patch, void* stream);

/* Same on host memory (NIC / socket buffers). Synchronous. Descriptors may come in any order;
 * each run of ascending offsets is staged as a contiguous span (a NIC ring burst that wraps past
 * the ring's end is two runs; ABI 1 required one ascending run). Frames go H2D in
 * chunks on two streams (from a pageable arena through the context's pinned ring, copied by host
 * threads; a pinned arena — nfcs_host_alloc — is copied from directly), the kernel runs per
 * chunk, and only the 8-byte nfcs_patch records come back and are applied on the host. A frame
 * inside the arena longer than NFCS_FRAME_RELEVANT_BYTES is staged as its first
 * NFCS_FRAME_RELEVANT_BYTES bytes, with the same result (see nfcs_update_host_frames); before round 6
 * a frame larger than one 64 MiB staging slot was NFCS_EINVAL. Pinned bursts of up to 32 MiB run
 * zero-copy (below).
 * flags:
 *   NFCS_HOST_FRAMES     copy whole frames back instead of patch records (same bytes, slower;
 *                        each chunk's span goes back whole, so bytes between the burst's frames
 *                        are rewritten with the values read: not for a ring whose other slots
 *                        are being filled meanwhile — the default writes only checksum bytes)
 *   NFCS_HOST_ZERO_COPY  pinned arenas only: the kernel reads the frames over PCIe in place and
 *                        writes the checksum bytes straight back (no staging copies); the default
 *                        form for pinned bursts of up to 32 MiB (round 6: one launch, no DMA)
 *   NFCS_HOST_PATCH_ONLY the default since ABI 1 session 2; accepted and ignored
 * Rates: DESIGN.md §7. */
/* A pinned burst whose frames (its runs of ascending offsets, gaps included) span at most this many bytes
 * runs zero-copy unless NFCS_HOST_FRAMES is given (round 6): one kernel launch and no DMA, the kernel
 * reading only the frames' own bytes; larger bursts go through the copy engines. */
#define NFCS_HOST_ZERO_COPY_AUTO_BYTES (32u << 20)
#define NFCS_HOST_PATCH_ONLY 1u
#define NFCS_HOST_ZERO_COPY 2u
#define NFCS_HOST_FRAMES 4u
NFCS_API int nfcs_update_host(nfcs_ctx* ctx, uint8_t* h_arena, uint64_t arena_bytes,
                              const nfcs_desc* h_desc, uint32_t n, uint8_t* h_status,
                              uint32_t flags);

/* Batched Packet::update_checksums() over n frames scattered in host memory, one pointer each —
 * the form a NetFlow++ caller holds them in: frames[i] / lens[i] = the i-th packet's
 * PacketBuffer::get_data_start_ptr() / get_data_length() (packet_buffer.hpp:21-31, 51-52: one
 * `new[]` per buffer, BufferPool::allocate_buffer, buffer_pool.hpp:57-94). Synchronous. The frames
 * are gathered in chunks (16-byte aligned, back to back) into the context's NUMA-local pinned ring
 * by its copy threads, moved H2D, checksummed on the GPU in the records-only form, and the 2+2
 * checksum bytes written back into each frame in place (ip field first, then l4, the reference's
 * write order); the gather, the transfers, the kernel and the write-back of successive chunks
 * overlap on two streams. Only the bytes the reference writes are written. frames[i] == NULL or
 * lens[i] == 0: nothing read or written, status NFCS_ST_NONE. A frame longer than
 * NFCS_FRAME_RELEVANT_BYTES is processed as its first NFCS_FRAME_RELEVANT_BYTES bytes, with the same
 * result: update_checksums() reads, and compares with data_len, no offset past 65,613 (l2 18 + IHL 60
 * + a 16-bit length; packet.hpp:728-889), so any longer length passes each of its bounds tests alike
 * (ABI 2 as first shipped returned NFCS_EINVAL above 64 MiB). Frames must not overlap.
 *   h_status  optional (NULL) n status bytes, NFCS_ST_*
 *   flags     0 (reserved) */
#define NFCS_FRAME_RELEVANT_BYTES 131072u
NFCS_API int nfcs_update_host_frames(nfcs_ctx* ctx, uint8_t* const* frames, const uint32_t* lens, uint32_t n,
                                     uint8_t* h_status, uint32_t flags);

/* ---- fused L3 forward ------------------------------------------------- */

/* One next hop: the MACs Switch::process_received_packet writes (switch.hpp:286-289). */
typedef struct nfcs_nexthop {
    uint8_t dst_mac[6]; /* ARP-resolved next-hop MAC (arp_processor_.lookup_mac)      */
    uint8_t src_mac[6]; /* egress interface MAC (interface_manager_.get_interface_mac) */
} nfcs_nexthop;
#define NFCS_NH_NONE 0xFFFFFFFFu

/* Batched data path of the switch's transit-IPv4 forward (switch.hpp:247-294) in one HBM read pass:
 * for packet i with L3 EtherType IPv4 and an IPv4 header, TTL <= 1 -> NFCS_ST_TTL_EXPIRED;
 * d_nh[i] >= table_n -> NFCS_ST_NO_ROUTE; else TTL--, dst/src MAC = d_table[d_nh[i]], then
 * Packet::update_checksums(), status = its status | NFCS_ST_FLAG_FWD. Frames that are not
 * forwarded are untouched. The decision in front of it (is_my_ip, route and ARP lookup) arrives as
 * next-hop indexes: nfcs_route_lookup_device (below) computes them on the device from a nfcs_fib,
 * whose table nfcs_fib_nexthops hands in as d_table; a caller with its own control plane may still
 * pass any indexes into any table. The ACL in front of both is nfcs_acl_eval_device (further
 * below): run between the lookup and the forward it sets d_nh[i] = NFCS_NH_NONE for every packet
 * the ingress ACL does not permit, so this call leaves that frame untouched. Classification stays
 * with the caller (nfcs_flow_keys_device computes its keys).
 *   d_nh     n device-resident u32 next-hop indexes (NFCS_NH_NONE = no route)
 *   d_table  table_n device-resident next hops
 * Launches (speed only): one kernel; a burst of more than 1M long frames runs as 512K-packet
 * sub-batches whose long-frame waves write their header rewrites in a second pass.
 * Asynchronous on the stream; d_nh and d_table must stay valid until it completes. */
NFCS_API int nfcs_l3_forward_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                                    const nfcs_desc* d_desc, const uint32_t* d_nh, uint32_t n,
                                    const nfcs_nexthop* d_table, uint32_t table_n,
                                    uint8_t* d_status, void* stream);

/* ---- route and ARP lookup in front of the forward ----------------------------------------- */

/* The symbols of this section were added without changing NFCS_ABI_VERSION (it stays 2): a caller
 * that may meet an older library detects them by symbol lookup (dlsym "nfcs_fib_create"). */

/* The switch's L3 decision for one packet (switch.hpp:259-301), in the order it is taken. */
enum {
    NFCS_RT_FORWARD = 0,     /* d_nh[i] = index into the FIB's next-hop table                        */
    NFCS_RT_BAD_DESC = 1,    /* descriptor reaches outside the arena: frame not read                 */
    NFCS_RT_NOT_IPV4 = 2,    /* the forward's predicate: len < 14, or the L3 EtherType after at most
                                one 0x8100 tag is not 0x0800 (a tagged frame shorter than 18 keeps
                                0x8100), or len < 34 (38 if tagged): ipv4() absent (259-269)         */
    NFCS_RT_LOCAL = 3,       /* dst is one of the switch's own addresses (is_my_ip, 270)             */
    NFCS_RT_TTL_EXPIRED = 4, /* TTL <= 1 (279)                                                       */
    NFCS_RT_NO_ROUTE = 5,    /* no route entry matches (282-283, 301)                                */
    NFCS_RT_ARP_MISS = 6,    /* the next hop (the gateway, or dst itself when next_hop_ip == 0) has
                                no ARP entry (285-288, 300)                                          */
    NFCS_RT_NO_IF_MAC = 7    /* the route's egress interface has no MAC (291-292)                    */
};
#define NFCS_IF_NONE 0xFFFFFFFFu /* d_egress_if[i] of every verdict but NFCS_RT_FORWARD */

/* One route, RouteEntry without its metric (routing_manager.hpp). IPv4 addresses here and below are
 * uint32_t in network byte order — the four address bytes as they lie in the frame, read as one
 * u32 — which is the value of the reference's IpAddress. */
typedef struct nfcs_fib_route {
    uint32_t network;     /* destination_network (already masked)   */
    uint32_t mask;        /* subnet_mask; need not be contiguous    */
    uint32_t next_hop_ip; /* 0 = directly connected                 */
    uint32_t egress_if;   /* egress_interface_id                    */
} nfcs_fib_route;
typedef struct nfcs_fib_arp {
    uint32_t ip;
    uint8_t mac[6];
    uint8_t pad[2];
} nfcs_fib_arp;
typedef struct nfcs_fib_if_mac {
    uint32_t egress_if;
    uint8_t mac[6];
    uint8_t pad[2];
} nfcs_fib_if_mac;

#define NFCS_FIB_MAX_ROUTES 4096u /* 32 KiB of {network, mask} pairs in LDS */

/* The forwarding table: routes, ARP entries, interface MACs and the switch's own addresses, compiled
 * by nfcs_fib_commit into what the lookup reads and a static next-hop table for the forward.
 *   routes    in LOOKUP ORDER: the first entry with (dst & mask) == network wins, exactly as
 *             RoutingManager::lookup_route scans its vector (routing_manager.cpp:80-92). The order is
 *             taken as given — pass RoutingManager::get_routing_table() as it is. The reference's own
 *             sort (popcount of mask, metric, network; a std::sort, so ties land in unspecified
 *             order) is not re-implemented here. More than NFCS_FIB_MAX_ROUTES: NFCS_EINVAL.
 *   arp       {ip, mac} in any order; of duplicates the last one wins (std::map assignment).
 *   if_macs   {egress_if, mac}; of duplicates the last one wins.
 *   local     the switch's own addresses (InterfaceManager::is_my_ip).
 * Each setter copies its array (NULL with n > 0: NFCS_EINVAL) and invalidates an earlier commit:
 * nfcs_fib_lookup_host and nfcs_fib_nexthops_host then return NFCS_EINVAL until the next
 * nfcs_fib_commit. An earlier upload is NOT invalidated: nfcs_route_lookup_device and
 * nfcs_fib_nexthops keep serving the tables of the last nfcs_fib_upload, so the device may run on
 * while the host prepares the next table — and host and device answers can differ from the first
 * setter call until the next commit AND upload. A caller that needs them equal uploads after
 * every commit.
 * The compiled next-hop table has one entry per distinct ARP address, then one per route with a
 * gateway. ARP entry a serves packets whose destination is ip[a] on a connected route: every address
 * has exactly one first-matching route, so its entry is {mac[a], if_mac(route(ip[a]).egress_if)},
 * and unusable when that route is missing, has a gateway, or its interface has no MAC. A gateway
 * route resolves arp(next_hop_ip) and if_mac(egress_if) once, at commit; a miss becomes the route's
 * verdict. Unusable entries stay in the table as zeros so indexes do not shift; the lookup never
 * hands them out. */
typedef struct nfcs_fib nfcs_fib;
NFCS_API int nfcs_fib_create(nfcs_fib** out);
NFCS_API int nfcs_fib_destroy(nfcs_fib* fib); /* also frees what nfcs_fib_upload allocated */
NFCS_API int nfcs_fib_set_routes(nfcs_fib* fib, const nfcs_fib_route* routes, uint32_t n);
NFCS_API int nfcs_fib_set_arp(nfcs_fib* fib, const nfcs_fib_arp* arp, uint32_t n);
NFCS_API int nfcs_fib_set_if_macs(nfcs_fib* fib, const nfcs_fib_if_mac* if_macs, uint32_t n);
NFCS_API int nfcs_fib_set_local_ips(nfcs_fib* fib, const uint32_t* ips, uint32_t n);
NFCS_API int nfcs_fib_commit(nfcs_fib* fib);
/* Copies the committed tables to ctx's device (synchronous; replaces an earlier upload, which must
 * no longer be in use). NFCS_EINVAL before nfcs_fib_commit. The fib must be destroyed before ctx. */
NFCS_API int nfcs_fib_upload(nfcs_ctx* ctx, nfcs_fib* fib);
/* The uploaded next-hop table, for nfcs_l3_forward_device's d_table / table_n (table_n may be 0,
 * *d_table then NULL). NFCS_EINVAL before nfcs_fib_upload. */
NFCS_API int nfcs_fib_nexthops(const nfcs_fib* fib, const nfcs_nexthop** d_table, uint32_t* table_n);
/* The committed next-hop table on the host: copies min(cap, table_n) entries to `out` (may be NULL)
 * and returns table_n through *table_n. */
NFCS_API int nfcs_fib_nexthops_host(const nfcs_fib* fib, nfcs_nexthop* out, uint32_t cap, uint32_t* table_n);
/* The decision for one IPv4 destination and TTL on the CPU, from the same compiled tables the
 * kernel reads: *verdict = NFCS_RT_LOCAL .. NFCS_RT_NO_IF_MAC or NFCS_RT_FORWARD, *nh = the next-hop
 * index or NFCS_NH_NONE, *egress_if = the route's interface or NFCS_IF_NONE (each may be NULL).
 * NFCS_EINVAL before nfcs_fib_commit. */
NFCS_API int nfcs_fib_lookup_host(const nfcs_fib* fib, uint32_t dst_ip, uint32_t ttl, uint32_t* verdict,
                                  uint32_t* nh, uint32_t* egress_if);

/* Batched decision of the switch's L3 path (switch.hpp:259-301) over device-resident frames: one
 * kernel, read-only on the frames (bytes 0..47 of each at most), asynchronous on the stream.
 *   d_nh         n u32: the next-hop index for NFCS_RT_FORWARD, NFCS_NH_NONE for every other verdict
 *                (so nfcs_l3_forward_device leaves that frame untouched)
 *   d_egress_if  optional (NULL) n u32: the route's egress interface, or NFCS_IF_NONE
 *   d_verdict    optional (NULL) n bytes NFCS_RT_*
 * fib must be uploaded to ctx (else NFCS_EINVAL) and stay unchanged until the call completes.
 * Lookup then forward: where this verdict and the forward's status differ, the verdict is the
 * switch's decision. The forward tests TTL before its index, so a packet to a local address with
 * TTL 1 reads NFCS_RT_LOCAL here and NFCS_ST_TTL_EXPIRED there (the switch hands it to the CPU), and
 * every non-forwarded IPv4 frame with TTL > 1 reads NFCS_ST_NO_ROUTE there whatever the reason here. */
NFCS_API int nfcs_route_lookup_device(nfcs_ctx* ctx, const nfcs_fib* fib, const uint8_t* d_arena,
                                      uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n,
                                      uint32_t* d_nh, uint32_t* d_egress_if, uint8_t* d_verdict,
                                      void* stream);

/* ---- ACL evaluation in front of the route lookup and the forward --------------------------- */

/* AclManager::evaluate (acl_manager.cpp:161-278) for a batch of device-resident frames: the first
 * step of process_received_packet (switch.hpp:219-245, the ingress port's ACL) and the last of
 * process_egress_pipeline (the egress ACL). The symbols of this section were added without changing
 * NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup (dlsym "nfcs_acl_create"). */

/* The decision per packet: the values of the reference's AclActionType, and one of this library's. */
#define NFCS_ACL_PERMIT 0u   /* a PERMIT rule matched first, or no rule matched (the default)       */
#define NFCS_ACL_DENY 1u     /* a DENY rule matched first, or a REDIRECT rule WITHOUT a port did    */
#define NFCS_ACL_REDIRECT 2u /* a REDIRECT rule with a port matched first                            */
#define NFCS_ACL_BAD_DESC 3u /* the descriptor reaches outside the arena: the frame is not read      */

#define NFCS_ACL_NO_MATCH 0xFFFFFFFFu /* d_rule[i] when no rule matched (or NFCS_ACL_BAD_DESC)       */
#define NFCS_ACL_MAX_RULES 512u       /* 32 KiB of compiled rules in LDS                             */

/* nfcs_acl_rule.fields: which match fields the rule sets (AclRule's engaged std::optionals). A field
 * whose bit is clear is a wildcard and its value is ignored. */
#define NFCS_ACL_F_SRC_MAC 0x001u
#define NFCS_ACL_F_DST_MAC 0x002u
#define NFCS_ACL_F_VLAN_ID 0x004u
#define NFCS_ACL_F_ETHERTYPE 0x008u
#define NFCS_ACL_F_SRC_IP 0x010u
#define NFCS_ACL_F_DST_IP 0x020u
#define NFCS_ACL_F_PROTOCOL 0x040u
#define NFCS_ACL_F_SRC_PORT 0x080u
#define NFCS_ACL_F_DST_PORT 0x100u
#define NFCS_ACL_F_ALL 0x1FFu

/* One rule, AclRule (acl_manager.hpp:28-69) without its priority.
 *
 * !!! BYTE ORDER: src_ip, dst_ip and their masks are in HOST byte order (10.1.2.3 = 0x0A010203), as
 * !!! AclRule holds them (check_match compares ntohl(header field) with them). This is the OPPOSITE
 * !!! of nfcs_fib_route / nfcs_fib_arp above, whose addresses are in NETWORK byte order like the
 * !!! reference's IpAddress. vlan_id, ethertype and the ports are host-order numbers as well.
 *
 * src_ip_mask / dst_ip_mask extend the reference (its own TODO, acl_manager.hpp:48): the address
 * matches when (ntohl(packet address) & mask) == (rule address & mask). 0xFFFFFFFF is the
 * reference's exact match; a mask of 0 matches every address but still needs an IPv4 header. */
typedef struct nfcs_acl_rule {
    uint32_t fields;        /* NFCS_ACL_F_* bits; any other bit: NFCS_EINVAL                        */
    uint32_t rule_id;       /* informational only: the decision reports the rule's INDEX in the list */
    uint8_t src_mac[6];
    uint8_t dst_mac[6];
    uint16_t vlan_id;       /* compared with TCI & 0x0FFF                                            */
    uint16_t ethertype;     /* compared with the EtherType after at most one 0x8100 tag              */
    uint32_t src_ip;        /* HOST byte order                                                       */
    uint32_t dst_ip;        /* HOST byte order                                                       */
    uint32_t src_ip_mask;   /* HOST byte order; 0xFFFFFFFF = exact                                   */
    uint32_t dst_ip_mask;
    uint16_t src_port;
    uint16_t dst_port;
    uint8_t protocol;
    uint8_t action;         /* NFCS_ACL_PERMIT / DENY / REDIRECT; anything else: NFCS_EINVAL         */
    uint8_t pad[2];
    uint32_t redirect_port; /* redirect_port_id, NFCS_IF_NONE = absent (REDIRECT then decides DENY)  */
} nfcs_acl_rule;
#ifdef __cplusplus
static_assert(sizeof(nfcs_acl_rule) == 52, "nfcs_acl_rule is a 52-byte record");
#endif

/* One rule list (one named ACL of AclManager).
 *   rules   scanned IN THE ORDER GIVEN: the first rule whose check_match holds decides, exactly as
 *           AclManager::evaluate walks its vector — compiled or not. Pass get_all_rules(name) as it
 *           is; compile_rules' sort (priority descending, then rule id) is not redone here. No rule
 *           matching: NFCS_ACL_PERMIT. A REDIRECT rule without a port decides NFCS_ACL_DENY at that
 *           rule (the scan stops there). More than NFCS_ACL_MAX_RULES: NFCS_EINVAL. An empty list is
 *           valid: every frame is permitted.
 * check_match per rule over a frame of len bytes: the MACs need len >= 14; vlan_id needs an 0x8100 tag
 * and len >= 18; the EtherType is bytes 12-13, or 16-17 behind a tag with len >= 18, and is unknown
 * otherwise — a rule that sets any of ethertype / src_ip / dst_ip / protocol / the ports then fails,
 * a rule that sets none of them can still match (a rule without fields matches every frame, a 10-byte
 * one included). Any of src_ip / dst_ip / protocol / the ports needs EtherType 0x0800 and l2 + 20 <= len
 * (l2 = 18 behind a tag, else 14; the version nibble is not tested). The ports sit at l4 = l2 + IHL*4
 * (IHL 0-4 puts them inside the IPv4 header, as the reference does) and need protocol 6 with
 * l4 + 19 <= len or protocol 17 with l4 + 8 <= len. No byte past 81 is read.
 * nfcs_acl_set_rules copies its array (NULL with n > 0: NFCS_EINVAL) and invalidates an earlier commit:
 * nfcs_acl_eval_host then returns NFCS_EINVAL until the next nfcs_acl_commit. An earlier upload is NOT
 * invalidated: nfcs_acl_eval_device keeps serving the rules of the last nfcs_acl_upload, exactly as
 * with nfcs_fib. A caller that needs host and device answers equal uploads after every commit. */
typedef struct nfcs_acl nfcs_acl;
NFCS_API int nfcs_acl_create(nfcs_acl** out);
NFCS_API int nfcs_acl_destroy(nfcs_acl* acl); /* also frees what nfcs_acl_upload allocated */
NFCS_API int nfcs_acl_set_rules(nfcs_acl* acl, const nfcs_acl_rule* rules, uint32_t n);
NFCS_API int nfcs_acl_commit(nfcs_acl* acl);
/* Copies the committed rules to ctx's device (synchronous; replaces an earlier upload, which must no
 * longer be in use). NFCS_EINVAL before nfcs_acl_commit. The acl must be destroyed before ctx. */
NFCS_API int nfcs_acl_upload(nfcs_ctx* ctx, nfcs_acl* acl);
/* The decision for one frame on the CPU, from the same compiled arrays the kernel reads:
 * *action = NFCS_ACL_PERMIT / DENY / REDIRECT, *rule_index = the deciding rule's index in the list or
 * NFCS_ACL_NO_MATCH, *redirect_port = the port for NFCS_ACL_REDIRECT, else NFCS_IF_NONE (each may be
 * NULL). frame may be NULL when len is 0. NFCS_EINVAL before nfcs_acl_commit. */
NFCS_API int nfcs_acl_eval_host(const nfcs_acl* acl, const uint8_t* frame, uint32_t len, uint32_t* action,
                                uint32_t* rule_index, uint32_t* redirect_port);

/* Batched AclManager::evaluate over device-resident frames: one kernel, read-only on the frames
 * (bytes 0..95 of each at most), asynchronous on the stream.
 *   d_action    n bytes NFCS_ACL_*
 *   d_rule      optional (NULL) n u32: the index of the deciding rule, or NFCS_ACL_NO_MATCH
 *   d_redirect  optional (NULL) n u32: the port for NFCS_ACL_REDIRECT, else NFCS_IF_NONE
 *   d_nh        optional (NULL) n u32, IN/OUT: d_nh[i] = NFCS_NH_NONE for every packet whose action is
 *               not NFCS_ACL_PERMIT; every other entry is left as it is (a store, not a read-modify-
 *               write). In stream order nfcs_route_lookup_device -> this -> nfcs_l3_forward_device
 *               forwards only permitted packets with no host step (the ingress ACL); the same call
 *               after the forward, on the egress port's rules, serves the egress ACL.
 * n == 0 returns NFCS_OK without a launch. acl must be uploaded to ctx (else NFCS_EINVAL) and stay
 * unchanged until the call completes.
 * ONE rule list per call: RX bursts arrive per port, so this is the ingress ACL's form. The egress
 * side, where every packet of a burst has its own egress port and with it its own list, is
 * nfcs_egress_acl_device (the egress ACLs' section further down): it chooses the list per packet and
 * keeps this scan wave-uniform by scanning each list present in a wave once. */
NFCS_API int nfcs_acl_eval_device(nfcs_ctx* ctx, const nfcs_acl* acl, const uint8_t* d_arena,
                                  uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n,
                                  uint8_t* d_action, uint32_t* d_rule, uint32_t* d_redirect,
                                  uint32_t* d_nh, void* stream);

/* ---- L2 forwarding: FDB lookup, port / VLAN checks, learning --------------------------------- */

/* The L2 data plane of Switch::process_received_packet (switch.hpp:305-326) for a batch of
 * device-resident frames: the VLAN used for the lookup, ForwardingDatabase::lookup_port(dst_mac, vlan),
 * the same-port, link, STP and VlanManager::should_forward checks, flood on a miss, and what
 * learn_mac(src_mac, ingress_port, vlan) would do. Every frame the route lookup marks
 * NFCS_RT_NOT_IPV4 ends here. The symbols of this section were added without changing
 * NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup (dlsym "nfcs_fdb_create").
 * Flooded packets are replicated by nfcs_flood_expand_device (the next section), which takes this call's
 * d_verdict and d_vlan. OUT OF SCOPE: punting ARP, LLDP and BPDU frames (the reference's lines for LLDP and BPDU are
 * placeholders; the caller classifies with nfcs_flow_keys_device's EtherType); LACP resolution (elided
 * in the reference); aging; any write to the table from the device. */

/* The decision per packet (d_verdict). */
enum {
    NFCS_L2_FORWARD = 0,        /* the entry's port passed every check: d_egress_port[i] is that port    */
    NFCS_L2_BAD_DESC = 1,       /* the descriptor reaches outside the arena (the frame is not read), or
                                   d_rt_verdict[i] is NFCS_RT_BAD_DESC                                   */
    NFCS_L2_SKIP = 2,           /* d_rt_verdict[i] is neither NFCS_RT_NOT_IPV4 nor NFCS_RT_BAD_DESC: the
                                   L3 block took the packet (switch.hpp:266-303)                         */
    NFCS_L2_NO_ETH = 3,         /* len < 14: ethernet() is null, the switch logs "unhandled" (328)       */
    NFCS_L2_FLOOD = 4,          /* lookup_port misses (322-324); nothing further is tested               */
    NFCS_L2_DROP_SAME_PORT = 5, /* on a hit, the first true term of the || chain at 314-316, in its order */
    NFCS_L2_DROP_LINK_DOWN = 6,
    NFCS_L2_DROP_STP = 7,
    NFCS_L2_DROP_VLAN = 8       /* !should_forward(ingress, port, vlan): either port lacks a VLAN config,
                                   or the VLAN's bit is clear in the ingress or the egress bitmap        */
};
/* What learn_mac(src_mac, ingress_port, vlan) would do (d_learn), for the frames the call decides (those
 * not BAD_DESC, SKIP or NO_ETH; the others read NFCS_L2_LEARN_NONE). The table is NOT modified: the host
 * applies the few NEW and MOVED entries and uploads again, which is how switch silicon reports learning. A
 * batch of learn_mac calls from one port reaches the same table in any order, so nothing about order is
 * lost. */
enum {
    NFCS_L2_LEARN_NONE = 0,    /* the entry is static: learn_mac leaves it                                */
    NFCS_L2_LEARN_NEW = 1,     /* no entry exists                                                         */
    NFCS_L2_LEARN_REFRESH = 2, /* a dynamic entry is already on the ingress port: only its timestamp      */
    NFCS_L2_LEARN_MOVED = 3    /* a dynamic entry is on another port                                      */
};

typedef struct nfcs_fdb_entry { /* FdbEntry without its timestamp */
    uint8_t mac[6];
    uint16_t vlan_id;
    uint32_t port;
    uint8_t is_static;
    uint8_t pad[3];
} nfcs_fdb_entry;
typedef struct nfcs_l2_port { /* one port's state as the L2 block reads it */
    uint32_t port_id;
    uint8_t link_up;         /* InterfaceManager::is_port_link_up                         */
    uint8_t stp_forwarding;  /* get_port_stp_state(port) == PortState::FORWARDING         */
    uint8_t has_vlan_config; /* VlanManager::get_port_config(port).has_value()            */
    uint8_t type;            /* 0 ACCESS, 1 TRUNK, 2 HYBRID                               */
    uint16_t native_vlan;
    uint16_t pad;
} nfcs_l2_port;
#ifdef __cplusplus
static_assert(sizeof(nfcs_fdb_entry) == 16, "nfcs_fdb_entry is a 16-byte record");
static_assert(sizeof(nfcs_l2_port) == 12, "nfcs_l2_port is a 12-byte record");
#endif

#define NFCS_FDB_MAX_ENTRIES (1u << 20)
#define NFCS_L2_MAX_PORTS 1024u

/* The forwarding database and the port state the L2 block reads.
 *   entries  pass ForwardingDatabase::get_all_entries() as it is. Of two entries with the same
 *            (mac, vlan_id) the FIRST wins, as find_if returns the first (the reference itself never
 *            holds duplicates). More than NFCS_FDB_MAX_ENTRIES: NFCS_EINVAL. 00:00:00:00:00:00 on VLAN
 *            0 is a legal key: an empty slot is marked by a flag, not by a key value.
 *   ports    one nfcs_fdb_set_port per port (the same id again replaces it); allowed_vlans is the
 *            port's allowed set (NULL with n_allowed 0), ignored for ACCESS. port_id >=
 *            NFCS_L2_MAX_PORTS, a native_vlan or an allowed VLAN above 4095, or a type above 2:
 *            NFCS_EINVAL. A port never set, whatever its id (also one an FDB entry names), is the
 *            reference's default: link down, STP UNKNOWN, no VLAN config. nfcs_fdb_clear_ports forgets
 *            every port. Memory grows with the highest id set.
 * nfcs_fdb_commit compiles
 *   - the table: open addressing with linear probing over a power-of-two number of 16-byte slots
 *     (16-byte aligned: one probe is one 16-byte load), at least 2 x entries and at least 16. A slot
 *     holds the key, the port, an occupied flag and a static flag. commit records max_probe, the
 *     longest displacement of any entry plus one: every search makes at most max_probe probes, and a
 *     miss also ends at the first empty slot, so no loop depends on the table's contents alone to
 *     end. The hash is one function compiled for host and device from one definition
 *     (csrc/nfcs_fdb.h fdb_hash). Order carries no meaning (a key occurs once), so the table is
 *     bit-exact with the reference's linear scan by construction. The device never writes it.
 *   - per port one state byte and one 4096-bit VLAN bitmap: for ACCESS only the native VLAN's bit
 *     (should_forward compares with native_vlan and ignores the set), for TRUNK and HYBRID the allowed
 *     set, all zero without a VLAN config.
 * Setters, commit and upload behave exactly as in nfcs_fib: a setter (set_entries, set_port,
 * clear_ports) copies its input and invalidates an earlier commit, so nfcs_fdb_stats,
 * nfcs_fdb_lookup_host and nfcs_fdb_flood_ports_host return NFCS_EINVAL until the next
 * nfcs_fdb_commit; it does NOT invalidate an earlier upload, so nfcs_l2_lookup_device keeps serving
 * the tables of the last nfcs_fdb_upload. The fdb must be destroyed before the ctx. */
typedef struct nfcs_fdb nfcs_fdb;
NFCS_API int nfcs_fdb_create(nfcs_fdb** out);
NFCS_API int nfcs_fdb_destroy(nfcs_fdb* fdb); /* also frees what nfcs_fdb_upload allocated */
NFCS_API int nfcs_fdb_set_entries(nfcs_fdb* fdb, const nfcs_fdb_entry* entries, uint32_t n);
NFCS_API int nfcs_fdb_set_port(nfcs_fdb* fdb, const nfcs_l2_port* port, const uint16_t* allowed_vlans,
                               uint32_t n_allowed);
NFCS_API int nfcs_fdb_clear_ports(nfcs_fdb* fdb);
NFCS_API int nfcs_fdb_commit(nfcs_fdb* fdb);
/* Copies the committed tables to ctx's device (synchronous; replaces an earlier upload, which must no
 * longer be in use). NFCS_EINVAL before nfcs_fdb_commit. */
NFCS_API int nfcs_fdb_upload(nfcs_ctx* ctx, nfcs_fdb* fdb);
/* The committed table: distinct entries, slots, max_probe, and `wrapped`, the number of entries whose
 * probe sequence crossed from the last slot to slot 0 (each may be NULL). */
NFCS_API int nfcs_fdb_stats(const nfcs_fdb* fdb, uint32_t* entries, uint32_t* slots, uint32_t* max_probe,
                            uint32_t* wrapped);
/* The decision for one frame received on ingress_port, on the CPU, from the same compiled arrays the
 * kernel reads: *verdict = NFCS_L2_NO_ETH .. NFCS_L2_DROP_VLAN or NFCS_L2_FORWARD, *egress_port = the
 * port for NFCS_L2_FORWARD, else NFCS_IF_NONE, *vlan = the VLAN used for the lookup (0 for
 * NFCS_L2_NO_ETH), *learn = NFCS_L2_LEARN_* (each may be NULL). frame may be NULL when len is 0; no byte
 * past 15 is read. */
NFCS_API int nfcs_fdb_lookup_host(const nfcs_fdb* fdb, uint32_t ingress_port, const uint8_t* frame, uint32_t len,
                                  uint32_t* verdict, uint32_t* egress_port, uint32_t* vlan, uint32_t* learn);
/* flood_packet's port loop (switch.hpp:180-186) from the compiled port state: the ports i < num_ports
 * with i != ingress_port, link up, STP forwarding and should_forward(ingress_port, i, vlan), ascending.
 * *n = how many there are; the first min(cap, *n) go to ports (may be NULL when cap is 0). */
NFCS_API int nfcs_fdb_flood_ports_host(const nfcs_fdb* fdb, uint32_t ingress_port, uint32_t vlan, uint32_t num_ports,
                                       uint32_t* ports, uint32_t cap, uint32_t* n);

/* Batched L2 decision over device-resident frames: one kernel, read-only on the frames (bytes 0..15 of
 * each: the MACs, the EtherType and the TCI; `len >= 18` is a test of the length alone), asynchronous on
 * the stream.
 *   d_rt_verdict   optional (NULL) n bytes NFCS_RT_* from nfcs_route_lookup_device on the same burst:
 *                  NFCS_RT_NOT_IPV4 is decided here, NFCS_RT_BAD_DESC reads NFCS_L2_BAD_DESC, every other
 *                  value NFCS_L2_SKIP. NULL: every frame is decided here.
 *   d_egress_port  n u32: the port for NFCS_L2_FORWARD, else NFCS_IF_NONE
 *   d_verdict      optional (NULL) n bytes NFCS_L2_*
 *   d_vlan         optional (NULL) n u16: the VLAN used for the lookup (0 where none was formed): TCI &
 *                  0x0FFF when bytes 12-13 are 0x8100 and len >= 18, otherwise the ingress port's
 *                  native_vlan, or 1 when that port has no VLAN config (PortConfig()'s default). A tagged
 *                  frame of 14..17 bytes therefore uses the native VLAN (packet.hpp:609-617).
 *   d_learn        optional (NULL) n bytes NFCS_L2_LEARN_*; NULL skips the source probe entirely
 * n == 0 returns NFCS_OK without a launch. fdb must be uploaded to ctx (else NFCS_EINVAL) and stay
 * unchanged until the call completes.
 * ONE ingress port per call, for the reason given at nfcs_acl_eval_device: RX bursts arrive per port. */
NFCS_API int nfcs_l2_lookup_device(nfcs_ctx* ctx, const nfcs_fdb* fdb, uint32_t ingress_port,
                                   const uint8_t* d_arena, uint64_t arena_bytes, const nfcs_desc* d_desc,
                                   uint32_t n, const uint8_t* d_rt_verdict, uint32_t* d_egress_port,
                                   uint8_t* d_verdict, uint16_t* d_vlan, uint8_t* d_learn, void* stream);

/* ---- Flood replication: the egress item list and the frame copies ---------------------------- */

/* The FLOOD branch of the L2 block plus Switch::flood_packet (switch.hpp:322-324, 174-206) for a burst of
 * device-resident frames, and with it the compaction of the burst into the egress stage's work items. The
 * symbols of this section were added without changing NFCS_ABI_VERSION (it stays 2): detect them by symbol
 * lookup (dlsym "nfcs_flood_expand_device").
 *
 * The reference handles packets one after another. A packet with an egress port goes through
 * process_egress_pipeline as it is. A packet nfcs_l2_lookup_device marks NFCS_L2_FLOOD goes, from
 * ingress_port on VLAN v = pkt.vlan_id().value_or(native VLAN of the ingress port) (the lookup VLAN,
 * d_vlan[i] of nfcs_l2_lookup_device), to the ports p < num_ports with p != ingress_port, link up, STP
 * forwarding and should_forward(ingress_port, p, v), ascending (nfcs_fdb_flood_ports_host): per port the
 * reference allocates a buffer, copies the frame's len bytes and runs process_egress_pipeline(copy, p); the
 * original is not sent. A queue that receives unicast packets and flood copies therefore sees them
 * interleaved by source packet, and within one source packet by ascending port. process_egress only ever
 * pops a tag, so a copy never grows.
 *
 * ONE call turns the burst into the list of egress work items in that order and writes the flood copies
 * into a copy region [copy_base, arena_bytes) at the tail of the same arena. One descriptor array then
 * covers originals and copies, and the egress calls run on it unchanged.
 *
 * Which packets
 *  - The unicast port of packet i is nfcs_egress_plan_device's: d_l3_port[i] when that array is given, its
 *    entry is not NFCS_IF_NONE and, when d_fwd_status is given as well, d_fwd_status[i] & NFCS_ST_FLAG_FWD;
 *    otherwise d_l2_port[i] when that array is given; otherwise none.
 *  - NFCS_EINVAL, as in the plan: both port arrays NULL; d_fwd_status without d_l3_port; and d_l2_verdict
 *    without d_l2_vlan. d_l2_verdict == NULL is legal: nothing floods and the call is the compaction alone.
 *  - A packet is LIVE when off16*16 + round_up(len, 16) <= copy_base (copy_base <= arena_bytes, else
 *    NFCS_EINVAL). A packet that is not live yields no item; no source frame can overlap a copy.
 *  - Live with a unicast port: one item {d_desc[i], port, i}.
 *  - Live, no unicast port, d_l2_verdict[i] == NFCS_L2_FLOOD: one item {copy descriptor, port, i} per flood
 *    port of (ingress_port, d_l2_vlan[i], num_ports), ascending; none when no port is eligible. A d_l2_vlan[i]
 *    above 4095 floods to no port.
 *  - Every other packet: no item.
 * Where items and copies go
 *  - Items are numbered in packet order, within a packet in port order.
 *  - Copy slots are laid out in item order from copy_base, each round_up(len, copy_align) bytes. copy_align
 *    is a power of two >= 16 and copy_base a multiple of it; anything else is NFCS_EINVAL.
 *  - A copy holds the source's whole 16-byte chunks [0, round_up(len, 16)), so the bytes behind len are the
 *    source's; the rest of its slot is not written. Its len is the source's.
 *  - An item is a copy exactly when its off16*16 >= copy_base.
 * Overflow (the reference's allocate_buffer failure, made deterministic)
 *  - Item k is emitted iff k < cap and the copy region used up to and including item k ends at or before
 *    arena_bytes. Both are prefix conditions: the emitted items are the first `items` of the full list.
 *  - items_needed and copy_bytes_needed say what the burst called for (copy_bytes_needed saturates at
 *    2^64 - 1). n * max(1, min(num_ports, NFCS_L2_MAX_PORTS)) must fit 32 bits, else NFCS_EINVAL.
 *  - Nothing is written outside [copy_base, arena_bytes) or the first cap item entries, ever.
 * Padding
 *  - Entries [items, cap) are written inert: desc {0, 0}, port NFCS_IF_NONE, src NFCS_ITEM_NONE. A caller can
 *    run plan / VLAN / enqueue over cap entries without a host sync; one that syncs on d_totals runs them
 *    over `items`. Either way: nfcs_egress_plan_device(..., d_item_desc, m, NULL, NULL, d_item_port, ...),
 *    nfcs_vlan_device on d_item_desc (it updates the item's length, not d_desc's), then
 *    nfcs_egress_enqueue_device. d_order then indexes items, and d_item_src maps back to packets.
 * Other conditions
 *  - n == 0: NFCS_OK, no launch, nothing written. fdb must be uploaded to ctx. ONE ingress port per call, for
 *    the reason given at nfcs_l2_lookup_device. cap == 0 lets the three item arrays be NULL.
 *  - Scratch (one 24-byte record per tile of NFCS_FLOOD_TILE_PKTS packets) belongs to the context, grows on
 *    demand and is freed by nfcs_ctx_destroy; a failed allocation returns NFCS_ENOMEM and leaves the context
 *    usable, as the enqueue does.
 * Per-port egress ACLs on the copies: nfcs_egress_acl_device over the item list, between nfcs_vlan_device
 * and nfcs_egress_enqueue_device (the egress ACLs' section).
 * The ingress ACL's REDIRECT path: nfcs_ingress_dispatch_device (the ingress dispatch's section) puts a valid
 * redirect's port into d_l2_port before this call. STILL OUT OF SCOPE: interface TX counters. */
#define NFCS_FLOOD_TILE_PKTS 1024u /* packets per scan tile; SPEED ONLY, tests place sizes around it */
#define NFCS_ITEM_NONE 0xFFFFFFFFu

typedef struct nfcs_flood_totals {
    uint32_t items;        /* emitted: entries [0, items) of the item arrays are valid            */
    uint32_t items_needed; /* what the burst calls for; > items means cap or the region ran out  */
    uint32_t copies;       /* emitted items that are flood copies                                 */
    uint32_t flooded;      /* packets taken as floods (live, verdict FLOOD, no unicast port)      */
    uint64_t copy_bytes;   /* bytes of the copy region the emitted copies occupy (slots)          */
    uint64_t copy_bytes_needed;
} nfcs_flood_totals;
#ifdef __cplusplus
static_assert(sizeof(nfcs_flood_totals) == 32, "nfcs_flood_totals is a 32-byte record");
#endif

/* d_arena 16-byte aligned; d_desc, the three port / status / verdict / VLAN arrays as the calls that made
 * them wrote them; d_item_desc (8-byte aligned), d_item_port, d_item_src: cap entries each; d_totals: one
 * record, 8-byte aligned. Asynchronous on the stream. Launches (speed only): count per tile, a scan of the
 * tile sums, emit + copy per tile, padding. */
NFCS_API int nfcs_flood_expand_device(nfcs_ctx* ctx, const nfcs_fdb* fdb, uint32_t ingress_port, uint32_t num_ports,
                                      uint8_t* d_arena, uint64_t arena_bytes, uint64_t copy_base, uint32_t copy_align,
                                      const nfcs_desc* d_desc, uint32_t n, const uint32_t* d_l3_port,
                                      const uint8_t* d_fwd_status, const uint32_t* d_l2_port,
                                      const uint8_t* d_l2_verdict, const uint16_t* d_l2_vlan, uint32_t cap,
                                      nfcs_desc* d_item_desc, uint32_t* d_item_port, uint32_t* d_item_src,
                                      nfcs_flood_totals* d_totals, void* stream);
/* The same sequential walk on the CPU (host arrays, same meanings): the definition the kernels equal bit for
 * bit. It lays the copies out and does not move frame bytes (it takes no arena). fdb must be committed. */
NFCS_API int nfcs_flood_expand_host(const nfcs_fdb* fdb, uint32_t ingress_port, uint32_t num_ports,
                                    uint64_t arena_bytes, uint64_t copy_base, uint32_t copy_align,
                                    const nfcs_desc* desc, uint32_t n, const uint32_t* l3_port,
                                    const uint8_t* fwd_status, const uint32_t* l2_port, const uint8_t* l2_verdict,
                                    const uint16_t* l2_vlan, uint32_t cap, nfcs_desc* item_desc, uint32_t* item_port,
                                    uint32_t* item_src, nfcs_flood_totals* totals);

/* ---- ICMP: echo replies and TTL / unreachable errors built on the device --------------------- */

/* The three verdicts of nfcs_route_lookup_device that the switch answers instead of dropping:
 *   NFCS_RT_LOCAL, protocol ICMP  switch.hpp:271, IcmpProcessor::process_icmp_packet (icmp_processor.cpp:33-81)
 *                                 -> echo reply (send_icmp_echo_reply, 83-188)
 *   NFCS_RT_TTL_EXPIRED           switch.hpp:279, send_time_exceeded (344-348) -> ICMP 11/0
 *   NFCS_RT_NO_ROUTE              switch.hpp:301, send_destination_unreachable(.., 0) (350-353) -> ICMP 3/0
 *                                 (both through send_icmp_error_packet_base, 193-342)
 * ONE call builds every message of a burst, checksums included, into a message region [msg_base, arena_bytes)
 * at the tail of the same arena, with a compacted message list (descriptor, port, source packet) in the form
 * of nfcs_flood_expand_device's item list. The symbols of this section were added without changing
 * NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup (dlsym "nfcs_icmp_create").
 * OUT OF SCOPE: the ARP request the reference sends on an ARP miss (NFCS_ICMP_ST_SRC_ARP_MISS names the
 * packet), packet_handler_ for other local traffic (NFCS_ICMP_ST_TO_CPU), ICMPv6, interface counters.
 *
 * Tables (nfcs_icmp). IPv4 addresses are u32 in NETWORK byte order, as in nfcs_fib.
 *   local    InterfaceManager::get_mac_for_ip(ip) for the switch's own addresses. Of two entries with one
 *            address the FIRST wins (the reference scans its interfaces ascending and stops).
 *   if_ips   InterfaceManager::get_interface_ip(egress_if): the interface's ip_configurations[0]. Of two
 *            entries with one interface the first wins.
 *   ports_up the ports p < num_ports with is_port_link_up(p): send_control_plane_packet's test
 *            (switch.hpp:143). num_ports above NFCS_L2_MAX_PORTS: NFCS_EINVAL; a listed port >= num_ports is
 *            ignored (it can never send).
 * Setters, commit and upload behave exactly as in nfcs_fdb: a setter copies its input (NULL with n > 0:
 * NFCS_EINVAL) and invalidates an earlier commit, so nfcs_icmp_respond_host returns NFCS_EINVAL until the
 * next nfcs_icmp_commit; it does NOT invalidate an earlier upload, so nfcs_icmp_respond_device keeps serving
 * the tables of the last nfcs_icmp_upload. The icmp must be destroyed before the ctx.
 * Routes, ARP and interface MACs come from the nfcs_fib given to the call (uploaded to the same ctx). */
typedef struct nfcs_icmp nfcs_icmp;
typedef struct nfcs_icmp_local { uint32_t ip; uint8_t mac[6]; uint8_t pad[2]; } nfcs_icmp_local;
typedef struct nfcs_icmp_if_ip { uint32_t egress_if; uint32_t ip; } nfcs_icmp_if_ip;
#ifdef __cplusplus
static_assert(sizeof(nfcs_icmp_local) == 12, "nfcs_icmp_local is a 12-byte record");
static_assert(sizeof(nfcs_icmp_if_ip) == 8, "nfcs_icmp_if_ip is an 8-byte record");
#endif
NFCS_API int nfcs_icmp_create(nfcs_icmp** out);
NFCS_API int nfcs_icmp_destroy(nfcs_icmp* icmp); /* also frees what nfcs_icmp_upload allocated */
NFCS_API int nfcs_icmp_set_local(nfcs_icmp* icmp, const nfcs_icmp_local* local, uint32_t n);
NFCS_API int nfcs_icmp_set_if_ips(nfcs_icmp* icmp, const nfcs_icmp_if_ip* if_ips, uint32_t n);
NFCS_API int nfcs_icmp_set_ports_up(nfcs_icmp* icmp, const uint32_t* ports, uint32_t n, uint32_t num_ports);
NFCS_API int nfcs_icmp_commit(nfcs_icmp* icmp);
/* Copies the committed tables to ctx's device (synchronous; replaces an earlier upload, which must no
 * longer be in use). NFCS_EINVAL before nfcs_icmp_commit. */
NFCS_API int nfcs_icmp_upload(nfcs_ctx* ctx, nfcs_icmp* icmp);

/* Route -> next hop -> ARP -> interface MAC for one address from the committed FIB, WITHOUT the is_my_ip and
 * TTL steps of nfcs_fib_lookup_host: what send_icmp_error_packet_base does for the original's source address
 * (icmp_processor.cpp:212-251). *verdict = NFCS_RT_FORWARD, NFCS_RT_NO_ROUTE, NFCS_RT_ARP_MISS or
 * NFCS_RT_NO_IF_MAC only; *nh = the next-hop index for NFCS_RT_FORWARD, else NFCS_NH_NONE; *egress_if = the
 * first matching route's interface WHENEVER a route matches (also for ARP_MISS and NO_IF_MAC: the ICMP stage
 * tests the interface's address before ARP), NFCS_IF_NONE for NFCS_RT_NO_ROUTE (each may be NULL). Wherever
 * nfcs_fib_lookup_host decides neither LOCAL nor TTL_EXPIRED its verdict and nh are these. NFCS_EINVAL before
 * nfcs_fib_commit. The kernels of this section call the device form of the same function. */
NFCS_API int nfcs_fib_resolve_host(const nfcs_fib* fib, uint32_t ip, uint32_t* verdict, uint32_t* nh,
                                   uint32_t* egress_if);

/* What became of source packet i (d_status). */
enum {
    NFCS_ICMP_ST_NONE = 0,           /* the verdict is none of the three, the packet is not live, or it fails the
                                        lookup's IPv4 predicate (a verdict the lookup would not have given)      */
    NFCS_ICMP_ST_ECHO_REPLY = 1,     /* message emitted                                                        */
    NFCS_ICMP_ST_TIME_EXCEEDED = 2,  /* message emitted (11/0)                                                 */
    NFCS_ICMP_ST_UNREACHABLE = 3,    /* message emitted (3/0)                                                  */
    NFCS_ICMP_ST_TO_CPU = 4,         /* local, not ICMP: packet_handler_'s (switch.hpp:273-275)                */
    NFCS_ICMP_ST_IGNORED = 5,        /* local ICMP that is not an answerable echo request: icmp() null, not type
                                        8 code 0, or total_length < ihl*4 + 8                                  */
    NFCS_ICMP_ST_NO_LOCAL_MAC = 6,   /* echo request, no `local` entry for the destination (lines 55-59)       */
    NFCS_ICMP_ST_SRC_NO_ROUTE = 7,   /* error: the original's source has no route (213-219)                    */
    NFCS_ICMP_ST_SRC_NO_IF_IP = 8,   /* error: the route's interface has no address (222-227)                  */
    NFCS_ICMP_ST_SRC_ARP_MISS = 9,   /* error: no ARP entry for the next hop (236-242); the reference sends an
                                        ARP request here, which stays the caller's                             */
    NFCS_ICMP_ST_SRC_NO_IF_MAC = 10, /* error: the route's interface has no MAC (245-250)                      */
    NFCS_ICMP_ST_PORT_DOWN = 11,     /* built, then dropped by send_control_plane_packet: port >= num_ports or
                                        not up. Not emitted.                                                   */
    NFCS_ICMP_ST_OOB = 12,           /* DEVIATION: an error's original with l2 + ihl*4 > len (the reference
                                        copies past its buffer). No message.                                   */
    NFCS_ICMP_ST_TOO_LONG = 13,      /* DEVIATION: a reply with 28 + payload > 65535 (the reference truncates
                                        total_length to 16 bits). No message.                                  */
    NFCS_ICMP_ST_OVERFLOW = 14       /* a message was called for and cap or the region ran out                 */
};

/* Rules (the overflow, padding and live conventions are nfcs_flood_expand_device's).
 * Region and descriptors
 *  - A source packet is LIVE when off16*16 + round_up(len, 16) <= msg_base (msg_base <= arena_bytes, else
 *    NFCS_EINVAL). A source that is not live produces nothing; no source frame can overlap a message.
 *  - Messages are numbered in source-packet order (a packet yields at most one). Message slots are laid out in
 *    that order from msg_base, each round_up(msg_len, msg_align) bytes. msg_align is a power of two >= 16 and
 *    msg_base a multiple of it; anything else is NFCS_EINVAL.
 *  - d_msg_desc[k] describes message k, d_msg_src[k] is its source packet, d_msg_port[k] the port
 *    send_control_plane_packet is called with. A message's bytes [msg_len, round_up(msg_len, 16)) are written
 *    zero; the rest of its slot is not written.
 *  - Message k is emitted iff k < cap and the region used up to and including message k ends at or before
 *    arena_bytes. Both are prefix conditions: the emitted messages are the first `messages` of the full list.
 *    The sources of the others read NFCS_ICMP_ST_OVERFLOW. messages_needed and msg_bytes_needed say what the
 *    burst called for.
 *  - Entries [messages, cap) are written inert: desc {0, 0}, port NFCS_IF_NONE, src NFCS_ITEM_NONE.
 *  - Nothing is written outside [msg_base, arena_bytes) or the first cap entries, ever.
 *  - n == 0: NFCS_OK, no launch, nothing written. cap == 0 lets the three message arrays be NULL.
 * Echo reply (d_rt_verdict[i] == NFCS_RT_LOCAL; ONE ingress port per call, as in nfcs_l2_lookup_device)
 *  - The request qualifies when protocol is 1; icmp() is present (l2 + ihl*4 + 8 <= len, l2 = 18 behind one
 *    0x8100 tag, else 14); type is 8 and code 0; a `local` entry exists for the destination; and
 *    total_length >= ihl*4 + 8.
 *  - payload = total_length - ihl*4 - 8, or 0 when l2 + ihl*4 + 8 + payload > len (lines 117-122).
 *  - The message is 42 + payload bytes (lines 136-173): Ethernet source = the local entry's MAC, destination =
 *    the request's source MAC, EtherType 0x0800, untagged also for a tagged request; IPv4 45 00, total length,
 *    id 0, no fragment, TTL 64, protocol 1, addresses swapped; ICMP type 0 code 0, identifier and sequence
 *    number copied, payload copied. Port = ingress_port.
 * Errors (NFCS_RT_TTL_EXPIRED -> 11/0, NFCS_RT_NO_ROUTE -> 3/0), checks in the reference's order
 *  - nfcs_fib_resolve_host on the original's source address: no route; then no if_ip for the route's
 *    interface; then ARP miss; then no interface MAC.
 *  - copied = ihl*4 + min(8, len - (l2 + ihl*4)) (lines 255-265; IHL < 5 as written there).
 *  - The message is 42 + copied bytes: MACs from the resolved next hop; IPv4 id = d_ip_id[i] (0 when d_ip_id
 *    is NULL; the reference draws rand()), TTL 64, source = the interface's first address, destination = the
 *    original's source; ICMP with 4 zero bytes behind the checksum, then the original's IPv4 header and L4
 *    bytes. Port = the route's interface.
 * Both kinds
 *  - A message whose port is >= num_ports or not up is dropped by send_control_plane_packet after it was
 *    built: it is not emitted and takes no slot (NFCS_ICMP_ST_PORT_DOWN).
 *  - Both checksums are what update_checksums() writes on the built message (lines 180, 336), the odd-length
 *    low-byte rule and the 0 / 0xFFFF cases included, computed from the message's own bytes in the pass that
 *    builds it: nothing is derived from the request's checksum, which may be wrong.
 * Downstream
 *  - The messages are untagged: nfcs_egress_plan_device(.., d_msg_desc, m, NULL, NULL, d_msg_port, ..) returns
 *    NFCS_VLAN_NOP for all of them and the queue is enqueue_packet's classification. The caller goes straight
 *    to nfcs_egress_enqueue_device and the append: no VLAN edit and no egress ACL, as
 *    send_control_plane_packet does.
 *  - ORDER, the one difference: within one (port, queue) the reference interleaves messages with data packets
 *    by source packet. Two lists (the flood stage's items, then these messages) enqueue the data packets
 *    first. Within the message list the order is the reference's.
 *  - Scratch (one 24-byte record per tile of NFCS_ICMP_TILE_PKTS packets) belongs to the context, grows on
 *    demand and is freed by nfcs_ctx_destroy; a failed allocation returns NFCS_ENOMEM and leaves the context
 *    usable, as the flood stage does. */
#define NFCS_ICMP_TILE_PKTS 1024u /* packets per scan tile; SPEED ONLY, tests place sizes around it */

typedef struct nfcs_icmp_totals {
    uint32_t messages;        /* emitted: entries [0, messages) of the message arrays are valid        */
    uint32_t messages_needed; /* what the burst calls for; > messages means cap or the region ran out  */
    uint32_t echo_replies;    /* emitted messages that are echo replies                                 */
    uint32_t errors;          /* emitted messages that are 11/0 or 3/0                                  */
    uint64_t msg_bytes;       /* bytes of the message region the emitted messages occupy (slots)        */
    uint64_t msg_bytes_needed;
} nfcs_icmp_totals;
#ifdef __cplusplus
static_assert(sizeof(nfcs_icmp_totals) == 32, "nfcs_icmp_totals is a 32-byte record");
#endif

/* d_arena 16-byte aligned; d_desc and d_rt_verdict (n bytes, required) as the lookup wrote them; d_ip_id
 * optional (NULL) n u16 in host order; d_msg_desc (8-byte aligned), d_msg_port, d_msg_src: cap entries each;
 * d_status optional (NULL) n bytes NFCS_ICMP_ST_*; d_totals: one record, 8-byte aligned. icmp and fib must be
 * uploaded to ctx and stay unchanged until the call completes. Asynchronous on the stream. Launches (speed
 * only): classify + size per tile, a scan of the tile sums, emit + build per tile, padding. */
NFCS_API int nfcs_icmp_respond_device(nfcs_ctx* ctx, const nfcs_icmp* icmp, const nfcs_fib* fib, uint32_t ingress_port,
                                      uint8_t* d_arena, uint64_t arena_bytes, uint64_t msg_base, uint32_t msg_align,
                                      const nfcs_desc* d_desc, uint32_t n, const uint8_t* d_rt_verdict,
                                      const uint16_t* d_ip_id, uint32_t cap, nfcs_desc* d_msg_desc, uint32_t* d_msg_port,
                                      uint32_t* d_msg_src, uint8_t* d_status, nfcs_icmp_totals* d_totals, void* stream);
/* The same sequential walk on the CPU (host arrays, same meanings): the definition the kernels equal bit for
 * bit. It takes the arena and writes the messages into it. icmp and fib must be committed. */
NFCS_API int nfcs_icmp_respond_host(const nfcs_icmp* icmp, const nfcs_fib* fib, uint32_t ingress_port, uint8_t* arena,
                                    uint64_t arena_bytes, uint64_t msg_base, uint32_t msg_align, const nfcs_desc* desc,
                                    uint32_t n, const uint8_t* rt_verdict, const uint16_t* ip_id, uint32_t cap,
                                    nfcs_desc* msg_desc, uint32_t* msg_port, uint32_t* msg_src, uint8_t* status,
                                    nfcs_icmp_totals* totals);

/* ---- VLAN push / pop + checksum ---------------------------------------- */

/* One VLAN edit per packet as a u32: the operation in bits 30-31, the priority in bits 13-15
 * and the VLAN id in bits 0-11 (the arguments of Packet::push_vlan, masked as
 * VlanHeader::set_vlan_id / set_priority mask them, packet.hpp:185-190). */
#define NFCS_VLAN_NOP 0x00000000u
#define NFCS_VLAN_PUSH 0x40000000u /* Packet::push_vlan(vid, prio)  packet.hpp:655-692 */
#define NFCS_VLAN_POP 0x80000000u  /* Packet::pop_vlan()            packet.hpp:694-720 */
#define NFCS_VLAN_OP_MASK 0xC0000000u
#define NFCS_VLAN_PUSH_OP(vid, prio) \
    (NFCS_VLAN_PUSH | (((uint32_t)(prio) & 7u) << 13) | ((uint32_t)(vid) & 0xFFFu))

/* Batched Packet::push_vlan / pop_vlan, each followed by the update_checksums() it ends with, on
 * device-resident frames in one HBM pass (VlanManager::process_ingress / process_egress call
 * them per packet, vlan_manager.cpp:90,159,174). Per packet i with edit op_i (d_ops[i], or
 * op_all when d_ops is NULL) and buffer capacity cap_i (d_caps[i], or cap_all; the bytes the
 * frame's buffer holds from the frame start, i.e. PacketBuffer capacity minus headroom):
 *   push, frame already tagged   -> TCI id/priority rewritten in place (DEI kept), checksums
 *   push, untagged, len+4 <= cap -> bytes [14, len) move up by 4, 0x8100 + TCI inserted at 12,
 *                                   len += 4, checksums
 *   pop, tagged and len >= 18    -> bytes [18, len) move down by 4, inner EtherType at 12,
 *                                   len -= 4, checksums
 *   anything else                -> untouched: NFCS_ST_VLAN_FAIL (the reference returns false)
 *                                   or NFCS_ST_NONE (NFCS_VLAN_NOP).
 * d_desc[i].len is updated in place. Frame bytes past the new length keep the values the
 * reference's memmove leaves. A push needs the 16-byte chunks up to len + 4 inside the arena
 * (else NFCS_ST_BAD_DESC) and cap_i must not reach into another frame.
 *   d_status  optional (NULL) n status bytes: NFCS_ST_FLAG_VLAN | update_checksums() status,
 *             NFCS_ST_VLAN_FAIL, NFCS_ST_NONE or NFCS_ST_BAD_DESC */
NFCS_API int nfcs_vlan_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                              nfcs_desc* d_desc, uint32_t n, const uint32_t* d_ops,
                              uint32_t op_all, const uint32_t* d_caps, uint32_t cap_all,
                              uint8_t* d_status, void* stream);

/* ---- Egress stage: VLAN egress plan, QoS classify, enqueue ------------------------------------ */

/* Switch::process_egress_pipeline(pkt, egress_port) (switch.hpp:113-139) for a burst of device-resident
 * frames: VlanManager::process_egress (vlan_manager.cpp:128-182) decides per egress port whether the tag
 * is popped, QosManager::classify_packet_to_queue (qos_manager.cpp:78-109) names the queue from the PCP of
 * the frame as it is after that edit, and QosManager::enqueue_packet (111-153) appends the packet to that
 * port's queue or tail-drops it at max_queue_depth. nfcs_egress_plan_device makes the two decisions per
 * packet (read-only on the frames), nfcs_vlan_device applies the edit it is handed (d_ops), and
 * nfcs_egress_enqueue_device gives, per (port, queue), the packet indexes in arrival order with the tail
 * drops counted: what a TX side consumes. The symbols of this section were added without changing
 * NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup (dlsym "nfcs_egress_create").
 * Flooded packets: NFCS_L2_FLOOD packets have no port and read NFCS_EQ_SKIP when these calls run over the
 * burst itself; run over the item list of nfcs_flood_expand_device (the section above VLAN) they cover the
 * flood copies as well.
 * Per-port egress ACLs over a mixed burst are nfcs_egress_acl_device (the egress ACLs' section below), run
 * between nfcs_vlan_device and nfcs_egress_enqueue_device on the plan's d_port.
 * OUT OF SCOPE:
 *  - token buckets and rate limits: the reference's are placeholders (should_transmit's bucket is a TODO,
 *    update_token_buckets is empty). Scheduling and dequeue are the TX queues' section below, which
 *    subtracts what it dequeues from d_depth;
 *  - interface TX counters. */

/* classify_packet_to_queue can name at most 8 distinct queues from the 8 PCP values, so a port has at most
 * this many queues here, and a port's keys are NFCS_QOS_MAX_QUEUES apart. */
#define NFCS_QOS_MAX_QUEUES 8u
#define NFCS_QUEUE_NONE 0xFFu
/* Packets per tile of nfcs_egress_enqueue_device's partition (one wave takes one tile). SPEED ONLY: the
 * result never depends on it. Tests place their sizes around it. */
#define NFCS_EGRESS_TILE_PKTS 1024u

typedef struct nfcs_egress_port {
    uint32_t port_id;         /* < NFCS_L2_MAX_PORTS (1024), else NFCS_EINVAL                            */
    uint8_t has_vlan_config;  /* VlanManager::get_port_config(port).has_value()                          */
    uint8_t type;             /* 0 ACCESS, 1 TRUNK, 2 HYBRID; above 2: NFCS_EINVAL                       */
    uint8_t tag_native;       /* PortConfig::tag_native                                                  */
    uint8_t has_qos;          /* QosManager::get_port_qos_config(port).has_value()                       */
    uint16_t native_vlan;     /* above 4095: NFCS_EINVAL                                                 */
    uint8_t num_queues;       /* 0 becomes 1 (validate_and_prepare); above NFCS_QOS_MAX_QUEUES: NFCS_EINVAL */
    uint8_t pad;
    uint32_t max_queue_depth; /* 0 becomes 1 (validate_and_prepare)                                      */
} nfcs_egress_port;
#ifdef __cplusplus
static_assert(sizeof(nfcs_egress_port) == 16, "nfcs_egress_port is a 16-byte record");
#endif

/* The egress ports. One nfcs_egress_set_port per port (the same id again replaces it); a port never set,
 * whatever its id, is the reference's default: no VLAN config and no QoS config. nfcs_egress_clear_ports
 * forgets every port. nfcs_egress_commit compiles one 16-byte record per port up to the highest id set
 * (`ports`); a (port, queue) pair is the key port * NFCS_QOS_MAX_QUEUES + queue, there are
 * keys = ports * NFCS_QOS_MAX_QUEUES of them, and the keys of queues a port does not have stay empty.
 * Setters, commit and upload behave exactly as in nfcs_fdb: a setter (set_port, clear_ports) invalidates an
 * earlier commit, so the host functions return NFCS_EINVAL until the next nfcs_egress_commit; it does NOT
 * invalidate an earlier upload. The object must be destroyed before the ctx. */
typedef struct nfcs_egress nfcs_egress;
NFCS_API int nfcs_egress_create(nfcs_egress** out);
NFCS_API int nfcs_egress_destroy(nfcs_egress* eg); /* also frees what nfcs_egress_upload allocated */
NFCS_API int nfcs_egress_set_port(nfcs_egress* eg, const nfcs_egress_port* port);
NFCS_API int nfcs_egress_clear_ports(nfcs_egress* eg);
NFCS_API int nfcs_egress_commit(nfcs_egress* eg);
/* Copies the committed records to ctx's device (synchronous; replaces an earlier upload, which must no
 * longer be in use). NFCS_EINVAL before nfcs_egress_commit. */
NFCS_API int nfcs_egress_upload(nfcs_ctx* ctx, nfcs_egress* eg);
/* The committed key space: *ports and *keys (each may be NULL). */
NFCS_API int nfcs_egress_keys(const nfcs_egress* eg, uint32_t* ports, uint32_t* keys);

/* The decision for one frame leaving through `port`, on the CPU, from the same records the kernel reads:
 * *op = NFCS_VLAN_POP or NFCS_VLAN_NOP, *queue = the queue (each may be NULL). port == NFCS_IF_NONE gives
 * NFCS_VLAN_NOP and NFCS_QUEUE_NONE. frame may be NULL when len is 0; only bytes 12..19 are read. */
NFCS_API int nfcs_egress_plan_host(const nfcs_egress* eg, uint32_t port, const uint8_t* frame, uint32_t len,
                                   uint32_t* op, uint32_t* queue);

/* The decision per packet over device-resident frames: one kernel, read-only on the frames (bytes 12..19
 * of each), asynchronous on the stream.
 *   egress port  d_l3_port[i] when that array is given and its entry is not NFCS_IF_NONE and, when
 *                d_fwd_status is given as well, d_fwd_status[i] & NFCS_ST_FLAG_FWD (a packet the ACL
 *                masked, or whose TTL expired, has no egress port); otherwise d_l2_port[i] when given;
 *                otherwise NFCS_IF_NONE. Both port arrays NULL, or d_fwd_status without d_l3_port:
 *                NFCS_EINVAL. A packet without a port, or whose descriptor reaches outside the arena (the
 *                frame is not read), gets NFCS_IF_NONE, NFCS_VLAN_NOP and NFCS_QUEUE_NONE.
 *   the edit     process_egress: with tagged = len >= 18 and bytes 12-13 = 0x8100 (when vlan_id() has a
 *                value, and what lets pop_vlan succeed, packet.hpp:604-617, 694-720), POP when the port has
 *                a VLAN config, the frame is tagged, (TCI & 0x0FFF) == native_vlan, and the port is ACCESS,
 *                or TRUNK / HYBRID with tag_native clear. NOP otherwise.
 *   the queue    classify_packet_to_queue on the frame as it will be after that edit. The PCP is that of
 *                the tag then at byte 14: after a pop the inner tag of a double-tagged frame (old bytes
 *                16-17 = 0x8100 and len - 4 >= 18, PCP from old byte 18), otherwise the frame's own tag
 *                when tagged and not popped, otherwise none. With a QoS config and a PCP: num_queues == 4
 *                maps PCP 6-7 / 4-5 / 2-3 / 0-1 to queue 0 / 1 / 2 / 3, any other count gives
 *                ((7 - pcp) * num_queues) / 8 in integers (the reference's division by 8.0, truncated),
 *                clamped to num_queues - 1. With a QoS config and no PCP: num_queues - 1. Without a QoS
 *                config: 0, as the reference returns.
 * d_port (n u32), d_ops (n u32, for nfcs_vlan_device) and d_queue (n bytes) are all required.
 * n == 0 returns NFCS_OK without a launch. eg must be uploaded to ctx (else NFCS_EINVAL). */
NFCS_API int nfcs_egress_plan_device(nfcs_ctx* ctx, const nfcs_egress* eg, const uint8_t* d_arena,
                                     uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n,
                                     const uint32_t* d_l3_port, const uint8_t* d_fwd_status,
                                     const uint32_t* d_l2_port, uint32_t* d_port, uint32_t* d_ops,
                                     uint8_t* d_queue, void* stream);

/* What enqueue_packet does with a packet (d_result). */
enum {
    NFCS_EQ_ENQUEUED = 0,
    NFCS_EQ_SKIP = 1,           /* d_port[i] == NFCS_IF_NONE                                       */
    NFCS_EQ_DROP_NO_CONFIG = 2, /* the port has no QoS config (or was never set)                   */
    NFCS_EQ_DROP_FULL = 3,      /* the queue was at max_queue_depth: tail drop                     */
    NFCS_EQ_BAD_QUEUE = 4       /* d_queue[i] >= the port's num_queues: not counted                */
};

/* enqueue_packet for the burst, frame-free: the packets of one key (port * NFCS_QOS_MAX_QUEUES + queue)
 * are taken in burst order, the first max(0, max_queue_depth - depth) of them are enqueued (the reference
 * tests size() >= max_queue_depth, so a depth already above the cap leaves no room), the rest are
 * NFCS_EQ_DROP_FULL, and d_depth[k] grows by the number enqueued, so successive bursts chain on the device.
 *   d_depth        keys u32, IN/OUT: each queue's depth before / after the burst
 *   d_result       optional (NULL) n bytes NFCS_EQ_*
 *   d_order        n u32: the indexes of the ENQUEUED packets grouped by key ascending, arrival order
 *                  within a key (the queue's FIFO order; the partition is stable and deterministic, no
 *                  position is handed out by an atomic). Entries past d_key_start[keys] are left as they were.
 *   d_key_start    keys + 1 u32: key k's packets are d_order[d_key_start[k] .. d_key_start[k+1])
 *   d_key_dropped  optional (NULL) keys u32: tail drops per key in this burst
 * n == 0 returns NFCS_OK without a launch (nothing is written). Scratch (a histogram per tile of
 * NFCS_EGRESS_TILE_PKTS packets) belongs to the context, grows on demand and is freed by nfcs_ctx_destroy;
 * a failed allocation returns NFCS_ENOMEM and leaves the context usable. With no port set (keys == 0)
 * every packet with a port reads NFCS_EQ_DROP_NO_CONFIG and d_key_start[0] = 0. */
NFCS_API int nfcs_egress_enqueue_device(nfcs_ctx* ctx, const nfcs_egress* eg, const uint32_t* d_port,
                                        const uint8_t* d_queue, uint32_t n, uint32_t* d_depth,
                                        uint8_t* d_result, uint32_t* d_order, uint32_t* d_key_start,
                                        uint32_t* d_key_dropped, void* stream);
/* The same sequential walk on the CPU (host arrays, same meanings; result and key_dropped may be NULL). */
NFCS_API int nfcs_egress_enqueue_host(const nfcs_egress* eg, const uint32_t* port, const uint8_t* queue,
                                      uint32_t n, uint32_t* depth, uint8_t* result, uint32_t* order,
                                      uint32_t* key_start, uint32_t* key_dropped);

/* ---- Egress ACLs: one rule list per egress port, one evaluation over a mixed-port burst ---------- */

/* The egress ACL of Switch::process_egress_pipeline (switch.hpp:113-139), the step between
 * VlanManager::process_egress and QosManager::enqueue_packet:
 *     name = get_applied_acl_name(egress_port, EGRESS); if evaluate(name, pkt) == DENY: tx stats, drop.
 * After the lookups and the flood expansion every item of a burst has its own egress port, so the list is
 * chosen PER PACKET from d_port[i]. An nfcs_aclset holds the rule lists (by id, 0..NFCS_ACLSET_MAX_LISTS-1)
 * and the port -> list bindings; nfcs_egress_acl_device evaluates a burst against it in one kernel that
 * reads every frame once. The symbols of this section were added without changing NFCS_ABI_VERSION (it stays
 * 2): detect them by symbol lookup (dlsym "nfcs_aclset_create").
 *
 * The list of a port. A port that was never bound, a port bound to a list that was never set or was removed
 * (AclManager::evaluate answers PERMIT for a name it does not know, acl_manager.cpp:162-166), a port bound to
 * an empty list, and a port id at or above the committed `ports` all have NO LIST: NFCS_ACL_PERMIT with
 * NFCS_ACL_NO_MATCH, and the frame is not read. Two ports may share a list. Inside a list everything is as
 * in nfcs_acl above: the order given is the scan order, the first match decides, a REDIRECT rule without a
 * port decides NFCS_ACL_DENY at that rule, the address masks are kept, nfcs_acl_rule's byte order holds. The
 * reported rule index counts inside the port's list.
 * What nfcs_aclset_commit lays out. `ports` = the highest bound port id + 1 (a binding to NFCS_ACL_LIST_NONE
 * is no binding). Every non-empty list that is set, bound or not, lies once, in list-id order, in ONE array
 * of compiled rules, each padded to a multiple of 4 with rules that match nothing, and each port has one
 * 8-byte record {first rule, padded count}; a port without a list reads count 0. The padded total must be at
 * most NFCS_ACL_MAX_RULES (the kernel stages the array in LDS), else nfcs_aclset_commit returns NFCS_EINVAL.
 * Argument errors (NFCS_EINVAL): a list id at or above NFCS_ACLSET_MAX_LISTS; a port at or above
 * NFCS_L2_MAX_PORTS; more than NFCS_ACL_MAX_RULES rules in one list; a rule nfcs_acl_set_rules would refuse.
 * Setters (set_list, remove_list, bind_port, clear), commit and upload behave exactly as in nfcs_acl, nfcs_fdb
 * and nfcs_egress: a setter invalidates an earlier commit, so the host functions return NFCS_EINVAL until the
 * next nfcs_aclset_commit; it does NOT invalidate an earlier upload. The set is destroyed before the ctx. */
#define NFCS_ACLSET_MAX_LISTS 128u     /* list ids 0..127 */
#define NFCS_ACL_LIST_NONE 0xFFFFFFFFu /* nfcs_aclset_bind_port: unbind */
#define NFCS_ACL_NO_PORT 4u /* d_action: d_port[i] was NFCS_IF_NONE; descriptor and frame not looked at */
typedef struct nfcs_aclset nfcs_aclset;
NFCS_API int nfcs_aclset_create(nfcs_aclset** out);
NFCS_API int nfcs_aclset_destroy(nfcs_aclset* set); /* also frees what nfcs_aclset_upload allocated */
/* Replaces list list_id with a copy of rules[0..n); n == 0 is an existing, empty list. */
NFCS_API int nfcs_aclset_set_list(nfcs_aclset* set, uint32_t list_id, const nfcs_acl_rule* rules, uint32_t n);
/* AclManager::delete_acl: the list is gone, bindings to it stay (and read "no list"). */
NFCS_API int nfcs_aclset_remove_list(nfcs_aclset* set, uint32_t list_id);
/* apply_acl_to_interface(port, name, EGRESS); NFCS_ACL_LIST_NONE unbinds. The list need not exist. */
NFCS_API int nfcs_aclset_bind_port(nfcs_aclset* set, uint32_t port_id, uint32_t list_id);
NFCS_API int nfcs_aclset_clear(nfcs_aclset* set); /* forgets every list and every binding */
NFCS_API int nfcs_aclset_commit(nfcs_aclset* set);
/* Copies the committed arrays to ctx's device (synchronous; replaces an earlier upload, which must no
 * longer be in use). NFCS_EINVAL before nfcs_aclset_commit. */
NFCS_API int nfcs_aclset_upload(nfcs_ctx* ctx, nfcs_aclset* set);
/* The committed layout: *ports, *lists (the non-empty lists laid out) and *rules_padded (their padded
 * total); each may be NULL. */
NFCS_API int nfcs_aclset_info(const nfcs_aclset* set, uint32_t* ports, uint32_t* lists, uint32_t* rules_padded);
/* The decision for one frame leaving through `port`, on the CPU, from the arrays the kernel reads; the
 * outputs as in nfcs_acl_eval_host, *rule_index inside the port's list. frame may be NULL when len is 0. */
NFCS_API int nfcs_aclset_eval_host(const nfcs_aclset* set, uint32_t port, const uint8_t* frame, uint32_t len,
                                   uint32_t* action, uint32_t* rule_index, uint32_t* redirect_port);

/* The egress ACL over device-resident frames: one kernel, read-only on the frames (bytes 0..95 of each at
 * most), asynchronous on the stream. It runs after nfcs_vlan_device and before nfcs_egress_enqueue_device,
 * on the plan's d_port and on the descriptors as the VLAN call left them (the reference evaluates the frame
 * after the pop, with its new length); the burst may be the packets themselves or the item list of
 * nfcs_flood_expand_device, where each flood copy then meets its own port's list (switch.hpp:188-190).
 * Per packet, in this order:
 *   d_port[i] == NFCS_IF_NONE      NFCS_ACL_NO_PORT; neither descriptor nor frame is looked at, d_port[i] stays
 *   the descriptor reaches outside the arena
 *                                  NFCS_ACL_BAD_DESC; d_port[i] = NFCS_IF_NONE; nothing is counted
 *   the port has no list           NFCS_ACL_PERMIT, NFCS_ACL_NO_MATCH; no frame byte is loaded
 *   otherwise the list is scanned  NFCS_ACL_DENY: d_port[i] = NFCS_IF_NONE, so the enqueue reads NFCS_EQ_SKIP
 *                                  and the packet takes no queue depth, and with the counter arrays given
 *                                  d_denied_pkts[port] += 1, d_denied_bytes[port] += len (the reference's
 *                                  _increment_tx_stats(port, len, false, true), switch.hpp:126, raises
 *                                  tx_packets, tx_bytes and tx_drops alike);
 *                                  NFCS_ACL_REDIRECT: reported in d_action / d_redirect, d_port[i] kept (the
 *                                  reference's egress path treats REDIRECT as PERMIT);
 *                                  NFCS_ACL_PERMIT: d_port[i] kept.
 *   d_port          n u32, IN/OUT: written only where stated above (stores, never a read-modify-write of
 *                   other entries)
 *   d_action        n bytes NFCS_ACL_*, required
 *   d_rule          optional (NULL) n u32: the deciding rule's index inside the port's list, or NFCS_ACL_NO_MATCH
 *   d_redirect      optional (NULL) n u32: the port for NFCS_ACL_REDIRECT, else NFCS_IF_NONE
 *   d_denied_pkts   optional `ports` u32 (as nfcs_aclset_info reports), IN/OUT: accumulates across calls
 *   d_denied_bytes  optional `ports` u64, IN/OUT; both counter arrays or neither, else NFCS_EINVAL. The sums
 *                   are integers added atomically, so the result does not depend on the order.
 * n == 0 returns NFCS_OK without a launch. set must be uploaded to ctx (else NFCS_EINVAL) and stay unchanged
 * until the call completes. A wave whose packets all leave by one port runs nfcs_acl_eval_device's scan;
 * a wave with several lists scans each of them once.
 * The ingress ACL's REDIRECT path, whose items bypass this ACL, is nfcs_egress_acl_items_device, and the interface
 * RX counters are nfcs_ingress_dispatch_device's (the ingress dispatch's section).
 * OUT OF SCOPE: choosing the INGRESS list per packet; interface TX counters other than the deny counters above. */
NFCS_API int nfcs_egress_acl_device(nfcs_ctx* ctx, const nfcs_aclset* set, const uint8_t* d_arena,
                                    uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n, uint32_t* d_port,
                                    uint8_t* d_action, uint32_t* d_rule, uint32_t* d_redirect,
                                    uint32_t* d_denied_pkts, uint64_t* d_denied_bytes, void* stream);
/* The same on the CPU (host arrays, same meanings; rule, redirect and the counter pair may be NULL).
 * NFCS_EINVAL before nfcs_aclset_commit. */
NFCS_API int nfcs_egress_acl_host(const nfcs_aclset* set, const uint8_t* arena, uint64_t arena_bytes,
                                  const nfcs_desc* desc, uint32_t n, uint32_t* port, uint8_t* action,
                                  uint32_t* rule, uint32_t* redirect, uint32_t* denied_pkts,
                                  uint64_t* denied_bytes);

/* ---- TX queues: persistent rings and the dequeue scheduler --------------------------------------- */

/* The queues behind QosManager::enqueue_packet (qos_manager.cpp:111-153) and the scheduler of
 * QosManager::select_packet_to_dequeue / dequeue_packet (155-240): one ring of 64-bit handles per (port,
 * queue) that lives on the device across bursts, nfcs_txq_append_device (the burst's emplace_back, after
 * nfcs_egress_enqueue_device) and nfcs_txq_dequeue_device (`budget` select_packet_to_dequeue calls per
 * port, into a per-port TX list in the reference's dequeue order). The symbols of this section were added
 * without changing NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup (dlsym "nfcs_txq_create").
 * REPRODUCED QUIRKS of the reference:
 *  - should_transmit is true for every non-empty queue (its token bucket is a TODO), so rate_limits_kbps
 *    has no effect there and none here;
 *  - WEIGHTED_ROUND_ROBIN and DEFICIT_ROUND_ROBIN share one branch that never reads queue_weights: both
 *    are plain round-robin over the non-empty queues, starting behind the port's last-serviced queue;
 *  - configure_port_qos sets the last-serviced queue to 0, so the first round-robin dequeue of a fresh
 *    port comes from queue 1 when that is non-empty.
 * The object is state: calls on one nfcs_txq from two streams (or threads) at once are the caller's error.
 * OUT OF SCOPE: token buckets and rate limits; weights having any effect; interface TX counters (the
 * handle is opaque; a caller using descriptor handles can sum len from d_tx); queue contents surviving a
 * re-commit of the egress table (a re-commit wants a new nfcs_txq). Per-port egress ACLs run before the
 * enqueue (nfcs_egress_acl_device): a denied packet never reaches a ring. */
enum { NFCS_SCHED_STRICT_PRIORITY = 0, NFCS_SCHED_WRR = 1, NFCS_SCHED_DRR = 2 };
typedef struct nfcs_txq nfcs_txq;

/* Snapshots the committed `eg` (else NFCS_EINVAL): ports, keys = ports * NFCS_QOS_MAX_QUEUES, and each
 * port's has_qos, num_queues and max_queue_depth; later changes to eg do not reach the object, and nothing
 * in eg is edited. Per key k it holds a ring of cap[k] = max_queue_depth handles for every queue the port
 * has (0 for the others and for ports without QoS), head[k] in [0, cap[k]), and per port the last-serviced
 * queue, 0 at first. It stores no tail: a queue's tail is head + depth, depth being the caller's d_depth[k],
 * the array the enqueue chains. Two independent copies of the state: the _host calls advance a host copy,
 * the _device calls a device copy on ctx's device, absent when ctx is NULL (device calls then return
 * NFCS_EINVAL). Scratch (per key and per port) is sized here and belongs to the object. A failed
 * allocation returns NFCS_ENOMEM and leaks nothing. Destroy the object before the ctx. */
NFCS_API int nfcs_txq_create(nfcs_ctx* ctx, const nfcs_egress* eg, nfcs_txq** out);
NFCS_API int nfcs_txq_destroy(nfcs_txq* txq);
/* QosConfig::scheduler of one port (default NFCS_SCHED_STRICT_PRIORITY, as QosConfig's). NFCS_EINVAL for
 * port_id >= ports or sched > 2. Updates both copies, the device copy synchronously: call it while the
 * object is idle. */
NFCS_API int nfcs_txq_set_scheduler(nfcs_txq* txq, uint32_t port_id, uint32_t sched);
/* Heads and last-serviced queues to 0 on both copies (configure_port_qos); synchronous. The caller zeroes
 * its depth arrays. */
NFCS_API int nfcs_txq_reset(nfcs_txq* txq);
/* *ports, *keys and *ring_slots (the sum of cap); each may be NULL. */
NFCS_API int nfcs_txq_info(const nfcs_txq* txq, uint32_t* ports, uint32_t* keys, uint64_t* ring_slots);
/* The state of one copy: head (keys u32) and last (ports bytes), each may be NULL. The device call waits
 * for `stream` (NULL: the context's) and downloads. */
NFCS_API int nfcs_txq_state_device(nfcs_txq* txq, uint32_t* head, uint8_t* last, void* stream);
NFCS_API int nfcs_txq_state_host(const nfcs_txq* txq, uint32_t* head, uint8_t* last);

/* enqueue_packet's emplace_back for the burst. Runs after nfcs_egress_enqueue_device of the same burst,
 * with that call's d_order and d_key_start and the d_depth it left, before any other enqueue or dequeue on
 * that depth array. For key k with cnt = key_start[k+1] - key_start[k] and before = depth[k] - cnt, for j
 * in [0, cnt):   ring[k][(head[k] + before + j) mod cap[k]] = handle(order[key_start[k] + j]).
 * The handle of packet i is d_handle[i] when that array is given, otherwise its descriptor's bits,
 * off16 | (uint64_t)len << 32, as they are when the call runs (after the VLAN edit). head and depth are
 * only read. A key with cap[k] == 0, depth[k] < cnt or depth[k] > cap[k] is inconsistent input and appends
 * nothing; entries of order that are >= n are skipped; no input carries a store outside the rings.
 * n == 0 returns NFCS_OK without a launch; d_handle and d_desc both NULL: NFCS_EINVAL. One kernel, one
 * lane per enqueued position, asynchronous on the stream. */
NFCS_API int nfcs_txq_append_device(nfcs_ctx* ctx, nfcs_txq* txq, const uint32_t* d_order,
                                    const uint32_t* d_key_start, const uint32_t* d_depth, const uint64_t* d_handle,
                                    const nfcs_desc* d_desc, uint32_t n, void* stream);
NFCS_API int nfcs_txq_append_host(nfcs_txq* txq, const uint32_t* order, const uint32_t* key_start,
                                  const uint32_t* depth, const uint64_t* handle, const nfcs_desc* desc, uint32_t n);

/* select_packet_to_dequeue, up to budget[port] times per port (budget_all when budget is NULL), ports
 * ascending; a port stops at the first nullopt, everything stops once tx_cap handles have been written.
 *   d_depth     keys u32, IN/OUT: falls by what was taken; the depth used is min(depth[k], cap[k])
 *   d_tx        tx_cap handles: port p's are d_tx[d_tx_start[p] .. d_tx_start[p+1]) in dequeue order;
 *               entries past the total are left alone
 *   d_tx_queue  optional (NULL) tx_cap bytes: the queue each entry came from
 *   d_tx_start  ports + 1 u32; d_tx_start[ports] is the total
 *   d_dequeued  optional (NULL) keys u32: this call's count per key (QueueStats::packets_dequeued)
 * head[k] advances by what was taken, mod cap. Strict priority: each call takes the lowest-numbered
 * non-empty queue and leaves last-serviced alone. WRR and DRR, alike: each call tests the queues
 * (last + 1 + i) % num_queues for i = 0..num_queues-1, takes the first non-empty one and sets last to it.
 * A port without a QoS config dequeues nothing. The device call is three kernels (plan, gather, commit),
 * asynchronous on the stream, computing the closed form of that walk; no position comes
 * from an atomic, so the same call on the same state gives the same d_tx. */
NFCS_API int nfcs_txq_dequeue_device(nfcs_ctx* ctx, nfcs_txq* txq, const uint32_t* d_budget, uint32_t budget_all,
                                     uint32_t* d_depth, uint64_t* d_tx, uint32_t tx_cap, uint8_t* d_tx_queue,
                                     uint32_t* d_tx_start, uint32_t* d_dequeued, void* stream);
NFCS_API int nfcs_txq_dequeue_host(nfcs_txq* txq, const uint32_t* budget, uint32_t budget_all, uint32_t* depth,
                                   uint64_t* tx, uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start,
                                   uint32_t* dequeued);
/* The closed form the kernels compute, for one port on the CPU: with num_queues (1..8) queues of the given
 * depths, scheduler sched and last-serviced queue last, `budget` select_packet_to_dequeue calls take
 * take[q] packets of queue q (num_queues entries) and leave *new_last; seq (optional, seq_cap bytes)
 * receives the queue of each call in order, placed by rank. Pure host code; tests hold it to the walk. */
NFCS_API int nfcs_txq_closed_form_host(uint32_t sched, uint32_t num_queues, uint32_t last, const uint32_t* depth,
                                       uint32_t budget, uint32_t* take, uint32_t* new_last, uint8_t* seq,
                                       uint32_t seq_cap);

/* ---- Ingress dispatch and the one-call RX pipeline --------------------------------------------- */

/* The lines of Switch::process_received_packet (switch.hpp:213-329) that belong to no manager, for one RX
 * burst of one ingress port: the ingress link test (215), the RX counters (216, 228, 235), DENY and REDIRECT
 * overriding the L3 and L2 decisions (226-243), REDIRECT's port test (233) and its bypass of the egress ACL
 * (238-240), and the LLDP, zero-MAC and ARP early returns (252, 253, 266). nfcs_ingress_dispatch_device runs
 * between nfcs_l2_lookup_device and nfcs_l3_forward_device on the arrays those calls and the ingress ACL
 * wrote; nfcs_switch_rx_device chains every stage of process_received_packet in one call. The symbols of this
 * section were added without changing NFCS_ABI_VERSION (it stays 2): detect them by symbol lookup (dlsym
 * "nfcs_ingress_dispatch_device"). */

/* Where process_received_packet stops for a frame (d_class). */
enum nfcs_sw_class {
    NFCS_SW_UNHANDLED = 0,  /* no Ethernet header: "Unhandled packet type" (328)                          */
    NFCS_SW_RX_DOWN = 1,    /* the ingress link is down, or ingress_port is no port of the fdb (215)      */
    NFCS_SW_IN_DENY = 2,    /* the ingress ACL denies (226-229): an RX drop                               */
    NFCS_SW_RED_OK = 3,     /* REDIRECT to a port below num_ports whose link is up (239-242)              */
    NFCS_SW_RED_DOWN = 4,   /* REDIRECT to a port whose link is down (233): an RX drop                    */
    NFCS_SW_RED_RANGE = 5,  /* REDIRECT to a port >= num_ports (233): an RX drop                          */
    NFCS_SW_LLDP = 6,       /* outer EtherType 0x88CC (252)                                               */
    NFCS_SW_ZERO_MAC = 7,   /* destination MAC 00:00:00:00:00:00, the reference's BPDU placeholder (253)  */
    NFCS_SW_ARP = 8,        /* L3 EtherType 0x0806 (259-266)                                              */
    NFCS_SW_LOCAL = 9,      /* NFCS_RT_LOCAL (270-276)                                                    */
    NFCS_SW_TTL = 10,       /* NFCS_RT_TTL_EXPIRED (279)                                                  */
    NFCS_SW_NO_ROUTE = 11,  /* NFCS_RT_NO_ROUTE (301)                                                     */
    NFCS_SW_ARP_MISS = 12,  /* NFCS_RT_ARP_MISS (300)                                                     */
    NFCS_SW_NO_IF_MAC = 13, /* NFCS_RT_NO_IF_MAC (292)                                                    */
    NFCS_SW_L3_FWD = 14,    /* NFCS_RT_FORWARD: process_egress_pipeline on the route's interface (296)    */
    NFCS_SW_L2_FWD = 15,    /* NFCS_L2_FORWARD (320)                                                      */
    NFCS_SW_L2_FLOOD = 16,  /* NFCS_L2_FLOOD (323)                                                        */
    NFCS_SW_SAME_PORT = 17, /* NFCS_L2_DROP_SAME_PORT (314)                                               */
    NFCS_SW_LINK_DOWN = 18, /* NFCS_L2_DROP_LINK_DOWN (314)                                               */
    NFCS_SW_STP = 19,       /* NFCS_L2_DROP_STP (315)                                                     */
    NFCS_SW_VLAN = 20,      /* NFCS_L2_DROP_VLAN (316)                                                    */
    NFCS_SW_BAD_DESC = 21   /* the descriptor reaches outside the arena: the frame is not read            */
};

/* InterfaceManager's RX counters of one port (_increment_rx_stats). */
typedef struct nfcs_rx_stats {
    uint64_t rx_packets, rx_bytes, rx_drops;
} nfcs_rx_stats;
#ifdef __cplusplus
static_assert(sizeof(nfcs_rx_stats) == 24, "nfcs_rx_stats is a 24-byte record");
#endif

/* The dispatch over device-resident frames: one kernel, one lane per frame, read-only on the frames (bytes
 * 0..15 of a permitted frame with len >= 14, bytes 16..19 as well with len >= 18; no other frame is read),
 * asynchronous on the stream. Per frame, in the reference's order:
 *  1. The ingress link is down (the fdb's state byte of ingress_port, 215) or ingress_port is at or above
 *     the fdb's ports: NFCS_SW_RX_DOWN for every frame, everything MASKED (d_nh[i] = NFCS_NH_NONE,
 *     d_l2_port[i] = NFCS_IF_NONE, d_l2_verdict[i] = NFCS_L2_SKIP), nothing counted.
 *  2. Otherwise rx_packets += 1 and rx_bytes += len (216).
 *  3. d_action[i] == NFCS_ACL_BAD_DESC, d_rt_verdict[i] == NFCS_RT_BAD_DESC or a descriptor that reaches
 *     outside the arena: NFCS_SW_BAD_DESC, masked, not read, not a drop.
 *  4. NFCS_ACL_DENY: NFCS_SW_IN_DENY (226-229). NFCS_ACL_REDIRECT with d_redirect[i] >= num_ports:
 *     NFCS_SW_RED_RANGE; to a port whose link is down (or that the fdb does not know): NFCS_SW_RED_DOWN
 *     (233). All three are masked and count rx_drops += 1 and, once more, rx_packets += 1 and rx_bytes += len:
 *     _increment_rx_stats(port, len, false, true) at 228 and 235 adds to all three counters, so the
 *     reference counts a dropped frame twice, and so does this call.
 *  5. A valid REDIRECT: NFCS_SW_RED_OK, d_nh[i] = NFCS_NH_NONE, d_l2_port[i] = d_redirect[i],
 *     d_l2_verdict[i] = NFCS_L2_SKIP, d_bypass[i] = 1 (239-240: process_egress and the enqueue on the
 *     redirect port, no egress ACL).
 *  6. NFCS_ACL_PERMIT with len >= 14, in this order: outer EtherType 0x88CC: NFCS_SW_LLDP (252); destination
 *     MAC all zero: NFCS_SW_ZERO_MAC (253); L3 EtherType 0x0806: NFCS_SW_ARP (266), the L3 EtherType being the
 *     inner one only when the outer is 0x8100 and len >= 18 (259-264). All three are masked.
 *  7. Every other frame is live: the three in/out arrays keep their values and the class follows
 *     d_rt_verdict[i], for NFCS_RT_NOT_IPV4 d_l2_verdict[i] (NFCS_SW_UNHANDLED without an Ethernet header).
 *   d_action, d_redirect  n bytes / n u32 of nfcs_acl_eval_device; both may be NULL: the port has no ingress
 *                         list and every frame is permitted. d_redirect alone NULL: every REDIRECT reads
 *                         NFCS_SW_RED_RANGE.
 *   d_rt_verdict          n bytes of nfcs_route_lookup_device, required
 *   d_nh, d_l2_port, d_l2_verdict   IN/OUT, required; written only where stated (stores, no read-modify-write
 *                         of other entries)
 *   d_class, d_bypass     optional (NULL) n bytes each: NFCS_SW_*, and 1 for NFCS_SW_RED_OK else 0
 *   d_rx_stats            optional (NULL) records indexed by port id, IN/OUT: d_rx_stats[ingress_port]
 *                         accumulates across calls on the device, as d_depth does; no other record is
 *                         touched. The sums are integers added atomically (one 64-bit atomic per counter per
 *                         workgroup), so the result does not depend on the order.
 * n == 0 returns NFCS_OK without a launch. fdb must be uploaded to ctx (else NFCS_EINVAL). */
NFCS_API int nfcs_ingress_dispatch_device(nfcs_ctx* ctx, const nfcs_fdb* fdb, uint32_t ingress_port,
                                          uint32_t num_ports, const uint8_t* d_arena, uint64_t arena_bytes,
                                          const nfcs_desc* d_desc, uint32_t n, const uint8_t* d_action,
                                          const uint32_t* d_redirect, const uint8_t* d_rt_verdict, uint32_t* d_nh,
                                          uint32_t* d_l2_port, uint8_t* d_l2_verdict, uint8_t* d_class,
                                          uint8_t* d_bypass, nfcs_rx_stats* d_rx_stats, void* stream);
/* The same sequential walk on the CPU (host arrays, same meanings): the definition the kernel equals bit for
 * bit (csrc/nfcs_switch.h). fdb must be committed. */
NFCS_API int nfcs_ingress_dispatch_host(const nfcs_fdb* fdb, uint32_t ingress_port, uint32_t num_ports,
                                        const uint8_t* arena, uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n,
                                        const uint8_t* action, const uint32_t* redirect, const uint8_t* rt_verdict,
                                        uint32_t* nh, uint32_t* l2_port, uint8_t* l2_verdict, uint8_t* cls,
                                        uint8_t* bypass, nfcs_rx_stats* rx_stats);

/* nfcs_egress_acl_device over an item list whose redirected items bypass the ACL (switch.hpp:238-240).
 *   d_item_src, d_bypass  both or neither (else NFCS_EINVAL): item i is BYPASSED when d_port[i] is not
 *                         NFCS_IF_NONE, d_item_src[i] < n_src and d_bypass[d_item_src[i]] != 0 (d_bypass: n_src
 *                         bytes of nfcs_ingress_dispatch_device, d_item_src of nfcs_flood_expand_device). A
 *                         bypassed item keeps its port, its descriptor and frame are not looked at, it is
 *                         counted nowhere, and d_action[i] = NFCS_ACL_BYPASS with NFCS_ACL_NO_MATCH.
 * Everything else is nfcs_egress_acl_device, which is this call with both arrays NULL. */
#define NFCS_ACL_BYPASS 5u
NFCS_API int nfcs_egress_acl_items_device(nfcs_ctx* ctx, const nfcs_aclset* set, const uint8_t* d_arena,
                                          uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n, uint32_t* d_port,
                                          const uint32_t* d_item_src, const uint8_t* d_bypass, uint32_t n_src,
                                          uint8_t* d_action, uint32_t* d_rule, uint32_t* d_redirect,
                                          uint32_t* d_denied_pkts, uint64_t* d_denied_bytes, void* stream);
NFCS_API int nfcs_egress_acl_items_host(const nfcs_aclset* set, const uint8_t* arena, uint64_t arena_bytes,
                                        const nfcs_desc* desc, uint32_t n, uint32_t* port, const uint32_t* item_src,
                                        const uint8_t* bypass, uint32_t n_src, uint8_t* action, uint32_t* rule,
                                        uint32_t* redirect, uint32_t* denied_pkts, uint64_t* denied_bytes);

/* process_received_packet for one RX burst as ONE call: route lookup, ingress ACL (when tables.ingress_acl
 * is given), L2 lookup, dispatch, fused forward, flood expand, egress plan, VLAN edit, egress ACL with bypass
 * (when tables.aclset is given), enqueue and TX-queue append (when tables.txq is given), in that order on one
 * stream, each stage exactly the call of its own section. No host synchronisation, no transfer: every
 * intermediate array lives in the caller's workspace. The dequeue (the reference's TX loop) and the ICMP
 * responder (the reference's call sites are comments) stay separate calls. */
typedef struct nfcs_switch_tables {
    const nfcs_fib* fib;         /* required */
    const nfcs_acl* ingress_acl; /* NULL: the ingress port has no list                                      */
    const nfcs_fdb* fdb;         /* required */
    const nfcs_egress* egress;   /* required */
    const nfcs_aclset* aclset;   /* NULL: no egress ACLs; d_denied_pkts / d_denied_bytes are not touched    */
    nfcs_txq* txq;               /* NULL: no append                                                         */
} nfcs_switch_tables;
typedef struct nfcs_switch_rx_io {
    /* the frames */
    uint8_t* d_arena;            /* 16-byte aligned; frames in [0, copy_base), flood copies behind          */
    uint64_t arena_bytes, copy_base;
    uint32_t copy_align;         /* as in nfcs_flood_expand_device                                          */
    uint32_t n, cap;             /* frames; item entries (an overflow is reported through d_totals)         */
    uint32_t ingress_port, num_ports;
    const nfcs_desc* d_desc;     /* n */
    /* state that chains from burst to burst on the device */
    uint32_t* d_depth;           /* keys u32, IN/OUT (nfcs_egress_enqueue_device)                           */
    uint32_t* d_denied_pkts;     /* optional pair, IN/OUT (nfcs_egress_acl_device)                          */
    uint64_t* d_denied_bytes;
    nfcs_rx_stats* d_rx_stats;   /* optional, IN/OUT (nfcs_ingress_dispatch_device)                         */
    /* outputs */
    nfcs_desc* d_item_desc;      /* cap: the items' descriptors after the VLAN edit                         */
    uint32_t* d_item_port;       /* cap: the items' FINAL ports, after the egress ACL                       */
    uint32_t* d_item_src;        /* cap */
    nfcs_flood_totals* d_totals; /* one record, 8-byte aligned                                              */
    uint32_t* d_order;           /* cap */
    uint32_t* d_key_start;       /* keys + 1 */
    uint32_t* d_key_dropped;     /* optional keys u32 */
    uint8_t* d_class;            /* optional n bytes NFCS_SW_* */
    uint64_t handle_base;        /* the append's handle of item k is handle_base + k                        */
    /* every intermediate array; nfcs_switch_rx_workspace_bytes(n, cap) bytes at least, 16-byte aligned     */
    void* d_workspace;
    uint64_t workspace_bytes;
} nfcs_switch_rx_io;
/* The workspace one nfcs_switch_rx_device call over n frames and cap items needs; every sub-array of it
 * starts on a 16-byte boundary. */
NFCS_API uint64_t nfcs_switch_rx_workspace_bytes(uint32_t n, uint32_t cap);
/* NFCS_EINVAL, before anything is launched or written: a required table that is NULL or not uploaded to
 * ctx's device, an optional one that is given but not uploaded, a txq of another context, a workspace that is
 * NULL, misaligned or smaller than nfcs_switch_rx_workspace_bytes(n, cap), and every argument error of the
 * stages (alignment, copy_base, copy_align, the counter pair). n == 0 returns NFCS_OK without a launch. The
 * context's scratch grows on demand as in the stages (NFCS_ENOMEM leaves the context usable). */
NFCS_API int nfcs_switch_rx_device(nfcs_ctx* ctx, const nfcs_switch_tables* tables, const nfcs_switch_rx_io* io,
                                   void* stream);

/* ---- flow-key extract + hash -------------------------------------------- */

/* PacketClassifier::FlowKey + hash_flow (packet_classifier.hpp:15-56, packet_classifier.cpp:12-108)
 * as one 64-byte record per packet. Integers little-endian in host order (the reference stores
 * ntohs/ntohl values); an IPv4 address is the host-order u32 key.src_ip/dst_ip in bytes 0-3 of
 * its 16-byte field (the rest zero), an IPv6 address its 16 bytes. */
typedef struct nfcs_flow_key {
    uint32_t hash;        /* PacketClassifier::hash_flow(key)                          */
    uint16_t vlan_id;     /* key.vlan_id (TCI & 0xFFF of the first tag, 0 if none)      */
    uint16_t ethertype;   /* key.ethertype (inner EtherType after one tag)             */
    uint8_t src_mac[6];
    uint8_t dst_mac[6];
    uint8_t protocol;     /* IPv4 protocol / IPv6 next header                          */
    uint8_t is_ipv6;
    uint16_t src_port;
    uint16_t dst_port;
    uint8_t reserved[6];  /* zero */
    uint8_t src_ip[16];
    uint8_t dst_ip[16];
} nfcs_flow_key;

/* Batched PacketClassifier::extract_flow_key + hash_flow over device-resident frames (read
 * only: the first 128 bytes of each frame at most). d_keys (n records) and d_hash (n u32) are
 * each optional; a descriptor outside the arena yields a zero record and hash 0. */
NFCS_API int nfcs_flow_keys_device(nfcs_ctx* ctx, const uint8_t* d_arena, uint64_t arena_bytes,
                                   const nfcs_desc* d_desc, uint32_t n, nfcs_flow_key* d_keys,
                                   uint32_t* d_hash, void* stream);

/* ---- multi-GPU partition ----------------------------------------------- */

/* Split a batch into `parts` contiguous packet ranges balanced by frame bytes: part p owns packets
 * [bounds[p], bounds[p+1]) (bounds has parts + 1 entries, bounds[0] = 0, bounds[parts] = n), and
 * its frame bytes (sum of len) differ from total / parts by less than one frame. Packets are
 * independent (packet.hpp:722-890 reads only its own frame), so each part goes to its own GPU with
 * its own context and no collective. Pure host code. */
NFCS_API int nfcs_shard_bytes(const nfcs_desc* h_desc, uint32_t n, uint32_t parts, uint32_t* bounds);

/* ---- synthetic batches and digests (bench / parity support; not on the hot path) ------ */

/* Lay out n frames of a config (packet indices first_index .. first_index+n-1), frame starts
 * aligned to `align` bytes (a multiple of 16: 16 packs frames densely, 64 matches NIC
 * buffer rings); fills h_desc (may be NULL) and returns the arena bytes needed through
 * *arena_bytes. Pure host code. */
NFCS_API int nfcs_layout_config(int config, uint64_t seed, uint64_t first_index, uint32_t n,
                                uint32_t align, nfcs_desc* h_desc, uint64_t* arena_bytes);

/* Fill the frames of a laid-out config batch on the device (d_desc from nfcs_layout_config);
 * the whole arena is zeroed first, so padding between aligned frames is defined. */
NFCS_API int nfcs_gen_config_device(nfcs_ctx* ctx, int config, uint64_t seed,
                                    uint64_t first_index, uint32_t n, uint8_t* d_arena,
                                    uint64_t arena_bytes, const nfcs_desc* d_desc, void* stream);

/* A measurement helper: flips the high byte of the IPv4 (byte 24) and the L4 (byte 40) checksum field of
 * one frame (at a hashed place) in every group of `every` consecutive frames (0: none) of a batch of untagged UDP-over-IPv4 frames such as config C1's, so that
 * the next update finds exactly those frames in need of a store (tools/store_case_bench.py --stale-every).
 * Frames shorter than 42 bytes or outside the arena are left alone. Added without changing
 * NFCS_ABI_VERSION. */
NFCS_API int nfcs_stale_every_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                                     const nfcs_desc* d_desc, uint32_t n, uint32_t every, void* stream);

/* Order-independent 64-bit digest of the n frames (packet index first_index + i):
 *   digest = sum_i mix64(frame_hash(frame_i) ^ ((first_index + i) * 0xA0761D6478BD642F))
 * (DESIGN.md §6 gives frame_hash). Synchronous; result in *h_digest. */
NFCS_API int nfcs_digest_device(nfcs_ctx* ctx, const uint8_t* d_arena, uint64_t arena_bytes,
                                const nfcs_desc* d_desc, uint32_t n, uint64_t first_index,
                                uint64_t* h_digest, void* stream);

/* ---- memory helpers for callers without their own HIP runtime ------------------------- */
NFCS_API int nfcs_device_alloc(nfcs_ctx* ctx, size_t bytes, void** out);
NFCS_API int nfcs_device_free(nfcs_ctx* ctx, void* p);
NFCS_API int nfcs_host_alloc(nfcs_ctx* ctx, size_t bytes, void** out); /* pinned */
NFCS_API int nfcs_host_free(nfcs_ctx* ctx, void* p);
NFCS_API int nfcs_memcpy_h2d(nfcs_ctx* ctx, void* dst, const void* src, size_t bytes);
NFCS_API int nfcs_memcpy_d2h(nfcs_ctx* ctx, void* dst, const void* src, size_t bytes);
NFCS_API int nfcs_stream_sync(nfcs_ctx* ctx, void* stream);

/* ---- timing (bench support): HIP events on the given stream ---------------------------- */
/* Time `iters` back-to-back nfcs_update_device launches on `stream` with HIP events recorded
 * on that same stream; returns total milliseconds in *ms. */
NFCS_API int nfcs_time_update_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                                     const nfcs_desc* d_desc, uint32_t n, uint8_t* d_status,
                                     int iters, void* stream, float* ms);
/* The steady state of a NIC ring: `iters` back-to-back nfcs_update_device calls rotating over
 * `batches` separate batches (call i runs batch i % batches: d_arenas[b], arena_bytes[b],
 * d_descs[b], n packets each), so no call re-processes the frames the previous call wrote; HIP
 * events on `stream` around all of them. Total milliseconds in *ms. */
NFCS_API int nfcs_time_update_batches(nfcs_ctx* ctx, uint32_t batches, uint8_t* const* d_arenas,
                                      const uint64_t* arena_bytes, const nfcs_desc* const* d_descs,
                                      uint32_t n, int iters, void* stream, float* ms);
/* Same for nfcs_flow_keys_device. */
NFCS_API int nfcs_time_flow_keys_device(nfcs_ctx* ctx, const uint8_t* d_arena, uint64_t arena_bytes,
                                        const nfcs_desc* d_desc, uint32_t n, nfcs_flow_key* d_keys,
                                        uint32_t* d_hash, int iters, void* stream, float* ms);
/* Same for nfcs_l3_forward_device (after the first launch every TTL has been decremented
 * again, so repeated launches keep forwarding until TTLs reach 1: the bench restores them). */
NFCS_API int nfcs_time_l3_forward_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                                         const nfcs_desc* d_desc, const uint32_t* d_nh,
                                         uint32_t n, const nfcs_nexthop* d_table, uint32_t table_n,
                                         uint8_t* d_status, int iters, void* stream, float* ms);

/* The read-stream reference the bench compares its kernels with: `iters` pure
 * non-temporal reads of the first `bytes` (16-byte multiple, 16-byte aligned) of d_buf, nothing
 * written; form 0 = the checksum read pass's shape and load policies (6 KiB per wave, 6 loads in
 * flight, XCD-aware order, the first load default-policy and the rest non-temporal), 1 = 512
 * workgroups striding with 4 non-temporal loads per lane in flight, 2 = form 0 with every load
 * non-temporal, 3 / 4 / 5 = 8 / 16 / 4 non-temporal loads per lane (8 / 16 / 4 KiB per wave) with
 * no occupancy cap. Total milliseconds in *ms. */
NFCS_API int nfcs_time_stream_read(nfcs_ctx* ctx, const uint8_t* d_buf, uint64_t bytes, int form,
                                   int iters, void* stream, float* ms);
/* The read-only floor of the checksum read pass's own access pattern: `iters` launches that read the
 * n frames of d_desc in d_arena exactly as nfcs_update_device's read pass does (16-lane rows, 6
 * slots, the same load policies, order and occupancy), computing and writing nothing. Total
 * milliseconds in *ms. */
NFCS_API int nfcs_time_frames_read(nfcs_ctx* ctx, const uint8_t* d_arena, uint64_t arena_bytes,
                                   const nfcs_desc* d_desc, uint32_t n, int iters, void* stream, float* ms);
/* Same for nfcs_vlan_device with a uniform edit: launches alternate between op_all (even
 * iterations) and op_alt (odd), so a push / pop pair leaves every frame as it was. */
NFCS_API int nfcs_time_vlan_device(nfcs_ctx* ctx, uint8_t* d_arena, uint64_t arena_bytes,
                                   nfcs_desc* d_desc, uint32_t n, uint32_t op_all,
                                   uint32_t op_alt, uint32_t cap_all, uint8_t* d_status, int iters,
                                   void* stream, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* NFCS_H */

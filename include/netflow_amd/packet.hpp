// netflow_amd/packet.hpp — C++ host API for NetFlow++ callers of the checksum path.
//
// Mirrors the reference types a caller of Packet::update_checksums() holds:
//   netflow::PacketBuffer   include/netflow++/packet_buffer.hpp:10-111
//   netflow::Packet         include/netflow++/packet.hpp:344-918 (ctor/dtor 346-357,
//                           get_buffer 379, update_checksums 722-890)
// with the same member names, argument meaning and error behaviour, and adds the batched
// entry point that the reference lacks:
//   netflow_amd::update_checksums_batch(Packet* const*, size_t)
// which hands each PacketBuffer's data window to nfcs_update_host_frames (include/nfcs.h): the
// frames are gathered chunk by chunk into a pinned, NUMA-local ring, checksummed on the gfx950
// engine, and the 2+2 checksum bytes written back into each PacketBuffer in place, the chunks
// pipelined — bit-exact with the reference; and
// the batched form of Packet::push_vlan / pop_vlan (packet.hpp:655-720)
//   netflow_amd::vlan_batch(Packet* const*, const uint32_t* ops, size_t, bool* ok)
// (nfcs_vlan_device: tag insert / strip / re-tag and the checksums in one pass); the switch's
// transit-IPv4 forward (switch.hpp:247-294) for a burst
//   netflow_amd::l3_forward_batch(Packet* const*, const uint32_t* next_hop, size_t, table, ...)
// (nfcs_l3_forward_device: TTL--, MAC rewrite and the checksums in one pass); and
// PacketClassifier::extract_flow_key + hash_flow (packet_classifier.cpp:12-108) for a burst
//   netflow_amd::flow_keys_batch(Packet* const*, size_t, nfcs_flow_key*, uint32_t* hashes)
// (nfcs_flow_keys_device: 64-byte FlowKey records in host order + hash_flow values); and
// AclManager::evaluate (acl_manager.cpp:161-278) for a burst, from a rule list built by make_acl_from
//   netflow_amd::acl_eval_batch(Packet* const*, size_t, const nfcs_acl*, uint8_t* action, ...)
// (nfcs_acl_eval_device: the first matching rule in the given order; masks a next-hop vector); and
// the switch's L2 data plane (switch.hpp:305-326) for a burst, from a database built by make_fdb_from
//   netflow_amd::l2_lookup_batch(Packet* const*, size_t, const nfcs_fdb*, ingress_port, egress_port, ...)
// (nfcs_l2_lookup_device: FDB lookup, same-port / link / STP / VLAN checks, flood, learn classes).
// The egress stage (Switch::process_egress_pipeline, switch.hpp:113-139) from ports built by make_egress_from
//   netflow_amd::egress_plan_batch(Packet* const*, size_t, const nfcs_egress*, egress_port, ops, queue)
//   netflow_amd::egress_enqueue_batch(const nfcs_egress*, port, queue, n, depth, result, order, key_start, ...)
// (nfcs_egress_plan_device: the VLAN edit and the queue per packet; nfcs_egress_enqueue_device: per
// (port, queue) the packet indexes in arrival order, tail drops counted). The TX queues behind it
// (QosManager::select_packet_to_dequeue, qos_manager.cpp:197-240), from make_txq and set_schedulers_from
//   netflow_amd::txq_append_batch(nfcs_txq*, order, key_start, depth, handle, n)
//   netflow_amd::txq_dequeue_batch(nfcs_txq*, budget, budget_all, depth, tx, tx_cap, tx_queue, tx_start, ...)
// (nfcs_txq_append_device / nfcs_txq_dequeue_device: rings that persist across bursts, drained per port in
// the reference's dequeue order). The egress ACLs between the VLAN edit and the enqueue (one rule list per
// egress port, chosen per packet) run through the C ABI on device arrays (nfcs_egress_acl_device); their
// nfcs_aclset comes from make_acl_set_from (named rule vectors + (port, applied name) pairs).
//
// The batch entry points are templates over the packet type: they take this header's Packet or
// the reference's own netflow::Packet (include/netflow_amd/netflow_adapter.hpp), whose buffers
// offer the same PacketBuffer members. Bursts run on the GPU only — there is no CPU fallback, and
// constructing the engine without a gfx950 device throws std::runtime_error ("fail loudly"). The
// single-packet members (Packet::update_checksums, push_vlan, pop_vlan) run on the host CPU like
// the reference's (include/netflow_amd/cpu_update.hpp): void / bool, never throwing.
// Header-only; link with -lnfcs (netflow_amd/libnfcs.so).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "nfcs.h"
#include "netflow_amd/cpu_update.hpp"

namespace netflow_amd {

namespace detail {
// f(i0, i1) over [0, n) split across up to 8 threads for big bursts (the per-packet Packet ->
// PacketBuffer loads of a burst of a million scattered objects take ~10 ms on one core); never throws:
// a thread that cannot be started runs its range here.
template <class F>
void parallel_ranges(size_t n, F&& f) {
    const size_t nt = n >= (size_t(1) << 16) ? 8 : 1;
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; ++t) {
        try {
            th.emplace_back([&f, n, t, nt] { f(n * t / nt, n * (t + 1) / nt); });
        } catch (...) {
            f(n * t / nt, n * (t + 1) / nt);
        }
    }
    f(size_t(0), n / nt);
    for (auto& x : th) x.join();
}
}  // namespace detail

// The caller-facing contract of netflow::PacketBuffer (packet_buffer.hpp:10-111): the same
// constructor arguments, accessors, ref_count and refcount calls, bool results of the window edits,
// and exception types (std::invalid_argument from the constructor, std::out_of_range from
// reset_offsets_and_len). Held here as a window [head_, head_ + len_) into cap_ bytes of storage
// that the buffer owns, or, built External, borrows (a BufferPool's pinned arena slot).
class PacketBuffer {
public:
    std::atomic<int> ref_count{1};

    PacketBuffer(size_t capacity, size_t initial_headroom = 0, size_t initial_data_len = 0)
        : owned_(window_fits(capacity, initial_headroom, initial_data_len, "PacketBuffer")
                     ? new unsigned char[capacity] : nullptr),
          base_(owned_.get()), cap_(capacity), head_(initial_headroom), len_(initial_data_len) {}
    struct External {};
    PacketBuffer(External, unsigned char* storage, size_t capacity, size_t initial_headroom = 0,
                 size_t initial_data_len = 0)
        : base_(window_fits(capacity, initial_headroom, initial_data_len, "PacketBuffer(External)")
                    ? storage : nullptr),
          cap_(capacity), head_(initial_headroom), len_(initial_data_len) {}
    PacketBuffer(const PacketBuffer&) = delete;
    PacketBuffer& operator=(const PacketBuffer&) = delete;

    void increment_ref() { ref_count.fetch_add(1, std::memory_order_relaxed); }
    // true when this call dropped the last reference
    bool decrement_ref() { return ref_count.fetch_sub(1, std::memory_order_acq_rel) == 1; }

    unsigned char* get_data_start_ptr() const { return base_ + head_; }
    size_t get_data_length() const { return len_; }
    size_t get_capacity() const { return cap_; }
    size_t get_headroom() const { return head_; }
    size_t get_tailroom() const { return cap_ - head_ - len_; }
    unsigned char* storage() const { return base_; }  // byte 0 of the capacity

    // Window edits: false (and no change) when the new window would leave [0, capacity).
    bool set_data_len(size_t n) { return place(head_, n); }
    bool append_data(size_t n) { return n <= get_tailroom() && place(head_, len_ + n); }
    bool prepend_data(size_t n) { return n <= head_ && place(head_ - n, len_ + n); }
    bool consume_data_front(size_t n) { return n <= len_ && place(head_ + n, len_ - n); }
    bool consume_data_end(size_t n) { return n <= len_ && place(head_, len_ - n); }
    void reset_offsets_and_len(size_t new_offset, size_t new_len) {
        if (!place(new_offset, new_len))
            throw std::out_of_range("netflow_amd::PacketBuffer::reset_offsets_and_len: window past capacity");
    }

private:
    static bool window_fits(size_t cap, size_t head, size_t len, const char* who) {
        if (len > cap || head > cap - len)
            throw std::invalid_argument(std::string("netflow_amd::") + who + ": headroom + data length > capacity");
        return true;
    }
    bool place(size_t head, size_t len) {
        if (len > cap_ || head > cap_ - len) return false;
        head_ = head;
        len_ = len;
        return true;
    }

    std::unique_ptr<unsigned char[]> owned_;
    unsigned char* base_;
    size_t cap_, head_, len_;
};

class Packet;

// One engine per device: owns the nfcs context plus reusable pinned/device staging. Calls
// on one engine are serialised by an internal mutex.
class ChecksumEngine {
public:
    explicit ChecksumEngine(int device = 0) {
        nfcs_ctx* c = nullptr;
        const int rc = nfcs_ctx_create(device, &c);
        if (rc != NFCS_OK)
            throw std::runtime_error(std::string("netflow_amd: no gfx950 engine on device ") +
                                     std::to_string(device) + ": " + nfcs_strerror(rc));
        ctx_ = c;
    }
    // Non-throwing form: *rc receives nfcs_ctx_create's result; the engine is usable iff it is 0.
    ChecksumEngine(int device, std::nothrow_t, int* rc) noexcept {
        nfcs_ctx* c = nullptr;
        const int r = nfcs_ctx_create(device, &c);
        if (rc) *rc = r;
        ctx_ = r == NFCS_OK ? c : nullptr;
    }
    ~ChecksumEngine() {
        if (!ctx_) return;
        release();
        nfcs_ctx_destroy(ctx_);
    }
    ChecksumEngine(const ChecksumEngine&) = delete;
    ChecksumEngine& operator=(const ChecksumEngine&) = delete;

    // Process-wide engine on device 0 (created on first use); throws if there is none.
    static ChecksumEngine& instance() {
        ChecksumEngine* e = try_instance();
        if (!e) throw std::runtime_error("netflow_amd: no gfx950 engine on device 0");
        return *e;
    }
    // The same engine, or nullptr when none could be created (*rc: the nfcs error code). The batch
    // free functions use this and return the code instead of throwing.
    static ChecksumEngine* try_instance(int* rc = nullptr) noexcept {
        static int err = NFCS_OK;
        static ChecksumEngine e(0, std::nothrow, &err);
        if (rc) *rc = err;
        return err == NFCS_OK ? &e : nullptr;
    }

    // Batched Packet::update_checksums(): frames updated in place in their PacketBuffers.
    // status (optional) receives one NFCS_ST_* byte per packet. Returns 0 or an NFCS_E* code.
    // Pkt: netflow_amd::Packet or netflow::Packet (anything whose get_buffer() has the
    // PacketBuffer window members).
    template <class Pkt>
    int update_checksums_batch(Pkt* const* pkts, size_t n, uint8_t* status = nullptr);

    // Batched Packet::push_vlan(vid, prio) / pop_vlan() (packet.hpp:655-720), each with the
    // update_checksums() it ends with. ops[i] is an NFCS_VLAN_* edit word (NFCS_VLAN_PUSH_OP(vid,
    // prio), NFCS_VLAN_POP or NFCS_VLAN_NOP); ok[i] (optional) receives what the reference call
    // returns; each PacketBuffer's data length changes as the reference changes it. The buffer's
    // room for a push is its capacity minus headroom (tailroom = that minus the length).
    template <class Pkt>
    int vlan_batch(Pkt* const* pkts, const uint32_t* ops, size_t n, bool* ok = nullptr,
                   uint8_t* status = nullptr);

    // Batched data path of the switch's transit-IPv4 forward (switch.hpp:247-294): for packet i
    // with an IPv4 header, TTL <= 1 -> NFCS_ST_TTL_EXPIRED and next_hop[i] >= table_n ->
    // NFCS_ST_NO_ROUTE (frame untouched, as the switch drops or punts it); otherwise TTL--,
    // dst/src MAC = table[next_hop[i]] and update_checksums(), status | NFCS_ST_FLAG_FWD. The
    // route and ARP lookups stay with the caller (next_hop indexes; NFCS_NH_NONE = no route).
    template <class Pkt>
    int l3_forward_batch(Pkt* const* pkts, const uint32_t* next_hop, size_t n,
                         const nfcs_nexthop* table, uint32_t table_n, uint8_t* status = nullptr);

    // PacketClassifier::extract_flow_key(pkt) and hash_flow(key) (packet_classifier.cpp:12-108)
    // for a batch: keys[i] (optional) = the FlowKey fields in host order (nfcs_flow_key, with
    // the hash in .hash), hashes[i] (optional) = hash_flow(key).
    template <class Pkt>
    int flow_keys_batch(Pkt* const* pkts, size_t n, nfcs_flow_key* keys, uint32_t* hashes = nullptr);

    // The switch's L3 decision in front of l3_forward_batch (switch.hpp:259-301: is_my_ip, TTL,
    // RoutingManager::lookup_route, ArpProcessor::lookup_mac, the interface MAC) for a batch, from a
    // committed forwarding table (nfcs_fib_*; upload_fib first): next_hop[i] = the index into the fib's
    // next-hop table (nfcs_fib_nexthops_host) or NFCS_NH_NONE, egress_if[i] (optional) = the route's
    // interface or NFCS_IF_NONE, verdict[i] (optional) = NFCS_RT_*. Reads the first 48 bytes of each
    // packet and nothing more (every byte the decision reads lies below 38); the packets are not changed.
    template <class Pkt>
    int route_lookup_batch(Pkt* const* pkts, size_t n, const nfcs_fib* fib, uint32_t* next_hop,
                           uint32_t* egress_if = nullptr, uint8_t* verdict = nullptr);
    // nfcs_fib_upload to this engine's device, serialised with its other calls. The fib must be
    // destroyed before the engine.
    int upload_fib(nfcs_fib* fib) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_fib_upload(ctx_, fib);
    }

    // AclManager::evaluate (acl_manager.cpp:161-278) for a batch, from a committed rule list (nfcs_acl_*;
    // upload_acl first): action[i] = NFCS_ACL_PERMIT / DENY / REDIRECT, rule_index[i] (optional) = the
    // index of the deciding rule in the list or NFCS_ACL_NO_MATCH, redirect_port[i] (optional) = the port
    // of a REDIRECT or NFCS_IF_NONE. next_hop (optional, n entries, in/out): every entry whose packet is
    // not permitted becomes NFCS_NH_NONE, so l3_forward_batch then leaves that packet alone; the others
    // keep their values. Reads the first 112 bytes of each packet at most (every length the decision
    // tests is at most 97); the packets are not changed.
    template <class Pkt>
    int acl_eval_batch(Pkt* const* pkts, size_t n, const nfcs_acl* acl, uint8_t* action,
                       uint32_t* rule_index = nullptr, uint32_t* redirect_port = nullptr, uint32_t* next_hop = nullptr);
    // nfcs_acl_upload to this engine's device, serialised with its other calls. The acl must be
    // destroyed before the engine.
    int upload_acl(nfcs_acl* acl) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_acl_upload(ctx_, acl);
    }

    // The switch's L2 data plane (switch.hpp:305-326) for a batch received on ingress_port, from a
    // committed forwarding database (nfcs_fdb_*; upload_fdb first): egress_port[i] = the port for
    // NFCS_L2_FORWARD or NFCS_IF_NONE, verdict[i] (optional) = NFCS_L2_*, vlan[i] (optional) = the VLAN
    // used for the lookup, learn[i] (optional) = NFCS_L2_LEARN_*, what learn_mac(src_mac, ingress_port,
    // vlan) would do (the table is not changed). rt_verdict (optional, n bytes from route_lookup_batch
    // on the same packets): only NFCS_RT_NOT_IPV4 packets are decided, the others read NFCS_L2_SKIP.
    // Reads the first 32 bytes of each packet at most (the decision tests lengths against 14 and 18
    // only); the packets are not changed.
    template <class Pkt>
    int l2_lookup_batch(Pkt* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                        uint32_t* egress_port, uint8_t* verdict = nullptr, uint16_t* vlan = nullptr,
                        uint8_t* learn = nullptr, const uint8_t* rt_verdict = nullptr);
    // What Switch::process_received_packet does between the stages (switch.hpp:215-266; nfcs_ingress_dispatch_device)
    // for a batch received on ingress_port of a switch with num_ports ports, after route_lookup_batch,
    // acl_eval_batch and l2_lookup_batch on the same packets: rt_verdict is the route lookup's, action and
    // redirect_port the ingress ACL's (both nullptr: the port has no ingress list), next_hop, l2_port and l2_verdict
    // (in/out, all required) the three calls' outputs. A frame the switch drops, punts (LLDP, zero MAC, ARP) or
    // redirects loses its next hop, port and flood; a valid REDIRECT gets its port in l2_port and bypass[i] = 1.
    // cls[i] (optional) = NFCS_SW_*. rx (optional): the RX counters of ingress_port, added to. The staged copies
    // are cut to 32 bytes, so the counters are summed here from the classes and the packets' own lengths by the
    // rule of nfcs_ingress_dispatch_device (a dropped frame counts twice, as in the reference). Reads the first 32
    // bytes of each packet at most; the packets are not changed.
    template <class Pkt>
    int ingress_dispatch_batch(Pkt* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port, uint32_t num_ports,
                               const uint8_t* rt_verdict, uint32_t* next_hop, uint32_t* l2_port, uint8_t* l2_verdict,
                               const uint8_t* action = nullptr, const uint32_t* redirect_port = nullptr,
                               uint8_t* cls = nullptr, uint8_t* bypass = nullptr, nfcs_rx_stats* rx = nullptr);
    // nfcs_fdb_upload to this engine's device, serialised with its other calls. The fdb must be
    // destroyed before the engine.
    int upload_fdb(nfcs_fdb* fdb) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_fdb_upload(ctx_, fdb);
    }

    // Flood replication (the FLOOD branch of the L2 block plus Switch::flood_packet, switch.hpp:322-324,
    // 174-206; nfcs_flood_expand_device) for the batch l2_lookup_batch just decided, received on
    // ingress_port of a switch with num_ports ports: egress_port, l2_verdict and l2_vlan are that call's
    // outputs (l2_verdict and l2_vlan may both be nullptr: nothing floods). The burst is staged with tail
    // room for the copies (sized by nfcs_flood_expand_host first, so nothing is cut). out gets the egress
    // work items in the reference's processing order: per item the source packet's index, the port and the
    // length; an item with copy_off != FloodItems::kOriginal is a flood copy whose len bytes lie at
    // copies[copy_off], for the caller to wrap in buffers of its own; the others are the packets themselves.
    // The packets are not changed. The fdb must be committed and uploaded (upload_fdb).
    struct FloodItems {
        static constexpr uint64_t kOriginal = ~0ull;
        std::vector<uint32_t> src, port, len;  // per item
        std::vector<uint64_t> copy_off;        // per item: offset into copies, or kOriginal
        std::vector<uint8_t> copies;           // the copy region, slots of round_up(len, 16) bytes
        nfcs_flood_totals totals{};
    };
    template <class Pkt>
    int flood_expand_batch(Pkt* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port, uint32_t num_ports,
                           const uint32_t* egress_port, const uint8_t* l2_verdict, const uint16_t* l2_vlan,
                           FloodItems* out);

    // The switch's ICMP answers (switch.hpp:271 / 279 / 301 with IcmpProcessor, icmp_processor.cpp; nfcs_icmp_respond_device)
    // for the batch route_lookup_batch just decided, received on ingress_port: rt_verdict is that call's verdict
    // array, ip_id (optional) the IPv4 identification per error message (the reference draws rand()). The burst is
    // staged with tail room for the messages (bounded from the lengths, so nothing is cut). out gets the messages
    // in the reference's order: per message the source packet's index, the port send_control_plane_packet is called
    // with, the length and the offset of its bytes in `bytes`, checksums included, for the caller to wrap in
    // buffers of its own; status (optional in the C ABI, always filled here) says per packet what became of it
    // (NFCS_ICMP_ST_*). The packets are not changed. icmp and fib must be committed and uploaded (upload_icmp,
    // upload_fib).
    struct IcmpMessages {
        std::vector<uint32_t> src, port, len;  // per message
        std::vector<uint64_t> off;             // per message: offset into bytes
        std::vector<uint8_t> bytes;            // the message region, slots of round_up(len, 16) bytes
        std::vector<uint8_t> status;           // per packet
        nfcs_icmp_totals totals{};
    };
    template <class Pkt>
    int icmp_respond_batch(Pkt* const* pkts, size_t n, const nfcs_icmp* icmp, const nfcs_fib* fib, uint32_t ingress_port,
                           const uint8_t* rt_verdict, const uint16_t* ip_id, IcmpMessages* out);
    // nfcs_icmp_upload to this engine's device, serialised with its other calls. The icmp must be destroyed
    // before the engine.
    int upload_icmp(nfcs_icmp* icmp) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_icmp_upload(ctx_, icmp);
    }

    // The egress decision (VlanManager::process_egress + QosManager::classify_packet_to_queue) for a batch
    // whose packet i leaves through egress_port[i] (NFCS_IF_NONE: none), from committed egress ports
    // (nfcs_egress_*; upload_egress first): ops[i] = NFCS_VLAN_POP or NFCS_VLAN_NOP (what process_egress
    // does to the packet), queue[i] = the queue of the packet as it is after that edit, NFCS_QUEUE_NONE
    // without a port. Reads bytes 12..19 of each packet; the packets are not changed.
    template <class Pkt>
    int egress_plan_batch(Pkt* const* pkts, size_t n, const nfcs_egress* eg, const uint32_t* egress_port,
                          uint32_t* ops, uint8_t* queue);
    // QosManager::enqueue_packet for a burst (nfcs_egress_enqueue_device; host arrays, copied in and out):
    // port[i] and queue[i] as egress_plan_batch gives them, depth = one u32 per key (nfcs_egress_keys), in /
    // out; order (n u32, the first key_start[keys] are written), key_start (keys + 1 u32); result (n bytes
    // NFCS_EQ_*) and key_dropped (keys u32) optional.
    int egress_enqueue_batch(const nfcs_egress* eg, const uint32_t* port, const uint8_t* queue, size_t n,
                             uint32_t* depth, uint8_t* result, uint32_t* order, uint32_t* key_start,
                             uint32_t* key_dropped = nullptr);
    // nfcs_egress_upload to this engine's device, serialised with its other calls. The object must be
    // destroyed before the engine.
    int upload_egress(nfcs_egress* eg) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_egress_upload(ctx_, eg);
    }

    // The TX queues of committed egress ports with a device copy on this engine's device (nfcs_txq_create:
    // persistent rings per (port, queue) and the scheduler of QosManager::select_packet_to_dequeue). Set the
    // schedulers with set_schedulers_from; nfcs_txq_destroy the object before the engine.
    int make_txq(const nfcs_egress* eg, nfcs_txq** out) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_txq_create(ctx_, eg, out);
    }
    // enqueue_packet's emplace_back for a burst (nfcs_txq_append_device; host arrays, copied in): order,
    // key_start and depth as egress_enqueue_batch left them, handle[i] = the caller's 64-bit name of packet i
    // (n of them; a pointer, an index).
    int txq_append_batch(nfcs_txq* txq, const uint32_t* order, const uint32_t* key_start, const uint32_t* depth,
                         const uint64_t* handle, size_t n);
    // Up to budget[port] (budget_all when budget is null) select_packet_to_dequeue calls per port
    // (nfcs_txq_dequeue_device; host arrays, copied in and out): depth in / out, tx (tx_cap handles: port p's at
    // tx_start[p] .. tx_start[p+1] in dequeue order), tx_start (ports + 1 u32); tx_queue (tx_cap bytes) and
    // dequeued (keys u32) optional.
    int txq_dequeue_batch(nfcs_txq* txq, const uint32_t* budget, uint32_t budget_all, uint32_t* depth, uint64_t* tx,
                          uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start, uint32_t* dequeued = nullptr);

    nfcs_ctx* ctx() const { return ctx_; }

    // nfcs_update_host on this engine's context, serialised with its other calls.
    int update_host(uint8_t* h_arena, uint64_t arena_bytes, const nfcs_desc* h_desc, uint32_t n,
                    uint8_t* h_status, uint32_t flags) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_update_host(ctx_, h_arena, arena_bytes, h_desc, n, h_status, flags);
    }
    // nfcs_update_host_frames on this engine's context, serialised with its other calls.
    int update_host_frames(uint8_t* const* frames, const uint32_t* lens, uint32_t n, uint8_t* h_status) {
        std::lock_guard<std::mutex> lock(mu_);
        return nfcs_update_host_frames(ctx_, frames, lens, n, h_status, 0);
    }

private:
    // A device buffer for one call (next-hop tables, flow-key records).
    struct DevTmp {
        nfcs_ctx* c;
        void* p = nullptr;
        DevTmp(nfcs_ctx* c_, size_t bytes, int& rc) : c(c_) {
            if (!rc) rc = nfcs_device_alloc(c, bytes ? bytes : 16, &p);
        }
        ~DevTmp() { if (p) nfcs_device_free(c, p); }
    };
    // Gather each packet's first min(len, limit) bytes (limit 0: all) into 16-byte aligned
    // slots of the pinned arena; returns the arena bytes used.
    template <class Pkt>
    size_t gather(Pkt* const* pkts, size_t n, size_t limit);

    void release() {
        if (h_arena_) nfcs_host_free(ctx_, h_arena_);
        if (h_desc_) nfcs_host_free(ctx_, h_desc_);
        if (h_patch_) nfcs_host_free(ctx_, h_patch_);
        if (d_arena_) nfcs_device_free(ctx_, d_arena_);
        if (d_desc_) nfcs_device_free(ctx_, d_desc_);
        if (d_patch_) nfcs_device_free(ctx_, d_patch_);
        if (d_status_) nfcs_device_free(ctx_, d_status_);
        if (h_ops_) nfcs_host_free(ctx_, h_ops_);
        if (d_ops_) nfcs_device_free(ctx_, d_ops_);
        h_arena_ = h_desc_ = h_patch_ = d_arena_ = d_desc_ = d_patch_ = d_status_ = nullptr;
        h_ops_ = d_ops_ = nullptr;
        arena_cap_ = pkt_cap_ = 0;
    }
    int reserve(size_t arena_bytes, size_t n) {
        if (arena_bytes <= arena_cap_ && n <= pkt_cap_) return NFCS_OK;
        release();
        arena_cap_ = arena_bytes < (1u << 20) ? (1u << 20) : arena_bytes;
        pkt_cap_ = n < 4096 ? 4096 : n;
        int rc = NFCS_OK;
        if (!rc) rc = nfcs_host_alloc(ctx_, arena_cap_, &h_arena_);
        if (!rc) rc = nfcs_host_alloc(ctx_, pkt_cap_ * sizeof(nfcs_desc), &h_desc_);
        if (!rc) rc = nfcs_host_alloc(ctx_, pkt_cap_ * sizeof(nfcs_patch), &h_patch_);
        if (!rc) rc = nfcs_device_alloc(ctx_, arena_cap_, &d_arena_);
        if (!rc) rc = nfcs_device_alloc(ctx_, pkt_cap_ * sizeof(nfcs_desc), &d_desc_);
        if (!rc) rc = nfcs_device_alloc(ctx_, pkt_cap_ * sizeof(nfcs_patch), &d_patch_);
        if (!rc) rc = nfcs_device_alloc(ctx_, pkt_cap_, &d_status_);
        if (!rc) rc = nfcs_host_alloc(ctx_, pkt_cap_ * 2 * sizeof(uint32_t), &h_ops_);  // ops, caps
        if (!rc) rc = nfcs_device_alloc(ctx_, pkt_cap_ * 2 * sizeof(uint32_t), &d_ops_);
        if (rc) release();
        return rc;
    }

    nfcs_ctx* ctx_ = nullptr;
    std::mutex mu_;
    void *h_arena_ = nullptr, *h_desc_ = nullptr, *h_patch_ = nullptr;
    void *d_arena_ = nullptr, *d_desc_ = nullptr, *d_patch_ = nullptr, *d_status_ = nullptr;
    void *h_ops_ = nullptr, *d_ops_ = nullptr;
    size_t arena_cap_ = 0, pkt_cap_ = 0;
    std::vector<uint8_t*> frames_;  // update_checksums_batch's frame pointers and lengths
    std::vector<uint32_t> lens_;
};

// Same interface as netflow::Packet for what the checksum path touches.
class Packet {
public:
    explicit Packet(PacketBuffer* buf) : buffer_(buf) {
        if (!buffer_) throw std::invalid_argument("PacketBuffer cannot be null.");
        buffer_->increment_ref();
    }
    ~Packet() {
        if (buffer_) buffer_->decrement_ref();
    }
    Packet(const Packet&) = delete;
    Packet& operator=(const Packet&) = delete;
    Packet(Packet&& o) noexcept : buffer_(o.buffer_) { o.buffer_ = nullptr; }
    Packet& operator=(Packet&& o) noexcept {
        if (this != &o) {
            if (buffer_) buffer_->decrement_ref();
            buffer_ = o.buffer_;
            o.buffer_ = nullptr;
        }
        return *this;
    }

    PacketBuffer* get_buffer() const { return buffer_; }

    // packet.hpp:655 / 694 on one packet, on the host CPU (cpu_update.hpp), each ending with
    // update_checksums() like the reference; returns what the reference returns, never throws.
    // Bursts: vlan_batch (GPU).
    bool push_vlan(uint16_t vlan_id_val, uint8_t priority = 0) noexcept {
        if (!buffer_) return false;
        size_t len = buffer_->get_data_length();
        const size_t room = buffer_->get_capacity() - buffer_->get_headroom();
        if (!cpu::push_vlan(buffer_->get_data_start_ptr(), &len, room, vlan_id_val, priority)) return false;
        return buffer_->set_data_len(len);
    }
    bool pop_vlan() noexcept {
        if (!buffer_) return false;
        size_t len = buffer_->get_data_length();
        if (!cpu::pop_vlan(buffer_->get_data_start_ptr(), &len)) return false;
        return buffer_->set_data_len(len);
    }

    // packet.hpp:722 on one packet, on the host CPU (cpu_update.hpp): void, never throws, like
    // the reference. A single packet would only pay a PCIe round trip on the GPU; bursts go to
    // update_checksums_batch (GPU).
    void update_checksums() noexcept {
        if (buffer_) cpu::update_checksums(buffer_->get_data_start_ptr(), buffer_->get_data_length());
    }

private:
    PacketBuffer* buffer_;
};

template <class Pkt>
int ChecksumEngine::update_checksums_batch(Pkt* const* pkts, size_t n, uint8_t* status) {
    if (n == 0) return NFCS_OK;
    if (!pkts || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // each packet's data window as the C ABI's (pointer, length) pair: nfcs_update_host_frames
    // gathers the frames chunk by chunk into the context's pinned ring, checksums them on the GPU and
    // writes the 2+2 checksum bytes back into each PacketBuffer in place, the chunks' gather,
    // transfers, kernel and write-back overlapped (round 5; before, one gather of the whole burst,
    // then the transfers, then one scatter, one after the other)
    frames_.resize(n);
    lens_.resize(n);
    // a data window longer than NFCS_FRAME_RELEVANT_BYTES goes as its first NFCS_FRAME_RELEVANT_BYTES
    // bytes: update_checksums() gives the same result (nfcs.h), so no PacketBuffer size is refused
    detail::parallel_ranges(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
            const size_t len = b ? b->get_data_length() : 0;
            frames_[i] = b ? b->get_data_start_ptr() : nullptr;
            lens_[i] = static_cast<uint32_t>(std::min<size_t>(len, NFCS_FRAME_RELEVANT_BYTES));
        }
    });
    return nfcs_update_host_frames(ctx_, frames_.data(), lens_.data(), static_cast<uint32_t>(n), status, 0);
}

template <class Pkt>
int ChecksumEngine::vlan_batch(Pkt* const* pkts, const uint32_t* ops, size_t n, bool* ok,
                               uint8_t* status) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !ops || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // gather: each frame in a slot of round_up(len + 4, 16) bytes (room for a pushed tag)
    auto slot = [](size_t len) { return (len + 4 + 15) & ~size_t(15); };
    size_t bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        bytes += slot(b ? b->get_data_length() : 0);
    }
    if (bytes / 16 > 0xFFFFFFFFu) return NFCS_EINVAL;
    int rc = reserve(bytes + 16, n);
    if (rc) return rc;
    uint8_t* arena = static_cast<uint8_t*>(h_arena_);
    nfcs_desc* desc = static_cast<nfcs_desc*>(h_desc_);
    uint32_t* hops = static_cast<uint32_t*>(h_ops_);
    uint32_t* hcaps = hops + pkt_cap_;
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        const size_t len = b ? b->get_data_length() : 0;
        if (len) std::memcpy(arena + off, b->get_data_start_ptr(), len);
        // bytes past the frame: the buffer's own bytes where it has them (a re-tag of a runt
        // writes bytes 14-15 past len, a pop leaves its last 4 bytes), zeros otherwise
        const size_t have = b ? b->get_capacity() - b->get_headroom() : 0;
        const size_t tail = slot(len) - len, keep = have > len ? (have - len < tail ? have - len : tail) : 0;
        if (keep) std::memcpy(arena + off + len, b->get_data_start_ptr() + len, keep);
        std::memset(arena + off + len + keep, 0, tail - keep);
        desc[i] = nfcs_desc{static_cast<uint32_t>(off >> 4), static_cast<uint32_t>(len)};
        hops[i] = b ? ops[i] : NFCS_VLAN_NOP;
        hcaps[i] = static_cast<uint32_t>(have < 0xFFFFFFFFu ? have : 0xFFFFFFFFu);
        off += slot(len);
    }
    const uint32_t m = static_cast<uint32_t>(n);
    uint32_t* dops = static_cast<uint32_t*>(d_ops_);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, arena, off))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, desc, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dops, hops, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dops + pkt_cap_, hcaps, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_vlan_device(ctx_, static_cast<uint8_t*>(d_arena_), off,
                               static_cast<nfcs_desc*>(d_desc_), m, dops, 0, dops + pkt_cap_, 0,
                               static_cast<uint8_t*>(d_status_), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, arena, d_arena_, off))) return rc;
    std::vector<nfcs_desc> nd(n);
    if ((rc = nfcs_memcpy_d2h(ctx_, nd.data(), d_desc_, n * sizeof(nfcs_desc)))) return rc;
    std::vector<uint8_t> st(n);
    if ((rc = nfcs_memcpy_d2h(ctx_, st.data(), d_status_, n))) return rc;
    // scatter: the edited window back into each PacketBuffer and its new data length
    for (size_t i = 0; i < n; ++i) {
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        const bool done = (st[i] & NFCS_ST_FLAG_VLAN) != 0;
        if (ok) ok[i] = done;
        if (status) status[i] = st[i];
        if (!b || !done) continue;
        const size_t len = desc[i].len, nlen = nd[i].len;
        const size_t have = b->get_capacity() - b->get_headroom();
        size_t w = len > nlen ? len : nlen;
        if (w < 16 && have >= 16) w = 16;  // re-tag of a runt: TCI bytes 14-15
        std::memcpy(b->get_data_start_ptr(), arena + (size_t)desc[i].off16 * 16, w < have ? w : have);
        b->set_data_len(nlen);
    }
    return NFCS_OK;
}

template <class Pkt>
size_t ChecksumEngine::gather(Pkt* const* pkts, size_t n, size_t limit) {
    uint8_t* arena = static_cast<uint8_t*>(h_arena_);
    nfcs_desc* desc = static_cast<nfcs_desc*>(h_desc_);
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {  // layout first
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        size_t len = b ? b->get_data_length() : 0;
        if (limit && len > limit) len = limit;
        desc[i] = nfcs_desc{static_cast<uint32_t>(off >> 4), static_cast<uint32_t>(len)};
        off += (len + 15) & ~size_t(15);
    }
    // then the copies, by up to 8 host threads over disjoint packet ranges (one thread copies
    // ~10 GB/s, well under the PCIe rate the batch then moves at)
    auto copy = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            const size_t len = desc[i].len, o = (size_t)desc[i].off16 * 16;
            if (len) std::memcpy(arena + o, pkts[i]->get_buffer()->get_data_start_ptr(), len);
            std::memset(arena + o + len, 0, ((len + 15) & ~size_t(15)) - len);
        }
    };
    const size_t nt = off >= (size_t(32) << 20) ? 8 : 1;
    if (nt == 1) {
        copy(0, n);
    } else {
        std::vector<std::thread> th;
        th.reserve(nt);
        for (size_t t = 0; t < nt; ++t) {
            try {
                th.emplace_back(copy, n * t / nt, n * (t + 1) / nt);
            } catch (...) {  // no thread to be had: copy that range here (never throw)
                copy(n * t / nt, n * (t + 1) / nt);
            }
        }
        for (auto& t : th) t.join();
    }
    return off;
}

template <class Pkt>
int ChecksumEngine::l3_forward_batch(Pkt* const* pkts, const uint32_t* next_hop, size_t n,
                                     const nfcs_nexthop* table, uint32_t table_n, uint8_t* status) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !next_hop || (table_n && !table) || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    size_t bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        bytes += ((b ? b->get_data_length() : 0) + 15) & ~size_t(15);
    }
    if (bytes / 16 > 0xFFFFFFFFu) return NFCS_EINVAL;
    int rc = reserve(bytes + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 0);
    uint8_t* arena = static_cast<uint8_t*>(h_arena_);
    const nfcs_desc* desc = static_cast<const nfcs_desc*>(h_desc_);
    uint32_t* hnh = static_cast<uint32_t*>(h_ops_);
    for (size_t i = 0; i < n; ++i) hnh[i] = next_hop[i];
    DevTmp dtab(ctx_, table_n * sizeof(nfcs_nexthop), rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, arena, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, desc, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_ops_, hnh, n * sizeof(uint32_t)))) return rc;
    if (table_n && (rc = nfcs_memcpy_h2d(ctx_, dtab.p, table, table_n * sizeof(nfcs_nexthop)))) return rc;
    if ((rc = nfcs_l3_forward_device(ctx_, static_cast<uint8_t*>(d_arena_), off ? off : 16,
                                     static_cast<nfcs_desc*>(d_desc_), static_cast<uint32_t*>(d_ops_),
                                     m, static_cast<nfcs_nexthop*>(dtab.p), table_n,
                                     static_cast<uint8_t*>(d_status_), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, arena, d_arena_, off ? off : 16))) return rc;
    std::vector<uint8_t> st(n);
    if ((rc = nfcs_memcpy_d2h(ctx_, st.data(), d_status_, n))) return rc;
    // scatter: every byte the forward writes lies below byte 128 (MACs, TTL, the IPv4 checksum,
    // the L4 checksum at most at l2 18 + IHL 60 + 16)
    for (size_t i = 0; i < n; ++i) {
        if (status) status[i] = st[i];
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        if (!b || !(st[i] & NFCS_ST_FLAG_FWD)) continue;
        const size_t len = desc[i].len, w = len < 128 ? len : 128;
        std::memcpy(b->get_data_start_ptr(), arena + (size_t)desc[i].off16 * 16, w);
    }
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::flow_keys_batch(Pkt* const* pkts, size_t n, nfcs_flow_key* keys, uint32_t* hashes) {
    if (n == 0) return NFCS_OK;
    if (!pkts || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // every field the key reads lies below byte 98 (l2 18 + IHL 60 + the 19-byte TcpHeader's
    // bounds check), so the first 128 bytes with len clamped to 128 give the same key
    int rc = reserve(n * 128 + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 128);
    DevTmp dkeys(ctx_, n * sizeof(nfcs_flow_key), rc);
    DevTmp dhash(ctx_, n * sizeof(uint32_t), rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_flow_keys_device(ctx_, static_cast<uint8_t*>(d_arena_), off ? off : 16,
                                    static_cast<nfcs_desc*>(d_desc_), m,
                                    static_cast<nfcs_flow_key*>(dkeys.p),
                                    static_cast<uint32_t*>(dhash.p), nullptr)))
        return rc;
    if (keys && (rc = nfcs_memcpy_d2h(ctx_, keys, dkeys.p, n * sizeof(nfcs_flow_key)))) return rc;
    if (hashes && (rc = nfcs_memcpy_d2h(ctx_, hashes, dhash.p, n * sizeof(uint32_t)))) return rc;
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::route_lookup_batch(Pkt* const* pkts, size_t n, const nfcs_fib* fib, uint32_t* next_hop,
                                       uint32_t* egress_if, uint8_t* verdict) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !fib || !next_hop || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // gather clamps each length to 48: the decision tests lengths against 14, 18, 34 and 38 only
    int rc = reserve(n * 48 + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 48);
    DevTmp dnh(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dif(ctx_, n * sizeof(uint32_t), rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_route_lookup_device(ctx_, fib, static_cast<uint8_t*>(d_arena_), off ? off : 16,
                                       static_cast<nfcs_desc*>(d_desc_), m, static_cast<uint32_t*>(dnh.p),
                                       static_cast<uint32_t*>(dif.p), static_cast<uint8_t*>(d_status_), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, next_hop, dnh.p, n * sizeof(uint32_t)))) return rc;
    if (egress_if && (rc = nfcs_memcpy_d2h(ctx_, egress_if, dif.p, n * sizeof(uint32_t)))) return rc;
    if (verdict && (rc = nfcs_memcpy_d2h(ctx_, verdict, d_status_, n))) return rc;
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::acl_eval_batch(Pkt* const* pkts, size_t n, const nfcs_acl* acl, uint8_t* action,
                                   uint32_t* rule_index, uint32_t* redirect_port, uint32_t* next_hop) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !acl || !action || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // gather clamps each length to 112: the decision tests lengths against l4 + 19 <= 97 at most
    int rc = reserve(n * 112 + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 112);
    DevTmp drule(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dnh(ctx_, n * sizeof(uint32_t), rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if (next_hop && (rc = nfcs_memcpy_h2d(ctx_, dnh.p, next_hop, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_acl_eval_device(ctx_, acl, static_cast<uint8_t*>(d_arena_), off ? off : 16,
                                   static_cast<nfcs_desc*>(d_desc_), m, static_cast<uint8_t*>(d_status_),
                                   static_cast<uint32_t*>(drule.p), static_cast<uint32_t*>(dport.p),
                                   next_hop ? static_cast<uint32_t*>(dnh.p) : nullptr, nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, action, d_status_, n))) return rc;
    if (rule_index && (rc = nfcs_memcpy_d2h(ctx_, rule_index, drule.p, n * sizeof(uint32_t)))) return rc;
    if (redirect_port && (rc = nfcs_memcpy_d2h(ctx_, redirect_port, dport.p, n * sizeof(uint32_t)))) return rc;
    if (next_hop && (rc = nfcs_memcpy_d2h(ctx_, next_hop, dnh.p, n * sizeof(uint32_t)))) return rc;
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::l2_lookup_batch(Pkt* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                                    uint32_t* egress_port, uint8_t* verdict, uint16_t* vlan, uint8_t* learn,
                                    const uint8_t* rt_verdict) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !fdb || !egress_port || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // gather clamps each length to 32: the decision tests lengths against 14 and 18 only
    int rc = reserve(n * 32 + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 32);
    DevTmp dport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dvlan(ctx_, n * sizeof(uint16_t), rc);
    DevTmp dlearn(ctx_, n, rc);
    DevTmp drt(ctx_, n, rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if (rt_verdict && (rc = nfcs_memcpy_h2d(ctx_, drt.p, rt_verdict, n))) return rc;
    if ((rc = nfcs_l2_lookup_device(ctx_, fdb, ingress_port, static_cast<uint8_t*>(d_arena_), off ? off : 16,
                                    static_cast<nfcs_desc*>(d_desc_), m,
                                    rt_verdict ? static_cast<uint8_t*>(drt.p) : nullptr,
                                    static_cast<uint32_t*>(dport.p), static_cast<uint8_t*>(d_status_),
                                    static_cast<uint16_t*>(dvlan.p),
                                    learn ? static_cast<uint8_t*>(dlearn.p) : nullptr, nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, egress_port, dport.p, n * sizeof(uint32_t)))) return rc;
    if (verdict && (rc = nfcs_memcpy_d2h(ctx_, verdict, d_status_, n))) return rc;
    if (vlan && (rc = nfcs_memcpy_d2h(ctx_, vlan, dvlan.p, n * sizeof(uint16_t)))) return rc;
    if (learn && (rc = nfcs_memcpy_d2h(ctx_, learn, dlearn.p, n))) return rc;
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::ingress_dispatch_batch(Pkt* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                                           uint32_t num_ports, const uint8_t* rt_verdict, uint32_t* next_hop,
                                           uint32_t* l2_port, uint8_t* l2_verdict, const uint8_t* action,
                                           const uint32_t* redirect_port, uint8_t* cls, uint8_t* bypass,
                                           nfcs_rx_stats* rx) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !fdb || !rt_verdict || !next_hop || !l2_port || !l2_verdict || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // gather clamps each length to 32: the decision tests lengths against 14 and 18 only
    int rc = reserve(n * 32 + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 32);
    DevTmp dnh(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dred(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dl2v(ctx_, n, rc);
    DevTmp drt(ctx_, n, rc);
    DevTmp dact(ctx_, n, rc);
    DevTmp dbyp(ctx_, n, rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, drt.p, rt_verdict, n))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dnh.p, next_hop, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dport.p, l2_port, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dl2v.p, l2_verdict, n))) return rc;
    if (action && (rc = nfcs_memcpy_h2d(ctx_, dact.p, action, n))) return rc;
    if (redirect_port && (rc = nfcs_memcpy_h2d(ctx_, dred.p, redirect_port, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_ingress_dispatch_device(ctx_, fdb, ingress_port, num_ports, static_cast<uint8_t*>(d_arena_),
                                           off ? off : 16, static_cast<nfcs_desc*>(d_desc_), m,
                                           action ? static_cast<uint8_t*>(dact.p) : nullptr,
                                           redirect_port ? static_cast<uint32_t*>(dred.p) : nullptr,
                                           static_cast<uint8_t*>(drt.p), static_cast<uint32_t*>(dnh.p),
                                           static_cast<uint32_t*>(dport.p), static_cast<uint8_t*>(dl2v.p),
                                           static_cast<uint8_t*>(d_status_), static_cast<uint8_t*>(dbyp.p), nullptr,
                                           nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, next_hop, dnh.p, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, l2_port, dport.p, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, l2_verdict, dl2v.p, n))) return rc;
    if (bypass && (rc = nfcs_memcpy_d2h(ctx_, bypass, dbyp.p, n))) return rc;
    std::vector<uint8_t> own;
    if (rx && !cls) {
        own.resize(n);
        cls = own.data();
    }
    if (cls && (rc = nfcs_memcpy_d2h(ctx_, cls, d_status_, n))) return rc;
    if (rx) {
        for (size_t i = 0; i < n; ++i) {
            if (cls[i] == NFCS_SW_RX_DOWN) continue;  // switch.hpp:215 returns before 216
            auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
            const uint64_t len = b ? b->get_data_length() : 0;
            const bool drop = cls[i] == NFCS_SW_IN_DENY || cls[i] == NFCS_SW_RED_DOWN || cls[i] == NFCS_SW_RED_RANGE;
            rx->rx_packets += drop ? 2u : 1u;  // 216, and once more at 228 / 235
            rx->rx_bytes += drop ? 2u * len : len;
            rx->rx_drops += drop ? 1u : 0u;
        }
    }
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::flood_expand_batch(Pkt* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                                       uint32_t num_ports, const uint32_t* egress_port, const uint8_t* l2_verdict,
                                       const uint16_t* l2_vlan, FloodItems* out) {
    if (!out) return NFCS_EINVAL;
    *out = FloodItems{};
    if (n == 0) return NFCS_OK;
    if (!pkts || !fdb || !egress_port || n > 0xFFFFFFFFu || (l2_verdict && !l2_vlan)) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    const uint32_t m = static_cast<uint32_t>(n);
    // what the burst calls for, from the lengths alone: the host walk over the layout gather will make
    std::vector<nfcs_desc> lay(n);
    size_t frames = 0;
    for (size_t i = 0; i < n; ++i) {
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        const size_t len = b ? b->get_data_length() : 0;
        lay[i] = nfcs_desc{static_cast<uint32_t>(frames >> 4), static_cast<uint32_t>(len)};
        frames += (len + 15) & ~size_t(15);
    }
    if (frames / 16 > 0xFFFFFFFFu) return NFCS_EINVAL;
    const uint64_t copy_base = (frames + 127) & ~uint64_t(127);
    nfcs_flood_totals need{};
    int rc = nfcs_flood_expand_host(fdb, ingress_port, num_ports, ~0ull, copy_base, 16, lay.data(), m, nullptr, nullptr,
                                    egress_port, l2_verdict, l2_vlan, 0, nullptr, nullptr, nullptr, &need);
    if (rc) return rc;
    const uint64_t arena_bytes = copy_base + need.copy_bytes_needed;
    if (arena_bytes / 16 > 0xFFFFFFFFu) return NFCS_EINVAL;
    const uint32_t cap = need.items_needed;
    if ((rc = reserve(arena_bytes + 16, n))) return rc;
    gather(pkts, n, 0);
    DevTmp dport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dvlan(ctx_, n * sizeof(uint16_t), rc);
    DevTmp didesc(ctx_, (size_t)cap * sizeof(nfcs_desc), rc);
    DevTmp diport(ctx_, (size_t)cap * sizeof(uint32_t), rc);
    DevTmp disrc(ctx_, (size_t)cap * sizeof(uint32_t), rc);
    DevTmp dtot(ctx_, sizeof(nfcs_flood_totals), rc);
    if (rc) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, frames ? frames : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dport.p, egress_port, n * sizeof(uint32_t)))) return rc;
    if (l2_verdict && (rc = nfcs_memcpy_h2d(ctx_, d_status_, l2_verdict, n))) return rc;
    if (l2_verdict && (rc = nfcs_memcpy_h2d(ctx_, dvlan.p, l2_vlan, n * sizeof(uint16_t)))) return rc;
    if ((rc = nfcs_flood_expand_device(ctx_, fdb, ingress_port, num_ports, static_cast<uint8_t*>(d_arena_), arena_bytes,
                                       copy_base, 16, static_cast<nfcs_desc*>(d_desc_), m, nullptr, nullptr,
                                       static_cast<uint32_t*>(dport.p),
                                       l2_verdict ? static_cast<uint8_t*>(d_status_) : nullptr,
                                       l2_verdict ? static_cast<uint16_t*>(dvlan.p) : nullptr, cap,
                                       static_cast<nfcs_desc*>(didesc.p), static_cast<uint32_t*>(diport.p),
                                       static_cast<uint32_t*>(disrc.p), static_cast<nfcs_flood_totals*>(dtot.p), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, &out->totals, dtot.p, sizeof(nfcs_flood_totals)))) return rc;
    const uint32_t items = out->totals.items;
    if (items > cap || out->totals.copy_bytes > need.copy_bytes_needed) return NFCS_EHIP;
    std::vector<nfcs_desc> idesc(items);
    out->src.resize(items);
    out->port.resize(items);
    out->len.resize(items);
    out->copy_off.resize(items);
    out->copies.resize(out->totals.copy_bytes);
    if (items) {
        if ((rc = nfcs_memcpy_d2h(ctx_, idesc.data(), didesc.p, items * sizeof(nfcs_desc)))) return rc;
        if ((rc = nfcs_memcpy_d2h(ctx_, out->port.data(), diport.p, items * sizeof(uint32_t)))) return rc;
        if ((rc = nfcs_memcpy_d2h(ctx_, out->src.data(), disrc.p, items * sizeof(uint32_t)))) return rc;
    }
    if (!out->copies.empty() &&
        (rc = nfcs_memcpy_d2h(ctx_, out->copies.data(), static_cast<uint8_t*>(d_arena_) + copy_base, out->copies.size())))
        return rc;
    for (uint32_t k = 0; k < items; ++k) {
        const uint64_t o = (uint64_t)idesc[k].off16 * 16;
        out->len[k] = idesc[k].len;
        out->copy_off[k] = o >= copy_base && out->src[k] < n && o != (uint64_t)lay[out->src[k]].off16 * 16
                               ? o - copy_base : FloodItems::kOriginal;
    }
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::icmp_respond_batch(Pkt* const* pkts, size_t n, const nfcs_icmp* icmp, const nfcs_fib* fib,
                                       uint32_t ingress_port, const uint8_t* rt_verdict, const uint16_t* ip_id,
                                       IcmpMessages* out) {
    if (!out) return NFCS_EINVAL;
    *out = IcmpMessages{};
    if (n == 0) return NFCS_OK;
    if (!pkts || !icmp || !fib || !rt_verdict || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    const uint32_t m = static_cast<uint32_t>(n);
    // the region's bound from the lengths alone: a reply is shorter than its request, an error at most 110 bytes
    size_t frames = 0, bound = 0;
    for (size_t i = 0; i < n; ++i) {
        auto* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
        const size_t len = b ? b->get_data_length() : 0;
        frames += (len + 15) & ~size_t(15);
        bound += ((len + 15) & ~size_t(15)) + 112;
    }
    const uint64_t msg_base = (frames + 127) & ~uint64_t(127), arena_bytes = msg_base + bound;
    if (arena_bytes / 16 > 0xFFFFFFFFu) return NFCS_EINVAL;
    int rc = reserve(arena_bytes + 16, n);
    if (rc) return rc;
    gather(pkts, n, 0);
    DevTmp dv(ctx_, n, rc);
    DevTmp did(ctx_, n * sizeof(uint16_t), rc);
    DevTmp dmdesc(ctx_, n * sizeof(nfcs_desc), rc);
    DevTmp dmport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dmsrc(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dtot(ctx_, sizeof(nfcs_icmp_totals), rc);
    if (rc) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, frames ? frames : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dv.p, rt_verdict, n))) return rc;
    if (ip_id && (rc = nfcs_memcpy_h2d(ctx_, did.p, ip_id, n * sizeof(uint16_t)))) return rc;
    if ((rc = nfcs_icmp_respond_device(ctx_, icmp, fib, ingress_port, static_cast<uint8_t*>(d_arena_), arena_bytes, msg_base,
                                       16, static_cast<nfcs_desc*>(d_desc_), m, static_cast<uint8_t*>(dv.p),
                                       ip_id ? static_cast<uint16_t*>(did.p) : nullptr, m,
                                       static_cast<nfcs_desc*>(dmdesc.p), static_cast<uint32_t*>(dmport.p),
                                       static_cast<uint32_t*>(dmsrc.p), static_cast<uint8_t*>(d_status_),
                                       static_cast<nfcs_icmp_totals*>(dtot.p), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, &out->totals, dtot.p, sizeof(nfcs_icmp_totals)))) return rc;
    const uint32_t msgs = out->totals.messages;
    if (msgs > m || msgs != out->totals.messages_needed || out->totals.msg_bytes > bound) return NFCS_EHIP;
    std::vector<nfcs_desc> mdesc(msgs);
    out->src.resize(msgs);
    out->port.resize(msgs);
    out->len.resize(msgs);
    out->off.resize(msgs);
    out->status.resize(n);
    out->bytes.resize(out->totals.msg_bytes);
    if ((rc = nfcs_memcpy_d2h(ctx_, out->status.data(), d_status_, n))) return rc;
    if (msgs) {
        if ((rc = nfcs_memcpy_d2h(ctx_, mdesc.data(), dmdesc.p, msgs * sizeof(nfcs_desc)))) return rc;
        if ((rc = nfcs_memcpy_d2h(ctx_, out->port.data(), dmport.p, msgs * sizeof(uint32_t)))) return rc;
        if ((rc = nfcs_memcpy_d2h(ctx_, out->src.data(), dmsrc.p, msgs * sizeof(uint32_t)))) return rc;
        if ((rc = nfcs_memcpy_d2h(ctx_, out->bytes.data(), static_cast<uint8_t*>(d_arena_) + msg_base, out->bytes.size())))
            return rc;
    }
    for (uint32_t k = 0; k < msgs; ++k) {
        out->len[k] = mdesc[k].len;
        out->off[k] = (uint64_t)mdesc[k].off16 * 16 - msg_base;
        if (out->off[k] + ((mdesc[k].len + 15u) & ~15u) > out->bytes.size()) return NFCS_EHIP;
    }
    return NFCS_OK;
}

template <class Pkt>
int ChecksumEngine::egress_plan_batch(Pkt* const* pkts, size_t n, const nfcs_egress* eg, const uint32_t* egress_port,
                                      uint32_t* ops, uint8_t* queue) {
    if (n == 0) return NFCS_OK;
    if (!pkts || !eg || !egress_port || !ops || !queue || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    // gather clamps each length to 32: the decision tests lengths against 14, 18 and 22 only
    int rc = reserve(n * 32 + 16, n);
    if (rc) return rc;
    const size_t off = gather(pkts, n, 32);
    DevTmp din(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dops(ctx_, n * sizeof(uint32_t), rc);
    if (rc) return rc;
    const uint32_t m = static_cast<uint32_t>(n);
    if ((rc = nfcs_memcpy_h2d(ctx_, d_arena_, h_arena_, off ? off : 16))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, d_desc_, h_desc_, n * sizeof(nfcs_desc)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, din.p, egress_port, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_egress_plan_device(ctx_, eg, static_cast<uint8_t*>(d_arena_), off ? off : 16,
                                      static_cast<nfcs_desc*>(d_desc_), m, nullptr, nullptr,
                                      static_cast<uint32_t*>(din.p), static_cast<uint32_t*>(dport.p),
                                      static_cast<uint32_t*>(dops.p), static_cast<uint8_t*>(d_status_), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, ops, dops.p, n * sizeof(uint32_t)))) return rc;
    return nfcs_memcpy_d2h(ctx_, queue, d_status_, n);
}

inline int ChecksumEngine::egress_enqueue_batch(const nfcs_egress* eg, const uint32_t* port, const uint8_t* queue,
                                                size_t n, uint32_t* depth, uint8_t* result, uint32_t* order,
                                                uint32_t* key_start, uint32_t* key_dropped) {
    uint32_t keys = 0;
    if (!eg || !key_start || nfcs_egress_keys(eg, nullptr, &keys)) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!port || !queue || !order || (keys && !depth) || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    int rc = NFCS_OK;
    DevTmp dport(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dqueue(ctx_, n, rc);
    DevTmp dres(ctx_, n, rc);
    DevTmp dorder(ctx_, n * sizeof(uint32_t), rc);
    DevTmp ddepth(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    DevTmp dks(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    DevTmp ddrop(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    if (rc) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dport.p, port, n * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dqueue.p, queue, n))) return rc;
    if (keys && (rc = nfcs_memcpy_h2d(ctx_, ddepth.p, depth, keys * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_egress_enqueue_device(ctx_, eg, static_cast<uint32_t*>(dport.p), static_cast<uint8_t*>(dqueue.p),
                                         static_cast<uint32_t>(n), static_cast<uint32_t*>(ddepth.p),
                                         static_cast<uint8_t*>(dres.p), static_cast<uint32_t*>(dorder.p),
                                         static_cast<uint32_t*>(dks.p), static_cast<uint32_t*>(ddrop.p), nullptr)))
        return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, key_start, dks.p, (keys + 1u) * sizeof(uint32_t)))) return rc;
    if (key_start[keys] > n) return NFCS_EHIP;
    if (key_start[keys] && (rc = nfcs_memcpy_d2h(ctx_, order, dorder.p, key_start[keys] * sizeof(uint32_t)))) return rc;
    if (keys && (rc = nfcs_memcpy_d2h(ctx_, depth, ddepth.p, keys * sizeof(uint32_t)))) return rc;
    if (result && (rc = nfcs_memcpy_d2h(ctx_, result, dres.p, n))) return rc;
    if (key_dropped && keys && (rc = nfcs_memcpy_d2h(ctx_, key_dropped, ddrop.p, keys * sizeof(uint32_t)))) return rc;
    return NFCS_OK;
}

inline int ChecksumEngine::txq_append_batch(nfcs_txq* txq, const uint32_t* order, const uint32_t* key_start,
                                            const uint32_t* depth, const uint64_t* handle, size_t n) {
    uint32_t keys = 0;
    if (!txq || nfcs_txq_info(txq, nullptr, &keys, nullptr)) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!order || !key_start || !handle || (keys && !depth) || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    if (key_start[keys] > n) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    int rc = NFCS_OK;
    DevTmp dorder(ctx_, n * sizeof(uint32_t), rc);
    DevTmp dks(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    DevTmp ddepth(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    DevTmp dhandle(ctx_, n * sizeof(uint64_t), rc);
    if (rc) return rc;
    if (key_start[keys] && (rc = nfcs_memcpy_h2d(ctx_, dorder.p, order, key_start[keys] * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dks.p, key_start, (keys + 1u) * sizeof(uint32_t)))) return rc;
    if (keys && (rc = nfcs_memcpy_h2d(ctx_, ddepth.p, depth, keys * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_memcpy_h2d(ctx_, dhandle.p, handle, n * sizeof(uint64_t)))) return rc;
    if ((rc = nfcs_txq_append_device(ctx_, txq, static_cast<uint32_t*>(dorder.p), static_cast<uint32_t*>(dks.p),
                                     static_cast<uint32_t*>(ddepth.p), static_cast<uint64_t*>(dhandle.p), nullptr,
                                     static_cast<uint32_t>(n), nullptr)))
        return rc;
    return nfcs_stream_sync(ctx_, nullptr);  // the temporaries are freed on return
}

inline int ChecksumEngine::txq_dequeue_batch(nfcs_txq* txq, const uint32_t* budget, uint32_t budget_all, uint32_t* depth,
                                             uint64_t* tx, uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start,
                                             uint32_t* dequeued) {
    uint32_t ports = 0, keys = 0;
    if (!txq || !tx_start || nfcs_txq_info(txq, &ports, &keys, nullptr)) return NFCS_EINVAL;
    if ((keys && !depth) || (tx_cap && !tx)) return NFCS_EINVAL;
    std::lock_guard<std::mutex> lock(mu_);
    int rc = NFCS_OK;
    DevTmp dbudget(ctx_, (ports + 1u) * sizeof(uint32_t), rc);
    DevTmp ddepth(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    DevTmp dtx(ctx_, (static_cast<size_t>(tx_cap) + 1u) * sizeof(uint64_t), rc);
    DevTmp dtxq(ctx_, static_cast<size_t>(tx_cap) + 1u, rc);
    DevTmp dstart(ctx_, (ports + 1u) * sizeof(uint32_t), rc);
    DevTmp ddeq(ctx_, (keys + 1u) * sizeof(uint32_t), rc);
    if (rc) return rc;
    if (budget && ports && (rc = nfcs_memcpy_h2d(ctx_, dbudget.p, budget, ports * sizeof(uint32_t)))) return rc;
    if (keys && (rc = nfcs_memcpy_h2d(ctx_, ddepth.p, depth, keys * sizeof(uint32_t)))) return rc;
    if ((rc = nfcs_txq_dequeue_device(ctx_, txq, budget ? static_cast<uint32_t*>(dbudget.p) : nullptr, budget_all,
                                      static_cast<uint32_t*>(ddepth.p), static_cast<uint64_t*>(dtx.p), tx_cap,
                                      static_cast<uint8_t*>(dtxq.p), static_cast<uint32_t*>(dstart.p),
                                      static_cast<uint32_t*>(ddeq.p), nullptr)))
        return rc;
    if ((rc = nfcs_stream_sync(ctx_, nullptr))) return rc;
    if ((rc = nfcs_memcpy_d2h(ctx_, tx_start, dstart.p, (ports + 1u) * sizeof(uint32_t)))) return rc;
    const uint32_t total = tx_start[ports];
    if (total > tx_cap) return NFCS_EHIP;
    if (total && (rc = nfcs_memcpy_d2h(ctx_, tx, dtx.p, total * sizeof(uint64_t)))) return rc;
    if (total && tx_queue && (rc = nfcs_memcpy_d2h(ctx_, tx_queue, dtxq.p, total))) return rc;
    if (keys && (rc = nfcs_memcpy_d2h(ctx_, depth, ddepth.p, keys * sizeof(uint32_t)))) return rc;
    if (dequeued && keys && (rc = nfcs_memcpy_d2h(ctx_, dequeued, ddeq.p, keys * sizeof(uint32_t)))) return rc;
    return NFCS_OK;
}

// Same interface as netflow::BufferPool (buffer_pool.hpp:57-123: allocate_buffer(payload,
// headroom), free_buffer(buffer) with the PacketBuffer reference count), except that every
// buffer up to slot_bytes is a slot of ONE pinned arena (nfcs_host_alloc). update_checksums_batch
// builds the descriptors straight from the slots: frames that fill most of their slots go as spans
// DMA'd from the pinned arena (nfcs_update_host, patch records back; or, with NFCS_HOST_ZERO_COPY,
// read by the kernel over PCIe in place); frames that fill less than 85% of them are gathered by the
// library's copy threads first (nfcs_update_host_frames), so the slots' unused bytes do not cross PCIe.
// Buffers larger than a slot are heap PacketBuffers, as the reference allocates them.
// The default slot is 2176 bytes (a 2048-byte data room + 128 bytes of headroom, DPDK's mbuf
// layout): power-of-two slots alias on MI355X — C1's frames in 2048-byte slots checksum at 0.716 of
// 8 TB/s (read pass 232 µs, write pass 41.7 µs) against 0.781 in 2176-byte slots (222 / 28.5 µs;
// round 3, profiles/r03_stride_*.json).
class BufferPool {
public:
    explicit BufferPool(size_t slots = 65536, size_t slot_bytes = 2176,
                        ChecksumEngine& engine = ChecksumEngine::instance())
        : eng_(engine), slots_(slots), slot_bytes_((slot_bytes + 15) & ~size_t(15)) {
        if (slots_ == 0 || slots_ * slot_bytes_ / 16 > 0xFFFFFFFFull)
            throw std::invalid_argument("BufferPool: slots x slot_bytes must address < 64 GiB");
        void* p = nullptr;
        const int rc = nfcs_host_alloc(eng_.ctx(), slots_ * slot_bytes_, &p);
        if (rc != NFCS_OK) throw std::bad_alloc();
        arena_ = static_cast<unsigned char*>(p);
        bufs_.reserve(slots_);
        free_.reserve(slots_);
        for (size_t i = 0; i < slots_; ++i) {
            bufs_.emplace_back(new PacketBuffer(PacketBuffer::External{}, arena_ + i * slot_bytes_, slot_bytes_));
            free_.push_back(static_cast<uint32_t>(slots_ - 1 - i));  // allocate in arena order
        }
    }
    ~BufferPool() {
        std::lock_guard<std::mutex> lock(mu_);
        for (PacketBuffer* b : heap_free_) delete b;
        bufs_.clear();
        nfcs_host_free(eng_.ctx(), arena_);
    }
    BufferPool(const BufferPool&) = delete;
    BufferPool& operator=(const BufferPool&) = delete;

    // buffer_pool.hpp:66-103: data length 0, the given headroom, reference count 1.
    PacketBuffer* allocate_buffer(size_t required_data_payload_size, size_t required_headroom = 32) {
        std::lock_guard<std::mutex> lock(mu_);
        const size_t need = required_data_payload_size + required_headroom;
        if (need <= slot_bytes_ && !free_.empty()) {
            PacketBuffer* b = bufs_[free_.back()].get();
            free_.pop_back();
            b->ref_count.store(1, std::memory_order_relaxed);
            b->reset_offsets_and_len(required_headroom, 0);
            return b;
        }
        for (auto it = heap_free_.begin(); it != heap_free_.end(); ++it) {
            if ((*it)->get_capacity() >= need) {
                PacketBuffer* b = *it;
                heap_free_.erase(it);
                b->ref_count.store(1, std::memory_order_relaxed);
                b->reset_offsets_and_len(required_headroom, 0);
                return b;
            }
        }
        return new PacketBuffer(need, required_headroom, 0);
    }

    // buffer_pool.hpp:106-123: back to the pool when the last reference is released.
    void free_buffer(PacketBuffer* buffer) {
        if (!buffer || !buffer->decrement_ref()) return;
        std::lock_guard<std::mutex> lock(mu_);
        if (in_arena(buffer)) free_.push_back(slot_of(buffer));
        else heap_free_.push_back(buffer);
    }

    bool in_arena(const PacketBuffer* b) const {
        return b && b->storage() >= arena_ && b->storage() < arena_ + slots_ * slot_bytes_;
    }
    size_t available() {
        std::lock_guard<std::mutex> lock(mu_);
        return free_.size();
    }
    unsigned char* arena() const { return arena_; }

    // Batched Packet::update_checksums() on packets whose buffers are pool slots with 16-byte
    // aligned data starts (the default headroom of 32 keeps them aligned): no gather or scatter
    // copies. Other packets make the call fall back to ChecksumEngine::update_checksums_batch.
    // flags: 0 (frames DMA'd from the pinned arena) or NFCS_HOST_ZERO_COPY.
    int update_checksums_batch(Packet* const* pkts, size_t n, uint8_t* status = nullptr,
                               uint32_t flags = 0);

private:
    uint32_t slot_of(const PacketBuffer* b) const {
        return static_cast<uint32_t>((b->storage() - arena_) / slot_bytes_);
    }

    ChecksumEngine& eng_;
    size_t slots_, slot_bytes_;
    unsigned char* arena_ = nullptr;
    std::vector<std::unique_ptr<PacketBuffer>> bufs_;
    std::vector<uint32_t> free_;
    std::vector<PacketBuffer*> heap_free_;
    std::mutex mu_;
};

inline int BufferPool::update_checksums_batch(Packet* const* pkts, size_t n, uint8_t* status,
                                              uint32_t flags) {
    if (n == 0) return NFCS_OK;
    if (!pkts || n > 0xFFFFFFFFu) return NFCS_EINVAL;
    std::vector<nfcs_desc> desc(n);
    std::atomic<bool> foreign{false};  // a packet whose buffer is not a 16-byte aligned slot of the pool
    detail::parallel_ranges(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            PacketBuffer* b = pkts[i] ? pkts[i]->get_buffer() : nullptr;
            const unsigned char* d = b ? b->get_data_start_ptr() : nullptr;
            if (!b || !in_arena(b) || ((d - arena_) & 15)) {
                foreign.store(true, std::memory_order_relaxed);
                break;
            }
            desc[i] = nfcs_desc{static_cast<uint32_t>((d - arena_) >> 4), static_cast<uint32_t>(b->get_data_length())};
        }
    });
    if (foreign.load()) return eng_.update_checksums_batch(pkts, n, status);
    size_t drops = 0;  // places where the burst's arena offsets go down (a wrap of the pool's slots)
    uint64_t frame_bytes = 0, span = 0, lo = 0, hi = 0;  // span: the runs' bytes, as nfcs_update_host stages them
    for (size_t i = 0; i < n; ++i) {
        const uint64_t o = (uint64_t)desc[i].off16 * 16, e = o + ((desc[i].len + 15u) & ~15u);
        if (i && desc[i].off16 < desc[i - 1].off16) {
            ++drops;
            span += hi - lo;
            lo = hi = o;
        } else if (i == 0) {
            lo = hi = o;
        }
        hi = std::max(hi, e);
        frame_bytes += desc[i].len;
    }
    span += hi - lo;
    // Frames that fill less than 85% of their slots: DMA'd as spans, the slots' unused bytes would
    // cross PCIe too (C1's 1500-byte frames in 2176-byte slots: 33 GB/s of frames); gathered by the
    // library's copy threads first, only frame bytes do (49 GB/s; round 5, profiles/r05_b_adapter_t8.json).
    // A burst spanning at most NFCS_HOST_ZERO_COPY_AUTO_BYTES runs zero-copy in nfcs_update_host, where the
    // kernel reads only the frames' bytes in place: no gather then (round 6). NFCS_HOST_ZERO_COPY stays a
    // span read in place.
    if (flags == 0 && frame_bytes < n * slot_bytes_ * 85 / 100 && span > NFCS_HOST_ZERO_COPY_AUTO_BYTES) {
        std::vector<uint8_t*> fr(n);
        std::vector<uint32_t> ln(n);
        for (size_t i = 0; i < n; ++i) {
            fr[i] = arena_ + (size_t)desc[i].off16 * 16;
            ln[i] = desc[i].len;
        }
        return eng_.update_host_frames(fr.data(), ln.data(), static_cast<uint32_t>(n), status);
    }
    // nfcs_update_host stages each run of ascending offsets as one span: a burst in allocation order
    // (the pool hands slots out in arena order) or wrapping once goes as it is; a burst in an order
    // the pool's reuse has scrambled is sorted first, so its spans stay long. A wrap is one drop whose
    // second run ends at or before the first run's first frame ([100..199, 0, 9000] also
    // has one drop, but staged as is its second span would carry every slot from 0 to 9000)
    const bool wrap = drops == 1 && (uint64_t)desc[n - 1].off16 * 16 + desc[n - 1].len <= (uint64_t)desc[0].off16 * 16;
    if (drops == 0 || wrap) {
        return eng_.update_host(arena_, slots_ * slot_bytes_, desc.data(), static_cast<uint32_t>(n), status, flags);
    }
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return desc[a].off16 < desc[b].off16; });
    std::vector<nfcs_desc> sorted(n);
    for (size_t j = 0; j < n; ++j) sorted[j] = desc[order[j]];
    std::vector<uint8_t> st(status ? n : 0);
    const int rc = eng_.update_host(arena_, slots_ * slot_bytes_, sorted.data(), static_cast<uint32_t>(n),
                                    status ? st.data() : nullptr, flags);
    if (rc) return rc;
    if (status)
        for (size_t j = 0; j < n; ++j) status[order[j]] = st[j];
    return NFCS_OK;
}

// Free-function forms on the process-wide engine: they return NFCS_ENODEV (or the error
// nfcs_ctx_create reported) instead of throwing when no gfx950 engine exists.
namespace detail {
template <class F>
int on_default_engine(F&& f) noexcept {
    int rc = NFCS_OK;
    ChecksumEngine* e = ChecksumEngine::try_instance(&rc);
    if (!e) return rc ? rc : NFCS_ENODEV;
    try {
        return f(*e);
    } catch (...) {  // std::bad_alloc from the host-side gather: the reference's only escape too
        return NFCS_ENOMEM;
    }
}
}  // namespace detail

inline int update_checksums_batch(Packet* const* pkts, size_t n, uint8_t* status = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.update_checksums_batch(pkts, n, status); });
}
inline int update_checksums_batch(const std::vector<Packet*>& pkts, uint8_t* status = nullptr) {
    return update_checksums_batch(pkts.data(), pkts.size(), status);
}
inline int vlan_batch(Packet* const* pkts, const uint32_t* ops, size_t n, bool* ok = nullptr,
                      uint8_t* status = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.vlan_batch(pkts, ops, n, ok, status); });
}
inline int l3_forward_batch(Packet* const* pkts, const uint32_t* next_hop, size_t n,
                            const nfcs_nexthop* table, uint32_t table_n, uint8_t* status = nullptr) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.l3_forward_batch(pkts, next_hop, n, table, table_n, status); });
}
// A committed nfcs_fib from any routing table object: rm.get_routing_table() yields entries with
// destination_network, subnet_mask, next_hop_ip and egress_interface_id (RoutingManager's RouteEntry),
// taken in the order given (the lookup order); arp_entries / interface_macs pair an address / interface
// id with a MAC type that has `bytes[6]`. *out: the table (nfcs_fib_destroy it), or nullptr on error.
template <class RoutingTable, class Mac>
inline int make_fib_from(const RoutingTable& rm, const std::vector<std::pair<uint32_t, Mac>>& arp_entries,
                         const std::vector<std::pair<uint32_t, Mac>>& interface_macs,
                         const std::vector<uint32_t>& local_ips, nfcs_fib** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    std::vector<nfcs_fib_route> routes;
    for (const auto& e : rm.get_routing_table())
        routes.push_back(nfcs_fib_route{e.destination_network, e.subnet_mask, e.next_hop_ip, e.egress_interface_id});
    std::vector<nfcs_fib_arp> arp;
    for (const auto& a : arp_entries) {
        nfcs_fib_arp r{};
        r.ip = a.first;
        std::memcpy(r.mac, a.second.bytes, 6);
        arp.push_back(r);
    }
    std::vector<nfcs_fib_if_mac> ifm;
    for (const auto& m : interface_macs) {
        nfcs_fib_if_mac r{};
        r.egress_if = m.first;
        std::memcpy(r.mac, m.second.bytes, 6);
        ifm.push_back(r);
    }
    nfcs_fib* fib = nullptr;
    int rc = nfcs_fib_create(&fib);
    if (!rc) rc = nfcs_fib_set_routes(fib, routes.data(), static_cast<uint32_t>(routes.size()));
    if (!rc) rc = nfcs_fib_set_arp(fib, arp.data(), static_cast<uint32_t>(arp.size()));
    if (!rc) rc = nfcs_fib_set_if_macs(fib, ifm.data(), static_cast<uint32_t>(ifm.size()));
    if (!rc) rc = nfcs_fib_set_local_ips(fib, local_ips.data(), static_cast<uint32_t>(local_ips.size()));
    if (!rc) rc = nfcs_fib_commit(fib);
    if (rc && fib) nfcs_fib_destroy(fib);
    else *out = fib;
    return rc;
}

inline int route_lookup_batch(Packet* const* pkts, size_t n, const nfcs_fib* fib, uint32_t* next_hop,
                              uint32_t* egress_if = nullptr, uint8_t* verdict = nullptr) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.route_lookup_batch(pkts, n, fib, next_hop, egress_if, verdict); });
}
// A committed nfcs_acl from a rule vector with AclRule's members (acl_manager.hpp:28-69), taken in
// the order given (the order evaluate walks: pass get_all_rules(name) as it is): rule_id, action
// (an enum or integer with PERMIT 0, DENY 1, REDIRECT 2), redirect_port_id and the nine match fields
// src_mac / dst_mac (a MAC type with `bytes[6]`), vlan_id, ethertype, src_ip, dst_ip (host byte order),
// protocol, src_port, dst_port, each a std::optional (anything with operator bool and operator*). An
// engaged optional sets the field's bit; the address masks are full, which is the reference's exact
// match. *out: the list (nfcs_acl_destroy it), or nullptr on error.
template <class Rule>
inline std::vector<nfcs_acl_rule> acl_records_from(const std::vector<Rule>& rules) {
    std::vector<nfcs_acl_rule> recs;
    recs.reserve(rules.size());
    for (const Rule& a : rules) {
        nfcs_acl_rule r{};
        r.rule_id = a.rule_id;
        r.action = static_cast<uint8_t>(static_cast<int>(a.action));
        r.redirect_port = a.redirect_port_id ? static_cast<uint32_t>(*a.redirect_port_id) : NFCS_IF_NONE;
        r.src_ip_mask = r.dst_ip_mask = 0xFFFFFFFFu;
        if (a.src_mac) { r.fields |= NFCS_ACL_F_SRC_MAC; std::memcpy(r.src_mac, (*a.src_mac).bytes, 6); }
        if (a.dst_mac) { r.fields |= NFCS_ACL_F_DST_MAC; std::memcpy(r.dst_mac, (*a.dst_mac).bytes, 6); }
        if (a.vlan_id) { r.fields |= NFCS_ACL_F_VLAN_ID; r.vlan_id = *a.vlan_id; }
        if (a.ethertype) { r.fields |= NFCS_ACL_F_ETHERTYPE; r.ethertype = *a.ethertype; }
        if (a.src_ip) { r.fields |= NFCS_ACL_F_SRC_IP; r.src_ip = *a.src_ip; }
        if (a.dst_ip) { r.fields |= NFCS_ACL_F_DST_IP; r.dst_ip = *a.dst_ip; }
        if (a.protocol) { r.fields |= NFCS_ACL_F_PROTOCOL; r.protocol = *a.protocol; }
        if (a.src_port) { r.fields |= NFCS_ACL_F_SRC_PORT; r.src_port = *a.src_port; }
        if (a.dst_port) { r.fields |= NFCS_ACL_F_DST_PORT; r.dst_port = *a.dst_port; }
        recs.push_back(r);
    }
    return recs;
}

template <class Rule>
inline int make_acl_from(const std::vector<Rule>& rules, nfcs_acl** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    const std::vector<nfcs_acl_rule> recs = acl_records_from(rules);
    nfcs_acl* acl = nullptr;
    int rc = nfcs_acl_create(&acl);
    if (!rc) rc = nfcs_acl_set_rules(acl, recs.data(), static_cast<uint32_t>(recs.size()));
    if (!rc) rc = nfcs_acl_commit(acl);
    if (rc && acl) nfcs_acl_destroy(acl);
    else *out = acl;
    return rc;
}

// A committed nfcs_aclset (the egress ACLs, one list per egress port) from the switch's named ACLs and its
// bindings: `lists` maps a name to AclManager::get_all_rules(name) as it is (rules as make_acl_from takes
// them), port_to_name holds (port, InterfaceManager::get_applied_acl_name(port, EGRESS)) for every bound
// port. The names get list ids in the map's order. A bound name that `lists` does not hold binds its port to
// a removed list, which reads as the reference's "ACL not found": PERMIT. More than NFCS_ACLSET_MAX_LISTS
// names (absent ones included), a port at or above NFCS_L2_MAX_PORTS, or lists that pad to more than
// NFCS_ACL_MAX_RULES rules together: NFCS_EINVAL. *out: the set (nfcs_aclset_destroy it; upload it with
// nfcs_aclset_upload before nfcs_egress_acl_device), or nullptr on error.
template <class Rule>
inline int make_acl_set_from(const std::map<std::string, std::vector<Rule>>& lists,
                             const std::vector<std::pair<uint32_t, std::string>>& port_to_name, nfcs_aclset** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    nfcs_aclset* set = nullptr;
    int rc = nfcs_aclset_create(&set);
    std::map<std::string, uint32_t> id_of;
    for (const auto& kv : lists) {
        if (rc) break;
        const uint32_t id = static_cast<uint32_t>(id_of.size());
        id_of[kv.first] = id;
        const std::vector<nfcs_acl_rule> recs = acl_records_from(kv.second);
        rc = nfcs_aclset_set_list(set, id, recs.data(), static_cast<uint32_t>(recs.size()));
    }
    for (const auto& pn : port_to_name) {
        if (rc) break;
        auto it = id_of.find(pn.second);
        if (it == id_of.end()) {  // a name without a list: an id of its own, set and removed
            it = id_of.emplace(pn.second, static_cast<uint32_t>(id_of.size())).first;
            rc = nfcs_aclset_remove_list(set, it->second);
        }
        if (!rc) rc = nfcs_aclset_bind_port(set, pn.first, it->second);
    }
    if (!rc) rc = nfcs_aclset_commit(set);
    if (rc && set) nfcs_aclset_destroy(set);
    else *out = set;
    return rc;
}

inline int acl_eval_batch(Packet* const* pkts, size_t n, const nfcs_acl* acl, uint8_t* action,
                          uint32_t* rule_index = nullptr, uint32_t* redirect_port = nullptr,
                          uint32_t* next_hop = nullptr) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.acl_eval_batch(pkts, n, acl, action, rule_index, redirect_port, next_hop); });
}
// A committed nfcs_fdb from the switch's L2 state, by member name: fdb.get_all_entries() yields entries
// with mac (a MAC type with `bytes[6]`), vlan_id, port and is_static (ForwardingDatabase's FdbEntry),
// passed on as they are; vlans.get_port_config(port) yields an optional (operator bool, operator->) of a
// config with type (an enum or integer with ACCESS 0, TRUNK 1, HYBRID 2), native_vlan and allowed_vlans
// (any range of VLAN ids: VlanManager::PortConfig); link_up(port) and stp_forwarding(port) are
// InterfaceManager::is_port_link_up and get_port_stp_state(port) == PortState::FORWARDING as callables.
// Ports 0 .. num_ports - 1 are set (num_ports at most NFCS_L2_MAX_PORTS). *out: the database
// (nfcs_fdb_destroy it; upload it with ChecksumEngine::upload_fdb before l2_lookup_batch), or nullptr
// on error.
template <class FdbT, class VlanT, class LinkUp, class StpForwarding>
inline int make_fdb_from(const FdbT& fdb, const VlanT& vlans, LinkUp&& link_up, StpForwarding&& stp_forwarding,
                         uint32_t num_ports, nfcs_fdb** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    std::vector<nfcs_fdb_entry> recs;
    for (const auto& e : fdb.get_all_entries()) {
        nfcs_fdb_entry r{};
        std::memcpy(r.mac, e.mac.bytes, 6);
        r.vlan_id = e.vlan_id;
        r.port = e.port;
        r.is_static = e.is_static ? 1 : 0;
        recs.push_back(r);
    }
    nfcs_fdb* f = nullptr;
    int rc = nfcs_fdb_create(&f);
    if (!rc) rc = nfcs_fdb_set_entries(f, recs.data(), static_cast<uint32_t>(recs.size()));
    for (uint32_t p = 0; !rc && p < num_ports; ++p) {
        nfcs_l2_port port{};
        port.port_id = p;
        port.link_up = link_up(p) ? 1 : 0;
        port.stp_forwarding = stp_forwarding(p) ? 1 : 0;
        std::vector<uint16_t> allowed;
        const auto cfg = vlans.get_port_config(p);
        if (cfg) {
            port.has_vlan_config = 1;
            port.type = static_cast<uint8_t>(static_cast<int>(cfg->type));
            port.native_vlan = cfg->native_vlan;
            for (const auto v : cfg->allowed_vlans) allowed.push_back(static_cast<uint16_t>(v));
        }
        rc = nfcs_fdb_set_port(f, &port, allowed.data(), static_cast<uint32_t>(allowed.size()));
    }
    if (!rc) rc = nfcs_fdb_commit(f);
    if (rc && f) nfcs_fdb_destroy(f);
    else *out = f;
    return rc;
}

// Committed egress ports from the switch's VLAN and QoS state, by member name: vlans.get_port_config(port)
// yields an optional (operator bool, operator->) of a config with type (an enum or integer with ACCESS 0,
// TRUNK 1, HYBRID 2), native_vlan and tag_native (VlanManager::PortConfig); qos.get_port_qos_config(port)
// yields an optional of a config with num_queues and max_queue_depth (QosConfig, as configure_port_qos
// stored it). Ports 0 .. num_ports - 1 are set (num_ports at most NFCS_L2_MAX_PORTS). *out: the object
// (nfcs_egress_destroy it; upload it with ChecksumEngine::upload_egress before egress_plan_batch), or
// nullptr on error.
template <class VlanT, class QosT>
inline int make_egress_from(const VlanT& vlans, const QosT& qos, uint32_t num_ports, nfcs_egress** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    nfcs_egress* g = nullptr;
    int rc = nfcs_egress_create(&g);
    for (uint32_t p = 0; !rc && p < num_ports; ++p) {
        nfcs_egress_port port{};
        port.port_id = p;
        const auto cfg = vlans.get_port_config(p);
        if (cfg) {
            port.has_vlan_config = 1;
            port.type = static_cast<uint8_t>(static_cast<int>(cfg->type));
            port.tag_native = cfg->tag_native ? 1 : 0;
            port.native_vlan = cfg->native_vlan;
        }
        const auto qc = qos.get_port_qos_config(p);
        if (qc) {
            port.has_qos = 1;
            port.num_queues = static_cast<uint8_t>(qc->num_queues);
            port.max_queue_depth = static_cast<uint32_t>(qc->max_queue_depth);
        }
        rc = nfcs_egress_set_port(g, &port);
    }
    if (!rc) rc = nfcs_egress_commit(g);
    if (rc && g) nfcs_egress_destroy(g);
    else *out = g;
    return rc;
}

inline int egress_plan_batch(Packet* const* pkts, size_t n, const nfcs_egress* eg, const uint32_t* egress_port,
                             uint32_t* ops, uint8_t* queue) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.egress_plan_batch(pkts, n, eg, egress_port, ops, queue); });
}
inline int egress_enqueue_batch(const nfcs_egress* eg, const uint32_t* port, const uint8_t* queue, size_t n,
                                uint32_t* depth, uint8_t* result, uint32_t* order, uint32_t* key_start,
                                uint32_t* key_dropped = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.egress_enqueue_batch(eg, port, queue, n, depth, result, order, key_start, key_dropped);
    });
}

// The schedulers of a TX queue object from the switch's QoS state, by member name:
// qos.get_port_qos_config(port) yields an optional of a config with `scheduler` (an enum or integer with
// STRICT_PRIORITY 0, WEIGHTED_ROUND_ROBIN 1, DEFICIT_ROUND_ROBIN 2: QosConfig). Ports 0 .. num_ports - 1 that
// have a config and lie within the object are set; make_egress_from does not read `scheduler`.
template <class QosT>
inline int set_schedulers_from(const QosT& qos, uint32_t num_ports, nfcs_txq* txq) {
    uint32_t ports = 0;
    int rc = nfcs_txq_info(txq, &ports, nullptr, nullptr);
    for (uint32_t p = 0; !rc && p < num_ports && p < ports; ++p) {
        const auto qc = qos.get_port_qos_config(p);
        if (qc) rc = nfcs_txq_set_scheduler(txq, p, static_cast<uint32_t>(static_cast<int>(qc->scheduler)));
    }
    return rc;
}
inline int make_txq(const nfcs_egress* eg, nfcs_txq** out) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.make_txq(eg, out); });
}
inline int txq_append_batch(nfcs_txq* txq, const uint32_t* order, const uint32_t* key_start, const uint32_t* depth,
                            const uint64_t* handle, size_t n) {
    return detail::on_default_engine(
        [&](ChecksumEngine& e) { return e.txq_append_batch(txq, order, key_start, depth, handle, n); });
}
inline int txq_dequeue_batch(nfcs_txq* txq, const uint32_t* budget, uint32_t budget_all, uint32_t* depth, uint64_t* tx,
                             uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start, uint32_t* dequeued = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.txq_dequeue_batch(txq, budget, budget_all, depth, tx, tx_cap, tx_queue, tx_start, dequeued);
    });
}

inline int l2_lookup_batch(Packet* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                           uint32_t* egress_port, uint8_t* verdict = nullptr, uint16_t* vlan = nullptr,
                           uint8_t* learn = nullptr, const uint8_t* rt_verdict = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.l2_lookup_batch(pkts, n, fdb, ingress_port, egress_port, verdict, vlan, learn, rt_verdict);
    });
}
inline int ingress_dispatch_batch(Packet* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                                  uint32_t num_ports, const uint8_t* rt_verdict, uint32_t* next_hop, uint32_t* l2_port,
                                  uint8_t* l2_verdict, const uint8_t* action = nullptr,
                                  const uint32_t* redirect_port = nullptr, uint8_t* cls = nullptr,
                                  uint8_t* bypass = nullptr, nfcs_rx_stats* rx = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.ingress_dispatch_batch(pkts, n, fdb, ingress_port, num_ports, rt_verdict, next_hop, l2_port, l2_verdict,
                                        action, redirect_port, cls, bypass, rx);
    });
}
inline int flood_expand_batch(Packet* const* pkts, size_t n, const nfcs_fdb* fdb, uint32_t ingress_port,
                              uint32_t num_ports, const uint32_t* egress_port, const uint8_t* l2_verdict,
                              const uint16_t* l2_vlan, ChecksumEngine::FloodItems* out) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.flood_expand_batch(pkts, n, fdb, ingress_port, num_ports, egress_port, l2_verdict, l2_vlan, out);
    });
}
inline int icmp_respond_batch(Packet* const* pkts, size_t n, const nfcs_icmp* icmp, const nfcs_fib* fib, uint32_t ingress_port,
                              const uint8_t* rt_verdict, const uint16_t* ip_id, ChecksumEngine::IcmpMessages* out) {
    return detail::on_default_engine([&](ChecksumEngine& e) {
        return e.icmp_respond_batch(pkts, n, icmp, fib, ingress_port, rt_verdict, ip_id, out);
    });
}

// A committed ICMP table set (nfcs_icmp) from an interface manager: per configured interface, ascending as
// InterfaceManager scans them, every address with the interface's MAC (get_mac_for_ip), the first address
// (get_interface_ip), and the ports below num_ports whose link is up (send_control_plane_packet's test). `ifm`
// needs get_all_port_configs() (a map from id to a config with mac_address.bytes and ip_configurations[].address)
// and is_port_link_up(id): netflow::InterfaceManager's names. Returns NFCS_OK and the tables in *out
// (nfcs_icmp_destroy them; upload them with ChecksumEngine::upload_icmp), or a negative NFCS_E* code.
template <class InterfaceManagerT>
inline int make_icmp_from(const InterfaceManagerT& ifm, uint32_t num_ports, nfcs_icmp** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    std::vector<nfcs_icmp_local> local;
    std::vector<nfcs_icmp_if_ip> if_ips;
    std::vector<uint32_t> up;
    for (const auto& kv : ifm.get_all_port_configs()) {
        const uint32_t id = static_cast<uint32_t>(kv.first);
        for (const auto& c : kv.second.ip_configurations) {
            nfcs_icmp_local l{};
            l.ip = c.address;
            std::memcpy(l.mac, kv.second.mac_address.bytes, 6);
            local.push_back(l);
            if_ips.push_back(nfcs_icmp_if_ip{id, c.address});
        }
        if (id < num_ports && ifm.is_port_link_up(id)) up.push_back(id);
    }
    nfcs_icmp* t = nullptr;
    int rc = nfcs_icmp_create(&t);
    if (rc) return rc;
    if ((rc = nfcs_icmp_set_local(t, local.data(), static_cast<uint32_t>(local.size()))) ||
        (rc = nfcs_icmp_set_if_ips(t, if_ips.data(), static_cast<uint32_t>(if_ips.size()))) ||
        (rc = nfcs_icmp_set_ports_up(t, up.data(), static_cast<uint32_t>(up.size()), num_ports)) || (rc = nfcs_icmp_commit(t))) {
        nfcs_icmp_destroy(t);
        return rc;
    }
    *out = t;
    return NFCS_OK;
}
inline int flow_keys_batch(Packet* const* pkts, size_t n, nfcs_flow_key* keys,
                           uint32_t* hashes = nullptr) {
    return detail::on_default_engine([&](ChecksumEngine& e) { return e.flow_keys_batch(pkts, n, keys, hashes); });
}

}  // namespace netflow_amd

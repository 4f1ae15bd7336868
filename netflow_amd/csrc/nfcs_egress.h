// nfcs_egress.h — the egress stage's host side: the ports' inputs, the compile step of
// nfcs_egress_commit (one 16-byte record per port), the one-frame decision of nfcs_egress_plan_host and
// the sequential walk of nfcs_egress_enqueue_host. Pure C++ (no HIP), so it also builds into a
// stand-alone host program (tests/cpp/egress_compile_main.cpp, run under the host sanitizers). The device
// side (upload, launches) is in nfcs_api.hip / nfcs_kernels.hip; nfcs_internal.h includes this file, so the
// record layout, the plan and the packet classes below are the kernels' as well: one definition each.
#pragma once

#include <stdint.h>

#include <vector>

#include "nfcs.h"

#if defined(__HIPCC__)
#define NFCS_EG_HD __host__ __device__
#else
#define NFCS_EG_HD
#endif

namespace nfcs {

// One port as the kernels read it, 16 bytes: one 16-byte load per packet. A port never set is all zero:
// no VLAN config, no QoS config.
//   flags      kEgVlanCfg | kEgUntagNative | kEgQos
//   native     native_vlan
//   queues     num_queues, 1..NFCS_QOS_MAX_QUEUES (0 without a QoS config)
//   max_depth  max_queue_depth, at least 1 (0 without a QoS config)
struct alignas(16) EgressRec {
    uint32_t flags, native, queues, max_depth;
};
static_assert(sizeof(EgressRec) == 16, "one port is one 16-byte load");
constexpr uint32_t kEgVlanCfg = 1u;      // get_port_config(port).has_value()
constexpr uint32_t kEgUntagNative = 2u;  // ACCESS, or TRUNK / HYBRID with tag_native clear
constexpr uint32_t kEgQos = 4u;          // get_port_qos_config(port).has_value()

struct EgressPortIn {
    bool set = false;
    nfcs_egress_port port{};
};

struct EgressInputs {
    std::vector<EgressPortIn> ports;  // indexed by port id, as long as the highest id set + 1
};

struct EgressTables {
    std::vector<EgressRec> recs;  // `ports` records
    uint32_t ports = 0;           // the highest port id set, plus one
    uint32_t keys = 0;            // ports * NFCS_QOS_MAX_QUEUES
};

inline void egress_compile(const EgressInputs& in, EgressTables& t) {
    t = EgressTables{};
    t.ports = (uint32_t)in.ports.size();
    t.keys = t.ports * NFCS_QOS_MAX_QUEUES;
    t.recs.assign(t.ports, EgressRec{0, 0, 0, 0});
    for (uint32_t p = 0; p < t.ports; ++p) {
        const EgressPortIn& pi = in.ports[p];
        if (!pi.set) continue;
        EgressRec& r = t.recs[p];
        if (pi.port.has_vlan_config) {
            r.flags |= kEgVlanCfg;
            r.native = pi.port.native_vlan;
            if (pi.port.type == 0 || !pi.port.tag_native) r.flags |= kEgUntagNative;
        }
        if (pi.port.has_qos) {  // QosConfig::validate_and_prepare: 0 queues and depth 0 each become 1
            r.flags |= kEgQos;
            r.queues = pi.port.num_queues ? pi.port.num_queues : 1u;
            r.max_depth = pi.port.max_queue_depth ? pi.port.max_queue_depth : 1u;
        }
    }
}

// process_egress + classify_packet_to_queue from the port's record, the frame's length and its bytes
// 12..19 as two little-endian words (w3: bytes 12-15, w4: bytes 16-19; a word whose bytes lie past the
// frame may hold anything: every use is guarded by the length). Host and device, this one definition.
NFCS_EG_HD inline void egress_plan_rec(const EgressRec& r, uint32_t len, uint32_t w3, uint32_t w4, uint32_t* op,
                                       uint32_t* queue) {
    const bool tagged = len >= 18u && (w3 & 0xFFFFu) == 0x0081u;  // vlan_id().has_value()
    const uint32_t tci = ((w3 >> 8) & 0xFF00u) | (w3 >> 24);
    const bool pop = tagged && (r.flags & kEgVlanCfg) && (r.flags & kEgUntagNative) && (tci & 0x0FFFu) == r.native;
    // the tag at byte 14 after the edit
    bool has_pcp = tagged;
    uint32_t pcp = tci >> 13;
    if (pop) {
        has_pcp = (w4 & 0xFFFFu) == 0x0081u && len - 4u >= 18u;
        pcp = (w4 >> 21) & 7u;  // old byte 18, bits 5-7
    }
    uint32_t q = 0;
    if (r.flags & kEgQos) {
        if (has_pcp) {
            q = r.queues == 4u ? 3u - (pcp >> 1) : ((7u - pcp) * r.queues) / 8u;
            if (q >= r.queues) q = r.queues - 1u;
        } else {
            q = r.queues - 1u;
        }
    }
    *op = pop ? NFCS_VLAN_POP : NFCS_VLAN_NOP;
    *queue = q;
}

// What enqueue_packet does with a packet before it looks at the queue's depth: NFCS_EQ_SKIP,
// NFCS_EQ_DROP_NO_CONFIG, NFCS_EQ_BAD_QUEUE, or NFCS_EQ_ENQUEUED with *key set (the depth then decides
// between ENQUEUED and DROP_FULL). `has_rec` false: the port is past the compiled records.
NFCS_EG_HD inline uint32_t egress_class(uint32_t port, uint32_t queue, bool has_rec, const EgressRec& r, uint32_t* key) {
    if (port == NFCS_IF_NONE) return NFCS_EQ_SKIP;
    if (!has_rec || !(r.flags & kEgQos)) return NFCS_EQ_DROP_NO_CONFIG;
    if (queue >= r.queues) return NFCS_EQ_BAD_QUEUE;
    *key = port * NFCS_QOS_MAX_QUEUES + queue;
    return NFCS_EQ_ENQUEUED;
}

inline void egress_plan(const EgressTables& t, uint32_t port, const uint8_t* f, uint32_t len, uint32_t* op,
                        uint32_t* queue) {
    uint32_t o = NFCS_VLAN_NOP, q = NFCS_QUEUE_NONE;
    if (port != NFCS_IF_NONE) {
        const EgressRec none{0, 0, 0, 0};
        uint32_t w[2] = {0, 0};  // bytes 12..19, as far as the frame has them
        for (uint32_t b = 12; b < 20 && b < len; ++b) w[(b - 12) >> 2] |= (uint32_t)f[b] << (8u * (b & 3u));
        egress_plan_rec(port < t.ports ? t.recs[port] : none, len >= 14u ? len : 0u, w[0], w[1], &o, &q);
    }
    if (op) *op = o;
    if (queue) *queue = q;
}

// enqueue_packet over the burst in order. depth: keys, in/out; order: n; key_start: keys + 1; result (n)
// and key_dropped (keys) may be null. Two passes, so that d_order comes out grouped by key.
inline void egress_enqueue(const EgressTables& t, const uint32_t* port, const uint8_t* queue, uint32_t n,
                           uint32_t* depth, uint8_t* result, uint32_t* order, uint32_t* key_start,
                           uint32_t* key_dropped) {
    const EgressRec none{0, 0, 0, 0};
    std::vector<uint32_t> enq(t.keys, 0u), room(t.keys, 0u), fill(t.keys, 0u);
    for (uint32_t k = 0; k < t.keys; ++k) {
        const EgressRec& r = t.recs[k / NFCS_QOS_MAX_QUEUES];
        room[k] = r.max_depth > depth[k] ? r.max_depth - depth[k] : 0u;  // size() >= max_queue_depth: full
        if (key_dropped) key_dropped[k] = 0;
    }
    std::vector<uint8_t> res(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t key = 0;
        const bool has = port[i] < t.ports;
        uint32_t c = egress_class(port[i], queue[i], has, has ? t.recs[port[i]] : none, &key);
        if (c == NFCS_EQ_ENQUEUED) {
            if (enq[key] < room[key]) ++enq[key];
            else {
                c = NFCS_EQ_DROP_FULL;
                if (key_dropped) ++key_dropped[key];
            }
        }
        res[i] = (uint8_t)c;
        if (result) result[i] = (uint8_t)c;
    }
    uint32_t run = 0;
    for (uint32_t k = 0; k < t.keys; ++k) {
        key_start[k] = run;
        run += enq[k];
        depth[k] += enq[k];
    }
    key_start[t.keys] = run;
    for (uint32_t i = 0; i < n; ++i) {
        if (res[i] != NFCS_EQ_ENQUEUED) continue;
        const uint32_t key = port[i] * NFCS_QOS_MAX_QUEUES + queue[i];
        order[key_start[key] + fill[key]++] = i;
    }
}

}  // namespace nfcs

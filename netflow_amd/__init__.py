"""netflow_amd — MI355X-native batched Internet-checksum engine for NetFlow++'s
``Packet::update_checksums()`` path (include/netflow++/packet.hpp:722-912).

The compute lives in ``libnfcs.so`` (hand-written gfx950 HIP kernels behind the C ABI in
``include/nfcs.h``). This module is a thin ctypes host layer over that ABI: device buffers,
contexts, the batched update on device-resident or host-resident frames, synthetic batches
and digests. It never computes a checksum itself and has no CPU fallback: if the HIP
library is missing or no gfx950 device is present, it raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("NFCS_LIB") or os.path.join(HERE, "libnfcs.so")
HEADER = os.path.join(ROOT, "include", "nfcs.h")
SOURCES = [os.path.join(HERE, "csrc", "nfcs_kernels.hip"), os.path.join(HERE, "csrc", "nfcs_api.hip")]

DESC_DTYPE = np.dtype([("off16", "<u4"), ("len", "<u4")])
PATCH_DTYPE = np.dtype([("ip_off", "<u2"), ("l4_off", "<u2"), ("ip", "u1", (2,)), ("l4", "u1", (2,))])

# status codes (include/nfcs.h)
ST_NONE, ST_V4, ST_V4_TCP, ST_V4_UDP, ST_V4_ICMP, ST_V4_L4SKIP = 0, 1, 2, 3, 4, 5
ST_V6, ST_V6_TCP, ST_V6_UDP, ST_V6_L4SKIP, ST_OOB, ST_BAD_DESC = 6, 7, 8, 9, 14, 15
ST_FLAG_OVERLAP = 0x40
ST_NO_ROUTE, ST_NOT_IPV4, ST_TTL_EXPIRED, ST_FLAG_FWD = 11, 12, 13, 0x80
NH_NONE = 0xFFFFFFFF
ST_VLAN_FAIL, ST_FLAG_VLAN = 16, 0x20
VLAN_NOP, VLAN_PUSH, VLAN_POP = 0, 0x40000000, 0x80000000


def vlan_push_op(vid: int, prio: int = 0) -> int:
    """NFCS_VLAN_PUSH_OP(vid, prio): the edit word of Packet::push_vlan(vid, prio)."""
    return VLAN_PUSH | ((prio & 7) << 13) | (vid & 0xFFF)

# nfcs_route_lookup_device verdicts (include/nfcs.h NFCS_RT_*)
RT_FORWARD, RT_BAD_DESC, RT_NOT_IPV4, RT_LOCAL, RT_TTL_EXPIRED, RT_NO_ROUTE, RT_ARP_MISS, RT_NO_IF_MAC = range(8)
IF_NONE = 0xFFFFFFFF
FIB_MAX_ROUTES = 4096
FIB_ROUTE_DTYPE = np.dtype([("network", "<u4"), ("mask", "<u4"), ("next_hop_ip", "<u4"), ("egress_if", "<u4")])
FIB_ARP_DTYPE = np.dtype([("ip", "<u4"), ("mac", "u1", (6,)), ("pad", "u1", (2,))])
FIB_IF_MAC_DTYPE = np.dtype([("egress_if", "<u4"), ("mac", "u1", (6,)), ("pad", "u1", (2,))])

# nfcs_acl_eval_device / nfcs_acl_eval_host (include/nfcs.h NFCS_ACL_*)
ACL_PERMIT, ACL_DENY, ACL_REDIRECT, ACL_BAD_DESC = range(4)
ACL_NO_MATCH = 0xFFFFFFFF
ACL_MAX_RULES = 512
ACL_GROUP = 4  # rules per trip of the kernel's scan (csrc/nfcs_acl.h kAclGroup)
(ACL_F_SRC_MAC, ACL_F_DST_MAC, ACL_F_VLAN_ID, ACL_F_ETHERTYPE, ACL_F_SRC_IP, ACL_F_DST_IP, ACL_F_PROTOCOL,
 ACL_F_SRC_PORT, ACL_F_DST_PORT) = (1 << k for k in range(9))
# nfcs_acl_rule: addresses and their masks in HOST byte order (10.1.2.3 = 0x0A010203), unlike the FIB's
ACL_RULE_DTYPE = np.dtype([("fields", "<u4"), ("rule_id", "<u4"), ("src_mac", "u1", (6,)), ("dst_mac", "u1", (6,)),
                           ("vlan_id", "<u2"), ("ethertype", "<u2"), ("src_ip", "<u4"), ("dst_ip", "<u4"),
                           ("src_ip_mask", "<u4"), ("dst_ip_mask", "<u4"), ("src_port", "<u2"), ("dst_port", "<u2"),
                           ("protocol", "u1"), ("action", "u1"), ("pad", "u1", (2,)), ("redirect_port", "<u4")])
assert ACL_RULE_DTYPE.itemsize == 52
# nfcs_aclset / nfcs_egress_acl_device (the egress ACLs: one list per egress port)
ACL_NO_PORT = 4  # the packet had no egress port (IF_NONE): neither descriptor nor frame looked at
ACL_LIST_NONE = 0xFFFFFFFF
ACLSET_MAX_LISTS = 128

# nfcs_l2_lookup_device / nfcs_fdb_lookup_host (include/nfcs.h NFCS_L2_*)
(L2_FORWARD, L2_BAD_DESC, L2_SKIP, L2_NO_ETH, L2_FLOOD, L2_DROP_SAME_PORT, L2_DROP_LINK_DOWN, L2_DROP_STP,
 L2_DROP_VLAN) = range(9)
L2_LEARN_NONE, L2_LEARN_NEW, L2_LEARN_REFRESH, L2_LEARN_MOVED = range(4)
L2_ACCESS, L2_TRUNK, L2_HYBRID = range(3)  # nfcs_l2_port.type
FDB_MAX_ENTRIES = 1 << 20
L2_MAX_PORTS = 1024
FDB_ENTRY_DTYPE = np.dtype([("mac", "u1", (6,)), ("vlan_id", "<u2"), ("port", "<u4"), ("is_static", "u1"),
                            ("pad", "u1", (3,))])
L2_PORT_DTYPE = np.dtype([("port_id", "<u4"), ("link_up", "u1"), ("stp_forwarding", "u1"), ("has_vlan_config", "u1"),
                          ("type", "u1"), ("native_vlan", "<u2"), ("pad", "<u2")])
assert FDB_ENTRY_DTYPE.itemsize == 16 and L2_PORT_DTYPE.itemsize == 12

# flood replication (include/nfcs.h nfcs_flood_expand_*)
FLOOD_TILE_PKTS = 1024  # NFCS_FLOOD_TILE_PKTS: the scan's tile, speed only
ITEM_NONE = 0xFFFFFFFF
FLOOD_TOTALS_DTYPE = np.dtype([("items", "<u4"), ("items_needed", "<u4"), ("copies", "<u4"), ("flooded", "<u4"),
                               ("copy_bytes", "<u8"), ("copy_bytes_needed", "<u8")])
assert FLOOD_TOTALS_DTYPE.itemsize == 32

# the ICMP responder (include/nfcs.h nfcs_icmp_*, NFCS_ICMP_ST_*)
ICMP_TILE_PKTS = 1024  # NFCS_ICMP_TILE_PKTS: the scan's tile, speed only
(ICMP_ST_NONE, ICMP_ST_ECHO_REPLY, ICMP_ST_TIME_EXCEEDED, ICMP_ST_UNREACHABLE, ICMP_ST_TO_CPU, ICMP_ST_IGNORED,
 ICMP_ST_NO_LOCAL_MAC, ICMP_ST_SRC_NO_ROUTE, ICMP_ST_SRC_NO_IF_IP, ICMP_ST_SRC_ARP_MISS, ICMP_ST_SRC_NO_IF_MAC,
 ICMP_ST_PORT_DOWN, ICMP_ST_OOB, ICMP_ST_TOO_LONG, ICMP_ST_OVERFLOW) = range(15)
ICMP_LOCAL_DTYPE = np.dtype([("ip", "<u4"), ("mac", "u1", (6,)), ("pad", "u1", (2,))])
ICMP_IF_IP_DTYPE = np.dtype([("egress_if", "<u4"), ("ip", "<u4")])
ICMP_TOTALS_DTYPE = np.dtype([("messages", "<u4"), ("messages_needed", "<u4"), ("echo_replies", "<u4"),
                              ("errors", "<u4"), ("msg_bytes", "<u8"), ("msg_bytes_needed", "<u8")])
assert ICMP_LOCAL_DTYPE.itemsize == 12 and ICMP_IF_IP_DTYPE.itemsize == 8 and ICMP_TOTALS_DTYPE.itemsize == 32

# the egress stage (include/nfcs.h nfcs_egress_*, NFCS_EQ_*)
QOS_MAX_QUEUES = 8      # classify_packet_to_queue names at most 8 queues from 8 PCP values
QUEUE_NONE = 0xFF
EGRESS_TILE_PKTS = 1024  # NFCS_EGRESS_TILE_PKTS: the enqueue's tile, speed only
EQ_ENQUEUED, EQ_SKIP, EQ_DROP_NO_CONFIG, EQ_DROP_FULL, EQ_BAD_QUEUE = range(5)
EGRESS_PORT_DTYPE = np.dtype([("port_id", "<u4"), ("has_vlan_config", "u1"), ("type", "u1"), ("tag_native", "u1"),
                              ("has_qos", "u1"), ("native_vlan", "<u2"), ("num_queues", "u1"), ("pad", "u1"),
                              ("max_queue_depth", "<u4")])
assert EGRESS_PORT_DTYPE.itemsize == 16
# the TX queues (include/nfcs.h nfcs_txq_*, NFCS_SCHED_*); WRR and DRR are the reference's one plain round-robin
SCHED_STRICT_PRIORITY, SCHED_WRR, SCHED_DRR = range(3)

# the ingress dispatch and the one-call RX pipeline (include/nfcs.h nfcs_sw_class, nfcs_rx_stats)
(SW_UNHANDLED, SW_RX_DOWN, SW_IN_DENY, SW_RED_OK, SW_RED_DOWN, SW_RED_RANGE, SW_LLDP, SW_ZERO_MAC, SW_ARP, SW_LOCAL,
 SW_TTL, SW_NO_ROUTE, SW_ARP_MISS, SW_NO_IF_MAC, SW_L3_FWD, SW_L2_FWD, SW_L2_FLOOD, SW_SAME_PORT, SW_LINK_DOWN, SW_STP,
 SW_VLAN, SW_BAD_DESC) = range(22)
ACL_BYPASS = 5  # egress_acl_items_*: the item's source frame was redirected by the ingress ACL
RX_STATS_DTYPE = np.dtype([("rx_packets", "<u8"), ("rx_bytes", "<u8"), ("rx_drops", "<u8")])
assert RX_STATS_DTYPE.itemsize == 24

NEXTHOP_DTYPE = np.dtype([("dst_mac", "u1", (6,)), ("src_mac", "u1", (6,))])
FLOW_KEY_DTYPE = np.dtype([("hash", "<u4"), ("vlan_id", "<u2"), ("ethertype", "<u2"),
                           ("src_mac", "u1", (6,)), ("dst_mac", "u1", (6,)), ("protocol", "u1"),
                           ("is_ipv6", "u1"), ("src_port", "<u2"), ("dst_port", "<u2"),
                           ("reserved", "u1", (6,)), ("src_ip", "u1", (16,)), ("dst_ip", "u1", (16,))])
assert FLOW_KEY_DTYPE.itemsize == 64
CFG_C0, CFG_C1, CFG_C2, CFG_C3 = 0, 1, 2, 3
HOST_PATCH_ONLY, HOST_ZERO_COPY, HOST_FRAMES = 1, 2, 4
PATCH_NONE = 0xFFFF
# nfcs_ctx_set_store_policy / nfcs_ctx_store_state (include/nfcs.h NFCS_STORE_*)
STORE_AUTO, STORE_DEFERRED, STORE_SPARSE = 0, 1, 2


class NfcsError(RuntimeError):
    pass


# The first 8 kernel arguments go into SGPRs at dispatch (gfx950 kernarg preloading): the row
# kernel orders its arguments so that everything a wave reads before its frame loads is among them
# (nfcs_kernels.hip, update_rows_kernel). Round 3 A/B on one box: C3 +0.5-0.8%, 1M x 64 B +1.7%,
# flow keys +1%, C1 / C2 / the fused forward / VLAN within +-0.5% (profiles/r03_s1_ab_kernarg_preload.jsonl).
KERNARG_PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=8"]


def build(verbose: bool = False) -> str:
    """Compile the gfx950 kernels + C ABI into netflow_amd/libnfcs.so (in-tree). The measurement
    build (extra launch forms for A/B runs) is separate: tools/r04/build.sh."""
    out = os.path.join(HERE, "libnfcs.so")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17", *KERNARG_PRELOAD,
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(HERE, "csrc"), *SOURCES, "-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return out


# include/nfcs.h NFCS_ABI_VERSION: 2 = nfcs_update_host_frames, descriptors in any order for
# nfcs_update_host
ABI_VERSION = 2
_lib = None
_vp = ctypes.c_void_p
_u32 = ctypes.c_uint32
_u64 = ctypes.c_uint64
_TABLES = ("fib", "acl", "fdb", "icmp", "egress", "aclset")


def _declare(L):
    sig = {
        "nfcs_abi_version": ([], ctypes.c_int),
        "nfcs_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "nfcs_last_hip_error": ([], ctypes.c_int),
        "nfcs_ctx_create": ([ctypes.c_int, ctypes.POINTER(_vp)], ctypes.c_int),
        "nfcs_ctx_destroy": ([_vp], ctypes.c_int),
        "nfcs_ctx_stream": ([_vp], _vp),
        "nfcs_ctx_set_slot_bytes": ([_vp, ctypes.c_uint32], ctypes.c_int),
        "nfcs_ctx_launch_footprint": ([_vp, _u64, _vp, _u32, ctypes.POINTER(_u64)], ctypes.c_int),
        "nfcs_ctx_set_store_policy": ([_vp, ctypes.c_int], ctypes.c_int),
        "nfcs_ctx_store_state": ([_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_u32), ctypes.POINTER(_u32)],
                                 ctypes.c_int),
        "nfcs_update_device": ([_vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_update_host": ([_vp, _vp, _u64, _vp, _u32, _vp, _u32], ctypes.c_int),
        "nfcs_update_host_frames": ([_vp, _vp, _vp, _u32, _vp, _u32], ctypes.c_int),
        "nfcs_layout_config": ([ctypes.c_int, _u64, _u64, _u32, _u32, _vp, ctypes.POINTER(_u64)], ctypes.c_int),
        "nfcs_shard_bytes": ([_vp, _u32, _u32, _vp], ctypes.c_int),
        "nfcs_ctx_host_numa": ([_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "nfcs_gen_config_device": ([_vp, ctypes.c_int, _u64, _u64, _u32, _vp, _u64, _vp, _vp], ctypes.c_int),
        "nfcs_stale_every_device": ([_vp, _vp, _u64, _vp, _u32, _u32, _vp], ctypes.c_int),
        "nfcs_digest_device": ([_vp, _vp, _u64, _vp, _u32, _u64, ctypes.POINTER(_u64), _vp], ctypes.c_int),
        "nfcs_device_alloc": ([_vp, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
        "nfcs_device_free": ([_vp, _vp], ctypes.c_int),
        "nfcs_host_alloc": ([_vp, ctypes.c_size_t, ctypes.POINTER(_vp)], ctypes.c_int),
        "nfcs_host_free": ([_vp, _vp], ctypes.c_int),
        "nfcs_memcpy_h2d": ([_vp, _vp, _vp, ctypes.c_size_t], ctypes.c_int),
        "nfcs_memcpy_d2h": ([_vp, _vp, _vp, ctypes.c_size_t], ctypes.c_int),
        "nfcs_stream_sync": ([_vp, _vp], ctypes.c_int),
        "nfcs_time_update_device": ([_vp, _vp, _u64, _vp, _u32, _vp, ctypes.c_int, _vp,
                                     ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "nfcs_time_update_batches": ([_vp, _u32, _vp, _vp, _vp, _u32, ctypes.c_int, _vp,
                                      ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "nfcs_l3_forward_device": ([_vp, _vp, _u64, _vp, _vp, _u32, _vp, _u32, _vp, _vp],
                                   ctypes.c_int),
        "nfcs_vlan_device": ([_vp, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp],
                             ctypes.c_int),
        "nfcs_time_vlan_device": ([_vp, _vp, _u64, _vp, _u32, _u32, _u32, _u32, _vp, ctypes.c_int,
                                   _vp, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "nfcs_flow_keys_device": ([_vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_time_stream_read": ([_vp, _vp, _u64, ctypes.c_int, ctypes.c_int, _vp, _vp], ctypes.c_int),
        "nfcs_time_frames_read": ([_vp, _vp, _u64, _vp, _u32, ctypes.c_int, _vp, _vp], ctypes.c_int),
        "nfcs_time_flow_keys_device": ([_vp, _vp, _u64, _vp, _u32, _vp, _vp, ctypes.c_int, _vp,
                                        ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "nfcs_time_l3_forward_device": ([_vp, _vp, _u64, _vp, _vp, _u32, _vp, _u32, _vp,
                                         ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_float)],
                                        ctypes.c_int),
        "nfcs_fib_set_routes": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_fib_set_arp": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_fib_set_if_macs": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_fib_set_local_ips": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_fib_nexthops": ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_fib_nexthops_host": ([_vp, _vp, _u32, ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_fib_lookup_host": ([_vp, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                  ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_route_lookup_device": ([_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_acl_set_rules": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_acl_eval_host": ([_vp, _vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_acl_eval_device": ([_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_fdb_set_entries": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_fdb_set_port": ([_vp, _vp, _vp, _u32], ctypes.c_int),
        "nfcs_fdb_clear_ports": ([_vp], ctypes.c_int),
        "nfcs_fdb_stats": ([_vp] + [ctypes.POINTER(_u32)] * 4, ctypes.c_int),
        "nfcs_fdb_lookup_host": ([_vp, _u32, _vp, _u32] + [ctypes.POINTER(_u32)] * 4, ctypes.c_int),
        "nfcs_fdb_flood_ports_host": ([_vp, _u32, _u32, _u32, _vp, _u32, ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_l2_lookup_device": ([_vp, _vp, _u32, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp],
                                  ctypes.c_int),
        "nfcs_flood_expand_device": ([_vp, _vp, _u32, _u32, _vp, _u64, _u64, _u32, _vp, _u32] + [_vp] * 5 + [_u32] +
                                     [_vp] * 5, ctypes.c_int),
        "nfcs_flood_expand_host": ([_vp, _u32, _u32, _u64, _u64, _u32, _vp, _u32] + [_vp] * 5 + [_u32] + [_vp] * 4,
                                   ctypes.c_int),
        "nfcs_icmp_set_local": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_icmp_set_if_ips": ([_vp, _vp, _u32], ctypes.c_int),
        "nfcs_icmp_set_ports_up": ([_vp, _vp, _u32, _u32], ctypes.c_int),
        "nfcs_fib_resolve_host": ([_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32)],
                                  ctypes.c_int),
        "nfcs_icmp_respond_device": ([_vp, _vp, _vp, _u32, _vp, _u64, _u64, _u32, _vp, _u32, _vp, _vp, _u32] +
                                     [_vp] * 6, ctypes.c_int),
        "nfcs_icmp_respond_host": ([_vp, _vp, _u32, _vp, _u64, _u64, _u32, _vp, _u32, _vp, _vp, _u32] + [_vp] * 5,
                                   ctypes.c_int),
        "nfcs_egress_set_port": ([_vp, _vp], ctypes.c_int),
        "nfcs_egress_clear_ports": ([_vp], ctypes.c_int),
        "nfcs_egress_keys": ([_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_egress_plan_host": ([_vp, _u32, _vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32)], ctypes.c_int),
        "nfcs_egress_enqueue_host": ([_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_egress_plan_device": ([_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_egress_enqueue_device": ([_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_aclset_set_list": ([_vp, _u32, _vp, _u32], ctypes.c_int),
        "nfcs_aclset_remove_list": ([_vp, _u32], ctypes.c_int),
        "nfcs_aclset_bind_port": ([_vp, _u32, _u32], ctypes.c_int),
        "nfcs_aclset_clear": ([_vp], ctypes.c_int),
        "nfcs_aclset_info": ([_vp] + [ctypes.POINTER(_u32)] * 3, ctypes.c_int),
        "nfcs_aclset_eval_host": ([_vp, _u32, _vp, _u32] + [ctypes.POINTER(_u32)] * 3, ctypes.c_int),
        "nfcs_egress_acl_host": ([_vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_egress_acl_device": ([_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_ingress_dispatch_device": ([_vp, _vp, _u32, _u32, _vp, _u64, _vp, _u32] + [_vp] * 10, ctypes.c_int),
        "nfcs_ingress_dispatch_host": ([_vp, _u32, _u32, _vp, _u64, _vp, _u32] + [_vp] * 9, ctypes.c_int),
        "nfcs_egress_acl_items_device": ([_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _u32] + [_vp] * 6, ctypes.c_int),
        "nfcs_egress_acl_items_host": ([_vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _u32] + [_vp] * 5, ctypes.c_int),
        "nfcs_switch_rx_workspace_bytes": ([_u32, _u32], _u64),
        "nfcs_switch_rx_device": ([_vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_txq_create": ([_vp, _vp, ctypes.POINTER(_vp)], ctypes.c_int),
        "nfcs_txq_destroy": ([_vp], ctypes.c_int),
        "nfcs_txq_set_scheduler": ([_vp, _u32, _u32], ctypes.c_int),
        "nfcs_txq_reset": ([_vp], ctypes.c_int),
        "nfcs_txq_info": ([_vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u64)], ctypes.c_int),
        "nfcs_txq_state_device": ([_vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_txq_state_host": ([_vp, _vp, _vp], ctypes.c_int),
        "nfcs_txq_append_device": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp], ctypes.c_int),
        "nfcs_txq_append_host": ([_vp, _vp, _vp, _vp, _vp, _vp, _u32], ctypes.c_int),
        "nfcs_txq_dequeue_device": ([_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_txq_dequeue_host": ([_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp], ctypes.c_int),
        "nfcs_txq_closed_form_host": ([_u32, _u32, _u32, _vp, _u32, _vp, ctypes.POINTER(_u32), _vp, _u32], ctypes.c_int),
    }
    for t in _TABLES:  # the life cycle every table object shares
        sig.update({f"nfcs_{t}_create": ([ctypes.POINTER(_vp)], ctypes.c_int), f"nfcs_{t}_destroy": ([_vp], ctypes.c_int),
                    f"nfcs_{t}_commit": ([_vp], ctypes.c_int), f"nfcs_{t}_upload": ([_vp, _vp], ctypes.c_int)})
    for name, (args, res) in sig.items():
        # a measurement build of an earlier round (NFCS_LIB, A/B runs) may lack a later entry point;
        # the product library exports every one (tests/test_abi.py)
        if os.environ.get("NFCS_LIB") and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    return L


def lib() -> ctypes.CDLL:
    """Load libnfcs.so. Raises if the HIP library has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NfcsError(f"{LIB_PATH} is missing: build it with netflow_amd.build() "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = _declare(ctypes.CDLL(LIB_PATH))
        v = _lib.nfcs_abi_version()
        # a measurement build of an earlier round (NFCS_LIB) may carry an older ABI
        if v != ABI_VERSION and not (os.environ.get("NFCS_LIB") and 1 <= v < ABI_VERSION):
            raise NfcsError(f"libnfcs.so ABI {v}, this package needs {ABI_VERSION}")
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        L = lib()
        raise NfcsError(f"{what}: {L.nfcs_strerror(rc).decode()} (rc={rc}, hip={L.nfcs_last_hip_error()})")


def layout_config(config: int, seed: int, first: int, n: int, align: int = 16):
    """Descriptors of n synthetic frames of `config` (`align`-byte aligned, arena order)."""
    desc = np.zeros(n, dtype=DESC_DTYPE)
    nbytes = _u64()
    _check(lib().nfcs_layout_config(config, seed, first, n, align, desc.ctypes.data if n else None,
                                    ctypes.byref(nbytes)), "nfcs_layout_config")
    return desc, int(nbytes.value)


def shard_bytes(desc: np.ndarray, parts: int) -> np.ndarray:
    """nfcs_shard_bytes: parts + 1 packet bounds; part p = packets [b[p], b[p+1]), its frame bytes
    within one frame of total / parts (multi-GPU partition)."""
    desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
    bounds = np.zeros(parts + 1, dtype=np.uint32)
    _check(lib().nfcs_shard_bytes(desc.ctypes.data if len(desc) else None, len(desc), parts,
                                  bounds.ctypes.data), "nfcs_shard_bytes")
    return bounds


def ip4(a: str) -> int:
    """A dotted IPv4 address as the u32 the tables and frames hold: network byte order, i.e. the four
    address bytes in frame order read as one little-endian u32 (the reference's IpAddress)."""
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "little")


class _Handle:
    """One C object nfcs_<_c>_*: `ptr` until close() destroys it, once; a half-built one has no ptr."""
    _c = ""
    ptr = None

    def _call(self, fn, *args):
        """nfcs_<_c>_<fn>(ptr, *args), checked."""
        name = f"nfcs_{self._c}_{fn}"
        _check(getattr(lib(), name)(self.ptr, *args), name)
        return self

    def close(self):
        if self.ptr:
            getattr(lib(), f"nfcs_{self._c}_destroy")(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Table(_Handle):
    """A table object: setters, then commit() (compile), then upload(engine) (snapshot to its device). A
    setter invalidates the commit, not the device copy, which stays as it is until the next upload."""

    def __init__(self):
        p = _vp()
        _check(getattr(lib(), f"nfcs_{self._c}_create")(ctypes.byref(p)), f"nfcs_{self._c}_create")
        self.ptr = p.value

    def _set_array(self, fn, arr, dtype, head=(), tail=()):
        """The setters that pass one array: nfcs_<_c>_<fn>(ptr, *head, records, count, *tail)."""
        arr = np.ascontiguousarray(arr, dtype=dtype)
        return self._call(fn, *head, arr.ctypes.data if len(arr) else None, len(arr), *tail)

    def commit(self):
        return self._call("commit")

    def upload(self, engine: "Engine"):
        _check(getattr(lib(), f"nfcs_{self._c}_upload")(engine.ctx, self.ptr), f"nfcs_{self._c}_upload")
        return self


class Fib(_Table):
    """The forwarding table behind Engine.route_lookup_device (nfcs_fib): routes in lookup order (the
    first match wins: pass RoutingManager::get_routing_table() as it is), ARP entries, interface MACs
    and the switch's own addresses. Addresses are u32 in network byte order (ip4())."""
    _c = "fib"

    def set_routes(self, routes):
        """FIB_ROUTE_DTYPE records {network, mask, next_hop_ip, egress_if}, in lookup order."""
        return self._set_array("set_routes", routes, FIB_ROUTE_DTYPE)

    def set_arp(self, arp):
        """FIB_ARP_DTYPE records {ip, mac}; of duplicates the last one wins."""
        return self._set_array("set_arp", arp, FIB_ARP_DTYPE)

    def set_if_macs(self, if_macs):
        """FIB_IF_MAC_DTYPE records {egress_if, mac}."""
        return self._set_array("set_if_macs", if_macs, FIB_IF_MAC_DTYPE)

    def set_local_ips(self, ips):
        return self._set_array("set_local_ips", ips, np.dtype("<u4"))

    def upload(self, engine: "Engine"):
        """Copy the committed tables to the engine's device; close the Fib before the engine."""
        return super().upload(engine)

    def nexthops(self) -> tuple[int, int]:
        """(device pointer, entries) of the uploaded next-hop table, for l3_forward_device."""
        p, n = _vp(), _u32()
        _check(lib().nfcs_fib_nexthops(self.ptr, ctypes.byref(p), ctypes.byref(n)), "nfcs_fib_nexthops")
        return p.value or 0, int(n.value)

    def nexthops_host(self) -> np.ndarray:
        """The committed next-hop table as NEXTHOP_DTYPE records."""
        n = _u32()
        _check(lib().nfcs_fib_nexthops_host(self.ptr, None, 0, ctypes.byref(n)), "nfcs_fib_nexthops_host")
        out = np.zeros(n.value, dtype=NEXTHOP_DTYPE)
        if n.value:
            _check(lib().nfcs_fib_nexthops_host(self.ptr, out.ctypes.data, n.value, ctypes.byref(n)),
                   "nfcs_fib_nexthops_host")
        return out

    def lookup_host(self, dst_ip: int, ttl: int) -> tuple[int, int, int]:
        """(verdict, next-hop index, egress interface) for one destination and TTL, on the CPU, from
        the tables the kernel reads (nfcs_fib_lookup_host)."""
        v, h, e = _u32(), _u32(), _u32()
        _check(lib().nfcs_fib_lookup_host(self.ptr, int(dst_ip), int(ttl), ctypes.byref(v), ctypes.byref(h),
                                          ctypes.byref(e)), "nfcs_fib_lookup_host")
        return int(v.value), int(h.value), int(e.value)

    def resolve_host(self, ip: int) -> tuple[int, int, int]:
        """(verdict, next-hop index, the matching route's interface) for one address WITHOUT the is_my_ip and
        TTL steps (nfcs_fib_resolve_host): RT_FORWARD / RT_NO_ROUTE / RT_ARP_MISS / RT_NO_IF_MAC only; the
        interface is given whenever a route matches."""
        v, h, e = _u32(), _u32(), _u32()
        _check(lib().nfcs_fib_resolve_host(self.ptr, int(ip), ctypes.byref(v), ctypes.byref(h), ctypes.byref(e)),
               "nfcs_fib_resolve_host")
        return int(v.value), int(h.value), int(e.value)


class Acl(_Table):
    """One ACL rule list behind Engine.acl_eval_device (nfcs_acl): ACL_RULE_DTYPE records scanned in the
    order given, the first match decides (pass AclManager::get_all_rules(name) as it is), no match
    permits. Addresses and their masks are u32 in HOST byte order (10.1.2.3 = 0x0A010203), as AclRule
    holds them, unlike the Fib's network-order ones."""
    _c = "acl"

    def set_rules(self, rules):
        """ACL_RULE_DTYPE records, in scan order; at most ACL_MAX_RULES."""
        return self._set_array("set_rules", rules, ACL_RULE_DTYPE)

    def upload(self, engine: "Engine"):
        """Copy the committed rules to the engine's device; close the Acl before the engine."""
        return super().upload(engine)

    def eval_host(self, frame: bytes) -> tuple[int, int, int]:
        """(action, index of the deciding rule or ACL_NO_MATCH, redirect port or IF_NONE) for one frame,
        on the CPU, from the arrays the kernel reads (nfcs_acl_eval_host)."""
        a, r, p = _u32(), _u32(), _u32()
        frame = bytes(frame)
        _check(lib().nfcs_acl_eval_host(self.ptr, frame if frame else None, len(frame), ctypes.byref(a),
                                        ctypes.byref(r), ctypes.byref(p)), "nfcs_acl_eval_host")
        return int(a.value), int(r.value), int(p.value)


class AclSet(_Table):
    """The egress ACLs behind Engine.egress_acl_device (nfcs_aclset): rule lists by id (0..ACLSET_MAX_LISTS-1,
    ACL_RULE_DTYPE records as in Acl) and port -> list bindings. A port that is unbound, bound to a list that
    was never set or was removed, or bound to an empty list has no list: every frame is permitted unread.
    All non-empty lists together, each padded to ACL_GROUP, hold at most ACL_MAX_RULES rules (commit)."""
    _c = "aclset"

    def set_list(self, list_id: int, rules):
        """Replace list list_id; no rules is an existing, empty list."""
        return self._set_array("set_list", rules, ACL_RULE_DTYPE, head=(int(list_id),))

    def remove_list(self, list_id: int):
        """AclManager::delete_acl: bindings to the list stay and read "no list"."""
        return self._call("remove_list", int(list_id))

    def bind_port(self, port_id: int, list_id: int):
        """apply_acl_to_interface(port, list, EGRESS); ACL_LIST_NONE unbinds."""
        return self._call("bind_port", int(port_id), int(list_id))

    def clear(self):
        return self._call("clear")

    def upload(self, engine: "Engine"):
        """Copy the committed arrays to the engine's device; close the AclSet before the engine."""
        return super().upload(engine)

    def info(self) -> tuple[int, int, int]:
        """(ports = highest bound port id + 1, lists laid out, their padded rule total)."""
        a, b, c = _u32(), _u32(), _u32()
        _check(lib().nfcs_aclset_info(self.ptr, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "nfcs_aclset_info")
        return int(a.value), int(b.value), int(c.value)

    def eval_host(self, port: int, frame: bytes) -> tuple[int, int, int]:
        """(action, index of the deciding rule inside the port's list or ACL_NO_MATCH, redirect port or
        IF_NONE) for one frame leaving through port, on the CPU (nfcs_aclset_eval_host)."""
        a, r, p = _u32(), _u32(), _u32()
        frame = bytes(frame)
        _check(lib().nfcs_aclset_eval_host(self.ptr, int(port), frame if frame else None, len(frame), ctypes.byref(a),
                                           ctypes.byref(r), ctypes.byref(p)), "nfcs_aclset_eval_host")
        return int(a.value), int(r.value), int(p.value)

    def egress_acl_host(self, arena, desc, port, denied_pkts=None, denied_bytes=None) -> dict:
        """nfcs_egress_acl_host over host arrays: returns port (a copy, IF_NONE stored where the packet is
        denied or its descriptor is bad), action (u8), rule and redirect (u32). denied_pkts (`ports` u32) and
        denied_bytes (`ports` u64), both or neither, are updated in place."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        port = np.array(port, dtype=np.uint32)
        n = len(desc)
        assert len(port) == n
        for a, dt in ((denied_pkts, np.uint32), (denied_bytes, np.uint64)):
            assert a is None or (a.dtype == dt and a.flags.c_contiguous and a.flags.writeable)
        action = np.zeros(n, np.uint8)
        rule = np.zeros(n, np.uint32)
        redirect = np.zeros(n, np.uint32)
        cp = lambda a: None if a is None else a.ctypes.data
        _check(lib().nfcs_egress_acl_host(self.ptr, arena.ctypes.data, arena.nbytes, desc.ctypes.data, n,
                                          port.ctypes.data, action.ctypes.data, rule.ctypes.data, redirect.ctypes.data,
                                          cp(denied_pkts), cp(denied_bytes)), "nfcs_egress_acl_host")
        return {"port": port, "action": action, "rule": rule, "redirect": redirect}

    def egress_acl_items_host(self, arena, desc, port, item_src=None, bypass=None, denied_pkts=None,
                              denied_bytes=None) -> dict:
        """nfcs_egress_acl_items_host: egress_acl_host over an item list whose items of redirected frames bypass
        the ACL. item_src (n u32, flood_expand's) and bypass (one byte per source frame, ingress_dispatch's), both
        or neither: an item with a port whose source frame is marked keeps its port, is not read or counted and
        reads ACL_BYPASS. Without them it is egress_acl_host."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        port = np.array(port, dtype=np.uint32)
        n = len(desc)
        assert len(port) == n
        item_src = None if item_src is None else np.ascontiguousarray(item_src, dtype=np.uint32)
        bypass = None if bypass is None else np.ascontiguousarray(bypass, dtype=np.uint8)
        assert item_src is None or len(item_src) == n
        for a, dt in ((denied_pkts, np.uint32), (denied_bytes, np.uint64)):
            assert a is None or (a.dtype == dt and a.flags.c_contiguous and a.flags.writeable)
        action, rule, redirect = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        scratch = np.zeros(1, np.uint64)  # an array that was given stays given when it is empty
        cp = lambda a: None if a is None else (a.ctypes.data if a.size else scratch.ctypes.data)
        _check(lib().nfcs_egress_acl_items_host(self.ptr, arena.ctypes.data, arena.nbytes, desc.ctypes.data, n,
                                                port.ctypes.data, cp(item_src), cp(bypass),
                                                0 if bypass is None else len(bypass), action.ctypes.data,
                                                rule.ctypes.data, redirect.ctypes.data, cp(denied_pkts),
                                                cp(denied_bytes)), "nfcs_egress_acl_items_host")
        return {"port": port, "action": action, "rule": rule, "redirect": redirect}


class Fdb(_Table):
    """The L2 forwarding database and port state behind Engine.l2_lookup_device (nfcs_fdb): FDB_ENTRY_DTYPE
    records (pass ForwardingDatabase::get_all_entries() as it is; of two with one (mac, vlan_id) the first
    wins), compiled into an open-addressing hash table, and one L2_PORT_DTYPE record plus allowed VLANs per
    port. A port never set is link down, STP unknown, without a VLAN config."""
    _c = "fdb"

    def set_entries(self, entries):
        """FDB_ENTRY_DTYPE records; at most FDB_MAX_ENTRIES."""
        return self._set_array("set_entries", entries, FDB_ENTRY_DTYPE)

    def set_port(self, port_id: int, link_up=True, stp_forwarding=True, has_vlan_config=True, type=L2_ACCESS,
                 native_vlan: int = 1, allowed_vlans=()):
        """One port's state (nfcs_l2_port) and, for L2_TRUNK / L2_HYBRID, its allowed VLANs."""
        rec = np.zeros(1, dtype=L2_PORT_DTYPE)
        rec["port_id"], rec["link_up"], rec["stp_forwarding"] = port_id, bool(link_up), bool(stp_forwarding)
        rec["has_vlan_config"], rec["type"], rec["native_vlan"] = bool(has_vlan_config), type, native_vlan
        return self._set_array("set_port", list(allowed_vlans), np.uint16, head=(rec.ctypes.data,))

    def clear_ports(self):
        return self._call("clear_ports")

    def upload(self, engine: "Engine"):
        """Copy the committed tables to the engine's device; close the Fdb before the engine."""
        return super().upload(engine)

    def stats(self) -> dict:
        """The committed table: entries (distinct keys), slots, max_probe (longest displacement + 1) and
        wrapped (entries whose probe sequence crossed from the last slot to slot 0)."""
        v = [_u32() for _ in range(4)]
        _check(lib().nfcs_fdb_stats(self.ptr, *(ctypes.byref(x) for x in v)), "nfcs_fdb_stats")
        return dict(zip(("entries", "slots", "max_probe", "wrapped"), (int(x.value) for x in v)))

    def lookup_host(self, ingress_port: int, frame: bytes) -> tuple[int, int, int, int]:
        """(verdict L2_*, egress port or IF_NONE, VLAN used for the lookup, learn class L2_LEARN_*) for one
        frame received on ingress_port, on the CPU, from the arrays the kernel reads."""
        v = [_u32() for _ in range(4)]
        frame = bytes(frame)
        _check(lib().nfcs_fdb_lookup_host(self.ptr, int(ingress_port), frame if frame else None, len(frame),
                                          *(ctypes.byref(x) for x in v)), "nfcs_fdb_lookup_host")
        return tuple(int(x.value) for x in v)

    def flood_ports_host(self, ingress_port: int, vlan: int, num_ports: int) -> np.ndarray:
        """flood_packet's port list for a frame received on ingress_port on `vlan`, ascending."""
        n = _u32()
        out = np.zeros(max(num_ports, 1), dtype=np.uint32)
        _check(lib().nfcs_fdb_flood_ports_host(self.ptr, int(ingress_port), int(vlan), int(num_ports), out.ctypes.data,
                                               len(out), ctypes.byref(n)), "nfcs_fdb_flood_ports_host")
        return out[:n.value].copy()

    def flood_expand_host(self, ingress_port: int, num_ports: int, arena_bytes: int, copy_base: int, copy_align: int,
                          desc, cap: int, l3_port=None, fwd_status=None, l2_port=None, l2_verdict=None,
                          l2_vlan=None) -> dict:
        """The sequential walk behind Engine.flood_expand_device, on the CPU: the burst's egress work items in
        the reference's processing order, flood copies laid out from copy_base in slots of
        round_up(len, copy_align). Returns item_desc (cap DESC_DTYPE), item_port and item_src (cap u32 each; the
        entries past totals["items"] are inert: {0, 0}, IF_NONE, ITEM_NONE) and totals (one
        FLOOD_TOTALS_DTYPE record). No frame byte is moved."""
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        n = len(desc)
        arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        l3_port, l2_port = arr(l3_port, np.uint32), arr(l2_port, np.uint32)
        fwd_status, l2_verdict, l2_vlan = arr(fwd_status, np.uint8), arr(l2_verdict, np.uint8), arr(l2_vlan, np.uint16)
        for a in (l3_port, l2_port, fwd_status, l2_verdict, l2_vlan):
            if a is not None and len(a) != n:
                raise NfcsError("flood_expand_host: every per-packet array needs n entries")
        item_desc, item_port = np.zeros(cap, DESC_DTYPE), np.zeros(cap, np.uint32)
        item_src, totals = np.zeros(cap, np.uint32), np.zeros(1, FLOOD_TOTALS_DTYPE)
        dp = lambda a: a.ctypes.data if a is not None and len(a) else None
        # an array that was given stays given when n is 0: which arrays are given is part of the call
        given = lambda a: None if a is None else (a.ctypes.data if len(a) else totals.ctypes.data)
        _check(lib().nfcs_flood_expand_host(self.ptr, int(ingress_port), int(num_ports), int(arena_bytes),
                                            int(copy_base), int(copy_align), dp(desc), n, given(l3_port),
                                            given(fwd_status), given(l2_port), given(l2_verdict), given(l2_vlan),
                                            int(cap), dp(item_desc), dp(item_port), dp(item_src), totals.ctypes.data),
               "nfcs_flood_expand_host")
        return {"item_desc": item_desc, "item_port": item_port, "item_src": item_src, "totals": totals[0]}

    def ingress_dispatch_host(self, ingress_port: int, num_ports: int, arena, arena_bytes: int, desc, rt_verdict, nh,
                              l2_port, l2_verdict, action=None, redirect=None, rx_stats=None, want_class: bool = True,
                              want_bypass: bool = True) -> dict:
        """The sequential walk behind Engine.ingress_dispatch_device, on the CPU (nfcs_ingress_dispatch_host): what
        process_received_packet does between the stages for one RX burst of ingress_port. action / redirect (the
        ingress ACL's; None: no list, every frame permitted), rt_verdict, and nh / l2_port / l2_verdict as the
        route lookup, the ACL and the L2 lookup left them. Returns copies of nh, l2_port and l2_verdict with the
        masks applied, cls (n bytes SW_*) and bypass (n bytes; None where not wanted). rx_stats (RX_STATS_DTYPE
        records indexed by port) is updated in place."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        n = len(desc)
        arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        action, redirect, rt_verdict = arr(action, np.uint8), arr(redirect, np.uint32), arr(rt_verdict, np.uint8)
        nh, l2_port, l2_verdict = np.array(nh, np.uint32), np.array(l2_port, np.uint32), np.array(l2_verdict, np.uint8)
        if any(a is not None and len(a) != n for a in (action, redirect, rt_verdict, nh, l2_port, l2_verdict)):
            raise NfcsError("ingress_dispatch_host: every per-packet array needs n entries")
        assert rx_stats is None or (rx_stats.dtype == RX_STATS_DTYPE and rx_stats.flags.c_contiguous and
                                    rx_stats.flags.writeable and len(rx_stats) > ingress_port)
        cls = np.zeros(n, np.uint8) if want_class else None
        bypass = np.zeros(n, np.uint8) if want_bypass else None
        scratch = np.zeros(1, np.uint64)  # an array that was given stays given when n is 0
        dp = lambda a: None if a is None else (a.ctypes.data if a.size else scratch.ctypes.data)
        _check(lib().nfcs_ingress_dispatch_host(self.ptr, int(ingress_port), int(num_ports), dp(arena), int(arena_bytes),
                                                dp(desc), n, dp(action), dp(redirect), dp(rt_verdict), dp(nh), dp(l2_port),
                                                dp(l2_verdict), dp(cls), dp(bypass), dp(rx_stats)),
               "nfcs_ingress_dispatch_host")
        return {"nh": nh, "l2_port": l2_port, "l2_verdict": l2_verdict, "cls": cls, "bypass": bypass}


class Icmp(_Table):
    """The tables behind Engine.icmp_respond_device (nfcs_icmp): the switch's own addresses with their MACs
    (get_mac_for_ip), each interface's first address (get_interface_ip) and the ports that are up
    (send_control_plane_packet's test). Addresses are u32 in network byte order, as in Fib; of duplicates the
    first wins. Routes, ARP and interface MACs come from the Fib given to the call."""
    _c = "icmp"

    def set_local(self, local):
        """ICMP_LOCAL_DTYPE records {ip, mac}."""
        return self._set_array("set_local", local, ICMP_LOCAL_DTYPE)

    def set_if_ips(self, if_ips):
        """ICMP_IF_IP_DTYPE records {egress_if, ip}."""
        return self._set_array("set_if_ips", if_ips, ICMP_IF_IP_DTYPE)

    def set_ports_up(self, ports, num_ports: int):
        """The ports below num_ports whose link is up."""
        return self._set_array("set_ports_up", ports, np.uint32, tail=(int(num_ports),))

    def upload(self, engine: "Engine"):
        """Copy the committed tables to the engine's device; close the Icmp before the engine."""
        return super().upload(engine)

    def respond_host(self, fib: "Fib", ingress_port: int, arena, msg_base: int, msg_align: int, desc, rt_verdict,
                     cap: int, ip_id=None) -> dict:
        """The sequential walk behind Engine.icmp_respond_device, on the CPU (nfcs_icmp_respond_host): builds
        the burst's echo replies and TTL / unreachable errors into arena[msg_base:] IN PLACE (arena: a writable
        contiguous uint8 array) and returns msg_desc (cap DESC_DTYPE), msg_port and msg_src (cap u32 each; the
        entries past totals["messages"] are inert), status (n bytes ICMP_ST_*) and totals (one
        ICMP_TOTALS_DTYPE record)."""
        assert arena.dtype == np.uint8 and arena.flags.c_contiguous and arena.flags.writeable
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        n = len(desc)
        rt_verdict = np.ascontiguousarray(rt_verdict, dtype=np.uint8)
        ip_id = None if ip_id is None else np.ascontiguousarray(ip_id, dtype=np.uint16)
        if len(rt_verdict) != n or (ip_id is not None and len(ip_id) != n):
            raise NfcsError("respond_host: every per-packet array needs n entries")
        msg_desc, msg_port = np.zeros(cap, DESC_DTYPE), np.zeros(cap, np.uint32)
        msg_src, totals = np.zeros(cap, np.uint32), np.zeros(1, ICMP_TOTALS_DTYPE)
        status = np.zeros(n, np.uint8)
        dp = lambda a: a.ctypes.data if a is not None and len(a) else None
        _check(lib().nfcs_icmp_respond_host(self.ptr, fib.ptr, int(ingress_port), arena.ctypes.data, arena.nbytes,
                                            int(msg_base), int(msg_align), dp(desc), n, dp(rt_verdict), dp(ip_id),
                                            int(cap), dp(msg_desc), dp(msg_port), dp(msg_src), dp(status),
                                            totals.ctypes.data), "nfcs_icmp_respond_host")
        return {"msg_desc": msg_desc, "msg_port": msg_port, "msg_src": msg_src, "status": status, "totals": totals[0]}


class Egress(_Table):
    """The egress ports behind Engine.egress_plan_device / egress_enqueue_device (nfcs_egress): one
    EGRESS_PORT_DTYPE record per port, holding what VlanManager::process_egress and QosManager::enqueue_packet
    read of it. A port never set has no VLAN config and no QoS config. The (port, queue) pair is the key
    port * QOS_MAX_QUEUES + queue."""
    _c = "egress"

    def set_port(self, port_id: int, has_vlan_config=True, type=L2_ACCESS, tag_native=False, native_vlan: int = 1,
                 has_qos=True, num_queues: int = 4, max_queue_depth: int = 1000):
        """One port (nfcs_egress_port); the same id again replaces it. num_queues 0 and max_queue_depth 0 are
        each read as 1, as QosConfig::validate_and_prepare does."""
        rec = np.zeros(1, dtype=EGRESS_PORT_DTYPE)
        for name, v in (("port_id", port_id), ("type", type), ("native_vlan", native_vlan),
                        ("num_queues", num_queues), ("max_queue_depth", max_queue_depth)):
            if not 0 <= int(v) <= np.iinfo(EGRESS_PORT_DTYPE[name]).max:
                raise NfcsError(f"nfcs_egress_set_port: {name} = {v} does not fit its field")
            rec[name] = int(v)
        rec["has_vlan_config"], rec["tag_native"], rec["has_qos"] = bool(has_vlan_config), bool(tag_native), bool(has_qos)
        return self._call("set_port", rec.ctypes.data)

    def clear_ports(self):
        return self._call("clear_ports")

    def upload(self, engine: "Engine"):
        """Copy the committed records to the engine's device; close the Egress before the engine."""
        return super().upload(engine)

    def keys(self) -> tuple[int, int]:
        """(ports, keys) of the committed table: keys = ports * QOS_MAX_QUEUES."""
        a, b = _u32(), _u32()
        _check(lib().nfcs_egress_keys(self.ptr, ctypes.byref(a), ctypes.byref(b)), "nfcs_egress_keys")
        return int(a.value), int(b.value)

    def plan_host(self, port: int, frame: bytes) -> tuple[int, int]:
        """(VLAN_POP or VLAN_NOP, queue) for one frame leaving through `port`, on the CPU, from the records
        the kernel reads; (VLAN_NOP, QUEUE_NONE) for IF_NONE."""
        op, q = _u32(), _u32()
        frame = bytes(frame)
        _check(lib().nfcs_egress_plan_host(self.ptr, int(port), frame if frame else None, len(frame), ctypes.byref(op),
                                           ctypes.byref(q)), "nfcs_egress_plan_host")
        return int(op.value), int(q.value)

    def enqueue_host(self, port, queue, depth) -> dict:
        """enqueue_packet over a burst in order, on the CPU: port (n u32) and queue (n bytes) per packet,
        depth (keys u32) each queue's depth before. Returns depth (after), result (n bytes EQ_*), order (the
        enqueued packets' indexes grouped by key, arrival order within), key_start (keys + 1) and
        key_dropped (keys)."""
        port = np.ascontiguousarray(port, dtype=np.uint32)
        queue = np.ascontiguousarray(queue, dtype=np.uint8)
        n, keys = len(port), self.keys()[1]
        if len(queue) != n or len(depth) != keys:
            raise NfcsError("enqueue_host: port and queue need n entries each, depth one per key")
        depth = np.array(depth, dtype=np.uint32)
        result, order = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        key_start, key_dropped = np.zeros(keys + 1, np.uint32), np.zeros(keys, np.uint32)
        dp = lambda a: a.ctypes.data if len(a) else None
        _check(lib().nfcs_egress_enqueue_host(self.ptr, dp(port), dp(queue), n, dp(depth), dp(result), dp(order),
                                              key_start.ctypes.data, dp(key_dropped)), "nfcs_egress_enqueue_host")
        return {"depth": depth, "result": result, "order": order[:int(key_start[keys])], "key_start": key_start,
                "key_dropped": key_dropped}


class TxQueues(_Handle):
    """The TX queues of a committed Egress (nfcs_txq): one ring of 64-bit handles per (port, queue) and the
    scheduler of QosManager::select_packet_to_dequeue. With an engine it holds a device copy beside the host
    copy (Engine.txq_append_device / txq_dequeue_device advance it); without one it is host-only. It
    snapshots the Egress at creation; close it before the engine."""
    _c = "txq"

    def __init__(self, egress: "Egress", engine: "Engine | None" = None):
        p = _vp()
        _check(lib().nfcs_txq_create(engine.ctx if engine is not None else None, egress.ptr, ctypes.byref(p)),
               "nfcs_txq_create")
        self.ptr = p.value
        self.ports, self.keys, self.ring_slots = self.info()

    def set_scheduler(self, port_id: int, sched: int):
        """QosConfig::scheduler of one port (SCHED_*; default SCHED_STRICT_PRIORITY), on both copies."""
        if not (0 <= int(port_id) <= 0xFFFFFFFF and 0 <= int(sched) <= 0xFFFFFFFF):
            raise NfcsError("nfcs_txq_set_scheduler: invalid argument")
        return self._call("set_scheduler", int(port_id), int(sched))

    def reset(self):
        """Heads and last-serviced queues to 0 on both copies (configure_port_qos)."""
        return self._call("reset")

    def info(self) -> tuple[int, int, int]:
        """(ports, keys, ring_slots)."""
        a, b, c = _u32(), _u32(), _u64()
        _check(lib().nfcs_txq_info(self.ptr, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "nfcs_txq_info")
        return int(a.value), int(b.value), int(c.value)

    def _state(self, fn, what, *extra):
        head, last = np.zeros(self.keys, np.uint32), np.zeros(self.ports, np.uint8)
        dp = lambda a: a.ctypes.data if len(a) else None
        _check(fn(self.ptr, dp(head), dp(last), *extra), what)
        return head, last

    def state_host(self) -> tuple[np.ndarray, np.ndarray]:
        """(head per key, last-serviced queue per port) of the host copy."""
        return self._state(lib().nfcs_txq_state_host, "nfcs_txq_state_host")

    def state_device(self, stream=None) -> tuple[np.ndarray, np.ndarray]:
        """The same of the device copy, after waiting for the stream."""
        return self._state(lib().nfcs_txq_state_device, "nfcs_txq_state_device", stream)

    def append_host(self, order, key_start, depth, n: int, handle=None, desc=None):
        """enqueue_packet's emplace_back for a burst of n packets on the host copy: order / key_start /
        depth as enqueue_host left them; handle (n u64) or desc (n DESC_DTYPE) names the packets."""
        order = np.ascontiguousarray(order, dtype=np.uint32)
        key_start = np.ascontiguousarray(key_start, dtype=np.uint32)
        depth = np.ascontiguousarray(depth, dtype=np.uint32)
        if len(key_start) != self.keys + 1 or len(depth) != self.keys or len(order) < int(key_start[-1]):
            raise NfcsError("append_host: key_start needs keys + 1 entries, depth keys, order key_start[keys]")
        if handle is not None:
            handle = np.ascontiguousarray(handle, dtype=np.uint64)
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        if any(a is not None and len(a) < n for a in (handle, desc)):
            raise NfcsError("append_host: handle / desc need n entries")
        dp = lambda a: a.ctypes.data if a is not None and len(a) else None
        _check(lib().nfcs_txq_append_host(self.ptr, dp(order), key_start.ctypes.data, dp(depth), dp(handle), dp(desc),
                                          int(n)), "nfcs_txq_append_host")
        return self

    def dequeue_host(self, depth, tx_cap: int, budget=None, budget_all: int = 0) -> dict:
        """The sequential dequeue on the host copy: up to budget[port] (or budget_all) select_packet_to_dequeue
        calls per port, ports ascending, at most tx_cap handles. Returns depth (after), tx (the handles
        dequeued, port-major in dequeue order), tx_queue, tx_start (ports + 1) and dequeued (per key)."""
        depth = np.array(depth, dtype=np.uint32)
        if len(depth) != self.keys:
            raise NfcsError("dequeue_host: depth needs one entry per key")
        if budget is not None:
            budget = np.ascontiguousarray(budget, dtype=np.uint32)
            if len(budget) != self.ports:
                raise NfcsError("dequeue_host: budget needs one entry per port")
        tx, tx_queue = np.zeros(tx_cap, np.uint64), np.zeros(tx_cap, np.uint8)
        tx_start, dequeued = np.zeros(self.ports + 1, np.uint32), np.zeros(self.keys, np.uint32)
        dp = lambda a: a.ctypes.data if a is not None and len(a) else None
        _check(lib().nfcs_txq_dequeue_host(self.ptr, dp(budget), int(budget_all), dp(depth), dp(tx), int(tx_cap),
                                           dp(tx_queue), tx_start.ctypes.data, dp(dequeued)), "nfcs_txq_dequeue_host")
        total = int(tx_start[self.ports])
        return {"depth": depth, "tx": tx[:total], "tx_queue": tx_queue[:total], "tx_start": tx_start,
                "dequeued": dequeued}


def txq_closed_form_host(sched: int, depth, last: int, budget: int, want_seq: bool = True):
    """The closed form of the dequeue for one port (nfcs_txq_closed_form_host): (take per queue, new
    last-serviced queue, the queue of each select_packet_to_dequeue call in order, or None without want_seq)."""
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    nq = len(depth)
    take, new_last = np.zeros(nq, np.uint32), _u32()
    cap = int(min(int(depth.sum(dtype=np.uint64)), budget)) if want_seq else 0
    seq = np.full(cap, QUEUE_NONE, np.uint8)
    _check(lib().nfcs_txq_closed_form_host(int(sched), nq, int(last), depth.ctypes.data if nq else None, int(budget),
                                           take.ctypes.data if nq else None, ctypes.byref(new_last),
                                           seq.ctypes.data if cap else None, cap), "nfcs_txq_closed_form_host")
    return take, int(new_last.value), seq if want_seq else None


class _SwitchTables(ctypes.Structure):  # nfcs_switch_tables
    _fields_ = [(k, _vp) for k in ("fib", "ingress_acl", "fdb", "egress", "aclset", "txq")]


class _SwitchRxIo(ctypes.Structure):  # nfcs_switch_rx_io
    _fields_ = ([("d_arena", _vp), ("arena_bytes", _u64), ("copy_base", _u64)] +
                [(k, _u32) for k in ("copy_align", "n", "cap", "ingress_port", "num_ports")] +
                [(k, _vp) for k in ("d_desc", "d_depth", "d_denied_pkts", "d_denied_bytes", "d_rx_stats", "d_item_desc",
                                    "d_item_port", "d_item_src", "d_totals", "d_order", "d_key_start", "d_key_dropped",
                                    "d_class")] +
                [("handle_base", _u64), ("d_workspace", _vp), ("workspace_bytes", _u64)])


def switch_rx_workspace_bytes(n: int, cap: int) -> int:
    """nfcs_switch_rx_workspace_bytes: the device workspace one Engine.switch_rx_device call over n frames and
    cap items needs."""
    return int(lib().nfcs_switch_rx_workspace_bytes(int(n), int(cap)))


class DeviceBuffer:
    """A raw device allocation owned by an Engine (no torch types involved)."""

    def __init__(self, engine: "Engine", nbytes: int):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = _vp()
        _check(lib().nfcs_device_alloc(engine.ctx, max(self.nbytes, 16), ctypes.byref(p)), "device_alloc")
        self.ptr = p.value

    def upload(self, a: np.ndarray, offset: int = 0):
        """Copy `a` into the buffer at byte `offset`."""
        a = np.ascontiguousarray(a)
        if offset < 0 or offset + a.nbytes > self.nbytes:
            raise NfcsError(f"upload of {a.nbytes} B at {offset} past a {self.nbytes}-byte buffer")
        if a.nbytes:
            _check(lib().nfcs_memcpy_h2d(self.engine.ctx, self.ptr + offset, a.ctypes.data, a.nbytes), "h2d")
        return self

    def download(self, dtype=np.uint8, count: int | None = None, offset: int = 0) -> np.ndarray:
        """`count` items of `dtype` from byte `offset` (default: the rest of the buffer)."""
        dtype = np.dtype(dtype)
        count = (self.nbytes - offset) // dtype.itemsize if count is None else count
        if offset < 0 or offset + count * dtype.itemsize > self.nbytes:
            raise NfcsError(f"download of {count} x {dtype} at {offset} past a {self.nbytes}-byte buffer")
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            _check(lib().nfcs_memcpy_d2h(self.engine.ctx, out.ctypes.data, self.ptr + offset, out.nbytes), "d2h")
        return out

    def free(self):
        if self.ptr:
            lib().nfcs_device_free(self.engine.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One nfcs context on one device (nfcs_ctx_create)."""

    def __init__(self, device: int = 0):
        self.device = device
        self._pinned = {}  # address -> size of the host_array() allocations still held
        c = _vp()
        _check(lib().nfcs_ctx_create(device, ctypes.byref(c)), f"nfcs_ctx_create({device})")
        self.ctx = c.value

    def close(self):
        if getattr(self, "ctx", None):
            for p in list(self._pinned):
                lib().nfcs_host_free(self.ctx, p)
            self._pinned.clear()
            lib().nfcs_ctx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self) -> int:
        return lib().nfcs_ctx_stream(self.ctx)

    def set_slot_bytes(self, nbytes: int):
        """Launch-shape hint for the device-path calls that follow (nfcs_ctx_set_slot_bytes): the
        mean arena bytes per frame of bursts that fill only part of their arena; 0 = arena_bytes / n."""
        _check(lib().nfcs_ctx_set_slot_bytes(self.ctx, int(nbytes)), "set_slot_bytes")

    def launch_footprint(self, arena_bytes: int, desc, n: int) -> int:
        """The mean footprint per packet the next device call over this burst picks its launch
        shape from (nfcs_ctx_launch_footprint; speed only)."""
        m = _u64()
        p = desc.ptr if isinstance(desc, DeviceBuffer) else int(desc)
        _check(lib().nfcs_ctx_launch_footprint(self.ctx, arena_bytes, p, n, ctypes.byref(m)), "launch_footprint")
        return int(m.value)

    def set_store_policy(self, policy: int):
        """The form of large long-frame device updates (nfcs_ctx_set_store_policy): STORE_AUTO (the default:
        by the store demand of the last calls), STORE_DEFERRED or STORE_SPARSE. Speed only."""
        _check(lib().nfcs_ctx_set_store_policy(self.ctx, int(policy)), "set_store_policy")

    def store_state(self) -> tuple[int, int, int]:
        """(form the newest device update ran in: STORE_DEFERRED, STORE_SPARSE or 0; packets sampled; packets of
        them that needed a store) of the newest delivered observation (nfcs_ctx_store_state)."""
        form, sampled, storing = ctypes.c_int(), _u32(), _u32()
        _check(lib().nfcs_ctx_store_state(self.ctx, ctypes.byref(form), ctypes.byref(sampled), ctypes.byref(storing)),
               "store_state")
        return form.value, int(sampled.value), int(storing.value)

    def host_numa(self) -> tuple[int, bool]:
        """(NUMA node of this GPU or -1, whether the host staging ring is bound to it)."""
        node, local = ctypes.c_int(), ctypes.c_int()
        _check(lib().nfcs_ctx_host_numa(self.ctx, ctypes.byref(node), ctypes.byref(local)), "host_numa")
        return node.value, bool(local.value)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def host_array(self, nbytes: int) -> np.ndarray:
        """A pinned host uint8 array (nfcs_host_alloc). Release it with host_free(); whatever is
        still held when the engine closes is freed then (do not use such arrays afterwards)."""
        p = _vp()
        size = max(int(nbytes), 16)
        _check(lib().nfcs_host_alloc(self.ctx, size, ctypes.byref(p)), "host_alloc")
        self._pinned[p.value] = size
        return np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(p.value))[:nbytes]

    def host_free(self, arr: np.ndarray):
        """Free a host_array() allocation now (the array must not be used afterwards)."""
        p = arr.__array_interface__["data"][0]
        if self._pinned.pop(p, None) is None:
            raise NfcsError("host_free: not a live host_array of this engine")
        _check(lib().nfcs_host_free(self.ctx, p), "host_free")

    def sync(self, stream=None):
        _check(lib().nfcs_stream_sync(self.ctx, stream), "stream_sync")

    # ---- the hot path -------------------------------------------------------------------
    def update_device(self, arena: DeviceBuffer | int, arena_bytes: int, desc: DeviceBuffer | int,
                      n: int, status=None, patch=None, stream=None):
        """Batched update_checksums() on device-resident frames (async on `stream`)."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_update_device(self.ctx, ptr(arena), arena_bytes, ptr(desc), n,
                                        ptr(status), ptr(patch), stream), "nfcs_update_device")

    def update_host(self, arena: np.ndarray, desc: np.ndarray, want_status: bool = True,
                    mode: str = "patch") -> np.ndarray | None:
        """Batched update_checksums() on host frames (in place); returns status bytes.
        mode: "patch" (default: frames H2D, patch records back), "frames" (whole frames back),
        "zero_copy" (pinned arena from host_array(): the kernel reads it over PCIe in place)."""
        flags = {"patch": 0, "frames": HOST_FRAMES, "zero_copy": HOST_ZERO_COPY}[mode]
        assert arena.dtype == np.uint8 and arena.flags.c_contiguous
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        n = len(desc)
        status = np.zeros(n, dtype=np.uint8) if want_status else None
        _check(lib().nfcs_update_host(self.ctx, arena.ctypes.data, arena.nbytes,
                                      desc.ctypes.data if n else None, n,
                                      status.ctypes.data if want_status and n else None,
                                      flags), "nfcs_update_host")
        return status

    def update_host_frames(self, buf: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                           want_status: bool = True) -> np.ndarray | None:
        """Batched update_checksums() on n frames scattered in host memory (nfcs_update_host_frames):
        frame i is buf[offsets[i] : offsets[i] + lens[i]] (any byte offset, any order; offsets[i] < 0
        passes a NULL frame), updated in place; returns status bytes."""
        assert buf.dtype == np.uint8 and buf.flags.c_contiguous
        offsets = np.asarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = len(lens)
        assert len(offsets) == n and (n == 0 or int((offsets + lens.astype(np.int64)).max()) <= buf.nbytes)
        ptrs = np.where(offsets < 0, 0, np.uint64(buf.ctypes.data) + offsets.astype(np.uint64)).astype(np.uint64)
        status = np.zeros(n, dtype=np.uint8) if want_status else None
        _check(lib().nfcs_update_host_frames(self.ctx, ptrs.ctypes.data if n else None,
                                             lens.ctypes.data if n else None, n,
                                             status.ctypes.data if want_status and n else None, 0),
               "nfcs_update_host_frames")
        return status

    def l3_forward_device(self, arena, arena_bytes: int, desc, nh, n: int, table, table_n: int,
                          status=None, stream=None):
        """Fused transit-IPv4 forward (TTL--, MAC rewrite, update_checksums) on device frames;
        nh = n u32 next-hop indexes, table = table_n nfcs_nexthop records (12 bytes each)."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_l3_forward_device(self.ctx, ptr(arena), arena_bytes, ptr(desc), ptr(nh), n,
                                            ptr(table), table_n, ptr(status), stream),
               "nfcs_l3_forward_device")

    def route_lookup_device(self, fib: Fib, arena, arena_bytes: int, desc, n: int, nh, egress_if=None,
                            verdict=None, stream=None):
        """The switch's L3 decision per frame (is_my_ip, TTL, route, ARP, interface MAC) on device
        frames, read-only: nh = n u32 next-hop indexes into fib.nexthops() (NH_NONE unless the verdict
        is RT_FORWARD), ready for l3_forward_device; egress_if (n u32) and verdict (n bytes RT_*) optional."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_route_lookup_device(self.ctx, fib.ptr, ptr(arena), arena_bytes, ptr(desc), n, ptr(nh),
                                              ptr(egress_if), ptr(verdict), stream), "nfcs_route_lookup_device")

    def acl_eval_device(self, acl: Acl, arena, arena_bytes: int, desc, n: int, action, rule=None, redirect=None,
                        nh=None, stream=None):
        """AclManager::evaluate per frame on device frames, read-only: action = n bytes ACL_*; rule (n u32:
        the deciding rule's index or ACL_NO_MATCH), redirect (n u32: the REDIRECT port or IF_NONE) and nh
        (n u32, in/out: NH_NONE stored where the action is not ACL_PERMIT, the rest untouched) optional.
        Between route_lookup_device and l3_forward_device with their nh it is the ingress ACL."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_acl_eval_device(self.ctx, acl.ptr, ptr(arena), arena_bytes, ptr(desc), n, ptr(action),
                                          ptr(rule), ptr(redirect), ptr(nh), stream), "nfcs_acl_eval_device")

    def l2_lookup_device(self, fdb: "Fdb", ingress_port: int, arena, arena_bytes: int, desc, n: int, egress_port,
                         rt_verdict=None, verdict=None, vlan=None, learn=None, stream=None):
        """The switch's L2 decision per frame received on ingress_port (FDB lookup, same-port / link / STP /
        VLAN checks, flood on a miss) on device frames, read-only: egress_port = n u32 (the port for
        L2_FORWARD, else IF_NONE); rt_verdict (n bytes RT_* of route_lookup_device on the same burst: only
        RT_NOT_IPV4 frames are decided, the rest read L2_SKIP), verdict (n bytes L2_*), vlan (n u16: the
        VLAN used for the lookup) and learn (n bytes L2_LEARN_*; None skips the source probe) optional."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_l2_lookup_device(self.ctx, fdb.ptr, int(ingress_port), ptr(arena), arena_bytes, ptr(desc), n,
                                           ptr(rt_verdict), ptr(egress_port), ptr(verdict), ptr(vlan), ptr(learn),
                                           stream), "nfcs_l2_lookup_device")

    def flood_expand_device(self, fdb: "Fdb", ingress_port: int, num_ports: int, arena, arena_bytes: int,
                            copy_base: int, copy_align: int, desc, n: int, cap: int, item_desc, item_port, item_src,
                            totals, l3_port=None, fwd_status=None, l2_port=None, l2_verdict=None, l2_vlan=None,
                            stream=None):
        """The burst as the egress stage's work items, flood copies included (nfcs_flood_expand_device): per
        live packet with a unicast port (the plan's rule over l3_port / fwd_status / l2_port) one item, per
        live packet l2_lookup_device marked L2_FLOOD one item per flood port with a copy of the frame in the
        region [copy_base, arena_bytes) of the same arena, in slots of round_up(len, copy_align). item_desc
        (cap DESC_DTYPE), item_port, item_src (cap u32 each) and totals (one FLOOD_TOTALS_DTYPE record) are
        device buffers; entries past totals.items are written inert. Plan, VLAN and enqueue then run over
        item_desc / item_port."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_flood_expand_device(self.ctx, fdb.ptr, int(ingress_port), int(num_ports), ptr(arena),
                                              arena_bytes, copy_base, copy_align, ptr(desc), n, ptr(l3_port),
                                              ptr(fwd_status), ptr(l2_port), ptr(l2_verdict), ptr(l2_vlan), cap,
                                              ptr(item_desc), ptr(item_port), ptr(item_src), ptr(totals), stream),
               "nfcs_flood_expand_device")

    def icmp_respond_device(self, icmp: "Icmp", fib: Fib, ingress_port: int, arena, arena_bytes: int, msg_base: int,
                            msg_align: int, desc, n: int, rt_verdict, cap: int, msg_desc, msg_port, msg_src, totals,
                            ip_id=None, status=None, stream=None):
        """The burst's ICMP answers built on the device (nfcs_icmp_respond_device): per live packet whose
        rt_verdict (n bytes of route_lookup_device) is RT_LOCAL an echo reply where it is an answerable echo
        request, per RT_TTL_EXPIRED / RT_NO_ROUTE packet an ICMP 11/0 / 3/0 error, checksums included, in the
        region [msg_base, arena_bytes) of the same arena in slots of round_up(msg_len, msg_align). msg_desc (cap
        DESC_DTYPE), msg_port, msg_src (cap u32 each) and totals (one ICMP_TOTALS_DTYPE record) are device
        buffers; entries past totals.messages are written inert. ip_id (n u16: the errors' IPv4 ids) and status
        (n bytes ICMP_ST_*) optional. Plan and enqueue then run over msg_desc / msg_port."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_icmp_respond_device(self.ctx, icmp.ptr, fib.ptr, int(ingress_port), ptr(arena), arena_bytes,
                                              msg_base, msg_align, ptr(desc), n, ptr(rt_verdict), ptr(ip_id), cap,
                                              ptr(msg_desc), ptr(msg_port), ptr(msg_src), ptr(status), ptr(totals),
                                              stream), "nfcs_icmp_respond_device")

    def egress_plan_device(self, egress: "Egress", arena, arena_bytes: int, desc, n: int, port, ops, queue,
                           l3_port=None, fwd_status=None, l2_port=None, stream=None):
        """process_egress + classify_packet_to_queue per frame on device frames, read-only: port (n u32: the
        packet's egress port or IF_NONE), ops (n u32 VLAN_POP / VLAN_NOP, ready for vlan_device) and queue (n
        bytes, QUEUE_NONE without a port). The port is l3_port[i] (route_lookup_device's egress_if; with
        fwd_status, l3_forward_device's status, only where ST_FLAG_FWD is set), else l2_port[i]
        (l2_lookup_device's egress_port)."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_egress_plan_device(self.ctx, egress.ptr, ptr(arena), arena_bytes, ptr(desc), n, ptr(l3_port),
                                             ptr(fwd_status), ptr(l2_port), ptr(port), ptr(ops), ptr(queue), stream),
               "nfcs_egress_plan_device")

    def egress_enqueue_device(self, egress: "Egress", port, queue, n: int, depth, order, key_start, result=None,
                              key_dropped=None, stream=None):
        """enqueue_packet for the burst: depth (keys u32, in/out), order (n u32: the enqueued packets' indexes
        grouped by key, arrival order within), key_start (keys + 1 u32); result (n bytes EQ_*) and key_dropped
        (keys u32) optional."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_egress_enqueue_device(self.ctx, egress.ptr, ptr(port), ptr(queue), n, ptr(depth), ptr(result),
                                                ptr(order), ptr(key_start), ptr(key_dropped), stream),
               "nfcs_egress_enqueue_device")

    def egress_acl_device(self, aclset: "AclSet", arena, arena_bytes: int, desc, n: int, port, action, rule=None,
                          redirect=None, denied_pkts=None, denied_bytes=None, stream=None):
        """The egress ACL per frame on device frames, read-only, the list chosen by the packet's egress port:
        between vlan_device and egress_enqueue_device, on the plan's port (n u32, in/out: IF_NONE stored where
        the packet is denied or its descriptor is bad, the rest untouched). action = n bytes ACL_* (ACL_NO_PORT
        where port was IF_NONE); rule (n u32, inside the port's list), redirect (n u32) and the deny counters
        (denied_pkts: `ports` u32, denied_bytes: `ports` u64, both or neither, accumulating) optional."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_egress_acl_device(self.ctx, aclset.ptr, ptr(arena), arena_bytes, ptr(desc), n, ptr(port),
                                            ptr(action), ptr(rule), ptr(redirect), ptr(denied_pkts), ptr(denied_bytes),
                                            stream), "nfcs_egress_acl_device")

    def ingress_dispatch_device(self, fdb: "Fdb", ingress_port: int, num_ports: int, arena, arena_bytes: int, desc,
                                n: int, rt_verdict, nh, l2_port, l2_verdict, action=None, redirect=None, cls=None,
                                bypass=None, rx_stats=None, stream=None):
        """What process_received_packet does between the stages, per frame of one RX burst of ingress_port
        (nfcs_ingress_dispatch_device), between l2_lookup_device and l3_forward_device: the ingress link test,
        DENY / REDIRECT and the LLDP / zero-MAC / ARP early returns masking nh, l2_port and l2_verdict (in/out), a
        valid REDIRECT's port into l2_port, and the RX counters. action (n bytes) and redirect (n u32) are
        acl_eval_device's (None: the port has no ingress list); cls (n bytes SW_*), bypass (n bytes, for
        egress_acl_items_device) and rx_stats (RX_STATS_DTYPE records indexed by port, accumulating) optional."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_ingress_dispatch_device(self.ctx, fdb.ptr, int(ingress_port), int(num_ports), ptr(arena),
                                                  arena_bytes, ptr(desc), n, ptr(action), ptr(redirect), ptr(rt_verdict),
                                                  ptr(nh), ptr(l2_port), ptr(l2_verdict), ptr(cls), ptr(bypass),
                                                  ptr(rx_stats), stream), "nfcs_ingress_dispatch_device")

    def egress_acl_items_device(self, aclset: "AclSet", arena, arena_bytes: int, desc, n: int, port, action,
                                item_src=None, bypass=None, n_src: int = 0, rule=None, redirect=None,
                                denied_pkts=None, denied_bytes=None, stream=None):
        """egress_acl_device over an item list whose items of redirected frames bypass the ACL
        (nfcs_egress_acl_items_device): item_src (n u32, flood_expand_device's) and bypass (n_src bytes,
        ingress_dispatch_device's), both or neither. A bypassed item keeps its port and reads ACL_BYPASS."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_egress_acl_items_device(self.ctx, aclset.ptr, ptr(arena), arena_bytes, ptr(desc), n, ptr(port),
                                                  ptr(item_src), ptr(bypass), int(n_src), ptr(action), ptr(rule),
                                                  ptr(redirect), ptr(denied_pkts), ptr(denied_bytes), stream),
               "nfcs_egress_acl_items_device")

    def switch_rx_device(self, fib: Fib, fdb: "Fdb", egress: "Egress", ingress_port: int, num_ports: int, arena,
                         arena_bytes: int, copy_base: int, copy_align: int, desc, n: int, cap: int, depth, item_desc,
                         item_port, item_src, totals, order, key_start, workspace, workspace_bytes: int,
                         ingress_acl: "Acl | None" = None, aclset: "AclSet | None" = None,
                         txq: "TxQueues | None" = None, denied_pkts=None, denied_bytes=None, rx_stats=None,
                         key_dropped=None, cls=None, handle_base: int = 0, stream=None):
        """Switch::process_received_packet for one RX burst as one call on one stream, with no host step
        (nfcs_switch_rx_device): route lookup, ingress ACL, L2 lookup, dispatch, forward, flood expand, plan,
        VLAN edit, egress ACL with bypass, enqueue and, with txq, the append (handle of item k: handle_base + k).
        depth, denied_pkts / denied_bytes and rx_stats chain on the device from burst to burst; item_desc,
        item_port (final, after the egress ACL), item_src, totals, order, key_start, key_dropped and cls are the
        outputs; workspace: switch_rx_workspace_bytes(n, cap) bytes of device memory."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        hp = lambda t: None if t is None else t.ptr
        tb = _SwitchTables(hp(fib), hp(ingress_acl), hp(fdb), hp(egress), hp(aclset), hp(txq))
        io = _SwitchRxIo(ptr(arena), int(arena_bytes), int(copy_base), int(copy_align), int(n), int(cap),
                         int(ingress_port), int(num_ports), ptr(desc), ptr(depth), ptr(denied_pkts), ptr(denied_bytes),
                         ptr(rx_stats), ptr(item_desc), ptr(item_port), ptr(item_src), ptr(totals), ptr(order),
                         ptr(key_start), ptr(key_dropped), ptr(cls), int(handle_base), ptr(workspace),
                         int(workspace_bytes))
        _check(lib().nfcs_switch_rx_device(self.ctx, ctypes.byref(tb), ctypes.byref(io), stream), "nfcs_switch_rx_device")

    def txq_append_device(self, txq: "TxQueues", order, key_start, depth, n: int, handle=None, desc=None, stream=None):
        """enqueue_packet's emplace_back for the burst on the device copy of txq, after egress_enqueue_device
        with that call's order / key_start and the depth it left: the handles of the enqueued packets
        (handle, n u64, or the descriptor bits of desc as they are now) go to their rings."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_txq_append_device(self.ctx, txq.ptr, ptr(order), ptr(key_start), ptr(depth), ptr(handle),
                                            ptr(desc), n, stream), "nfcs_txq_append_device")

    def txq_dequeue_device(self, txq: "TxQueues", depth, tx, tx_cap: int, tx_start, budget=None, budget_all: int = 0,
                           tx_queue=None, dequeued=None, stream=None):
        """select_packet_to_dequeue up to budget[port] (ports u32) or budget_all times per port on the device
        copy: depth (keys u32, in/out), tx (tx_cap u64: port p's handles at tx_start[p]..tx_start[p+1] in
        dequeue order), tx_start (ports + 1 u32); tx_queue (tx_cap bytes) and dequeued (keys u32) optional."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_txq_dequeue_device(self.ctx, txq.ptr, ptr(budget), int(budget_all), ptr(depth), ptr(tx),
                                             int(tx_cap), ptr(tx_queue), ptr(tx_start), ptr(dequeued), stream),
               "nfcs_txq_dequeue_device")

    def vlan_device(self, arena, arena_bytes: int, desc, n: int, ops=None, op_all: int = 0,
                    caps=None, cap_all: int = 0, status=None, stream=None):
        """Batched Packet::push_vlan / pop_vlan + update_checksums on device frames; desc
        lengths are updated in place. ops: n u32 edit words (or op_all for every packet),
        caps: n u32 buffer capacities from the frame start (or cap_all)."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_vlan_device(self.ctx, ptr(arena), arena_bytes, ptr(desc), n, ptr(ops),
                                      op_all, ptr(caps), cap_all, ptr(status), stream),
               "nfcs_vlan_device")

    def time_vlan_device(self, arena, arena_bytes, desc, n, op_all, op_alt, cap_all, iters,
                         status=None, stream=None) -> float:
        ms = ctypes.c_float()
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_time_vlan_device(self.ctx, ptr(arena), arena_bytes, ptr(desc), n, op_all,
                                           op_alt, cap_all, ptr(status), iters, stream,
                                           ctypes.byref(ms)), "time_vlan_device")
        return float(ms.value)

    def flow_keys_device(self, arena, arena_bytes: int, desc, n: int, keys=None, hashes=None,
                         stream=None):
        """PacketClassifier::extract_flow_key + hash_flow on device frames: n 64-byte
        FLOW_KEY_DTYPE records and/or n u32 hashes."""
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_flow_keys_device(self.ctx, ptr(arena), arena_bytes, ptr(desc), n, ptr(keys),
                                           ptr(hashes), stream), "nfcs_flow_keys_device")

    def time_flow_keys_device(self, arena, arena_bytes, desc, n, keys, hashes, iters,
                              stream=None) -> float:
        ms = ctypes.c_float()
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_time_flow_keys_device(self.ctx, ptr(arena), arena_bytes, ptr(desc), n,
                                                ptr(keys), ptr(hashes), iters, stream,
                                                ctypes.byref(ms)), "time_flow_keys_device")
        return float(ms.value)

    def time_stream_read(self, buf, nbytes, iters, form=0, stream=None) -> float:
        """Total ms of `iters` pure reads of buf's first nbytes (nfcs_time_stream_read): the
        read-stream reference the bench reports its kernels against."""
        ms = ctypes.c_float()
        p = buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)
        _check(lib().nfcs_time_stream_read(self.ctx, p, nbytes & ~15, form, iters, stream,
                                           ctypes.byref(ms)), "time_stream_read")
        return float(ms.value)

    def time_frames_read(self, arena, arena_bytes, desc, n, iters, stream=None) -> float:
        """Total ms of `iters` reads of the batch's frames in the checksum read pass's own access
        pattern, nothing computed or written (nfcs_time_frames_read)."""
        ms = ctypes.c_float()
        p = lambda b: b.ptr if isinstance(b, DeviceBuffer) else int(b)
        _check(lib().nfcs_time_frames_read(self.ctx, p(arena), arena_bytes, p(desc), n, iters, stream,
                                           ctypes.byref(ms)), "time_frames_read")
        return float(ms.value)

    def time_l3_forward_device(self, arena, arena_bytes, desc, nh, n, table, table_n, iters,
                               status=None, stream=None) -> float:
        ms = ctypes.c_float()
        ptr = lambda b: None if b is None else (b.ptr if isinstance(b, DeviceBuffer) else int(b))
        _check(lib().nfcs_time_l3_forward_device(self.ctx, ptr(arena), arena_bytes, ptr(desc),
                                                 ptr(nh), n, ptr(table), table_n, ptr(status),
                                                 iters, stream, ctypes.byref(ms)),
               "time_l3_forward_device")
        return float(ms.value)

    def time_update_device(self, arena, arena_bytes, desc, n, iters, status=None, stream=None) -> float:
        ms = ctypes.c_float()
        _check(lib().nfcs_time_update_device(self.ctx, arena.ptr, arena_bytes, desc.ptr, n,
                                             None if status is None else status.ptr, iters, stream,
                                             ctypes.byref(ms)), "time_update_device")
        return float(ms.value)

    def time_update_batches(self, batches, n, iters, stream=None) -> float:
        """Total ms of `iters` back-to-back update_device calls rotating over `batches` — a list of
        (arena, arena_bytes, desc), n packets each — on one stream (nfcs_time_update_batches): the
        steady state of a NIC ring, where no call re-processes what the previous one wrote."""
        k = len(batches)
        p = lambda b: b.ptr if isinstance(b, DeviceBuffer) else int(b)
        arenas = (_vp * k)(*[p(a) for a, _, _ in batches])
        sizes = (_u64 * k)(*[int(nb) for _, nb, _ in batches])
        descs = (_vp * k)(*[p(d) for _, _, d in batches])
        ms = ctypes.c_float()
        _check(lib().nfcs_time_update_batches(self.ctx, k, arenas, sizes, descs, n, iters, stream,
                                              ctypes.byref(ms)), "time_update_batches")
        return float(ms.value)

    # ---- synthetic batches / digests ----------------------------------------------------
    def gen_config_device(self, config: int, seed: int, first: int, n: int,
                          arena: DeviceBuffer, arena_bytes: int, desc: DeviceBuffer, stream=None):
        _check(lib().nfcs_gen_config_device(self.ctx, config, seed, first, n, arena.ptr, arena_bytes,
                                            desc.ptr, stream), "gen_config_device")

    def stale_every_device(self, arena: DeviceBuffer, arena_bytes: int, desc: DeviceBuffer, n: int, every: int,
                           stream=None):
        """Make the checksum fields of every `every`-th frame of an updated C1-shaped batch stale again
        (nfcs_stale_every_device; a measurement helper)."""
        _check(lib().nfcs_stale_every_device(self.ctx, arena.ptr, arena_bytes, desc.ptr, n, every, stream),
               "stale_every_device")

    def digest_device(self, arena: DeviceBuffer, arena_bytes: int, desc: DeviceBuffer, n: int,
                      first: int = 0, stream=None) -> int:
        out = _u64()
        _check(lib().nfcs_digest_device(self.ctx, arena.ptr, arena_bytes, desc.ptr, n, first,
                                        ctypes.byref(out), stream), "digest_device")
        return int(out.value)

    def config_batch(self, config: int, seed: int, first: int, n: int, align: int = 16):
        """Lay out + generate a synthetic batch on the device. Returns (arena, nbytes, desc, host_desc)."""
        hdesc, nbytes = layout_config(config, seed, first, n, align)
        d_desc = self.alloc(max(hdesc.nbytes, 16)).upload(hdesc)
        d_arena = self.alloc(max(nbytes, 16))
        self.gen_config_device(config, seed, first, n, d_arena, nbytes, d_desc)
        self.sync()
        return d_arena, nbytes, d_desc, hdesc

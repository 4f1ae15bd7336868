"""Shared inputs for the stage edge tests (test_stage_edges.py, test_gpu_stage_edges.py,
test_gpu_stage_high_offsets.py): a truncation sweep whose frames keep their original bytes behind the
descriptor's length, one set of tables every base frame of the sweep hits, the host's and the Python
models' answers per stage, and one device runner per frame-reading stage call.

The sweep: twelve base frames with fixed headers, each cut to every length 0..96 and to 97, 127, 128 and 129.
place_live() writes the WHOLE base frame into the slot and sets desc.len to the cut length, so what lies
behind the length is the rest of a header the tables know, and the arena around the slots holds 0xA5. A
kernel that reads past a frame's length then sees bytes that change its answer: the full frame is forwarded
by the route lookup, denied by a port rule of the ACLs, found in the FDB and popped by the egress plan, and
the cut is what takes each of these away. The expected values are computed on full[:t] as bytes, so neither
the host functions nor the models can see the tail."""
import numpy as np

import netflow_amd as nf
from acl_common import eval_host as acl_eval_host
from acl_common import make_acl, model_eval, rule
from egress_acl_common import host_decision, model_per_list
from egress_common import model_plan
from egress_common import plan_host as egress_plan_host
from egress_common import set_ports as set_egress_ports
from l2_common import decide_host as l2_decide_host
from l2_common import entries_of
from l2_common import model_decide as l2_model_decide
from l2_common import set_ports as set_l2_ports
from route_common import decide_host as route_decide_host
from route_common import fixture_fib, fixture_model_inputs
from route_common import model_decide as route_model_decide
from route_common import route_fixture

NONE = 0xFFFFFFFF
FILL = 0xEE          # what output buffers hold before a call
GAP = 0xA5           # what the arena holds outside the slots
EE4, EE8 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
BASE_LEN = 144       # bytes of every base frame: nine 16-byte chunks
CUTS = list(range(97)) + [97, 127, 128, 129]

# ---- what the tables know -----------------------------------------------------------------------------
DMAC_U = bytes([0x02, 0, 0, 0, 0x0D, 0x01])   # destination of the untagged bases: in the FDB on VLAN 1
DMAC_T = bytes([0x02, 0, 0, 0, 0x0D, 0x02])   # destination of the tagged bases: in the FDB on VLAN 100 only
SMAC = bytes([0x02, 0, 0, 0, 0x05, 0x01])     # source of every base: learned on VLAN 100 (ingress) and VLAN 1 (port 5)
VID, INNER_VID = 100, 200
MAX_FRAMES_VID = 0x123  # the tag of test_gpu_edges.max_frames: egress port 8 pops it
INGRESS = 1
SPORT, UDP_DPORT, TCP_DPORT = 1000, 2000, 443
DST_A, DST_B, DST_C = "10.2.3.4", "10.1.77.77", "172.16.5.5"  # forwarded by table a of the route fixture
SRC_IP = "10.9.0.1"


def be16(v: int) -> bytes:
    return int(v).to_bytes(2, "big")


def ip_bytes(a: str) -> bytes:
    return bytes(int(x) for x in a.split("."))


def ip_host(a: str) -> int:
    """The ACL rules' form of an address: host byte order."""
    return int.from_bytes(ip_bytes(a), "big")


def pattern(n: int, salt: int) -> bytearray:
    """n bytes, none of them zero, fixed."""
    return bytearray(((i * 7 + salt * 13) % 251) + 1 for i in range(n))


def l2_header(tci=None, inner_tci=None, et=0x0800, dmac=None) -> bytes:
    tags = b"" if tci is None else b"\x81\x00" + be16(tci)
    if inner_tci is not None:
        tags += b"\x81\x00" + be16(inner_tci)
    dmac = dmac if dmac is not None else (DMAC_U if tci is None else DMAC_T)
    return dmac + SMAC + tags + be16(et)


def ipv4_frame(salt, tci=None, inner_tci=None, ihl=5, proto=17, dst=DST_A, src=SRC_IP, dport=None, version=4) -> bytes:
    """An IPv4 frame of BASE_LEN bytes: the L4 header is written first and the fixed IPv4 fields on top of it,
    so with IHL 3 (the L4 header starts inside the IPv4 header) source and destination address stay what they
    are and the ports are the source address's two halves."""
    l2 = l2_header(tci, inner_tci)
    b = pattern(BASE_LEN, salt)
    b[:len(l2)] = l2
    o = len(l2)
    l4 = o + 4 * ihl
    dport = dport if dport is not None else (UDP_DPORT if proto == 17 else TCP_DPORT)
    if proto == 17:
        b[l4:l4 + 8] = be16(SPORT) + be16(dport) + be16(BASE_LEN - l4) + b"\x5a\xa5"
    else:
        b[l4:l4 + 20] = be16(SPORT) + be16(dport) + bytes([1, 2, 3, 4, 5, 6, 7, 8, 0x50, 0x18]) + be16(4096) + b"\x5a\xa5\x11\x22"
    b[o] = (version << 4) | ihl
    b[o + 1] = 0
    b[o + 2:o + 4] = be16(BASE_LEN - o)
    b[o + 4:o + 8] = b"\x12\x34\x40\x00"
    b[o + 8], b[o + 9] = 64, proto
    b[o + 10:o + 12] = b"\xab\xcd"  # stale
    b[o + 12:o + 16] = ip_bytes(src)
    b[o + 16:o + 20] = ip_bytes(dst)
    return bytes(b)


def base_frames():
    """{name: frame}. PCP 6 / 3 / 5 on VLAN 100 in the outer tags, PCP 1 on VLAN 200 in the inner one."""
    t6, t3, t5, inner = (6 << 13) | VID, (3 << 13) | VID, (5 << 13) | VID, (1 << 13) | INNER_VID
    ports_in_src = ".".join(str(x) for x in be16(SPORT) + be16(UDP_DPORT))

    def ipv6_udp(salt, tci=None):
        l2 = l2_header(tci, et=0x86DD)
        b, o = pattern(BASE_LEN, salt), len(l2)
        b[:o] = l2
        b[o:o + 8] = bytes([0x60, 0, 0, 0]) + be16(BASE_LEN - o - 40) + bytes([17, 64])
        b[o + 40:o + 48] = be16(SPORT) + be16(UDP_DPORT) + be16(BASE_LEN - o - 40) + b"\x5a\xa5"
        return bytes(b)

    def arp(salt, tci=None):
        l2 = l2_header(tci, et=0x0806)
        b = pattern(BASE_LEN, salt)
        b[:len(l2)] = l2
        b[len(l2):len(l2) + 8] = bytes([0, 1, 8, 0, 6, 4, 0, 1])
        return bytes(b)

    return {
        "udp": ipv4_frame(1),
        "q_udp": ipv4_frame(2, tci=t6, dst=DST_B),
        "tcp_ihl8": ipv4_frame(3, ihl=8, proto=6, dst=DST_C),          # ports at 46..49: chunks 2 and 3
        "q_tcp_ihl7": ipv4_frame(4, tci=t3, ihl=7, proto=6),
        "udp_ihl15": ipv4_frame(5, ihl=15, dst=DST_B),                  # ports at 74..77
        "ihl3": ipv4_frame(6, ihl=3, src=ports_in_src),
        "qinq": ipv4_frame(7, tci=t5, inner_tci=inner),
        "ipv6_udp": ipv6_udp(8),
        "arp": arp(9),
        "version6": ipv4_frame(10, version=6, dst=DST_C),               # EtherType 0x0800, version nibble 6
        # two more tagged bases, so that the plan's thresholds (18, 22) move enough of the sweep
        "q_arp": arp(11, tci=(2 << 13) | VID),
        "q_ipv6_udp": ipv6_udp(12, tci=(7 << 13) | VID),
    }


def sweep_frames():
    """(full_frames, lens): per base frame one entry per length in CUTS."""
    full, lens = [], []
    for f in base_frames().values():
        assert len(f) == BASE_LEN >= max(CUTS)
        for t in CUTS:
            full.append(f)
            lens.append(t)
    return full, np.array(lens, np.uint32)


def cut(full_frames, lens):
    return [f[:int(t)] for f, t in zip(full_frames, lens)]


def round_up(x, a):
    return (int(x) + a - 1) // a * a


def place_live(full_frames, lens, offsets16, room=0):
    """One arena: frame i starts offsets16[i] 16-byte chunks past a 128-byte line, its slot holds the whole
    full_frames[i] (and `room` more bytes), its descriptor says lens[i]. Every byte outside the frames' own
    bytes is GAP."""
    desc = np.zeros(len(full_frames), dtype=nf.DESC_DTYPE)
    off = 0
    for i, f in enumerate(full_frames):
        assert int(lens[i]) <= len(f)
        off = round_up(off, 128) + 16 * int(offsets16[i])
        desc[i] = (off // 16, int(lens[i]))
        off += round_up(len(f) + room, 16)
    arena = np.full(max(off, 16), GAP, dtype=np.uint8)
    for d, f in zip(desc, full_frames):
        o = int(d["off16"]) * 16
        arena[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return arena, desc


def placed_sweep(room=0):
    """The sweep at each of the 8 line offsets: (full_frames, lens, arena, desc). 9,696 packets: the last
    wave is partial."""
    full, lens = sweep_frames()
    n = len(full)
    full, lens = full * 8, np.tile(lens, 8)
    arena, desc = place_live(full, lens, np.repeat(np.arange(8), n), room=room)
    assert len(desc) % 64 != 0
    return full, lens, arena, desc


# ---- the tables --------------------------------------------------------------------------------------------

def acl_rules():
    """The ingress list. The full IPv4 bases are denied by rule 0 or 1, which name a destination port; cut below
    the ports they fall to the rules that need less of the frame, one after the other."""
    return np.concatenate([
        rule(action=nf.ACL_DENY, dst_port=UDP_DPORT, protocol=17),
        rule(action=nf.ACL_DENY, dst_port=TCP_DPORT),
        rule(action=nf.ACL_REDIRECT, redirect_port=7, dst_ip=ip_host(DST_B)),
        rule(action=nf.ACL_REDIRECT, redirect_port=8, vlan_id=VID),
        rule(action=nf.ACL_PERMIT, ethertype=0x0800),
        rule(action=nf.ACL_DENY, ethertype=0x86DD),
        rule(action=nf.ACL_REDIRECT, redirect_port=9, src_mac=SMAC),
    ])


def chain_acl_rules():
    """The list of the whole-chain test: UDP frames pass, so that the forward has work."""
    return np.concatenate([
        rule(action=nf.ACL_DENY, dst_port=TCP_DPORT),
        rule(action=nf.ACL_REDIRECT, redirect_port=7, dst_ip=ip_host(DST_C)),
        rule(action=nf.ACL_DENY, ethertype=0x86DD),
    ])


def egress_lists():
    """{list id: rules} and {port: list id}. Ports 3 (unbound), 4 (bound to a list never set), 6 (an empty list)
    and IF_NONE have no list."""
    lists = {
        0: acl_rules(),
        1: np.concatenate([rule(action=nf.ACL_DENY, src_port=SPORT),
                           rule(action=nf.ACL_PERMIT, dst_ip=ip_host(DST_A)),
                           rule(action=nf.ACL_DENY, vlan_id=VID),
                           rule(action=nf.ACL_REDIRECT, redirect_port=11, dst_mac=DMAC_U)]),
        2: np.concatenate([rule(action=nf.ACL_REDIRECT, redirect_port=12, dst_port=UDP_DPORT),
                           rule(action=nf.ACL_DENY, protocol=6),
                           rule(action=nf.ACL_DENY, ethertype=0x0806),
                           rule(action=nf.ACL_PERMIT, src_mac=SMAC)]),
        3: np.concatenate([rule(action=nf.ACL_DENY, dst_port=TCP_DPORT, protocol=6),
                           rule(action=nf.ACL_DENY, dst_port=UDP_DPORT),
                           rule(action=nf.ACL_DENY, dst_ip=ip_host("10.0.0.0"), dst_ip_mask=0xFF000000),
                           rule(action=nf.ACL_REDIRECT, redirect_port=13, vlan_id=VID),
                           rule(action=nf.ACL_DENY, dst_mac=DMAC_U)]),
        9: np.zeros(0, nf.ACL_RULE_DTYPE),
    }
    return lists, {0: 0, 1: 1, 2: 2, 5: 3, 4: 77, 6: 9}


ACL_PORT_CYCLE = np.array([0, 1, 2, 5, 3, NONE, 0, 5, 1, 2, 6, 4, 5], np.uint32)   # 13: no multiple of 64 or 101
PLAN_PORT_CYCLE = np.array([0, 1, 2, 5, 0, 1, 3, NONE, 2, 7, 5], np.uint32)           # 11


def acl_ports(n):
    return ACL_PORT_CYCLE[np.arange(n) % len(ACL_PORT_CYCLE)].copy()


def plan_ports(n):
    return PLAN_PORT_CYCLE[np.arange(n) % len(PLAN_PORT_CYCLE)].copy()


def egress_port_records():
    """Ports 0 and 2 pop VLAN 100 (a trunk that leaves its native VLAN untagged, an access port), ports 1 and 5
    leave the tag (another native VLAN; a trunk that tags its native VLAN) and classify by its PCP; port 3 has
    no QoS, port 7 is never set, port 8 (not in the sweep's cycle) pops VLAN 0x123."""
    rows = [(0, 1, nf.L2_TRUNK, 0, 1, VID, 4), (1, 1, nf.L2_TRUNK, 0, 1, 1, 4), (2, 1, nf.L2_ACCESS, 0, 1, VID, 8),
            (5, 1, nf.L2_TRUNK, 1, 1, VID, 2), (3, 1, nf.L2_ACCESS, 0, 0, VID, 4),
            (8, 1, nf.L2_ACCESS, 0, 1, MAX_FRAMES_VID, 4)]
    recs = np.zeros(len(rows), nf.EGRESS_PORT_DTYPE)
    for r, (pid, cfg, typ, tag_native, qos, native, nq) in zip(recs, rows):
        r["port_id"], r["has_vlan_config"], r["type"], r["tag_native"] = pid, cfg, typ, tag_native
        r["has_qos"], r["native_vlan"], r["num_queues"], r["max_queue_depth"] = qos, native, nq, 100000
    return recs


def l2_tables():
    macs = np.array([list(DMAC_U), list(DMAC_T), list(SMAC), list(SMAC)], np.uint8)
    entries = entries_of(macs, [1, VID, VID, 1], [2, 3, INGRESS, 5])
    trunk = dict(link_up=1, stp_forwarding=1, has_vlan_config=1, type=nf.L2_TRUNK, native_vlan=1)
    ports = []
    for pid in (1, 2, 3, 5):
        p = np.zeros(1, nf.L2_PORT_DTYPE)[0]
        p["port_id"] = pid
        for k, v in trunk.items():
            p[k] = v
        ports.append((p, [1, VID]))
    return entries, ports


class Tables:
    """Every table of the sweep, committed, with the inputs the Python models take."""

    def __init__(self):
        z, _ = route_fixture()
        self.route_inputs = fixture_model_inputs(z, "a")
        self.fib = fixture_fib(z, "a")
        self.acl_rules, self.chain_rules = acl_rules(), chain_acl_rules()
        self.acl, self.chain_acl = make_acl(self.acl_rules), make_acl(self.chain_rules)
        self.l2_entries, self.l2_ports = l2_tables()
        self.fdb = set_l2_ports(nf.Fdb().set_entries(self.l2_entries), self.l2_ports).commit()
        recs = egress_port_records()
        self.eg_cfg = {int(r["port_id"]): r for r in recs}
        self.egress = set_egress_ports(nf.Egress(), recs).commit()
        self.lists, self.bound = egress_lists()
        self.aclset = nf.AclSet()
        for lid, r in self.lists.items():
            self.aclset.set_list(lid, r)
        for port, lid in self.bound.items():
            self.aclset.bind_port(port, lid)
        self.aclset.commit()

    def list_of(self, port: int):
        r = self.lists.get(self.bound.get(int(port), NONE))
        return r if r is not None and len(r) else None

    def upload(self, engine):
        for t in (self.fib, self.acl, self.chain_acl, self.fdb, self.egress, self.aclset):
            t.upload(engine)
        return self

    def close(self):
        for t in (self.fib, self.acl, self.chain_acl, self.fdb, self.egress, self.aclset):
            t.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- the host's and the models' answers, each a tuple of arrays ------------------------------------------------

def route_host(T, frames):
    """verdict, next-hop index, egress interface."""
    return route_decide_host(T.fib, frames)


def route_model(T, frames):
    """verdict, egress interface, MAC pairs."""
    return route_model_decide(*T.route_inputs, frames)


def acl_host(T, frames, acl=None):
    """action, rule, redirect."""
    return acl_eval_host(T.acl if acl is None else acl, frames)


def acl_model(T, frames, rules=None):
    return model_eval(T.acl_rules if rules is None else rules, frames)


def l2_host(T, frames):
    """verdict, egress port, VLAN, learn class."""
    return l2_decide_host(T.fdb, INGRESS, frames)


def l2_model(T, frames):
    return l2_model_decide(T.l2_entries, T.l2_ports, INGRESS, frames)


def plan_host(T, ports, frames):
    """ops, queue."""
    return egress_plan_host(T.egress, ports, frames)


def plan_model(T, ports, frames):
    n = len(frames)
    ops, queue = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i, (p, f) in enumerate(zip(ports, frames)):
        ops[i], queue[i] = model_plan(T.eg_cfg, int(p), f)
    return ops, queue


def eacl_host(T, ports, frames):
    """action, rule, redirect."""
    return host_decision(T.aclset, ports, frames)


def eacl_model(T, ports, frames):
    a, r, d = model_per_list(ports, frames, T.list_of)
    a[np.asarray(ports) == NONE] = nf.ACL_NO_PORT
    return a, r, d


def differs(a, b):
    """Per packet: whether two answers (tuples of arrays) differ in any array."""
    out = np.zeros(len(a[0]), bool)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        out |= (x != y) if x.ndim == 1 else (x != y).any(axis=1)
    return out


def same(got, want, names):
    """Arrays equal, one by one; a failure names the array and the first packet."""
    for g, w, name in zip(got, want, names):
        bad = np.flatnonzero(np.asarray(g) != np.asarray(w))
        assert len(bad) == 0, f"{name}: {len(bad)} differ, the first at packet {bad[0]}: {g[bad[0]]} != {w[bad[0]]}"


# ---- the device calls ------------------------------------------------------------------------------------------

def up(engine, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return engine.alloc(max(a.nbytes, 16)).upload(a)


def filled(engine, nbytes):
    return engine.alloc(nbytes + 16).upload(np.full(nbytes + 16, FILL, np.uint8))


def take(buf, dtype, n, what):
    """n elements of an output buffer made by filled(): the element behind them must be as it was."""
    a = buf.download(dtype, n + 1)
    assert a[n] == np.array(EE8).astype(dtype), f"{what}: a store past element n"
    buf.free()
    return a[:n].copy()


def dev_route(engine, T, d_arena, arena_bytes, d_desc, n):
    """verdict, next-hop index, egress interface."""
    d_nh, d_if, d_v = filled(engine, 4 * (n + 1)), filled(engine, 4 * (n + 1)), filled(engine, n + 1)
    engine.route_lookup_device(T.fib, d_arena, arena_bytes, d_desc, n, d_nh, d_if, d_v)
    engine.sync()
    return take(d_v, np.uint8, n, "verdict"), take(d_nh, np.uint32, n, "nh"), take(d_if, np.uint32, n, "egress_if")


def dev_acl(engine, acl, d_arena, arena_bytes, d_desc, n, nh_in):
    """action, rule, redirect, nh after the call."""
    d_a, d_r, d_p = filled(engine, n + 1), filled(engine, 4 * (n + 1)), filled(engine, 4 * (n + 1))
    d_nh = up(engine, np.concatenate([np.asarray(nh_in, np.uint32), np.full(1, EE4, np.uint32)]), np.uint32)
    engine.acl_eval_device(acl, d_arena, arena_bytes, d_desc, n, d_a, d_r, d_p, d_nh)
    engine.sync()
    return (take(d_a, np.uint8, n, "action"), take(d_r, np.uint32, n, "rule"), take(d_p, np.uint32, n, "redirect"),
            take(d_nh, np.uint32, n, "nh"))


def dev_l2(engine, fdb, ingress, d_arena, arena_bytes, d_desc, n, rt_verdict=None, learn=True):
    """verdict, egress port, VLAN, learn class (None without learn)."""
    d_p, d_v, d_vl = filled(engine, 4 * (n + 1)), filled(engine, n + 1), filled(engine, 2 * (n + 1))
    d_le = filled(engine, n + 1) if learn else None
    d_rt = None if rt_verdict is None else up(engine, rt_verdict, np.uint8)
    engine.l2_lookup_device(fdb, ingress, d_arena, arena_bytes, d_desc, n, d_p, rt_verdict=d_rt, verdict=d_v, vlan=d_vl,
                            learn=d_le)
    engine.sync()
    if d_rt is not None:
        d_rt.free()
    return (take(d_v, np.uint8, n, "verdict"), take(d_p, np.uint32, n, "port"), take(d_vl, np.uint16, n, "vlan"),
            take(d_le, np.uint8, n, "learn") if learn else None)


def dev_plan(engine, eg, d_arena, arena_bytes, d_desc, n, l2_port):
    """port, ops, queue."""
    d_port, d_ops, d_q = filled(engine, 4 * (n + 1)), filled(engine, 4 * (n + 1)), filled(engine, n + 1)
    d_l2 = up(engine, l2_port, np.uint32)
    engine.egress_plan_device(eg, d_arena, arena_bytes, d_desc, n, d_port, d_ops, d_q, l2_port=d_l2)
    engine.sync()
    d_l2.free()
    return take(d_port, np.uint32, n, "port"), take(d_ops, np.uint32, n, "ops"), take(d_q, np.uint8, n, "queue")


def dev_eacl(engine, aclset, d_arena, arena_bytes, d_desc, n, port, nports):
    """port after the call, action, rule, redirect, denied_pkts, denied_bytes (counters from zero)."""
    d_port = up(engine, np.concatenate([np.asarray(port, np.uint32), np.full(1, EE4, np.uint32)]), np.uint32)
    d_a, d_r, d_p = filled(engine, n + 1), filled(engine, 4 * (n + 1)), filled(engine, 4 * (n + 1))
    d_pk = up(engine, np.concatenate([np.zeros(nports, np.uint32), np.full(1, EE4, np.uint32)]), np.uint32)
    d_by = up(engine, np.concatenate([np.zeros(nports, np.uint64), np.full(1, EE8, np.uint64)]), np.uint64)
    engine.egress_acl_device(aclset, d_arena, arena_bytes, d_desc, n, d_port, d_a, d_r, d_p, d_pk, d_by)
    engine.sync()
    return (take(d_port, np.uint32, n, "port"), take(d_a, np.uint8, n, "action"), take(d_r, np.uint32, n, "rule"),
            take(d_p, np.uint32, n, "redirect"), take(d_pk, np.uint32, nports, "denied_pkts"),
            take(d_by, np.uint64, nports, "denied_bytes"))


EXPAND_DTYPES = {"l3_port": np.uint32, "fwd_status": np.uint8, "l2_port": np.uint32, "l2_verdict": np.uint8,
                 "l2_vlan": np.uint16}


def dev_expand(engine, fdb, ingress, num_ports, d_arena, arena_bytes, copy_base, align, d_desc, n, cap, arrays):
    """The dict Fdb.flood_expand_host returns, from the device."""
    d_in = {k: up(engine, v, EXPAND_DTYPES[k]) for k, v in arrays.items()}
    d_idesc, d_iport, d_isrc = filled(engine, 8 * (cap + 1)), filled(engine, 4 * (cap + 1)), filled(engine, 4 * (cap + 1))
    d_tot = filled(engine, 32)
    engine.flood_expand_device(fdb, ingress, num_ports, d_arena, arena_bytes, copy_base, align, d_desc, n, cap, d_idesc,
                               d_iport, d_isrc, d_tot, **d_in)
    engine.sync()
    for b in d_in.values():
        b.free()
    tot = d_tot.download(np.uint8, 48)
    d_tot.free()
    assert (tot[32:] == FILL).all(), "a store behind the totals"
    idesc = d_idesc.download(nf.DESC_DTYPE, cap + 1)
    d_idesc.free()
    assert idesc[cap]["off16"] == EE4 and idesc[cap]["len"] == EE4, "a store past cap"
    return {"item_desc": idesc[:cap].copy(), "item_port": take(d_iport, np.uint32, cap, "item_port"),
            "item_src": take(d_isrc, np.uint32, cap, "item_src"), "totals": tot[:32].copy().view(nf.FLOOD_TOTALS_DTYPE)[0]}


def flood_table(nports, vlan=1):
    """(Fdb committed, [(L2_PORT_DTYPE record, allowed VLANs)]): ports 0..nports-1, all ACCESS on one VLAN, link up
    and forwarding, so a flood from one of them reaches every other."""
    ports = []
    for pid in range(nports):
        p = np.zeros(1, nf.L2_PORT_DTYPE)[0]
        p["port_id"], p["link_up"], p["stp_forwarding"], p["has_vlan_config"] = pid, 1, 1, 1
        p["type"], p["native_vlan"] = nf.L2_ACCESS, vlan
        ports.append((p, []))
    return set_l2_ports(nf.Fdb(), ports).commit(), ports


def all_flooded(n, vlan=1):
    return dict(l2_port=np.full(n, NONE, np.uint32), l2_verdict=np.full(n, nf.L2_FLOOD, np.uint8),
                l2_vlan=np.full(n, vlan, np.uint16))

"""The six table classes (Fib, Acl, AclSet, Fdb, Icmp, Egress) behind one interface, for the life-cycle tests:
each case builds the smallest committed table that decides something about a burst of two frames, names every
setter of its class, one setter call that changes the decision, one the library rejects, the host decision over
the burst and the matching Engine.*_device call. Decisions are lists of numpy arrays, compared with same()."""
import struct

import numpy as np

import netflow_amd as nf
from acl_common import rule
from icmp_common import FAR, HOST, ME, device_respond, ipv4, pack_with_region, small_tables
from l2_common import decide_host as l2_host
from l2_common import entries_of, frame_of
from route_common import decide_host as route_host

ARENA_BYTES = 1024  # the two frames, then room for a flood copy or an ICMP message each
CAP = 4
ALIGN = 128         # of the flood copies and the ICMP messages


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def up(engine, a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return engine.alloc(max(a.nbytes, 16)).upload(a)


def no_rules(n=0):
    return np.zeros(n, nf.ACL_RULE_DTYPE)


class Case:
    """frames: the burst. setters: {name: call on a table}, each valid and enough to invalidate the commit."""
    deps = ()

    def __init__(self):
        self.arena, self.desc, self.base = pack_with_region(self.frames, 16, 0, ALIGN)
        self.arena = np.concatenate([self.arena, np.zeros(ARENA_BYTES - len(self.arena), np.uint8)])
        self.n = len(self.frames)

    def close(self):
        for d in self.deps:
            d.close()

    def uploaded(self, engine):
        """What the device call needs beside the table itself."""

    def on_device(self, engine):
        return up(engine, self.arena), up(engine, self.desc)


IP_FRAMES = [ipv4(0x0300000A, HOST, 1, bytes(8)), ipv4(0x0300000A, FAR, 17, bytes(8))]


class FibCase(Case):
    cls, frames = nf.Fib, IP_FRAMES
    setters = {"set_routes": lambda t: t.set_routes(np.zeros(0, nf.FIB_ROUTE_DTYPE)),
               "set_arp": lambda t: t.set_arp(np.zeros(0, nf.FIB_ARP_DTYPE)),
               "set_if_macs": lambda t: t.set_if_macs(np.zeros(0, nf.FIB_IF_MAC_DTYPE)),
               "set_local_ips": lambda t: t.set_local_ips([])}
    after_close = ("commit", "nexthops", "nexthops_host", lambda t: t.lookup_host(HOST, 64), lambda t: t.resolve_host(HOST))

    def build(self):
        fib, icmp = small_tables()
        icmp.close()
        return fib

    def change(self, t):  # the first frame's host is no longer resolved
        t.set_arp(np.zeros(0, nf.FIB_ARP_DTYPE))

    def reject(self, t):
        t.set_routes(np.zeros(nf.FIB_MAX_ROUTES + 1, nf.FIB_ROUTE_DTYPE))

    def host(self, t):
        return list(route_host(t, self.frames))

    def device(self, engine, t):
        d_arena, d_desc = self.on_device(engine)
        d_nh, d_if, d_v = engine.alloc(4 * self.n), engine.alloc(4 * self.n), engine.alloc(self.n)
        engine.route_lookup_device(t, d_arena, ARENA_BYTES, d_desc, self.n, d_nh, d_if, d_v)
        engine.sync()
        return [d_v.download(np.uint8, self.n), d_nh.download(np.uint32, self.n), d_if.download(np.uint32, self.n)]


class AclCase(Case):
    cls, frames = nf.Acl, IP_FRAMES
    setters = {"set_rules": lambda t: t.set_rules(no_rules())}
    after_close = ("commit", lambda t: t.eval_host(IP_FRAMES[0]))

    def build(self):
        return nf.Acl().set_rules(rule(nf.ACL_DENY, protocol=1)).commit()

    def change(self, t):  # denies the other frame
        t.set_rules(rule(nf.ACL_DENY, protocol=17))

    def reject(self, t):
        t.set_rules(no_rules(nf.ACL_MAX_RULES + 1))

    def host(self, t):
        return [np.array(x) for x in zip(*(t.eval_host(f) for f in self.frames))]

    def device(self, engine, t):
        d_arena, d_desc = self.on_device(engine)
        d_a, d_r, d_p = engine.alloc(self.n), engine.alloc(4 * self.n), engine.alloc(4 * self.n)
        engine.acl_eval_device(t, d_arena, ARENA_BYTES, d_desc, self.n, d_a, d_r, d_p)
        engine.sync()
        return [d_a.download(np.uint8, self.n), d_r.download(np.uint32, self.n), d_p.download(np.uint32, self.n)]


class AclSetCase(Case):
    cls, frames, ports = nf.AclSet, IP_FRAMES, [1, 1]
    setters = {"set_list": lambda t: t.set_list(1, no_rules()), "remove_list": lambda t: t.remove_list(5),
               "bind_port": lambda t: t.bind_port(2, 0), "clear": lambda t: t.clear()}
    after_close = ("commit", "info", lambda t: t.eval_host(1, IP_FRAMES[0]),
                   lambda t: t.egress_acl_host(np.zeros(64, np.uint8), np.zeros(1, nf.DESC_DTYPE), [1]))

    def build(self):
        return nf.AclSet().set_list(0, rule(nf.ACL_DENY, protocol=1)).bind_port(1, 0).commit()

    def change(self, t):
        t.set_list(0, rule(nf.ACL_DENY, protocol=17))

    def reject(self, t):
        t.bind_port(nf.L2_MAX_PORTS, 0)

    def host(self, t):
        out = t.egress_acl_host(self.arena, self.desc, self.ports)
        return [out[k] for k in ("port", "action", "rule", "redirect")]

    def device(self, engine, t):
        d_arena, d_desc = self.on_device(engine)
        d_port = up(engine, self.ports, np.uint32)
        d_a, d_r, d_p = engine.alloc(self.n), engine.alloc(4 * self.n), engine.alloc(4 * self.n)
        engine.egress_acl_device(t, d_arena, ARENA_BYTES, d_desc, self.n, d_port, d_a, d_r, d_p)
        engine.sync()
        return [d_port.download(np.uint32, self.n), d_a.download(np.uint8, self.n), d_r.download(np.uint32, self.n),
                d_p.download(np.uint32, self.n)]


MACS = np.array([[2, 0, 0, 0, 0, 1], [2, 0, 0, 0, 0, 2]], np.uint8)


class FdbCase(Case):
    """The L2 decision, then the burst's work items with the flood copies it makes."""
    cls, frames = nf.Fdb, [frame_of(MACS[0], MACS[1]), frame_of(MACS[1], MACS[0])]
    setters = {"set_entries": lambda t: t.set_entries(np.zeros(0, nf.FDB_ENTRY_DTYPE)), "set_port": lambda t: t.set_port(3),
               "clear_ports": lambda t: t.clear_ports()}
    after_close = ("commit", "stats", lambda t: t.lookup_host(0, bytes(64)), lambda t: t.flood_ports_host(0, 1, 3),
                   lambda t: t.flood_expand_host(0, 3, 1024, 128, 128, np.zeros(0, nf.DESC_DTYPE), 4))

    def build(self):  # the second frame's destination is unknown: flooded to ports 1 and 2
        fdb = nf.Fdb().set_entries(entries_of(MACS[:1], [1], [1]))
        for p in (0, 1, 2):
            fdb.set_port(p, native_vlan=1)
        return fdb.commit()

    def change(self, t):  # now it is known
        t.set_entries(entries_of(MACS, [1, 1], [1, 2]))

    def reject(self, t):
        t.set_port(nf.L2_MAX_PORTS)

    def host(self, t):
        v, e, vl, le = l2_host(t, 0, self.frames)
        out = t.flood_expand_host(0, 3, ARENA_BYTES, self.base, ALIGN, self.desc, CAP, l2_port=e, l2_verdict=v, l2_vlan=vl)
        return [v, e, vl, le, out["item_desc"], out["item_port"], out["item_src"], np.array(out["totals"])]

    def device(self, engine, t):
        d_arena, d_desc = self.on_device(engine)
        n = self.n
        d_e, d_v, d_vl, d_le = engine.alloc(4 * n), engine.alloc(n), engine.alloc(2 * n), engine.alloc(n)
        d_id, d_ip, d_is, d_tot = engine.alloc(8 * CAP), engine.alloc(4 * CAP), engine.alloc(4 * CAP), engine.alloc(32)
        engine.l2_lookup_device(t, 0, d_arena, ARENA_BYTES, d_desc, n, d_e, verdict=d_v, vlan=d_vl, learn=d_le)
        engine.flood_expand_device(t, 0, 3, d_arena, ARENA_BYTES, self.base, ALIGN, d_desc, n, CAP, d_id, d_ip, d_is, d_tot,
                                   l2_port=d_e, l2_verdict=d_v, l2_vlan=d_vl)
        engine.sync()
        return [d_v.download(np.uint8, n), d_e.download(np.uint32, n), d_vl.download(np.uint16, n), d_le.download(np.uint8, n),
                d_id.download(nf.DESC_DTYPE, CAP), d_ip.download(np.uint32, CAP), d_is.download(np.uint32, CAP),
                np.array(d_tot.download(nf.FLOOD_TOTALS_DTYPE, 1)[0])]


ECHO = ipv4(HOST, ME, 1, struct.pack(">BBHHH", 8, 0, 0, 1, 2) + b"abc")
EXPIRED = ipv4(HOST, FAR, 6, bytes(20), ttl=0)


class IcmpCase(Case):
    """An echo request to the switch and a frame whose TTL ran out: one message each, built in the arena."""
    cls, frames = nf.Icmp, [ECHO, EXPIRED]
    verdict = np.array([nf.RT_LOCAL, nf.RT_TTL_EXPIRED], np.uint8)
    setters = {"set_local": lambda t: t.set_local(np.zeros(0, nf.ICMP_LOCAL_DTYPE)),
               "set_if_ips": lambda t: t.set_if_ips(np.zeros(0, nf.ICMP_IF_IP_DTYPE)),
               "set_ports_up": lambda t: t.set_ports_up([0], 2)}

    def build(self):
        fib, icmp = small_tables()
        self.deps = self.deps + (fib,)
        self.fib = fib
        return icmp

    @property
    def after_close(self):
        return ("commit", lambda t: t.respond_host(self.fib, 0, self.arena.copy(), self.base, ALIGN, self.desc, self.verdict, CAP))

    def uploaded(self, engine):
        self.fib.upload(engine)

    def change(self, t):  # the switch no longer knows the MAC of its address: no echo reply
        t.set_local(np.zeros(0, nf.ICMP_LOCAL_DTYPE))

    def reject(self, t):
        t.set_ports_up([0], nf.L2_MAX_PORTS + 1)

    def answer(self, out, arena):
        return [out[k] for k in ("msg_desc", "msg_port", "msg_src", "status")] + [np.array(out["totals"]), arena]

    def host(self, t):
        arena = self.arena.copy()
        return self.answer(t.respond_host(self.fib, 0, arena, self.base, ALIGN, self.desc, self.verdict, CAP), arena)

    def device(self, engine, t):
        out = device_respond(engine, t, self.fib, 0, self.arena, self.base, ALIGN, self.desc, self.verdict, CAP)
        return self.answer(out, out["arena"])


TAGGED = bytes(12) + b"\x81\x00\x60\x0a\x88\xb5" + bytes(46)  # PCP 3, VLAN 10


class EgressCase(Case):
    cls, frames, ports = nf.Egress, [TAGGED, TAGGED], [5, 6]
    setters = {"set_port": lambda t: t.set_port(4), "clear_ports": lambda t: t.clear_ports()}
    after_close = ("commit", "keys", lambda t: t.plan_host(5, TAGGED), lambda t: t.enqueue_host([], [], []))

    def build(self):  # port 5 pops its native VLAN's tag, port 6 was never set
        return nf.Egress().set_port(5, type=nf.L2_ACCESS, native_vlan=10, num_queues=8).commit()

    def change(self, t):  # port 5 keeps the tag, so the PCP picks the queue
        t.set_port(5, type=nf.L2_TRUNK, tag_native=True, native_vlan=10, num_queues=8)

    def reject(self, t):
        t.set_port(nf.L2_MAX_PORTS)

    def host(self, t):
        ops, queue = zip(*(t.plan_host(p, f) for p, f in zip(self.ports, self.frames)))
        return [np.array(self.ports, np.uint32), np.array(ops, np.uint32), np.array(queue, np.uint8)]

    def device(self, engine, t):
        d_arena, d_desc = self.on_device(engine)
        d_l2 = up(engine, self.ports, np.uint32)
        d_port, d_ops, d_q = engine.alloc(4 * self.n), engine.alloc(4 * self.n), engine.alloc(self.n)
        engine.egress_plan_device(t, d_arena, ARENA_BYTES, d_desc, self.n, d_port, d_ops, d_q, l2_port=d_l2)
        engine.sync()
        return [d_port.download(np.uint32, self.n), d_ops.download(np.uint32, self.n), d_q.download(np.uint8, self.n)]


CASES = [FibCase, AclCase, AclSetCase, FdbCase, IcmpCase, EgressCase]
SETTERS = [(c, s) for c in CASES for s in c.setters]

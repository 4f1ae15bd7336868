"""Shared by the ingress-dispatch and RX-pipeline tests: the table from the library's SW_* classes to the codes
the reference-made fixture records (switch_common.C_*), the stage inputs of a burst as the route lookup, the
ingress ACL and the L2 lookup leave them, a hand-built list of edge frames with the class switch.hpp gives each
(written down here, not computed), switch_common.host_switch rewritten on the library's new host calls
(host_switch_rx), and the device calls with switch_common's guard bytes behind every array."""
import ctypes

import numpy as np

import netflow_amd as nf
import oracle
import switch_common as sw
from egress_common import plan_host
from flood_common import copy_model, pack_with_tail, round_up
from l2_common import decide_host as l2_decide_host
from route_common import decide_host as route_decide_host

NONE = 0xFFFFFFFF
FILL, GUARD = sw.FILL, sw.GUARD

# the library's class -> the code tests/golden/make_switch_golden.py recorded for the frame
CLASS_OF = {nf.SW_UNHANDLED: sw.C_UNHANDLED, nf.SW_RX_DOWN: sw.C_RX_DOWN, nf.SW_IN_DENY: sw.C_IN_DENY, nf.SW_RED_OK: sw.C_RED_OK,
            nf.SW_RED_DOWN: sw.C_RED_DOWN, nf.SW_RED_RANGE: sw.C_RED_RANGE, nf.SW_LLDP: sw.C_LLDP, nf.SW_ZERO_MAC: sw.C_ZERO_MAC,
            nf.SW_ARP: sw.C_ARP, nf.SW_LOCAL: sw.C_LOCAL, nf.SW_TTL: sw.C_TTL, nf.SW_NO_ROUTE: sw.C_NO_ROUTE,
            nf.SW_ARP_MISS: sw.C_ARP_MISS, nf.SW_NO_IF_MAC: sw.C_NO_IF_MAC, nf.SW_L3_FWD: sw.C_L3_FWD, nf.SW_L2_FWD: sw.C_L2_FWD,
            nf.SW_L2_FLOOD: sw.C_L2_FLOOD, nf.SW_SAME_PORT: sw.C_SAME_PORT, nf.SW_LINK_DOWN: sw.C_LINK_DOWN, nf.SW_STP: sw.C_STP,
            nf.SW_VLAN: sw.C_VLAN}
# the classes whose frames lose their next hop, port and flood; RED_OK keeps a port: the redirect's
MASKED = (nf.SW_RX_DOWN, nf.SW_BAD_DESC, nf.SW_IN_DENY, nf.SW_RED_RANGE, nf.SW_RED_DOWN, nf.SW_LLDP, nf.SW_ZERO_MAC, nf.SW_ARP)
DROPS = (nf.SW_IN_DENY, nf.SW_RED_RANGE, nf.SW_RED_DOWN)


def to_code(cls):
    return np.array([CLASS_OF[int(c)] for c in cls])


def stage_inputs(t, ingress, frames):
    """What the three lookups hand the dispatch for one burst: dict of rt, nh, eif, action, redirect (None without
    an ingress list), l2v, l2p, l2vlan."""
    n = len(frames)
    rt, nh, eif = route_decide_host(t["fib"], frames)
    acl = t["ingress_acl"].get(ingress)
    action = redirect = None
    if acl is not None:
        action, redirect = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32)
        for i, f in enumerate(frames):
            action[i], _, redirect[i] = acl.eval_host(f)
        nh = np.where(action == nf.ACL_PERMIT, nh, nf.NH_NONE).astype(np.uint32)  # the ACL stage masks nh itself
    l2v, l2p, l2vlan, _ = l2_decide_host(t["fdb"], ingress, frames)
    skip = rt != nf.RT_NOT_IPV4
    l2p, l2v = np.where(skip, nf.IF_NONE, l2p).astype(np.uint32), np.where(skip, nf.L2_SKIP, l2v).astype(np.uint8)
    return dict(rt=rt, nh=nh.astype(np.uint32), eif=eif, action=action, redirect=redirect, l2v=l2v, l2p=l2p, l2vlan=l2vlan)


def dispatch_host(t, ingress, arena, arena_bytes, desc, s, rx_stats=None, **kw):
    return t["fdb"].ingress_dispatch_host(ingress, t["num_ports"], arena, arena_bytes, desc, s["rt"], s["nh"], s["l2p"], s["l2v"],
                                          action=s["action"], redirect=s["redirect"], rx_stats=rx_stats, **kw)


def glue_of(t, frames, s):
    """switch_common's glue for the same inputs: (g, nh, l2_port, l2_verdict)."""
    n = len(frames)
    action = s["action"] if s["action"] is not None else np.zeros(n, np.uint8)
    redirect = s["redirect"] if s["redirect"] is not None else np.full(n, NONE, np.uint32)
    g = sw.glue(frames, action, redirect, t["num_ports"], t["link_up"])
    return (g,) + sw.glue_verdicts(g, redirect, s["nh"], s["l2p"], s["l2v"])


# ---- hand-built edges ---------------------------------------------------------------------------------------

EDGE_PORTS, EDGE_INGRESS, EDGE_DOWN = 6, 0, 3  # ports 0..5 of the edge table; 3 is down; num_ports = 6


def edge_fdb():
    fdb = nf.Fdb()
    for p in range(EDGE_PORTS):
        fdb.set_port(p, link_up=p != EDGE_DOWN, native_vlan=1)
    return fdb.commit()


def eth(et, dst=b"\x02\x00\x00\x00\x00\x09", tci=None, length=60, fill=0x5A):
    """An Ethernet frame cut to `length`: dst, a fixed source, an optional 0x8100 tag, the EtherType, filler."""
    b = dst + b"\x02\x00\x00\x00\x00\x01" + (b"\x81\x00" + tci.to_bytes(2, "big") if tci is not None else b"") + et.to_bytes(2, "big")
    return (b + bytes([fill]) * 64)[:length]


P, D, R, BAD = nf.ACL_PERMIT, nf.ACL_DENY, nf.ACL_REDIRECT, nf.ACL_BAD_DESC
NIP, FWD = nf.RT_NOT_IPV4, nf.RT_FORWARD
ZERO = bytes(6)
# (what, frame, the bytes behind it in its slot, action, redirect, rt_verdict, l2_verdict, the class, the class
# when the port has no ingress list). The classes are read off switch.hpp:213-329 by hand. The bytes behind a
# frame are chosen so that a read past len would change the class.
EDGES = [
    ("0 bytes", b"", b"\x00" * 12 + b"\x88\xCC", P, NONE, NIP, nf.L2_NO_ETH, nf.SW_UNHANDLED, None),
    ("13 bytes, 0x88 then 0xCC behind the frame", eth(0x88CC, length=13), b"\xCC", P, NONE, NIP, nf.L2_NO_ETH, nf.SW_UNHANDLED, None),
    ("14 bytes LLDP", eth(0x88CC, length=14), b"", P, NONE, NIP, nf.L2_FLOOD, nf.SW_LLDP, None),
    ("14 bytes ARP", eth(0x0806, length=14), b"", P, NONE, NIP, nf.L2_FLOOD, nf.SW_ARP, None),
    ("14 bytes, tag without a TCI: 0x8100 is the L3 type", eth(0x8100, length=14), b"\x00\x01\x08\x06", P, NONE, NIP, nf.L2_FLOOD,
     nf.SW_L2_FLOOD, None),
    ("17 bytes tagged, inner 0x08 then 0x06 behind the frame: not ARP", eth(0x0806, tci=5, length=17), b"\x06", P, NONE, NIP,
     nf.L2_FORWARD, nf.SW_L2_FWD, None),
    ("18 bytes tagged ARP", eth(0x0806, tci=5, length=18), b"", P, NONE, NIP, nf.L2_FLOOD, nf.SW_ARP, None),
    ("18 bytes tagged IPv4 stub", eth(0x0800, tci=5, length=18), b"", P, NONE, NIP, nf.L2_DROP_VLAN, nf.SW_VLAN, None),
    ("0x88CC behind a tag: not LLDP", eth(0x88CC, tci=7), b"", P, NONE, NIP, nf.L2_FORWARD, nf.SW_L2_FWD, None),
    ("IPv4 to the zero MAC", eth(0x0800, dst=ZERO), b"", P, NONE, FWD, nf.L2_SKIP, nf.SW_ZERO_MAC, None),
    ("LLDP to the zero MAC: LLDP is tested first", eth(0x88CC, dst=ZERO), b"", P, NONE, NIP, nf.L2_FLOOD, nf.SW_LLDP, None),
    ("ARP to the zero MAC: the MAC is tested first", eth(0x0806, dst=ZERO), b"", P, NONE, NIP, nf.L2_FLOOD, nf.SW_ZERO_MAC, None),
    ("redirect == num_ports", eth(0x0800), b"", R, EDGE_PORTS, FWD, nf.L2_SKIP, nf.SW_RED_RANGE, nf.SW_L3_FWD),
    ("redirect == num_ports - 1", eth(0x0800), b"", R, EDGE_PORTS - 1, FWD, nf.L2_SKIP, nf.SW_RED_OK, nf.SW_L3_FWD),
    ("redirect == 0xFFFFFFFF", eth(0x0800), b"", R, NONE, FWD, nf.L2_SKIP, nf.SW_RED_RANGE, nf.SW_L3_FWD),
    ("redirect to a down port", eth(0x0800), b"", R, EDGE_DOWN, NIP, nf.L2_FLOOD, nf.SW_RED_DOWN, nf.SW_L2_FLOOD),
    ("a redirected LLDP frame: the ACL wins", eth(0x88CC), b"", R, 1, NIP, nf.L2_FLOOD, nf.SW_RED_OK, nf.SW_LLDP),
    ("a redirected 10-byte frame", b"\x01" * 10, b"", R, 2, NIP, nf.L2_NO_ETH, nf.SW_RED_OK, nf.SW_UNHANDLED),
    ("a denied ARP frame: the ACL wins", eth(0x0806), b"", D, NONE, NIP, nf.L2_FLOOD, nf.SW_IN_DENY, nf.SW_ARP),
    ("a denied forwarded frame", eth(0x0800, length=98), b"", D, NONE, FWD, nf.L2_SKIP, nf.SW_IN_DENY, nf.SW_L3_FWD),
    ("ACL_BAD_DESC", eth(0x88CC), b"", BAD, NONE, nf.RT_BAD_DESC, nf.L2_BAD_DESC, nf.SW_BAD_DESC, nf.SW_BAD_DESC),
    ("RT_BAD_DESC alone", eth(0x0806), b"", P, NONE, nf.RT_BAD_DESC, nf.L2_BAD_DESC, nf.SW_BAD_DESC, None),
    ("local", eth(0x0800), b"", P, NONE, nf.RT_LOCAL, nf.L2_SKIP, nf.SW_LOCAL, None),
    ("ttl", eth(0x0800), b"", P, NONE, nf.RT_TTL_EXPIRED, nf.L2_SKIP, nf.SW_TTL, None),
    ("no route", eth(0x0800), b"", P, NONE, nf.RT_NO_ROUTE, nf.L2_SKIP, nf.SW_NO_ROUTE, None),
    ("arp miss", eth(0x0800), b"", P, NONE, nf.RT_ARP_MISS, nf.L2_SKIP, nf.SW_ARP_MISS, None),
    ("no interface mac", eth(0x0800), b"", P, NONE, nf.RT_NO_IF_MAC, nf.L2_SKIP, nf.SW_NO_IF_MAC, None),
    ("forwarded", eth(0x0800, length=1500), b"", P, NONE, FWD, nf.L2_SKIP, nf.SW_L3_FWD, None),
    ("l2 forward", eth(0x86DD), b"", P, NONE, NIP, nf.L2_FORWARD, nf.SW_L2_FWD, None),
    ("l2 flood", eth(0x86DD), b"", P, NONE, NIP, nf.L2_FLOOD, nf.SW_L2_FLOOD, None),
    ("same port", eth(0x86DD), b"", P, NONE, NIP, nf.L2_DROP_SAME_PORT, nf.SW_SAME_PORT, None),
    ("link down", eth(0x86DD), b"", P, NONE, NIP, nf.L2_DROP_LINK_DOWN, nf.SW_LINK_DOWN, None),
    ("stp", eth(0x86DD), b"", P, NONE, NIP, nf.L2_DROP_STP, nf.SW_STP, None),
]


class Edges:
    """The edge list as one burst: arena (32-byte slots at least, the bytes behind each frame as EDGES names them, FILL
    elsewhere), desc, the stage inputs with nh = 100 + i and l2_port = 200 + i, and the wanted classes."""

    def __init__(self, repeat=1):
        rows = EDGES * repeat
        self.n = n = len(rows)
        self.frames = [r[1] for r in rows]
        self.desc = np.zeros(n, nf.DESC_DTYPE)
        pos = 0
        for i, r in enumerate(rows):
            self.desc[i] = (pos // 16, len(r[1]))
            pos += round_up(max(len(r[1]) + len(r[2]), 32), 16)
        self.arena = np.full(pos, FILL, np.uint8)
        for d, r in zip(self.desc, rows):
            o, both = int(d["off16"]) * 16, r[1] + r[2]
            self.arena[o:o + len(both)] = np.frombuffer(both, np.uint8)
        col = lambda k, dt: np.array([r[k] for r in rows], dt)
        self.s = dict(action=col(3, np.uint8), redirect=col(4, np.uint32), rt=col(5, np.uint8), l2v=col(6, np.uint8),
                      nh=(100 + np.arange(n)).astype(np.uint32), l2p=(200 + np.arange(n)).astype(np.uint32))
        self.cls = col(7, np.uint8)
        self.cls_no_acl = np.array([r[7] if r[8] is None else r[8] for r in rows], np.uint8)
        self.t = {"num_ports": EDGE_PORTS}

    def want(self, cls, with_acl=True):
        """nh, l2_port, l2_verdict, bypass and the three counters that follow from the classes by the issue's rules."""
        s, lens = self.s, self.desc["len"].astype(np.uint64)
        red_ok = (cls == nf.SW_RED_OK) & with_acl
        gone = np.isin(cls, MASKED) | red_ok
        drop = np.isin(cls, DROPS)
        counted = cls != nf.SW_RX_DOWN
        return dict(nh=np.where(gone, nf.NH_NONE, s["nh"]), l2_port=np.where(red_ok, s["redirect"], np.where(gone, nf.IF_NONE, s["l2p"])),
                    l2_verdict=np.where(gone, nf.L2_SKIP, s["l2v"]), bypass=red_ok.astype(np.uint8),
                    rx=(int(counted.sum() + drop.sum()), int(lens[counted].sum() + lens[drop].sum()), int(drop.sum())))


def assert_dispatch(got, want, cls, rx=None, ingress=None, what=""):
    for k in ("nh", "l2_port", "l2_verdict", "bypass"):
        if got.get(k) is not None:
            bad = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))
            assert len(bad) == 0, f"{what}{k}: {len(bad)} differ, the first at frame {bad[0]}: {got[k][bad[0]]} != {want[k][bad[0]]}"
    if got.get("cls") is not None:
        bad = np.flatnonzero(got["cls"] != cls)
        assert len(bad) == 0, f"{what}class: {len(bad)} differ, the first at frame {bad[0]}: {got['cls'][bad[0]]} != {cls[bad[0]]}"
    if rx is not None:
        assert tuple(int(rx[ingress][k]) for k in ("rx_packets", "rx_bytes", "rx_drops")) == want["rx"], what + "counters"


# ---- the chain on the new host calls ------------------------------------------------------------------------

def per_burst(v, b, default):
    """A keyword that is one value for every burst or a list with one per burst; None: the default."""
    v = v[b] if isinstance(v, (list, tuple)) else v
    return default if v is None else int(v)


EXTRA = ("cls", "rx_stats", "totals", "idesc", "isrc", "iport", "iqueue", "order", "key_start", "key_dropped", "tx_raw")


def host_switch_rx(t, bursts, align=128, copy_align=128, egress_acl=True, cap=None, region=None, null=(), cut=False):
    """switch_common.host_switch with the library's ingress_dispatch_host and egress_acl_items_host in the place of
    glue(): the same result structure, plus cls (per burst, the SW_* class of every frame), rx_stats (per burst,
    the RX counters of every port after it) and, per burst, what the composite hands out: totals, idesc, isrc, iport
    (after the egress ACL), iqueue (the plan's queue per item; the host chain only: the composite keeps it in its
    workspace), order, key_start, key_dropped, and tx_raw = (tx, tx_start, tx_queue) of the dequeue.
    egress_acl False: the chain of a switch without egress lists. cap / region: the item capacity and the bytes of
    the copy region, one value or one per burst (default: FANOUT items per frame and room for all of them). Every item
    must fit unless the caller says cut=True. null: of "ingress_acl", "txq", "rx_stats", "key_dropped", what the device call leaves NULL
    (nothing is dequeued without txq)."""
    ports, keys = t["eg"].keys()
    caps, regions = cap, region
    res = dict(sw.empty_result(), **{k: [] for k in EXTRA})
    depth, dropped = np.zeros(keys, np.uint32), np.zeros(keys, np.uint32)
    acl_ports = max(t["aclset"].info()[0], 1)
    denied_pkts, denied_bytes = np.zeros(acl_ports, np.uint32), np.zeros(acl_ports, np.uint64)
    rx = np.zeros(t["num_ports"], nf.RX_STATS_DTYPE)
    nht = t["fib"].nexthops_host().view(np.uint8).reshape(-1, 12)
    firsts, idescs, srcs, arenas, tx_cap = [], [], [], [], 0
    with sw.make_txq(t) as txq:
        for b, (ingress, first, frames, budget) in enumerate(bursts):
            cap = per_burst(caps, b, sw.FANOUT * len(frames))
            arena, desc, copy_base = pack_with_tail(frames, align, per_burst(regions, b, sw.region_bytes(frames, copy_align)))
            s = stage_inputs(t if "ingress_acl" not in null else dict(t, ingress_acl={}), ingress, frames)
            d = dispatch_host(t, ingress, arena, copy_base, desc, s, rx_stats=None if "rx_stats" in null else rx)
            st = oracle.l3_forward_batch(arena[:copy_base], desc, d["nh"], nht)
            ex = t["fdb"].flood_expand_host(ingress, t["num_ports"], arena.nbytes, copy_base, copy_align, desc, cap, l3_port=s["eif"],
                                            fwd_status=st, l2_port=d["l2_port"], l2_verdict=d["l2_verdict"], l2_vlan=s["l2vlan"])
            assert cut or int(ex["totals"]["items"]) == int(ex["totals"]["items_needed"])
            arena = copy_model(arena, desc, ex, copy_base)
            idesc = ex["item_desc"].copy()
            ops, queue = plan_host(t["eg"], ex["item_port"], oracle.unpack_frames(arena, idesc))
            queue[ex["item_port"] == nf.IF_NONE] = nf.QUEUE_NONE
            oracle.vlan_batch(arena, idesc, ops, None, cap_all=0)
            port = ex["item_port"]
            if egress_acl:
                port = t["aclset"].egress_acl_items_host(arena, idesc, port, ex["item_src"], d["bypass"], denied_pkts, denied_bytes)["port"]
            r = t["eg"].enqueue_host(port, queue, depth)
            tx_cap += cap
            if "txq" in null:
                want = {"depth": r["depth"], "tx": np.zeros(0, np.uint64), "tx_start": np.zeros(ports + 1, np.uint32),
                        "tx_queue": np.zeros(0, np.uint8)}
            else:
                txq.append_host(r["order"], r["key_start"], r["depth"], cap, handle=(b << 32) + np.arange(cap, dtype=np.uint64))
                want = txq.dequeue_host(r["depth"], tx_cap, budget=budget)
            depth = want["depth"]
            for k, v in (("totals", ex["totals"]), ("idesc", idesc), ("isrc", ex["item_src"]), ("iport", port), ("iqueue", queue), ("order", r["order"]),
                         ("key_start", r["key_start"]), ("key_dropped", r["key_dropped"]),
                         ("tx_raw", (want["tx"], want["tx_start"], want.get("tx_queue")))):
                res[k].append(v)
            if "key_dropped" not in null:  # a call that is not handed the array reports no tail drops
                dropped = dropped + r["key_dropped"]
            firsts.append(first), idescs.append(idesc), srcs.append(ex["item_src"]), arenas.append(arena)
            sw.collect(res, firsts, ports, want, idescs, srcs, arenas, b)
            for k, v in (("depth", depth), ("dropped", dropped), ("denied_pkts", denied_pkts), ("denied_bytes", denied_bytes),
                         ("rx_stats", rx)):
                res[k].append(v.copy())
            res["rx_drops"].append(int(rx[ingress]["rx_drops"]))
            res["arena"].append(arena)
            res["cls"].append(d["cls"])
    return res


# ---- the device calls, GUARD bytes of FILL behind every array -----------------------------------------------------

class Guarded:
    def __init__(self, engine):
        self.engine, self.bufs = engine, []

    def out(self, nbytes):
        buf = self.engine.alloc(nbytes + GUARD).upload(np.full(nbytes + GUARD, FILL, np.uint8))
        self.bufs.append((buf, nbytes))
        return buf

    def up(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        buf = self.engine.alloc(a.nbytes + GUARD).upload(np.concatenate([a.view(np.uint8).reshape(-1), np.full(GUARD, FILL, np.uint8)]))
        self.bufs.append((buf, a.nbytes))
        return buf

    def check(self):
        for buf, nbytes in self.bufs:
            assert (buf.download(np.uint8, GUARD, offset=nbytes) == FILL).all(), "guard bytes behind a device array changed"

    def free(self):
        for buf, _ in self.bufs:
            buf.free()
        self.bufs = []


def device_dispatch(engine, fdb, ingress, num_ports, arena, arena_bytes, desc, s, d_rx=None, want=("cls", "bypass"), g=None):
    """One ingress_dispatch_device call on uploaded copies of the stage inputs; the arena is uploaded whole, with a
    guard behind it, and must come back unchanged. Returns the arrays as dispatch_host does (cls / bypass None where
    not wanted). d_rx: a device array of RX_STATS_DTYPE records that stays with the caller."""
    own = g is None
    g = g or Guarded(engine)
    n = len(desc)
    d_arena, d_desc = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE)
    opt = lambda a, dt: None if a is None else g.up(a, dt)
    d_act, d_red = opt(s["action"], np.uint8), opt(s["redirect"], np.uint32)
    d_rt, d_nh, d_l2p, d_l2v = g.up(s["rt"], np.uint8), g.up(s["nh"], np.uint32), g.up(s["l2p"], np.uint32), g.up(s["l2v"], np.uint8)
    d_cls = g.out(n) if "cls" in want else None
    d_byp = g.out(n) if "bypass" in want else None
    engine.ingress_dispatch_device(fdb, ingress, num_ports, d_arena, arena_bytes, d_desc, n, d_rt, d_nh, d_l2p, d_l2v, action=d_act,
                                   redirect=d_red, cls=d_cls, bypass=d_byp, rx_stats=d_rx)
    engine.sync()
    got = dict(nh=d_nh.download(np.uint32, n), l2_port=d_l2p.download(np.uint32, n), l2_verdict=d_l2v.download(np.uint8, n),
               cls=None if d_cls is None else d_cls.download(np.uint8, n), bypass=None if d_byp is None else d_byp.download(np.uint8, n))
    assert np.array_equal(d_arena.download(np.uint8, len(arena)), arena), "the dispatch wrote into the arena"
    assert np.array_equal(d_desc.download(nf.DESC_DTYPE, n), desc)
    for buf, a, dt in ((d_act, s["action"], np.uint8), (d_red, s["redirect"], np.uint32), (d_rt, s["rt"], np.uint8)):
        assert buf is None or np.array_equal(buf.download(dt, n), a), "the dispatch wrote into an input"
    g.check()
    if own:
        g.free()
    return got


def snapshot(engine, g, *pairs, stream=None):
    """Device-to-device copies of (buffer, bytes) pairs, queued on the engine's stream (or `stream`) behind what was
    launched there."""
    out = []
    for src, nbytes in pairs:
        dst = g.out(nbytes)
        rc = nf.lib().hipMemcpyAsync(ctypes.c_void_p(dst.ptr), ctypes.c_void_p(src.ptr), ctypes.c_size_t(nbytes), 3,
                                     ctypes.c_void_p(stream or engine.stream))  # 3: hipMemcpyDeviceToDevice
        assert rc == 0, f"hipMemcpyAsync: {rc}"
        out.append(dst)
    return out


def device_switch_rx(engine, t, bursts, align=128, copy_align=128, egress_acl=True, cap=None, region=None, null=(), workspace=None,
                     ws_bytes=None, stream=None):
    """The bursts through switch_rx_device and txq_dequeue_device: every burst is launched before anything is
    downloaded; depths, deny counters, RX counters and TX rings stay on the device and go on counting. What they
    held after each burst is kept by device-to-device copies queued on the same stream. Returns host_switch_rx's
    structure. cap, region: as host_switch_rx's. null: of "ingress_acl", "txq", "rx_stats", "cls", "key_dropped", what
    the call is handed as NULL (without txq nothing is appended or dequeued). workspace: a (buffer, bytes) pair every
    burst uses instead of one of its own; ws_bytes: the size the call is told instead of
    switch_rx_workspace_bytes(n, cap) (the workspace is allocated that large). stream: a caller's stream for the first
    burst's call, dequeue and state copies; the later bursts run on the context's own with no host synchronisation
    before them: the context's stream waits on the device for an event recorded behind the first burst (depths,
    counters and rings are the caller's data, and their order across streams is the caller's to keep)."""
    for obj in [t["fib"], t["fdb"], t["eg"], t["aclset"], *t["ingress_acl"].values()]:
        obj.upload(engine)
    ports, keys = t["eg"].keys()
    acl_ports = max(t["aclset"].info()[0], 1)
    g = Guarded(engine)
    try:
        return _switch_rx_bursts(engine, t, bursts, g, ports, keys, acl_ports, align, copy_align, egress_acl, cap, region, null,
                                 workspace, ws_bytes, stream)
    finally:
        g.free()  # also where the call is refused: a test that asks for a refusal leaves no device buffer behind


def _switch_rx_bursts(engine, t, bursts, g, ports, keys, acl_ports, align, copy_align, egress_acl, cap, region, null, workspace,
                      ws_bytes, stream):
    d_depth, d_dpk = g.up(np.zeros(keys, np.uint32), np.uint32), g.up(np.zeros(acl_ports, np.uint32), np.uint32)
    d_dby, d_rx = g.up(np.zeros(acl_ports, np.uint64), np.uint64), g.up(np.zeros(t["num_ports"], nf.RX_STATS_DTYPE), nf.RX_STATS_DTYPE)
    res = dict(sw.empty_result(), **{k: [] for k in EXTRA})
    launched, tx_cap = [], 0
    with sw.make_txq(t, engine) as txq:
        for b, (ingress, first, frames, budget) in enumerate(bursts):
            n, cap_b = len(frames), per_burst(cap, b, sw.FANOUT * len(frames))
            tx_cap += cap_b
            arena, desc, copy_base = pack_with_tail(frames, align, per_burst(region, b, sw.region_bytes(frames, copy_align)))
            d_arena, d_desc = g.up(arena, np.uint8), g.up(desc, nf.DESC_DTYPE)
            d_idesc, d_iport, d_isrc, d_tot = g.out(8 * cap_b), g.out(4 * cap_b), g.out(4 * cap_b), g.out(32)
            d_order, d_ks = g.out(4 * cap_b), g.out(4 * (keys + 1))
            d_kd, d_cls = None if "key_dropped" in null else g.out(4 * keys), None if "cls" in null else g.out(n)
            d_tx, d_start, d_txq = g.out(8 * tx_cap), g.out(4 * (ports + 1)), g.out(tx_cap)
            need = nf.switch_rx_workspace_bytes(n, cap_b) if ws_bytes is None else ws_bytes
            d_ws, told = (g.out(need), need) if workspace is None else workspace
            engine.switch_rx_device(t["fib"], t["fdb"], t["eg"], ingress, t["num_ports"], d_arena, arena.nbytes, copy_base, copy_align,
                                    d_desc, n, cap_b, d_depth, d_idesc, d_iport, d_isrc, d_tot, d_order, d_ks, d_ws, told,
                                    ingress_acl=None if "ingress_acl" in null else t["ingress_acl"].get(ingress),
                                    aclset=t["aclset"] if egress_acl else None, txq=None if "txq" in null else txq,
                                    denied_pkts=d_dpk if egress_acl else None, denied_bytes=d_dby if egress_acl else None,
                                    rx_stats=None if "rx_stats" in null else d_rx, key_dropped=d_kd, cls=d_cls, handle_base=b << 32,
                                    stream=stream if b == 0 else None)
            if "txq" not in null:
                engine.txq_dequeue_device(txq, d_depth, d_tx, tx_cap, d_start, budget=g.up(budget, np.uint32), tx_queue=d_txq,
                                          stream=stream if b == 0 else None)
            launched.append((first, arena.nbytes, d_arena, d_idesc, d_isrc, d_tx, tx_cap, d_start, d_kd, d_cls, n, cap_b, d_iport, d_tot,
                             d_order, d_ks, d_txq,
                             snapshot(engine, g, (d_depth, 4 * keys), (d_dpk, 4 * acl_ports), (d_dby, 8 * acl_ports),
                                      (d_rx, 24 * t["num_ports"]), stream=stream if b == 0 else None)))
            if stream and b == 0:
                hip, ev = nf.lib(), ctypes.c_void_p()
                assert hip.hipEventCreate(ctypes.byref(ev)) == 0 and hip.hipEventRecord(ev, ctypes.c_void_p(stream)) == 0
                assert hip.hipStreamWaitEvent(ctypes.c_void_p(engine.stream), ev, 0) == 0 and hip.hipEventDestroy(ev) == 0
        if stream:
            engine.sync(stream)
        engine.sync()
        dropped = np.zeros(keys, np.uint32)
        firsts, idescs, srcs, arenas = [], [], [], []
        for b, (first, nbytes, d_arena, d_idesc, d_isrc, d_tx, tx_cap, d_start, d_kd, d_cls, n, cap_b, d_iport, d_tot, d_order, d_ks,
                d_txq, snap) in enumerate(launched):
            firsts.append(first), idescs.append(d_idesc.download(nf.DESC_DTYPE, cap_b)), srcs.append(d_isrc.download(np.uint32, cap_b))
            arenas.append(d_arena.download(np.uint8, nbytes))
            if "txq" in null:
                start, tx, txqueue = np.zeros(ports + 1, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint8)
            else:
                start = d_start.download(np.uint32, ports + 1)
                tx, txqueue = d_tx.download(np.uint64, tx_cap), d_txq.download(np.uint8, tx_cap)
                assert (tx[int(start[ports]):] == 0xEEEEEEEEEEEEEEEE).all(), "d_tx was written past tx_start[ports]"
                tx, txqueue = tx[:int(start[ports])], txqueue[:int(start[ports])]
            sw.collect(res, firsts, ports, {"tx": tx, "tx_start": start}, idescs, srcs, arenas, b)
            kd = np.zeros(keys, np.uint32) if d_kd is None else d_kd.download(np.uint32, keys)
            dropped = dropped + kd
            res["depth"].append(snap[0].download(np.uint32, keys)), res["dropped"].append(dropped.copy())
            res["denied_pkts"].append(snap[1].download(np.uint32, acl_ports)), res["denied_bytes"].append(snap[2].download(np.uint64, acl_ports))
            res["rx_stats"].append(snap[3].download(nf.RX_STATS_DTYPE, t["num_ports"]))
            res["rx_drops"].append(int(res["rx_stats"][-1][bursts[b][0]]["rx_drops"]))
            res["arena"].append(arenas[-1])
            res["cls"].append(None if d_cls is None else d_cls.download(np.uint8, n))
            key_start = d_ks.download(np.uint32, keys + 1)
            order = d_order.download(np.uint32, cap_b)
            for k, v in (("totals", d_tot.download(nf.FLOOD_TOTALS_DTYPE, 1)[0]), ("idesc", idescs[-1]), ("isrc", srcs[-1]),
                         ("iport", d_iport.download(np.uint32, cap_b)), ("iqueue", None), ("order", order), ("key_start", key_start),
                         ("key_dropped", None if d_kd is None else kd), ("tx_raw", (tx, start, txqueue))):
                res[k].append(v)
        g.check()
    return res


def assert_same_rx(got, want, what=""):
    """What switch_common.assert_same does not cover: classes, RX counters and every array the composite hands out
    (order only where items were enqueued: the rest of it is not defined), the raw dequeue record."""
    for b in range(len(want["cls"])):
        w = f"{what}burst {b}: "
        if got["cls"][b] is not None:
            assert np.array_equal(got["cls"][b], want["cls"][b]), w + "classes"
        assert np.array_equal(got["rx_stats"][b], want["rx_stats"][b]), w + "RX counters"
        for k in nf.FLOOD_TOTALS_DTYPE.names:
            assert int(got["totals"][b][k]) == int(want["totals"][b][k]), w + "totals." + k
        for k in ("idesc", "isrc", "iport", "key_start"):
            assert np.array_equal(got[k][b], want[k][b]), w + k
        if got["key_dropped"][b] is not None:
            assert np.array_equal(got["key_dropped"][b], want["key_dropped"][b]), w + "key_dropped"
        m = int(want["key_start"][b][-1])
        assert np.array_equal(got["order"][b][:m], want["order"][b][:m]), w + "order"
        for x, y, name in zip(got["tx_raw"][b], want["tx_raw"][b], ("tx", "tx_start", "tx_queue")):
            assert np.array_equal(x, y), w + name

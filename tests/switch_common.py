"""Shared inputs for the whole-pipeline tests: the reference-made fixture tests/golden/switch_ref.npz
(tests/golden/make_switch_golden.py: a real netflow::Switch fed three bursts through process_received_packet, each
followed by the ports' TX loops), the nf objects built from the tables the reference's accessors reported, and the
pipeline chained twice in INTEGRATION.md's order: host_switch from the library's *_host functions and the oracle,
device_switch from the device calls. What the reference's switch does between the stages and no stage claims is
written once, in glue(), which both chains share.

Both chains and Fixture.want() return the same structure, one entry per burst in each list:
  tx            {port: [(source frame index over all bursts, bytes)]} in dequeue order
  depth         keys u32: every queue's depth after the burst's TX loops
  dropped       keys u32: tail drops so far
  denied_pkts   per port: egress-ACL denies so far (the reference's tx_drops)
  denied_bytes  per port: their bytes (the reference's tx_bytes)
  rx_drops      ingress-ACL drops so far on the burst's ingress port (the reference's rx_drops)
The chains add `arena`: the whole arena after the burst."""
import os

import numpy as np

import netflow_amd as nf
import oracle
from egress_common import plan_host
from flood_common import copy_model, pack_with_tail, round_up
from l2_common import decide_host as l2_decide_host
from route_common import decide_host as route_decide_host

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q = nf.QOS_MAX_QUEUES
NONE = 0xFFFFFFFF
FILL = 0xEE
GUARD = 64  # bytes of FILL behind every device array
FANOUT = 4  # no VLAN of the fixture's switch floods to more ports
(C_UNHANDLED, C_RX_DOWN, C_IN_DENY, C_RED_OK, C_RED_DOWN, C_RED_RANGE, C_LLDP, C_ZERO_MAC, C_ARP, C_LOCAL, C_TTL,
 C_NO_ROUTE, C_ARP_MISS, C_NO_IF_MAC, C_L3_FWD, C_L2_FWD, C_L2_FLOOD, C_SAME_PORT, C_LINK_DOWN, C_STP, C_VLAN) = range(21)
EV_ENQ, EV_FULL, EV_EDENY = 0, 1, 2


class Fixture:
    def __init__(self):
        self.z = z = np.load(os.path.join(GOLD, "switch_ref.npz"))
        fs, fb = z["frame_start"], z["frame_bytes"]
        self.frames = [bytes(fb[int(fs[i]):int(fs[i + 1])]) for i in range(len(fs) - 1)]
        self.num_ports = int(z["num_ports"])
        self.bursts = []  # (ingress, first frame index, frames, budget per port)
        for b, ingress in enumerate(z["ingress"]):
            lo, hi = int(z["burst_start"][b]), int(z["burst_start"][b + 1])
            self.bursts.append((int(ingress), lo, self.frames[lo:hi], z["budget"][b].astype(np.uint32)))

    def sent(self, b):
        """Burst b's TX record: [(port, source frame, bytes)]. A packet is stored as its XOR with the frame it came
        from, bytes 12..15 removed where it is four bytes shorter."""
        z, out, pos = self.z, [], 0
        start = z[f"tx_start_{b}"]
        for p in range(self.num_ports):
            for j in range(int(start[p]), int(start[p + 1])):
                src, ln = int(z[f"tx_src_{b}"][j]), int(z[f"tx_len_{b}"][j])
                f = self.frames[src]
                base = f if ln == len(f) else f[:12] + f[16:]
                assert len(base) == ln
                delta = z[f"tx_delta_{b}"][pos:pos + ln]
                out.append((p, src, (np.frombuffer(base, np.uint8) ^ delta).tobytes()))
                pos += ln
        assert pos == len(z[f"tx_delta_{b}"])
        return out

    def want(self):
        z, ports = self.z, self.num_ports
        w = {k: [] for k in ("tx", "depth", "dropped", "denied_pkts", "denied_bytes", "rx_drops")}
        for b, (ingress, _, _, _) in enumerate(self.bursts):
            tx = {p: [] for p in range(ports)}
            for p, src, data in self.sent(b):
                tx[p].append((src, data))
            stats = np.where(z[f"stats_{b}"] == NONE, 0, z[f"stats_{b}"]).reshape(ports * Q, 3)
            w["tx"].append(tx)
            w["depth"].append(stats[:, 2].astype(np.uint32))
            w["dropped"].append(stats[:, 1].astype(np.uint32))
            ps = z[f"port_stats_{b}"]  # rx_packets, rx_bytes, rx_drops, tx_packets, tx_bytes, tx_drops
            assert (ps[:, 3] == ps[:, 5]).all()  # the egress deny is the only place that counts TX at all
            w["denied_pkts"].append(ps[:, 5].astype(np.uint64))
            w["denied_bytes"].append(ps[:, 4].astype(np.uint64))
            w["rx_drops"].append(int(ps[ingress, 2]))
        return w


def tables(z):
    """The nf objects from the dump of the reference's tables; close them with close_tables()."""
    ports = int(z["num_ports"])
    t = {"num_ports": ports}
    routes = np.zeros(len(z["routes"]), nf.FIB_ROUTE_DTYPE)
    for k, name in enumerate(("network", "mask", "next_hop_ip", "egress_if")):
        routes[name] = z["routes"][:, k]
    arp = np.zeros(len(z["arp_ip"]), nf.FIB_ARP_DTYPE)
    arp["ip"], arp["mac"] = z["arp_ip"], z["arp_mac"]
    ifm = np.zeros(len(z["if_id"]), nf.FIB_IF_MAC_DTYPE)
    ifm["egress_if"], ifm["mac"] = z["if_id"], z["if_mac"]
    t["fib"] = nf.Fib().set_routes(routes).set_arp(arp).set_if_macs(ifm).set_local_ips(z["if_ips"].astype(np.uint32)).commit()
    rules = {int(l): np.ascontiguousarray(z[f"rules_{int(l)}"]).view(nf.ACL_RULE_DTYPE).reshape(-1).copy() for l in z["list_ids"]}
    by_id = {int(i): k for k, i in enumerate(z["if_id"])}
    t["link_up"] = np.array([bool(z["if_up"][by_id[p]]) if p in by_id else False for p in range(ports)])
    t["ingress_acl"] = {}
    fdb, eg, aclset = nf.Fdb(), nf.Egress(), nf.AclSet()
    fdb.set_entries(np.ascontiguousarray(z["fdb"]).view(nf.FDB_ENTRY_DTYPE).reshape(-1))
    for lid, r in rules.items():
        aclset.set_list(lid, r)
    for p in range(ports):
        k = by_id.get(p)
        has, typ, tagn, native = (int(x) for x in z["vlan"][p])
        allowed = [int(v) for v in z["allowed"][int(z["allowed_start"][p]):int(z["allowed_start"][p + 1])]]
        fdb.set_port(p, k is not None and z["if_up"][k], k is not None and z["if_stp"][k], has, typ, native, allowed)
        qhas, nq, _sched, depth = (int(x) for x in z["qos"][p])
        eg.set_port(p, has, typ, tagn, native, qhas, nq, depth)
        if k is not None and z["if_in_list"][k] != NONE:
            t["ingress_acl"][p] = nf.Acl().set_rules(rules[int(z["if_in_list"][k])]).commit()
        if k is not None and z["if_eg_list"][k] != NONE:
            aclset.bind_port(p, int(z["if_eg_list"][k]))
    t["fdb"], t["eg"], t["aclset"] = fdb.commit(), eg.commit(), aclset.commit()
    t["sched"] = {p: int(z["qos"][p][2]) for p in range(ports) if z["qos"][p][0]}
    return t


def close_tables(t):
    for obj in [t["fib"], t["fdb"], t["eg"], t["aclset"], *t["ingress_acl"].values()]:
        obj.close()


def make_txq(t, engine=None):
    txq = nf.TxQueues(t["eg"], engine)
    for p, sched in t["sched"].items():
        txq.set_scheduler(p, sched)
    return txq


# ---- what the switch does between the stages --------------------------------------------------------------

def glue(frames, action, redirect, num_ports, link_up):
    """Per-frame masks of what Switch::process_received_packet does and no stage claims, from the ingress ACL's
    action and redirect port and the frames' Ethernet headers."""
    lens = np.array([len(f) for f in frames])
    outer = np.array([int.from_bytes(f[12:14], "big") if len(f) >= 14 else 0 for f in frames])
    inner = np.array([int.from_bytes(f[16:18], "big") if len(f) >= 18 else 0 for f in frames])
    zero_mac = np.array([len(f) >= 14 and f[0:6] == bytes(6) for f in frames])
    l3_type = np.where((outer == 0x8100) & (lens >= 18), inner, outer)                    # switch.hpp:259-264
    g = {}
    g["punt"] = (outer == 0x88CC) | zero_mac | (l3_type == 0x0806)                        # 252, 253, 266: early returns
    g["live"] = (action == nf.ACL_PERMIT) & ~g["punt"]                                    # 226-243 decide before them
    valid = (redirect < num_ports) & link_up[np.minimum(redirect, num_ports - 1)]         # 233
    g["redirected"] = (action == nf.ACL_REDIRECT) & valid                                 # 239-240
    g["rx_drop"] = (action == nf.ACL_DENY) | ((action == nf.ACL_REDIRECT) & ~valid)       # 228, 235
    return g


def glue_verdicts(g, redirect, nh, l2_port, l2_verdict):
    """DENY, REDIRECT and the early returns override the L3 next hop and the L2 verdict."""
    nh = np.where(g["live"], nh, nf.NH_NONE).astype(np.uint32)                            # 229, 242, 252-266: no forward
    l2_port = np.where(g["live"], l2_port, np.where(g["redirected"], redirect, nf.IF_NONE)).astype(np.uint32)  # 239
    l2_verdict = np.where(g["live"], l2_verdict, nf.L2_SKIP).astype(np.uint8)             # nor a flood
    return nh, l2_port, l2_verdict


def glue_acl_ports(g, item_src, port):
    """The ports the egress ACL sees: a redirected packet bypasses it (238) and keeps its port."""
    red = (item_src != nf.ITEM_NONE) & g["redirected"][np.minimum(item_src, len(g["redirected"]) - 1)]
    return red, np.where(red, nf.IF_NONE, port).astype(np.uint32)


def region_bytes(frames, copy_align):
    return FANOUT * sum(round_up(len(f), copy_align) for f in frames)


def collect(result, first, ports, want_tx, idesc, item_src, arenas, burst):
    """want_tx's handles (burst << 32 | item) as {port: [(source frame, bytes)]} from the items' descriptors after
    the VLAN edit and the arenas as the bursts left them."""
    tx = {p: [] for p in range(ports)}
    for p in range(ports):
        for h in want_tx["tx"][int(want_tx["tx_start"][p]):int(want_tx["tx_start"][p + 1])]:
            b, k = int(h) >> 32, int(h) & 0xFFFFFFFF
            assert b <= burst
            d = idesc[b][k]
            o = int(d["off16"]) * 16
            tx[p].append((first[b] + int(item_src[b][k]), arenas[b][o:o + int(d["len"])].tobytes()))
    result["tx"].append(tx)


def empty_result():
    return {k: [] for k in ("tx", "depth", "dropped", "denied_pkts", "denied_bytes", "rx_drops", "arena")}


def host_switch(t, bursts, align=128, copy_align=128):
    """The pipeline on the CPU over bursts = [(ingress, first frame index, frames, budget)], the queues carried
    from burst to burst."""
    ports, keys = t["eg"].keys()
    res = empty_result()
    depth, dropped = np.zeros(keys, np.uint32), np.zeros(keys, np.uint32)
    acl_ports = max(t["aclset"].info()[0], 1)
    denied_pkts, denied_bytes = np.zeros(acl_ports, np.uint32), np.zeros(acl_ports, np.uint64)
    nht = t["fib"].nexthops_host().view(np.uint8).reshape(-1, 12)
    firsts, idescs, srcs, arenas, rx_drops = [], [], [], [], {}
    with make_txq(t) as txq:
        for b, (ingress, first, frames, budget) in enumerate(bursts):
            n, cap = len(frames), FANOUT * len(frames)
            arena, desc, copy_base = pack_with_tail(frames, align, region_bytes(frames, copy_align))
            rt, nh, eif = route_decide_host(t["fib"], frames)
            acl = t["ingress_acl"].get(ingress)
            action, redirect = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32)
            if acl is not None:
                for i, f in enumerate(frames):
                    action[i], _, redirect[i] = acl.eval_host(f)
                nh = np.where(action == nf.ACL_PERMIT, nh, nf.NH_NONE).astype(np.uint32)  # the stage masks nh itself
            l2v, l2p, l2vlan, _ = l2_decide_host(t["fdb"], ingress, frames)
            skip = rt != nf.RT_NOT_IPV4                                                  # the stage's rt_verdict input
            l2p, l2v = np.where(skip, nf.IF_NONE, l2p).astype(np.uint32), np.where(skip, nf.L2_SKIP, l2v).astype(np.uint8)
            g = glue(frames, action, redirect, t["num_ports"], t["link_up"])
            nh, l2p, l2v = glue_verdicts(g, redirect, nh, l2p, l2v)
            st = oracle.l3_forward_batch(arena[:copy_base], desc, nh, nht)
            ex = t["fdb"].flood_expand_host(ingress, t["num_ports"], arena.nbytes, copy_base, copy_align, desc, cap, l3_port=eif,
                                            fwd_status=st, l2_port=l2p, l2_verdict=l2v, l2_vlan=l2vlan)
            assert int(ex["totals"]["items"]) == int(ex["totals"]["items_needed"])
            arena = copy_model(arena, desc, ex, copy_base)
            idesc = ex["item_desc"].copy()
            ops, queue = plan_host(t["eg"], ex["item_port"], oracle.unpack_frames(arena, idesc))
            queue[ex["item_port"] == nf.IF_NONE] = nf.QUEUE_NONE
            oracle.vlan_batch(arena, idesc, ops, None, cap_all=0)
            red, seen = glue_acl_ports(g, ex["item_src"], ex["item_port"])
            out = t["aclset"].egress_acl_host(arena, idesc, seen, denied_pkts, denied_bytes)
            port = np.where(red, ex["item_port"], out["port"]).astype(np.uint32)
            r = t["eg"].enqueue_host(port, queue, depth)
            txq.append_host(r["order"], r["key_start"], r["depth"], cap, handle=(b << 32) + np.arange(cap, dtype=np.uint64))
            want = txq.dequeue_host(r["depth"], cap * (b + 1), budget=budget)
            depth = want["depth"]
            dropped = dropped + r["key_dropped"]
            rx_drops[ingress] = rx_drops.get(ingress, 0) + int(g["rx_drop"].sum())
            firsts.append(first), idescs.append(idesc), srcs.append(ex["item_src"]), arenas.append(arena)
            collect(res, firsts, ports, want, idescs, srcs, arenas, b)
            for k, v in (("depth", depth), ("dropped", dropped), ("denied_pkts", denied_pkts), ("denied_bytes", denied_bytes)):
                res[k].append(v.copy())
            res["rx_drops"].append(rx_drops[ingress])
            res["arena"].append(arena)
    return res


def device_switch(engine, t, bursts, align=128, copy_align=128):
    """The same with the device calls, in the order route lookup -> ACL -> L2 lookup -> forward -> flood expand ->
    plan -> VLAN -> egress ACL -> enqueue -> append -> dequeue. Depths, deny counters and the TX rings stay on the
    device from burst to burst; glue()'s masks are applied on the host between the calls. Nothing a burst reports
    is read back before the last burst is launched. Every device array has GUARD bytes of FILL behind it, which
    are checked at the end."""
    for obj in [t["fib"], t["fdb"], t["eg"], t["aclset"], *t["ingress_acl"].values()]:
        obj.upload(engine)
    ports, keys = t["eg"].keys()
    acl_ports = max(t["aclset"].info()[0], 1)
    guarded = []

    def out(nbytes):
        buf = engine.alloc(nbytes + GUARD).upload(np.full(nbytes + GUARD, FILL, np.uint8))
        guarded.append((buf, nbytes))
        return buf

    def up(a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        buf = engine.alloc(a.nbytes + GUARD).upload(np.concatenate([a.view(np.uint8).reshape(-1), np.full(GUARD, FILL, np.uint8)]))
        guarded.append((buf, a.nbytes))
        return buf

    d_depth, d_dpk, d_dby = up(np.zeros(keys, np.uint32), np.uint32), up(np.zeros(acl_ports, np.uint32), np.uint32), \
        up(np.zeros(acl_ports, np.uint64), np.uint64)
    d_tab, tab_n = t["fib"].nexthops()
    res = empty_result()
    launched, rx_drops = [], {}
    with make_txq(t, engine) as txq:
        for b, (ingress, first, frames, budget) in enumerate(bursts):
            n, cap = len(frames), FANOUT * len(frames)
            tx_cap = cap * (b + 1)
            arena, desc, copy_base = pack_with_tail(frames, align, region_bytes(frames, copy_align))
            nbytes = arena.nbytes
            d_arena, d_desc = up(arena, np.uint8), up(desc, nf.DESC_DTYPE)
            d_nh, d_if, d_rt, d_st = out(4 * n), out(4 * n), out(n), out(n)
            d_l2p, d_l2v, d_vlan = out(4 * n), out(n), out(2 * n)
            d_idesc, d_iport, d_isrc, d_tot = out(8 * cap), out(4 * cap), out(4 * cap), out(32)
            d_port, d_ops, d_queue, d_eact = out(4 * cap), out(4 * cap), out(cap), out(cap)
            d_order, d_ks, d_kd = out(4 * cap), out(4 * (keys + 1)), out(4 * keys)
            d_tx, d_start = out(8 * tx_cap), out(4 * (ports + 1))
            engine.route_lookup_device(t["fib"], d_arena, copy_base, d_desc, n, d_nh, egress_if=d_if, verdict=d_rt)
            acl = t["ingress_acl"].get(ingress)
            action, redirect = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32)
            if acl is not None:
                d_act, d_red = out(n), out(4 * n)
                engine.acl_eval_device(acl, d_arena, copy_base, d_desc, n, d_act, redirect=d_red, nh=d_nh)
            engine.l2_lookup_device(t["fdb"], ingress, d_arena, copy_base, d_desc, n, d_l2p, rt_verdict=d_rt, verdict=d_l2v, vlan=d_vlan)
            engine.sync()
            if acl is not None:
                action, redirect = d_act.download(np.uint8, n), d_red.download(np.uint32, n)
            g = glue(frames, action, redirect, t["num_ports"], t["link_up"])
            nh, l2p, l2v = glue_verdicts(g, redirect, d_nh.download(np.uint32, n), d_l2p.download(np.uint32, n),
                                         d_l2v.download(np.uint8, n))
            d_nh.upload(nh), d_l2p.upload(l2p), d_l2v.upload(l2v)
            engine.l3_forward_device(d_arena, copy_base, d_desc, d_nh, n, d_tab, tab_n, d_st)
            engine.flood_expand_device(t["fdb"], ingress, t["num_ports"], d_arena, nbytes, copy_base, copy_align, d_desc, n, cap,
                                       d_idesc, d_iport, d_isrc, d_tot, l3_port=d_if, fwd_status=d_st, l2_port=d_l2p,
                                       l2_verdict=d_l2v, l2_vlan=d_vlan)
            engine.egress_plan_device(t["eg"], d_arena, nbytes, d_idesc, cap, d_port, d_ops, d_queue, l2_port=d_iport)
            engine.vlan_device(d_arena, nbytes, d_idesc, cap, d_ops, 0, None, 0)
            engine.sync()
            planned = d_port.download(np.uint32, cap)
            red, seen = glue_acl_ports(g, d_isrc.download(np.uint32, cap), planned)
            d_port.upload(seen)
            engine.egress_acl_device(t["aclset"], d_arena, nbytes, d_idesc, cap, d_port, d_eact, denied_pkts=d_dpk, denied_bytes=d_dby)
            engine.sync()
            d_port.upload(np.where(red, planned, d_port.download(np.uint32, cap)).astype(np.uint32))
            engine.egress_enqueue_device(t["eg"], d_port, d_queue, cap, d_depth, d_order, d_ks, key_dropped=d_kd)
            engine.txq_append_device(txq, d_order, d_ks, d_depth, cap, handle=up((b << 32) + np.arange(cap, dtype=np.uint64), np.uint64))
            engine.txq_dequeue_device(txq, d_depth, d_tx, tx_cap, d_start, budget=up(budget, np.uint32))
            # the counters stay on the device and go on counting: a copy of their state now, looked at at the end
            snap = [out(4 * keys), out(4 * acl_ports), out(8 * acl_ports)]
            engine.sync()
            for dst, src, nb in zip(snap, (d_depth, d_dpk, d_dby), (4 * keys, 4 * acl_ports, 8 * acl_ports)):
                dst.upload(src.download(np.uint8, nb))
            rx_drops[ingress] = rx_drops.get(ingress, 0) + int(g["rx_drop"].sum())
            res["rx_drops"].append(rx_drops[ingress])
            launched.append((first, nbytes, d_arena, d_idesc, d_isrc, d_tx, tx_cap, d_start, d_kd, snap, cap))
        engine.sync()
        dropped = np.zeros(keys, np.uint32)
        firsts, idescs, srcs, arenas = [], [], [], []
        for b, (first, nbytes, d_arena, d_idesc, d_isrc, d_tx, tx_cap, d_start, d_kd, snap, cap) in enumerate(launched):
            firsts.append(first), idescs.append(d_idesc.download(nf.DESC_DTYPE, cap)), srcs.append(d_isrc.download(np.uint32, cap))
            arenas.append(d_arena.download(np.uint8, nbytes))
            start = d_start.download(np.uint32, ports + 1)
            tx = d_tx.download(np.uint64, tx_cap)
            assert (tx[int(start[ports]):] == 0xEEEEEEEEEEEEEEEE).all(), "d_tx was written past tx_start[ports]"
            collect(res, firsts, ports, {"tx": tx, "tx_start": start}, idescs, srcs, arenas, b)
            dropped = dropped + d_kd.download(np.uint32, keys)
            res["depth"].append(snap[0].download(np.uint32, keys)), res["dropped"].append(dropped.copy())
            res["denied_pkts"].append(snap[1].download(np.uint32, acl_ports)), res["denied_bytes"].append(snap[2].download(np.uint64, acl_ports))
            res["arena"].append(arenas[-1])
        for buf, nbytes in guarded:
            assert (buf.download(np.uint8, GUARD, offset=nbytes) == FILL).all(), "guard bytes behind a device array changed"
    return res


def assert_same(got, want, what="", arenas=False):
    """Everything of the structure, burst by burst; the counters over the ports both sides have."""
    for b in range(len(want["tx"])):
        w = f"{what}burst {b}: "
        for p, pkts in want["tx"][b].items():
            have = got["tx"][b].get(p, [])
            assert [s for s, _ in have] == [s for s, _ in pkts], f"{w}port {p} sends other frames or another order"
            for (s, x), (_, y) in zip(have, pkts):
                assert x == y, f"{w}port {p}: the bytes of frame {s} differ"
        assert np.array_equal(got["depth"][b], want["depth"][b]), w + "depths"
        assert np.array_equal(got["dropped"][b], want["dropped"][b]), w + "tail drops"
        for k in ("denied_pkts", "denied_bytes"):
            a, c = got[k][b].astype(np.uint64), want[k][b].astype(np.uint64)
            m = min(len(a), len(c))
            assert np.array_equal(a[:m], c[:m]) and not a[m:].any() and not c[m:].any(), w + k
        assert got["rx_drops"][b] == want["rx_drops"][b], w + "rx_drops"
        if arenas:
            assert np.array_equal(got["arena"][b], want["arena"][b]), w + "the arenas differ"


def outcome(result, n):
    """Per source frame: the sorted (port, length) of every packet sent for it over all bursts."""
    out = [[] for _ in range(n)]
    for tx in result["tx"]:
        for p, pkts in tx.items():
            for s, data in pkts:
                out[s].append((p, len(data)))
    return [sorted(x) for x in out]

"""Shared inputs for the route / ARP lookup tests: the reference-made fixture
tests/golden/route_ref.npz (tests/golden/make_route_golden.py), a Fib built from its tables, and the
frame-level decision on the CPU: the header predicate of include/nfcs.h NFCS_RT_NOT_IPV4 in front of
Fib.lookup_host."""
import os

import numpy as np

import netflow_amd as nf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLES = ("a", "b")  # a: with the default route; b: without it, so NO_ROUTE occurs


def route_fixture():
    z = np.load(os.path.join(GOLD, "route_ref.npz"))
    frames = [bytes(z["frames"][i, :int(ln)]) for i, ln in enumerate(z["lens"])]
    return z, frames


def make_fib(routes, arp_ip, arp_mac, if_id, if_mac, local_ip) -> nf.Fib:
    """routes: rows {network, mask, next_hop, if, ...} in lookup order."""
    routes = np.asarray(routes, dtype=np.uint32).reshape(-1, np.shape(routes)[-1] if np.size(routes) else 4)
    r = np.zeros(len(routes), dtype=nf.FIB_ROUTE_DTYPE)
    for k, name in enumerate(("network", "mask", "next_hop_ip", "egress_if")):
        r[name] = routes[:, k]
    a = np.zeros(len(arp_ip), dtype=nf.FIB_ARP_DTYPE)
    a["ip"] = arp_ip
    if len(a):
        a["mac"] = arp_mac
    m = np.zeros(len(if_id), dtype=nf.FIB_IF_MAC_DTYPE)
    m["egress_if"] = if_id
    if len(m):
        m["mac"] = if_mac
    return nf.Fib().set_routes(r).set_arp(a).set_if_macs(m).set_local_ips(np.asarray(local_ip, np.uint32)).commit()


def fixture_fib(z, table: str) -> nf.Fib:
    return make_fib(z["routes_" + table], z["arp_ip"], z["arp_mac"], z["if_id"], z["if_mac"], z["local_ip"])


def ipv4_dst_ttl(frame: bytes):
    """(dst as the tables' u32, ttl) when the frame passes the forward's IPv4 predicate, else None:
    len >= 14, L3 EtherType after at most one 0x8100 tag is 0x0800 (a tagged frame shorter than 18
    keeps 0x8100), len >= 34 (38 if tagged)."""
    n = len(frame)
    if n < 14:
        return None
    tagged = frame[12:14] == b"\x81\x00"
    et = frame[16:18] if tagged and n >= 18 else frame[12:14]
    l2 = 18 if tagged else 14
    if et != b"\x08\x00" or n < l2 + 20:
        return None
    return int.from_bytes(frame[l2 + 16:l2 + 20], "little"), frame[l2 + 8]


def decide_host(fib: nf.Fib, frames):
    """verdict (u8), next-hop index (u32), egress interface (u32) per frame, on the CPU."""
    v = np.zeros(len(frames), np.uint8)
    nh = np.full(len(frames), nf.NH_NONE, np.uint32)
    eif = np.full(len(frames), nf.IF_NONE, np.uint32)
    for i, f in enumerate(frames):
        h = ipv4_dst_ttl(f)
        if h is None:
            v[i] = nf.RT_NOT_IPV4
        else:
            v[i], nh[i], eif[i] = fib.lookup_host(*h)
    return v, nh, eif


def model_lookup(routes, arp, if_macs, local_ips, dst: int, ttl: int):
    """(verdict, egress interface, the 12 bytes dst MAC + src MAC the forward would write, or None) for one
    destination and TTL: a plain restatement of switch.hpp:270-294 over the inputs as they were given, sharing
    no code with the library. routes: rows {network, mask, next hop (0 = connected), interface, ...} in lookup
    order (RoutingManager::lookup_route returns the first that matches); arp: [(ip, mac bytes)], of two
    entries for one address the later one counts; if_macs: [(interface, mac bytes)]; addresses are the
    tables' u32 (nf.ip4)."""
    arp_of = {int(a): bytes(m) for a, m in arp}
    mac_of = {int(i): bytes(m) for i, m in if_macs}
    dst = int(dst)
    if dst in {int(a) for a in local_ips}:                     # is_my_ip (270)
        return nf.RT_LOCAL, nf.IF_NONE, None
    if ttl <= 1:                                               # 279
        return nf.RT_TTL_EXPIRED, nf.IF_NONE, None
    for row in routes:                                         # lookup_route (282)
        network, mask, gateway, ifid = (int(x) for x in row[:4])
        if dst & mask != network:
            continue
        target = gateway if gateway != 0 else dst             # 285-286: ARP for the gateway, or the destination
        if target not in arp_of:
            return nf.RT_ARP_MISS, nf.IF_NONE, None
        if ifid not in mac_of:                                 # 291-292
            return nf.RT_NO_IF_MAC, nf.IF_NONE, None
        return nf.RT_FORWARD, ifid, arp_of[target] + mac_of[ifid]
    return nf.RT_NO_ROUTE, nf.IF_NONE, None


def model_decide(routes, arp, if_macs, local_ips, frames):
    """model_lookup behind the IPv4 predicate, per frame: verdict (u8), egress interface (u32), MAC pairs
    ((n, 12) u8, zero unless the verdict is RT_FORWARD)."""
    n = len(frames)
    v, eif, macs = np.zeros(n, np.uint8), np.full(n, nf.IF_NONE, np.uint32), np.zeros((n, 12), np.uint8)
    for i, f in enumerate(frames):
        h = ipv4_dst_ttl(f)
        if h is None:
            v[i] = nf.RT_NOT_IPV4
            continue
        v[i], eif[i], m = model_lookup(routes, arp, if_macs, local_ips, *h)
        if m is not None:
            macs[i] = np.frombuffer(m, np.uint8)
    return v, eif, macs


def fixture_model_inputs(z, table: str):
    """(routes, arp, if_macs, local_ips) of the fixture in the form model_lookup takes."""
    return (z["routes_" + table], [(int(a), bytes(m)) for a, m in zip(z["arp_ip"], z["arp_mac"])],
            [(int(i), bytes(m)) for i, m in zip(z["if_id"], z["if_mac"])], [int(a) for a in z["local_ip"]])


def rewrite_dsts(frames, pool, rng, share=0.5):
    """Frames with the destination of `share` of ALL of them replaced by a draw from pool (u32s). Only
    frames that pass the IPv4 predicate have a destination to replace (a little over half of the
    oracle's fuzz frames), so the ones to rewrite are drawn from those: share * len(frames) of them,
    or all of them if there are fewer."""
    out = list(frames)
    v4 = [i for i, f in enumerate(frames) if ipv4_dst_ttl(f) is not None]
    k = min(len(v4), int(round(share * len(frames))))
    for i in rng.choice(v4, size=k, replace=False) if k else []:
        b = bytearray(frames[i])
        l2 = 18 if b[12:14] == b"\x81\x00" else 14
        b[l2 + 16:l2 + 20] = int(pool[int(rng.integers(0, len(pool)))]).to_bytes(4, "little")
        out[i] = bytes(b)
    return out


# Destinations the fixture's tables know (tests/golden/make_route_golden.py DSTS): forwarded under
# both tables, and the rest (default route / no route, ARP misses, no interface MAC, the switch's own).
FWD_DSTS = ["10.2.3.4", "10.1.2.7", "10.1.2.200", "10.1.77.77", "172.16.5.5", "172.31.255.1", "192.168.77.5",
            "10.200.1.1", "10.200.1.2", "10.77.0.1", "10.1.2.129"]
OTHER_DSTS = ["8.8.8.8", "203.0.113.9", "10.9.9.9", "192.168.9.77", "10.5.0.10", "10.5.0.9", "10.6.1.1",
              "10.0.0.100", "10.1.2.1", "192.168.1.5"]


def dst_pool(fwd_weight: int = 5):
    return [nf.ip4(a) for a in FWD_DSTS] * fwd_weight + [nf.ip4(a) for a in OTHER_DSTS]

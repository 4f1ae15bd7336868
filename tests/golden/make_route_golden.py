"""Generate tests/golden/route_ref.npz from the REFERENCE implementation.

Compiles tests/golden/route_probe.cpp against the reference's headers in place (plus its
src/netflow++/routing_manager.cpp) into oracle/_ref/route_probe (git-ignored), feeds it two route
tables, ARP entries, interface MACs, the switch's addresses and a list of frames, and records what
the reference decides per frame (switch.hpp:259-301): the routing table as get_routing_table()
returns it, and per frame the verdict, the egress interface and the MAC pair it would write.

Two tables, because one fixture cannot hold both a default route and a NO_ROUTE verdict: table "a"
has the default route, table "b" is the same input without it, given in another order. Every frame
runs against both. The script checks, against the reference alone, that every verdict occurs and
that FORWARD makes up at least a quarter of the frames under each table.

    python tests/golden/make_route_golden.py [reference root, default /root/reference]
"""
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "route_probe")
SEED = 20261
FRAME_CAP = 64  # frames are truncated to this many bytes (the decision reads none past 37)
FORWARD, BAD_DESC, NOT_IPV4, LOCAL, TTL_EXPIRED, NO_ROUTE, ARP_MISS, NO_IF_MAC = range(8)


def ip(a):
    """Dotted address -> the u32 the reference holds (network byte order read on this host)."""
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "little")


def mac(k):
    return bytes([0x02, 0xAA, (k >> 24) & 255, (k >> 16) & 255, (k >> 8) & 255, k & 255])


# {network, mask, next hop (0 = connected), interface, metric}, as given to add_static_route
ROUTES = [
    ("0.0.0.0", "0.0.0.0", "10.0.0.254", 1, 10),         # the default route (table a only)
    ("10.0.0.0", "255.0.0.0", "0.0.0.0", 1, 1),          # connected /8
    ("10.1.0.0", "255.255.0.0", "10.0.0.1", 2, 1),       # nested: /16 through a gateway,
    ("10.1.2.0", "255.255.255.0", "0.0.0.0", 3, 1),      #   a connected /24 inside it,
    ("10.1.2.128", "255.255.255.128", "10.0.0.2", 4, 1),  #   a /25 through a gateway inside that
    ("172.16.0.0", "255.240.0.0", "10.0.0.3", 2, 5),     # two routes to one prefix that differ in
    ("172.16.0.0", "255.240.0.0", "10.0.0.4", 3, 2),     #   metric (and so need another next hop)
    ("192.168.0.5", "255.255.0.255", "0.0.0.0", 2, 1),   # a non-contiguous mask, connected
    ("192.168.9.0", "255.255.255.0", "10.9.9.9", 1, 1),  # gateway without an ARP entry
    ("10.5.0.0", "255.255.0.0", "0.0.0.0", 5, 1),        # connected, interface 5 has no MAC
    ("10.6.0.0", "255.255.0.0", "10.0.0.5", 5, 1),       # gateway with ARP, interface 5 has no MAC
]
ARP = [("10.0.0.254", 1), ("10.0.0.1", 2), ("10.0.0.2", 3), ("10.0.0.3", 4), ("10.0.0.4", 5), ("10.0.0.5", 6),
       ("10.2.3.4", 7), ("10.1.2.7", 8), ("10.1.2.200", 9), ("192.168.77.5", 10), ("10.5.0.9", 11),
       ("10.2.3.4", 12),  # a duplicate: the last one wins
       ("10.200.1.1", 13), ("10.200.1.2", 14), ("10.77.0.1", 15)]
IF_MACS = [(1, 101), (2, 102), (3, 103), (4, 104)]
LOCAL_IPS = ["10.0.0.100", "10.1.2.1", "192.168.1.5"]
# destinations the frames draw from; the first rows forward
DSTS = ["10.2.3.4", "10.1.2.7", "10.1.2.200", "10.1.77.77", "172.16.5.5", "172.31.255.1", "192.168.77.5",
        "10.200.1.1", "10.200.1.2", "10.77.0.1", "10.1.2.129",
        "8.8.8.8", "203.0.113.9",                      # default route / no route
        "10.9.9.9", "192.168.9.77", "10.5.0.10",       # ARP misses (connected, gateway, on interface 5)
        "10.5.0.9", "10.6.1.1",                        # no interface MAC (connected, gateway)
        "10.0.0.100", "10.1.2.1", "192.168.1.5"]       # the switch's own
LENS = [13, 14, 17, 33, 34, 37, 38, 42, 60, 64]


def ipv4_frame(rng, dst, ttl, tagged, length):
    b = bytearray(rng.integers(0, 256, size=96, dtype=np.uint8).tobytes())
    b[12:14] = b"\x81\x00" if tagged else b"\x08\x00"
    l2 = 14
    if tagged:
        b[16:18] = b"\x08\x00"
        l2 = 18
    b[l2] = 0x45
    b[l2 + 8] = ttl
    b[l2 + 16: l2 + 20] = bytes(int(x) for x in dst.split("."))
    return bytes(b[:length])


def make_frames():
    rng = np.random.default_rng(SEED)
    frames = []
    # every destination x TTL {0, 1, 2, 64} x tagged / untagged, full headers
    for d in DSTS:
        for ttl in (0, 1, 2, 64):
            for tagged in (False, True):
                frames.append(ipv4_frame(rng, d, ttl, tagged, 64))
    # every edge length x tagged / untagged, forwarding destinations
    for ln in LENS:
        for tagged in (False, True):
            for d in DSTS[:4]:
                frames.append(ipv4_frame(rng, d, 64, tagged, ln))
    # other EtherTypes: ARP, IPv6, a tag around ARP, a double tag
    for et in (b"\x08\x06", b"\x86\xdd"):
        f = bytearray(ipv4_frame(rng, DSTS[0], 64, False, 64))
        f[12:14] = et
        frames.append(bytes(f))
        f = bytearray(ipv4_frame(rng, DSTS[0], 64, True, 64))
        f[16:18] = et
        frames.append(bytes(f))
    f = bytearray(ipv4_frame(rng, DSTS[0], 64, True, 64))
    f[16:18] = b"\x81\x00"
    frames.append(bytes(f))
    # random draws: destinations weighted towards the forwarding ones, TTL mostly alive
    for _ in range(360):
        d = DSTS[int(rng.integers(0, 11))] if rng.random() < 0.6 else DSTS[int(rng.integers(0, len(DSTS)))]
        ttl = int(rng.choice([0, 1, 2, 3, 64, 255], p=[0.05, 0.05, 0.2, 0.2, 0.4, 0.1]))
        frames.append(ipv4_frame(rng, d, ttl, bool(rng.random() < 0.4), int(rng.choice(LENS[6:]))))
    # the oracle's fuzz frames (IPv4 / IPv6 / tags / options / junk), truncated
    frames += [f[:FRAME_CAP] for f in oracle.fuzz_frames(SEED, 0, 200)]
    return frames


def pack_inputs(routes, frames):
    out = [struct.pack("<I", len(routes))]
    for net, mask, nh, ifid, metric in routes:
        out.append(struct.pack("<IIIIi", ip(net), ip(mask), ip(nh), ifid, metric))
    out.append(struct.pack("<I", len(ARP)))
    for a, k in ARP:
        out.append(struct.pack("<I", ip(a)) + mac(k) + b"\0\0")
    out.append(struct.pack("<I", len(IF_MACS)))
    for i, k in IF_MACS:
        out.append(struct.pack("<I", i) + mac(k) + b"\0\0")
    out.append(struct.pack("<I", len(LOCAL_IPS)))
    for a in LOCAL_IPS:
        out.append(struct.pack("<I", ip(a)))
    out.append(struct.pack("<I", len(frames)))
    for f in frames:
        out.append(struct.pack("<I", len(f)) + f)
    return b"".join(out)


def run_probe(routes, frames):
    res = subprocess.run([PROBE], input=pack_inputs(routes, frames), stdout=subprocess.PIPE, check=True).stdout
    nt = struct.unpack_from("<I", res, 0)[0]
    table = np.frombuffer(res, dtype="<u4", count=5 * nt, offset=4).reshape(nt, 5).copy()
    rec = np.frombuffer(res, dtype=np.dtype([("verdict", "<u4"), ("egress_if", "<u4"), ("macs", "u1", (12,))]),
                        count=len(frames), offset=4 + 20 * nt)
    assert 4 + 20 * nt + 20 * len(frames) == len(res)
    return table, rec


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "route_probe.cpp"),
                    os.path.join(ref_root, "src", "netflow++", "routing_manager.cpp"), "-o", PROBE], check=True)
    frames = make_frames()
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    data = np.zeros((len(frames), FRAME_CAP), dtype=np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    out = {"seed": np.uint64(SEED), "lens": lens, "frames": data,
           "arp_ip": np.array([ip(a) for a, _ in ARP], dtype=np.uint32),
           "arp_mac": np.array([list(mac(k)) for _, k in ARP], dtype=np.uint8),
           "if_id": np.array([i for i, _ in IF_MACS], dtype=np.uint32),
           "if_mac": np.array([list(mac(k)) for _, k in IF_MACS], dtype=np.uint8),
           "local_ip": np.array([ip(a) for a in LOCAL_IPS], dtype=np.uint32)}
    seen = set()
    for name, routes in (("a", ROUTES), ("b", ROUTES[:0:-1])):  # b: no default route, reversed input order
        table, rec = run_probe(routes, frames)
        assert len(table) == len(routes)
        share = float((rec["verdict"] == FORWARD).mean())
        assert share >= 0.25, (name, share)
        seen |= set(int(v) for v in rec["verdict"])
        out["routes_" + name] = table  # get_routing_table() order: {network, mask, next_hop, if, metric}
        out["verdict_" + name] = rec["verdict"].astype(np.uint8)
        out["egress_" + name] = rec["egress_if"].copy()
        out["macs_" + name] = rec["macs"].copy()
        print(f"table {name}: {len(table)} routes, {len(frames)} frames, forward share {share:.3f}, verdicts "
              + " ".join(f"{v}:{int((rec['verdict'] == v).sum())}" for v in sorted(set(rec['verdict']))))
    assert seen == {FORWARD, NOT_IPV4, LOCAL, TTL_EXPIRED, NO_ROUTE, ARP_MISS, NO_IF_MAC}, seen
    path = os.path.join(HERE, "route_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

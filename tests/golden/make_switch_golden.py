"""Generate tests/golden/switch_ref.npz from the REFERENCE implementation.

Compiles tests/golden/switch_probe.cpp against the reference's headers in place plus every file of its
src/netflow++/ (not the isis/ directory) into oracle/_ref/switch_probe (git-ignored), -O0 as the reference's own
build. The probe constructs a real netflow::Switch, configures it through its managers' setters and feeds three
bursts through Switch::process_received_packet, each followed by every port's TX loop
(QosManager::select_packet_to_dequeue up to a budget). It runs in an empty temporary directory and writes to a
file. The fixture keeps every frame fed, the tables as the reference's accessors report them, and per burst what
the reference left: per port the dequeued packets in order, every queue's counters, the interface counters.

The switch, 8 ports:
  0  ACCESS 10, 4 queues strict, ingress list 0                        burst 0 arrives here
  1  TRUNK {10,20,30} native 10 untagged, 8 queues WRR, ingress list 1, egress list 10      burst 1
  2  TRUNK {10,20} native 10 tag_native, 3 queues DRR of depth 6, egress list 10            burst 2 (no ingress ACL)
  3  ACCESS 20, 4 queues strict of depth 5
  4  ACCESS 10, 1 queue, egress list 11
  5  link down, ACCESS 10, 4 queues
  6  no VLAN config, STP blocking, 8 queues, egress list 12 (denies everything)
  7  TRUNK {10,30} native 30, no QoS config
Routes: connected networks on every port and on interface 11, which was never configured (no MAC); gateways with
an ARP entry on 1, 2, 3, 6, 7 and one without on 4; no default route.

Every frame carries its index over all bursts in its last four bytes (little-endian): the probe reads it from the
packets it dequeues, flood copies included. Payloads are one repeated byte, checksums arrive as zero and header
fields come from small pools, so that the file compresses; a dequeued packet is stored as its XOR with the frame
it came from (with bytes 12..15 removed where it is four bytes shorter), which is zero but for the bytes the
switch rewrote and is undone by tests/switch_common.py.

The script asserts, on the reference's output alone, the class counts of check_classes().

    python tests/golden/make_switch_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import glob
import io
import os
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import oracle  # noqa: E402
from make_acl_golden import DENY, NONE, PERMIT, REDIRECT, RULE, rule_record  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "switch_probe")
SEED = 20281
NUM_PORTS = 8
Q = 8
ACCESS, TRUNK = 0, 1
STRICT, WRR, DRR = 0, 1, 2
(C_UNHANDLED, C_RX_DOWN, C_IN_DENY, C_RED_OK, C_RED_DOWN, C_RED_RANGE, C_LLDP, C_ZERO_MAC, C_ARP, C_LOCAL, C_TTL,
 C_NO_ROUTE, C_ARP_MISS, C_NO_IF_MAC, C_L3_FWD, C_L2_FWD, C_L2_FLOOD, C_SAME_PORT, C_LINK_DOWN, C_STP, C_VLAN) = range(21)
EV_ENQ, EV_FULL, EV_EDENY = 0, 1, 2
BURSTS = ((0, 1100), (1, 800), (2, 750))  # (ingress port, frames): the first crosses the enqueue's tile of 1,024
BUDGETS = ([60] * 8, [60] * 8, [100000] * 8)
MIN_CLASS = 10


def ip4(s):
    """Dotted quad -> the u32 a little-endian load of its network-order bytes gives (the reference's IpAddress)."""
    return struct.unpack("<I", bytes(int(x) for x in s.split(".")))[0]


def hip(s):
    """Dotted quad -> the host-order u32 AclRule holds."""
    return int.from_bytes(bytes(int(x) for x in s.split(".")), "big")


def mac(k):
    return bytes([0x02, 0x5C, 0, 0, k >> 8, k & 0xFF])


# (id, link_up, stp_forwarding, mac, addresses)
INTERFACES = [(p, 0 if p == 5 else 1, 0 if p == 6 else 1, mac(0x100 + p), [] if p == 6 else ["10.0.%d.1" % p])
              for p in range(NUM_PORTS)]
# (id, type, tag_native, native, allowed)
VLANS = [(0, ACCESS, 0, 10, [10]), (1, TRUNK, 0, 10, [10, 20, 30]), (2, TRUNK, 1, 10, [10, 20]), (3, ACCESS, 0, 20, [20]),
         (4, ACCESS, 0, 10, [10]), (5, ACCESS, 0, 10, [10]), (7, TRUNK, 0, 30, [10, 30])]
# (id, queues, scheduler, depth)
QOS = [(0, 4, STRICT, 1000), (1, 8, WRR, 1000), (2, 3, DRR, 6), (3, 4, STRICT, 5), (4, 1, STRICT, 1000),
       (5, 4, STRICT, 1000), (6, 8, STRICT, 1000)]
ROUTES = [("10.0.%d.0" % p, "255.255.255.0", "0.0.0.0", p) for p in range(NUM_PORTS)] + [
    ("172.16.0.0", "255.255.0.0", "10.0.1.2", 1), ("172.17.0.0", "255.255.0.0", "10.0.3.2", 3),
    ("172.18.0.0", "255.255.0.0", "10.0.4.99", 4), ("172.19.0.0", "255.255.0.0", "10.0.2.2", 2),
    ("172.20.0.0", "255.255.0.0", "10.0.7.2", 7), ("172.21.0.0", "255.255.0.0", "10.0.6.2", 6),
    ("10.9.0.0", "255.255.255.0", "0.0.0.0", 11)]
ARP = [("10.0.%d.%d" % (p, h), mac(0x200 + 16 * p + h)) for p in range(NUM_PORTS) for h in (10, 11)] + [
    ("10.0.1.2", mac(0x301)), ("10.0.3.2", mac(0x303)), ("10.0.2.2", mac(0x302)), ("10.0.7.2", mac(0x307)),
    ("10.0.6.2", mac(0x306)), ("10.9.0.10", mac(0x309)),
    ("10.0.1.2", mac(0x3F1))]  # again: the later entry replaces the earlier
# destinations: (address, weight)
DST_FWD = ["10.0.%d.%d" % (p, h) for p in range(NUM_PORTS) for h in (10, 11)] + [
    "172.16.3.3", "172.17.1.9", "172.19.0.5", "172.20.8.8", "172.21.4.4", "172.16.200.1"]
DST_LOCAL = ["10.0.0.1", "10.0.3.1", "10.0.7.1"]
DST_NO_ROUTE = ["8.8.8.8", "192.168.1.1"]
DST_ARP_MISS = ["10.0.2.77", "172.18.5.5"]
DST_NO_IF_MAC = ["10.9.0.10"]
SRC_IPS = ["10.0.0.20", "10.0.1.20", "10.0.2.20", "172.16.9.9", "10.0.0.66", "10.0.1.66"]  # .66: denied at ingress
SRC_MACS = [mac(0x400 + k) for k in range(6)]
L4_PORTS = [80, 53, 443, 1234, 8080, 7004, 7005, 7006, 7009, 7103, 7105, 7106, 7108, 9999]
ET_L2, ET_L2_DENY, ET_L2_REDIRECT = 0x88B5, 0x88B6, 0x88B7
# the FDB: (kind 0 learn / 1 static, mac, vlan, port)
DMAC = [mac(0x500 + k) for k in range(20)]
FDB = [(0, DMAC[0], 10, 1), (1, DMAC[1], 10, 2), (0, DMAC[2], 10, 4), (0, DMAC[3], 20, 3), (1, DMAC[4], 20, 1),
       (0, DMAC[5], 10, 0), (0, DMAC[6], 10, 5), (0, DMAC[7], 10, 6), (0, DMAC[8], 10, 3), (0, DMAC[9], 20, 2),
       (0, DMAC[10], 10, 7), (0, DMAC[11], 20, 4), (1, DMAC[12], 30, 1), (0, DMAC[13], 30, 7), (0, DMAC[14], 10, 2),
       (0, DMAC[5], 20, 1), (0, DMAC[0], 20, 2), (0, DMAC[15], 10, 1)]
UNKNOWN = [mac(0x600 + k) for k in range(3)] + [b"\xff" * 6, bytes([0x01, 0x00, 0x5E, 0, 0, 9])]
# the ACLs: (rule id, action, redirect port or None, {field: value}), priority = position (all compiled)
LISTS = {
    0: [(1, DENY, None, dict(src_ip=hip("10.0.0.66"))),
        (2, DENY, None, dict(ethertype=ET_L2_DENY)),
        (3, REDIRECT, 6, dict(dst_port=7006)),
        (4, REDIRECT, 4, dict(ethertype=ET_L2_REDIRECT)),
        (5, REDIRECT, 5, dict(dst_port=7005)),
        (6, REDIRECT, 9, dict(dst_port=7009)),
        (7, REDIRECT, 4, dict(dst_port=7004)),
        (8, PERMIT, None, dict(protocol=1))],
    1: [(1, DENY, None, dict(protocol=17, dst_port=9999)),
        (2, DENY, None, dict(vlan_id=30, ethertype=ET_L2)),
        (3, DENY, None, dict(src_mac=SRC_MACS[5])),
        (4, REDIRECT, 6, dict(dst_port=7106)),
        (5, REDIRECT, 3, dict(dst_port=7103)),
        (6, REDIRECT, 2, dict(ethertype=ET_L2_REDIRECT)),
        (7, REDIRECT, 5, dict(dst_port=7105)),
        (8, REDIRECT, 8, dict(dst_port=7108)),
        (9, REDIRECT, None, dict(src_ip=hip("10.0.1.66")))],  # REDIRECT without a port decides DENY
    10: [(1, DENY, None, dict(vlan_id=10)),  # port 1 pops VLAN 10 before its list sees the frame, port 2 does not
         (2, DENY, None, dict(dst_port=80)),
         (3, REDIRECT, 4, dict(protocol=1)),
         (4, DENY, None, dict(src_mac=SRC_MACS[3]))],
    11: [(1, DENY, None, dict(protocol=17, dst_port=53)),
         (2, REDIRECT, 2, dict(ethertype=ET_L2)),
         (3, DENY, None, dict(vlan_id=20)),
         (4, DENY, None, dict(dst_mac=UNKNOWN[1]))],
    12: [(1, DENY, None, dict())],
}
BINDS = [(0, 0, 0), (1, 0, 1), (1, 1, 10), (2, 1, 10), (4, 1, 11), (6, 1, 12)]  # (port, 0 ingress / 1 egress, list)


def ip_frame(rng, index, dst, length, tagged):
    proto = int(rng.choice([6, 17, 1]))
    ihl = int(rng.choice([5, 5, 5, 5, 6, 8]))
    ttl = 64
    src = SRC_IPS[int(rng.choice(len(SRC_IPS), p=[0.3, 0.25, 0.2, 0.15, 0.05, 0.05]))]
    l4_len = {6: 20, 17: 8, 1: 8}[proto]
    l2 = 18 if tagged else 14
    length = max(length, l2 + ihl * 4 + l4_len + 4)
    ip = struct.pack(">BBHHHBBH", 0x40 | ihl, 0, length - l2, 0, 0, ttl, proto, 0) + struct.pack("<II", ip4(src), ip4(dst))
    ip += bytes([1] * (ihl * 4 - 20))  # options: no-ops
    sport, dport = 1024, int(rng.choice(L4_PORTS))
    if proto == 6:
        l4 = struct.pack(">HHIIBBHHH", sport, dport, 0, 0, 0x50, 0x10, 512, 0, 0)
    elif proto == 17:
        l4 = struct.pack(">HHHH", sport, dport, length - l2 - ihl * 4, 0)
    else:
        l4 = struct.pack(">BBHHH", 8, 0, 0, 1, 1)
    eth = mac(0x100) + SRC_MACS[int(rng.integers(0, len(SRC_MACS)))]
    if tagged:
        eth += b"\x81\x00" + struct.pack(">H", int(rng.choice([10, 10, 20, 30])) | (int(rng.integers(0, 8)) << 13))
    head = eth + b"\x08\x00" + ip + l4
    fill = bytes([int(rng.choice([0x11, 0x22, 0x44, 0x88]))])
    return bytearray(head + fill * (length - len(head) - 4) + struct.pack("<I", index))


def l2_frame(rng, index, dmac, ethertype, length, tagged):
    eth = dmac + SRC_MACS[int(rng.integers(0, len(SRC_MACS)))]
    if tagged:
        eth += b"\x81\x00" + struct.pack(">H", int(rng.choice([10, 10, 10, 20, 20, 30])) | (int(rng.integers(0, 8)) << 13))
    head = eth + struct.pack(">H", ethertype)
    fill = bytes([int(rng.choice([0x11, 0x22, 0x44, 0x88]))])
    return bytearray(head + fill * (max(length, len(head) + 4) - len(head) - 4) + struct.pack("<I", index))


def make_burst(rng, first, n):
    out = []
    long_at = set(int(x) for x in rng.choice(n, size=8, replace=False))
    for k in range(n):
        index = first + k
        length = int(rng.integers(60, 301))
        tagged = bool(rng.random() < 0.4)
        if k in long_at:
            length, tagged = int(rng.integers(1400, 1519)), True
        r = rng.random() * (0.89 if k in long_at else 1.0)  # a long frame is an IPv4 or an L2 data frame
        if r < 0.50 or (k in long_at and r < 0.8):
            kind = rng.random()
            dst = DST_FWD[int(rng.integers(0, len(DST_FWD)))]
            if kind > 0.80:
                pool = (DST_LOCAL, DST_NO_ROUTE, DST_ARP_MISS, DST_NO_IF_MAC, None)[int(rng.integers(0, 5))]
                if pool is not None:
                    dst = pool[int(rng.integers(0, len(pool)))]
            f = ip_frame(rng, index, dst, length, tagged)
            if kind > 0.80 and pool is None:
                f[(18 if tagged else 14) + 8] = int(rng.integers(0, 2))  # TTL 0 / 1
            if 0.78 < kind <= 0.80:
                f[0:6] = bytes(6)  # the all-zero destination MAC on an IPv4 frame
        elif r < 0.90:
            pool = DMAC[:16] if rng.random() < 0.6 else UNKNOWN
            et = int(rng.choice([ET_L2] * 7 + [ET_L2_DENY, ET_L2_REDIRECT, 0x86DD]))
            f = l2_frame(rng, index, pool[int(rng.integers(0, len(pool)))], et, length, tagged)
        else:
            kind = int(rng.integers(0, 5))
            if kind == 0:
                f = l2_frame(rng, index, b"\xff" * 6, 0x0806, 60, tagged)   # ARP, tagged too
            elif kind == 1:
                f = l2_frame(rng, index, bytes([1, 0x80, 0xC2, 0, 0, 0x0E]), 0x88CC, length, False)  # LLDP
            elif kind == 2:
                f = l2_frame(rng, index, bytes(6), ET_L2, length, tagged)   # the all-zero destination MAC
            elif kind == 3:
                f = l2_frame(rng, index, DMAC[int(rng.integers(0, 4))], 0x86DD, length, tagged)  # IPv6: an L2 frame
            else:
                f = bytearray(b"\x02\x5c\x00\x00\x05\x00" + struct.pack("<I", index))  # a 10-byte runt
        assert struct.unpack("<I", bytes(f[-4:]))[0] == index
        out.append(bytes(f))
    return out


def list_records(specs):
    n = len(specs)
    return np.array([rule_record(s, n - k) for k, s in enumerate(specs)]) if n else np.zeros(0, RULE)


def run_probe(bursts):
    inp = [struct.pack("<I", NUM_PORTS), struct.pack("<I", len(INTERFACES))]
    for pid, up, stp, m, ips in INTERFACES:
        inp.append(struct.pack("<IBB2x6s2xI", pid, up, stp, m, len(ips)) + b"".join(struct.pack("<I", ip4(a)) for a in ips))
    inp.append(struct.pack("<I", len(VLANS)))
    for pid, typ, tagn, native, allowed in VLANS:
        inp.append(struct.pack("<IBBHI", pid, typ, tagn, native, len(allowed)) +
                   b"".join(struct.pack("<H", v) for v in allowed) + (b"\0\0" if len(allowed) & 1 else b""))
    inp.append(struct.pack("<I", len(QOS)) + b"".join(struct.pack("<IBB2xI", p, nq, s, d) for p, nq, s, d in QOS))
    inp.append(struct.pack("<I", len(ROUTES)) +
               b"".join(struct.pack("<IIII", ip4(a), ip4(b), ip4(c), d) for a, b, c, d in ROUTES))
    inp.append(struct.pack("<I", len(ARP)) + b"".join(struct.pack("<I6s2x", ip4(a), m) for a, m in ARP))
    inp.append(struct.pack("<I", len(FDB)) + b"".join(struct.pack("<Bx6sH2xI", k, m, v, p) for k, m, v, p in FDB))
    inp.append(struct.pack("<I", len(LISTS)))
    for lid, specs in LISTS.items():
        inp.append(struct.pack("<II", lid, len(specs)) + list_records(specs).tobytes())
    inp.append(struct.pack("<I", len(BINDS)) + b"".join(struct.pack("<III", *b) for b in BINDS))
    inp.append(struct.pack("<I", len(bursts)))
    for (ingress, _), budget, frames in zip(BURSTS, BUDGETS, bursts):
        inp.append(struct.pack("<II", ingress, len(frames)) + struct.pack("<%dI" % NUM_PORTS, *budget))
        inp += [struct.pack("<I", len(f)) + f for f in frames]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.bin")
        subprocess.run([PROBE, path], input=b"".join(inp), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True,
                       cwd=tmp)
        res = open(path, "rb").read()
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from(fmt, res, pos)
        pos += struct.calcsize(fmt)
        return v

    def take_array(dtype, count):
        nonlocal pos
        a = np.frombuffer(res, dtype, count, pos).copy()
        pos += a.nbytes
        return a

    t = {"ifs": [], "vlan": [], "qos": [], "lists": {}}
    for _ in range(take("<I")[0]):
        pid, up, stp, m, lin, leg, nip = take("<IBB2x6s2xIII")
        t["ifs"].append((pid, up, stp, m, lin, leg, [take("<I")[0] for _ in range(nip)]))
    for _ in range(NUM_PORTS):
        has, typ, tagn, native, na = take("<BBBxHH")
        t["vlan"].append((has, typ, tagn, native, [take("<H")[0] for _ in range(na)]))
        if na & 1:
            take("<H")
    for _ in range(NUM_PORTS):
        t["qos"].append(take("<BBBxI"))
    t["routes"] = [take("<IIII") for _ in range(take("<I")[0])]
    t["arp"] = [take("<I6s2x") for _ in range(take("<I")[0])]
    t["fdb"] = take_array(np.uint8, 16 * take("<I")[0]).reshape(-1, 16)
    for _ in LISTS:
        lid, nt = take("<II")
        t["lists"][lid] = take_array(RULE, nt)
    out = []
    for frames in bursts:
        per, events = [], []
        for _ in frames:
            code, port, v4, ega, ne = take("<IIIII")
            per.append((code, port, v4, ega))
            events.append(take_array("<u4", ne))
        tx = []
        for _ in range(NUM_PORTS):
            pkts = []
            for _ in range(take("<I")[0]):
                src, ln = take("<II")
                pkts.append((src, res[pos:pos + ln]))
                pos += ln
            tx.append(pkts)
        stats = take_array("<u4", NUM_PORTS * Q * 3).reshape(NUM_PORTS, Q, 3)
        port_stats = take_array("<u8", NUM_PORTS * 6).reshape(NUM_PORTS, 6)
        out.append({"per": np.array(per, np.uint32).reshape(-1, 4), "events": events, "tx": tx, "stats": stats,
                    "port_stats": port_stats})
    assert pos == len(res)
    return t, out


def ragged(items, width=1):
    start = np.zeros(len(items) + 1, np.uint32)
    start[1:] = np.cumsum([len(x) // width for x in items])
    return start, np.frombuffer(b"".join(bytes(x) for x in items), np.uint8).copy()


def popped(f):
    return f[:12] + f[16:]


def tx_delta(src_frame, sent):
    """sent XOR the frame it came from (bytes 12..15 removed where sent is four bytes shorter)."""
    base = src_frame if len(sent) == len(src_frame) else popped(src_frame)
    assert len(base) == len(sent), (len(src_frame), len(sent))
    return (np.frombuffer(base, np.uint8) ^ np.frombuffer(sent, np.uint8)).tobytes()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that the file regenerates bit for bit."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def class_masks(z):
    """{class name: boolean mask over all frames} from the fixture's arrays: the reference's per-frame code, its
    counters' events and its TX record, plus what the fed frames themselves say (IPv4 protocol, tag, length). Shared
    with tests/switch_common.py, which asserts the same counts on the loaded file."""
    n = len(z["code"])
    code, v4, ega = z["code"], z["is_v4"].astype(bool), z["eg_action"]
    fs, fb = z["frame_start"], z["frame_bytes"]
    frames = [bytes(fb[int(fs[i]):int(fs[i + 1])]) for i in range(n)]
    tagged = np.array([len(f) >= 18 and f[12:14] == b"\x81\x00" for f in frames])
    l2 = np.where(tagged, 18, 14)
    proto = np.array([f[o + 9] if v else 0 for f, o, v in zip(frames, l2, v4)])
    ihl = np.array([f[o] & 15 if v else 0 for f, o, v in zip(frames, l2, v4)])
    es, ev = z["ev_start"], z["ev"]
    kinds = [ev[int(es[i]):int(es[i + 1])] >> 16 for i in range(n)]
    n_ev = np.array([len(k) for k in kinds])
    enq, full, edeny = (np.array([int((k == x).sum()) for k in kinds]) for x in (EV_ENQ, EV_FULL, EV_EDENY))
    sent_short = np.zeros(n, int)  # TX packets four bytes shorter than their frame
    lens = np.diff(fs.astype(np.int64))
    for b in range(len(z["ingress"])):
        src, ln = z[f"tx_src_{b}"].astype(np.int64), z[f"tx_len_{b}"].astype(np.int64)
        np.add.at(sent_short, src[ln == lens[src] - 4], 1)
    fwd = code == C_L3_FWD
    m = {"l3 forwarded": fwd & (enq == 1)}
    for name, p in (("tcp", 6), ("udp", 17), ("icmp", 1)):
        m[f"l3 forwarded {name} untagged"] = fwd & (enq == 1) & (proto == p) & ~tagged
        m[f"l3 forwarded {name} tagged"] = fwd & (enq == 1) & (proto == p) & tagged
    m["l3 forwarded with options"] = fwd & (enq == 1) & (ihl > 5)
    m["l3 forwarded, tag popped"] = fwd & (sent_short == 1)
    m["l3 egress deny"] = fwd & (edeny == 1)
    m["l3 egress redirect permitted"] = fwd & (ega == REDIRECT) & (enq == 1)
    m["ingress deny l3"] = (code == C_IN_DENY) & v4
    m["ingress deny l2"] = (code == C_IN_DENY) & ~v4 & (lens >= 14)
    m["ingress redirect"] = (code == C_RED_OK) & (enq == 1)
    m["ingress redirect, tag popped"] = (code == C_RED_OK) & (sent_short == 1)
    m["ingress redirect past a denying egress list"] = (code == C_RED_OK) & (ega == DENY) & (enq == 1)
    m["ingress redirect to a down port"] = code == C_RED_DOWN
    m["ingress redirect past num_ports"] = code == C_RED_RANGE
    for name, c in (("local", C_LOCAL), ("ttl", C_TTL), ("no route", C_NO_ROUTE), ("arp miss", C_ARP_MISS),
                    ("no interface mac", C_NO_IF_MAC), ("drop same port", C_SAME_PORT),
                    ("drop link down", C_LINK_DOWN), ("drop stp", C_STP), ("drop vlan", C_VLAN), ("arp", C_ARP),
                    ("lldp", C_LLDP), ("zero mac", C_ZERO_MAC)):
        m[name] = code == c
    m["l2 forward"] = (code == C_L2_FWD) & (enq == 1)
    flood = code == C_L2_FLOOD
    m["flood fan-out >= 2"] = flood & (n_ev >= 2)
    m["flood, one copy denied and one popped"] = flood & (edeny >= 1) & (sent_short >= 1)
    unicast = fwd | (code == C_L2_FWD) | (code == C_RED_OK)
    m["tail drop of a forwarded packet"] = unicast & (full == 1)
    m["l2 egress deny"] = (code == C_L2_FWD) & (edeny == 1)
    m["unicast to a port without a QoS config"] = unicast & (n_ev == 0)
    m["flood fan-out < 2"] = flood & (n_ev < 2)
    m["tail drop of a flood copy"] = flood & (full >= 1)
    m["ipv6"] = np.array([len(f) >= 14 and (f[16:18] if t else f[12:14]) == b"\x86\xdd" for f, t in zip(frames, tagged)])
    m["runt"] = lens == 10
    m["long tagged frame popped"] = (lens >= 1400) & tagged & (sent_short >= 1)
    return m


def check_classes(z, report=None):
    for name, mask in class_masks(z).items():
        count = int(mask.sum())
        if report:
            report(f"  {name}: {count}")
        need = 3 if name == "long tagged frame popped" else MIN_CLASS
        assert count >= need, (name, count)
    # nothing is sent for these: the ICMP call sites at switch.hpp:271/279/301 are comments
    quiet = np.isin(z["code"], [C_LOCAL, C_TTL, C_NO_ROUTE, C_ARP_MISS, C_NO_IF_MAC, C_ARP, C_LLDP, C_ZERO_MAC, C_IN_DENY,
                                C_RED_DOWN, C_RED_RANGE, C_UNHANDLED, C_SAME_PORT, C_LINK_DOWN, C_STP, C_VLAN])
    assert (np.diff(z["ev_start"].astype(np.int64))[quiet] == 0).all()


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(ref_root, "src", "netflow++", "*.cpp")))
    subprocess.run(["g++", "-std=c++17", "-O0", "-w", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "switch_probe.cpp"), *srcs, "-o", PROBE, "-lpthread"], check=True)
    rng = np.random.default_rng(SEED)
    bursts, first = [], 0
    for _, n in BURSTS:
        bursts.append(make_burst(rng, first, n))
        first += n
    frames = [f for b in bursts for f in b]
    t, res = run_probe(bursts)

    out = {"seed": np.uint64(SEED), "num_ports": np.uint32(NUM_PORTS),
           "ingress": np.array([b[0] for b in BURSTS], np.uint32), "budget": np.array(BUDGETS, np.uint32),
           "burst_start": np.cumsum([0] + [len(b) for b in bursts]).astype(np.uint32)}
    out["frame_start"], out["frame_bytes"] = ragged(frames)
    out["if_id"] = np.array([i[0] for i in t["ifs"]], np.uint32)
    out["if_up"] = np.array([i[1] for i in t["ifs"]], np.uint8)
    out["if_stp"] = np.array([i[2] for i in t["ifs"]], np.uint8)
    out["if_mac"] = np.frombuffer(b"".join(i[3] for i in t["ifs"]), np.uint8).reshape(-1, 6).copy()
    out["if_in_list"] = np.array([i[4] for i in t["ifs"]], np.uint32)
    out["if_eg_list"] = np.array([i[5] for i in t["ifs"]], np.uint32)
    out["if_ip_start"], ips = ragged([np.array(i[6], "<u4").tobytes() for i in t["ifs"]], 4)
    out["if_ips"] = ips.view("<u4").copy()
    out["vlan"] = np.array([v[:4] for v in t["vlan"]], np.uint16)  # has, type, tag_native, native per port
    out["allowed_start"], allowed = ragged([np.array(v[4], "<u2").tobytes() for v in t["vlan"]], 2)
    out["allowed"] = allowed.view("<u2").copy()
    out["qos"] = np.array(t["qos"], np.uint32)  # has, num_queues, scheduler, max_queue_depth per port
    out["routes"] = np.array(t["routes"], np.uint32).reshape(-1, 4)
    out["arp_ip"] = np.array([a[0] for a in t["arp"]], np.uint32)
    out["arp_mac"] = np.frombuffer(b"".join(a[1] for a in t["arp"]), np.uint8).reshape(-1, 6).copy()
    out["fdb"] = t["fdb"]
    out["list_ids"] = np.array(sorted(t["lists"]), np.uint32)
    for lid, table in t["lists"].items():
        sent = list_records(LISTS[lid])
        assert sorted(table["rule_id"].tolist()) == sorted(sent["rule_id"].tolist()), lid
        table = table.copy()
        table["src_ip_mask"] = table["dst_ip_mask"] = 0xFFFFFFFF  # the reference matches addresses exactly
        out[f"rules_{lid}"] = np.frombuffer(table.tobytes(), np.uint8).reshape(len(table), RULE.itemsize)[:, :52].copy()
    # the tables are what was configured
    assert sorted(tuple(x) for x in out["routes"].tolist()) == sorted((ip4(a), ip4(b), ip4(c), d) for a, b, c, d in ROUTES)
    assert dict(zip(out["arp_ip"].tolist(), [bytes(m) for m in out["arp_mac"]]))[ip4("10.0.1.2")] == mac(0x3F1)
    assert out["if_up"].tolist() == [i[1] for i in INTERFACES] and out["if_stp"].tolist() == [i[2] for i in INTERFACES]
    assert len(out["fdb"]) == len(FDB)

    per = np.concatenate([r["per"] for r in res])
    out["code"], out["port"] = per[:, 0].astype(np.uint8), per[:, 1].astype(np.uint32)
    out["is_v4"], out["eg_action"] = per[:, 2].astype(np.uint8), per[:, 3].astype(np.uint8)  # 255: no list / not unicast
    out["ev_start"], ev = ragged([e.tobytes() for r in res for e in r["events"]], 4)
    out["ev"] = ev.view("<u4").copy()
    for b, r in enumerate(res):
        flat = [p for pkts in r["tx"] for p in pkts]
        out[f"tx_start_{b}"] = np.cumsum([0] + [len(pkts) for pkts in r["tx"]]).astype(np.uint32)
        out[f"tx_src_{b}"] = np.array([s for s, _ in flat], np.uint32)
        out[f"tx_len_{b}"] = np.array([len(d) for _, d in flat], np.uint32)
        assert all(s < len(frames) for s, _ in flat)
        out[f"tx_delta_{b}"] = np.frombuffer(b"".join(tx_delta(frames[s], d) for s, d in flat), np.uint8).copy()
        out[f"stats_{b}"], out[f"port_stats_{b}"] = r["stats"], r["port_stats"]
        depth = np.where(r["stats"][:, :, 2] == NONE, 0, r["stats"][:, :, 2])
        print(f"burst {b}: {len(flat)} packets sent, {int(depth.sum())} left queued, "
              f"{int(np.where(r['stats'][:, :, 1] == NONE, 0, r['stats'][:, :, 1]).sum())} tail drops so far")
        if b < len(res) - 1:
            assert depth.sum() > 100, "bursts 0 and 1 leave packets queued"
        else:
            assert depth.sum() == 0, "burst 2 drains everything"
    # every enqueue the counters saw is sent in the end, and nothing else
    kinds = out["ev"] >> 16
    assert int((kinds == EV_ENQ).sum()) == sum(len(out[f"tx_src_{b}"]) for b in range(len(res)))
    print("classes (frames):")
    check_classes(out, print)
    path = os.path.join(HERE, "switch_ref.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes,", len(frames), "frames")
    assert os.path.getsize(path) < 100 * 1000


if __name__ == "__main__":
    main()

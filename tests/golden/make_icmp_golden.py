"""Generate tests/golden/icmp_ref.npz from the REFERENCE implementation.

Compiles tests/golden/icmp_probe.cpp against the reference's headers in place plus every file of its
src/netflow++/ (not the isis/ directory) into oracle/_ref/icmp_probe (git-ignored), -O0 as the reference's own
build (its byte_swap.hpp does not compile against glibc's optimised htons macros). The probe constructs a real
netflow::Switch, drives its icmp_processor_ at the three call sites of process_received_packet and captures what
send_control_plane_packet lets through. It runs in an empty temporary directory and writes to a file.

The switch: 8 ports. Interfaces 0, 1 (two addresses), 4 up with addresses; 2 down; 3 up without an address; 9 up
with an address but >= num_ports; 5-7 as the constructor leaves them. Routes (no default route): connected
networks on 0, 1, 2, 3, 9 and on 11 (an interface that was never configured), gateways with and without an ARP
entry. One `extra local` address that the lookup calls local and no interface holds.

Frames:
  echo requests  payloads 0-1,600 odd and even, untagged and tagged, IHL 5 / 6 / 15 / 2, wrong checksum in the
                 request, total_length below ihl*4 + 8, total_length past the frame, fewer than 8 bytes at L4, type 8
                 code 1, type 0, local non-ICMP, the extra local address
  originals      TTL 0 / 1 and no-route destinations with 0, 3, 8 and 64 bytes behind the IP header, tagged and
                 untagged, options and IHL 2, from sources that hit every step of the resolve order, a route whose
                 interface is down and one whose interface id is >= num_ports
  a few frames of other verdicts
Run 0 feeds all of them with ingress port 0; run 1 feeds every fourth with ingress port 2, which is down.

The script checks, on the reference's output alone: every status value occurs except OVERFLOW, OOB and TOO_LONG
(this library's own) and SRC_NO_IF_MAC, which the reference cannot reach: get_interface_ip and get_interface_mac
both ask for the port's configuration, so the first already fails; emitted messages are at least a quarter of the
frames of each kind. The error messages' IPv4 ids (rand() behind a fixed srand) are read from bytes 18-19.

    python tests/golden/make_icmp_golden.py [reference root, default oracle.REFERENCE_ROOT]
"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402

PROBE = os.path.join(ROOT, "oracle", "_ref", "icmp_probe")
SEED = 20271
NUM_PORTS = 8
RUNS = ((0, 1), (2, 4))  # (ingress port, every k-th frame)
RT_LOCAL, RT_TTL, RT_NO_ROUTE = 3, 4, 5
(ST_NONE, ST_ECHO, ST_TIME, ST_UNREACH, ST_TO_CPU, ST_IGNORED, ST_NO_LOCAL_MAC, ST_SRC_NO_ROUTE, ST_SRC_NO_IF_IP,
 ST_SRC_ARP_MISS, ST_SRC_NO_IF_MAC, ST_PORT_DOWN, ST_OOB, ST_TOO_LONG, ST_OVERFLOW) = range(15)


def ip4(s):
    """Dotted quad -> the u32 a little-endian load of its network-order bytes gives (the reference's IpAddress)."""
    return struct.unpack("<I", bytes(int(x) for x in s.split(".")))[0]


def mac(k):
    return bytes([0x02, 0xA0 + (k >> 8), k & 0xFF, 0x5E, 0x10, 0x20 + (k & 7)])


# (id, link_up, mac, addresses)
INTERFACES = [
    (0, 1, mac(0), ["10.0.0.1"]),
    (1, 1, mac(1), ["10.0.1.1", "10.0.1.254"]),
    (2, 0, mac(2), ["10.0.2.1"]),
    (3, 1, mac(3), []),
    (4, 1, mac(4), ["10.0.4.1"]),
    (9, 1, mac(9), ["10.0.9.1"]),
]
# (network, mask, next hop, interface)
ROUTES = [
    ("10.0.0.0", "255.255.255.0", "0.0.0.0", 0),
    ("10.0.1.0", "255.255.255.0", "0.0.0.0", 1),
    ("10.0.2.0", "255.255.255.0", "0.0.0.0", 2),
    ("10.0.3.0", "255.255.255.0", "0.0.0.0", 3),
    ("10.0.9.0", "255.255.255.0", "0.0.0.0", 9),
    ("172.16.0.0", "255.255.0.0", "10.0.1.2", 1),
    ("172.17.0.0", "255.255.0.0", "10.0.1.99", 1),
    ("172.18.0.0", "255.255.0.0", "10.0.4.2", 4),
    ("10.0.5.0", "255.255.255.0", "0.0.0.0", 11),
]
ARP = [("10.0.0.%d" % k, mac(0x100 + k)) for k in range(10, 20)] + [
    ("10.0.1.2", mac(0x201)), ("10.0.1.10", mac(0x20A)), ("10.0.2.10", mac(0x30A)), ("10.0.3.10", mac(0x40A)),
    ("10.0.9.10", mac(0x50A)), ("10.0.4.2", mac(0x602)), ("10.0.5.10", mac(0x70A)),
    ("10.0.0.10", mac(0x1FF)),  # again: the later entry replaces the earlier
]
EXTRA_LOCAL = ["10.0.7.7"]
LOCAL_DST = ["10.0.0.1", "10.0.1.254", "10.0.4.1", "10.0.1.1"]
# sources of originals: reachable ones first
SRC_OK = ["10.0.0.10", "10.0.0.15", "172.16.5.5", "172.18.200.1", "10.0.1.10"]
SRC_BAD = ["203.0.113.9",   # no route
           "10.0.3.10",     # the route's interface has no address
           "10.0.5.10",     # the route's interface was never configured
           "10.0.0.200",    # connected, no ARP entry
           "172.17.1.1",    # the gateway has no ARP entry
           "10.0.2.10",     # the route's interface is down
           "10.0.9.10"]     # the route's interface id is >= num_ports
DST_NO_ROUTE = ["192.168.1.1", "8.8.8.8", "11.1.1.1"]
DST_ROUTED = ["172.16.9.9", "10.0.1.10", "192.168.1.1"]  # TTL is tested before the route


def ip_sum(h):
    s = sum(struct.unpack(">%dH" % (len(h) // 2), h))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def frame(rng, src, dst, proto, l4, ttl=64, tagged=False, ihl=5, total_length=None, bad_csum=False, smac=None):
    opts = bytes(rng.integers(0, 16, max(ihl - 5, 0) * 4, dtype=np.uint8))
    hdr_len = ihl * 4
    tl = hdr_len + len(l4) if total_length is None else total_length
    ip = bytearray(struct.pack(">BBHHHBBH", 0x40 | ihl, 0, tl & 0xFFFF, int(rng.integers(0, 65536)), 0, ttl, proto, 0)
                   + struct.pack("<II", ip4(src), ip4(dst)) + opts)
    if ihl >= 5:
        struct.pack_into(">H", ip, 10, ip_sum(bytes(ip)) ^ (0x5A5A if bad_csum else 0))
    eth = mac(0xF00) + (smac or mac(0x800 + int(rng.integers(0, 64))))
    eth += (b"\x81\x00" + struct.pack(">H", int(rng.integers(1, 4095)) | (int(rng.integers(0, 8)) << 13)) if tagged else b"")
    # IHL < 5: the "header" is its first ihl*4 bytes and L4 starts inside the 20 fixed bytes, which stay whole
    return eth + b"\x08\x00" + bytes(ip) + l4


def icmp_msg(rng, typ, code, payload_len, bad=False):
    # few distinct byte values, so that the fixture compresses
    payload = bytes(rng.integers(0, 8, payload_len, dtype=np.uint8) * 17)
    m = bytearray(struct.pack(">BBHHH", typ, code, 0, int(rng.integers(0, 65536)), int(rng.integers(0, 65536))) + payload)
    c = ip_sum(bytes(m) + (b"\0" if len(m) & 1 else b""))
    struct.pack_into(">H", m, 2, c ^ (0x1234 if bad else 0))
    return bytes(m)


def make_frames(rng):
    out = []
    pick = lambda a: a[int(rng.integers(0, len(a)))]  # noqa: E731
    sizes = [0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 56, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 512, 513,
             1023, 1024, 1025, 1471, 1472, 1473, 1599, 1600]
    for tagged in (False, True):
        for p in sizes:
            out.append(frame(rng, pick(SRC_OK), pick(LOCAL_DST), 1, icmp_msg(rng, 8, 0, p), tagged=tagged))
    for ihl in (6, 15, 2):
        for p in (0, 1, 18, 33, 64, 201):
            for tagged in (False, True):
                out.append(frame(rng, pick(SRC_OK), pick(LOCAL_DST), 1, icmp_msg(rng, 8, 0, p), tagged=tagged, ihl=ihl))
    for k in range(40):
        p, tagged = int(rng.integers(0, 300)), bool(k & 1)
        kind = k % 10
        src, dst = pick(SRC_OK), pick(LOCAL_DST)
        if kind == 0:    # wrong checksums in the request
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 0, p, bad=True), tagged=tagged, bad_csum=True)
        elif kind == 1:  # total_length below ihl*4 + 8
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 0, p), tagged=tagged, total_length=20 + int(rng.integers(0, 8)))
        elif kind == 2:  # total_length past the frame: the payload becomes 0
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 0, p), tagged=tagged, total_length=28 + p + 1 + int(rng.integers(0, 900)))
        elif kind == 3:  # fewer than 8 bytes at L4
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 0, 0)[:int(rng.integers(0, 8))], tagged=tagged, total_length=28)
        elif kind == 4:  # type 8 code 1
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 1, p), tagged=tagged)
        elif kind == 5:  # an echo reply, a timestamp request
            f = frame(rng, src, dst, 1, icmp_msg(rng, pick([0, 13]), 0, p), tagged=tagged)
        elif kind == 6:  # local, not ICMP
            f = frame(rng, src, dst, pick([6, 17, 89]), bytes(rng.integers(0, 4, 20 + p, dtype=np.uint8)), tagged=tagged)
        elif kind == 7:  # local for the lookup, held by no interface
            f = frame(rng, src, EXTRA_LOCAL[0], 1, icmp_msg(rng, 8, 0, p), tagged=tagged)
        elif kind == 8:  # total_length short of the frame: the reply carries total_length's payload
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 0, p + 9), tagged=tagged, total_length=28 + p)
        else:            # TTL 1 to a local address is still local
            f = frame(rng, src, dst, 1, icmp_msg(rng, 8, 0, p), tagged=tagged, ttl=1)
        out.append(f)
    n_echo = len(out)
    # originals of the error path
    for behind in (0, 3, 8, 64):
        for tagged in (False, True):
            for ihl in (5, 7, 15, 2):
                for src in SRC_OK[:3] + SRC_BAD:
                    ttl_case = int(rng.integers(0, 3))  # 0, 1: expired; 2: no route
                    dst = pick(DST_ROUTED) if ttl_case < 2 else pick(DST_NO_ROUTE)
                    ttl = ttl_case if ttl_case < 2 else int(rng.integers(2, 255))
                    l4 = bytes(rng.integers(0, 8, behind, dtype=np.uint8) * 31)
                    out.append(frame(rng, src, dst, pick([1, 6, 17, 47]), l4, ttl=ttl, tagged=tagged, ihl=ihl))
    n_err = len(out) - n_echo
    # other verdicts: forwardable, not IPv4
    for k in range(8):
        out.append(frame(rng, pick(SRC_OK), "172.16.9.9", 17, bytes(26), ttl=64, tagged=bool(k & 1)))
    out.append(mac(1) + mac(2) + b"\x08\x06" + bytes(28))
    out.append(mac(1) + mac(2) + b"\x86\xdd" + bytes(60))
    return out, n_echo, n_err


def run_probe(frames, ingress):
    inp = [struct.pack("<III", NUM_PORTS, ingress, SEED), struct.pack("<I", len(INTERFACES))]
    for pid, up, m, ips in INTERFACES:
        inp.append(struct.pack("<IB3x6s2xI", pid, up, m, len(ips)) + b"".join(struct.pack("<I", ip4(a)) for a in ips))
    inp.append(struct.pack("<I", len(ROUTES)))
    for net, mask, nh, ifid in ROUTES:
        inp.append(struct.pack("<IIII", ip4(net), ip4(mask), ip4(nh), ifid))
    inp.append(struct.pack("<I", len(ARP)))
    for a, m in ARP:
        inp.append(struct.pack("<I6s2x", ip4(a), m))
    inp.append(struct.pack("<I", len(EXTRA_LOCAL)) + b"".join(struct.pack("<I", ip4(a)) for a in EXTRA_LOCAL))
    inp.append(struct.pack("<I", len(frames)))
    for f in frames:
        inp.append(struct.pack("<I", len(f)) + f)
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

    ifs = []
    for _ in range(take("<I")[0]):
        pid, up, m, nip = take("<IB3x6s2xI")
        ifs.append((pid, up, m, [take("<I")[0] for _ in range(nip)]))
    routes = [take("<IIII") for _ in range(take("<I")[0])]
    arp = [take("<I6s2x") for _ in range(take("<I")[0])]
    verdict, status, port, msgs = [], [], [], []
    for _ in frames:
        v, st, sent, p, ln = take("<IIIII")
        verdict.append(v)
        status.append(st)
        port.append(p)
        msgs.append(res[pos:pos + ln] if sent else None)
        pos += ln
    assert pos == len(res)
    return ifs, routes, arp, np.array(verdict, np.uint8), np.array(status, np.uint8), np.array(port, np.uint32), msgs


def ragged(items):
    start = np.zeros(len(items) + 1, np.uint32)
    start[1:] = np.cumsum([len(x) for x in items])
    return start, np.frombuffer(b"".join(items), np.uint8).copy()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that the file regenerates bit for bit."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else oracle.REFERENCE_ROOT
    os.makedirs(os.path.dirname(PROBE), exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(ref_root, "src", "netflow++", "*.cpp")))
    subprocess.run(["g++", "-std=c++17", "-O0", "-w", "-I" + os.path.join(ref_root, "include"),
                    os.path.join(HERE, "icmp_probe.cpp"), *srcs, "-o", PROBE, "-lpthread"], check=True)
    rng = np.random.default_rng(SEED)
    frames, n_echo, n_err = make_frames(rng)
    out = {"seed": np.uint64(SEED), "num_ports": np.uint32(NUM_PORTS), "n_echo": np.uint32(n_echo), "n_err": np.uint32(n_err),
           "ingress": np.array([r[0] for r in RUNS], np.uint32), "stride": np.array([r[1] for r in RUNS], np.uint32),
           "extra_local": np.array([ip4(a) for a in EXTRA_LOCAL], np.uint32)}
    out["frame_start"], out["frame_bytes"] = ragged(frames)
    seen = set()
    for r, (ingress, stride) in enumerate(RUNS):
        sub = frames[::stride]
        ifs, routes, arp, verdict, status, port, msgs = run_probe(sub, ingress)
        if r == 0:
            out["if_id"] = np.array([i[0] for i in ifs], np.uint32)
            out["if_up"] = np.array([i[1] for i in ifs], np.uint8)
            out["if_mac"] = np.frombuffer(b"".join(i[2] for i in ifs), np.uint8).reshape(-1, 6).copy()
            out["if_ip_start"], ips = ragged([np.array(i[3], "<u4").tobytes() for i in ifs])
            out["if_ip_start"] //= 4
            out["if_ips"] = ips.view("<u4").copy()
            out["routes"] = np.array(routes, np.uint32).reshape(-1, 4)
            out["arp_ip"] = np.array([a[0] for a in arp], np.uint32)
            out["arp_mac"] = np.frombuffer(b"".join(a[1] for a in arp), np.uint8).reshape(-1, 6).copy()
            # get_routing_table() order (the manager sorts): the fixture keeps it as it is
            assert sorted(tuple(x) for x in out["routes"].tolist()) == sorted((ip4(a), ip4(b), ip4(c), d) for a, b, c, d in ROUTES)
            assert dict(zip(out["arp_ip"].tolist(), [bytes(m) for m in out["arp_mac"]]))[ip4("10.0.0.10")] == mac(0x1FF)
        sent = np.array([m is not None for m in msgs])
        ip_id = np.array([(m[18] << 8 | m[19]) if m is not None and status[i] != ST_ECHO else 0 for i, m in enumerate(msgs)],
                         np.uint16)
        out[f"verdict_{r}"], out[f"status_{r}"], out[f"port_{r}"], out[f"ip_id_{r}"] = verdict, status, port, ip_id
        out[f"msg_start_{r}"], out[f"msg_bytes_{r}"] = ragged([m or b"" for m in msgs])
        # ---- what the fixture is meant to hold, read from the reference's results alone
        assert ((status == ST_ECHO) | (status == ST_TIME) | (status == ST_UNREACH) == sent).all()
        seen |= set(status.tolist())
        kind = {"echo": verdict == RT_LOCAL, "ttl": verdict == RT_TTL, "no route": verdict == RT_NO_ROUTE}
        for name, m in kind.items():
            print(f"run {r} (ingress {ingress}): {name}: {int(m.sum())} frames, {int(sent[m].sum())} messages; "
                  f"status counts {np.bincount(status[m], minlength=12).tolist()}")
            if r == 0:
                assert m.sum() >= 60 and sent[m].sum() * 4 >= m.sum(), name
        if r == 0:
            lens = np.array([len(m) for m in msgs if m is not None])
            assert (lens & 1).any() and (~lens & 1).any() and lens.max() >= 1642 and lens.min() == 42
        else:
            assert (status[verdict == RT_LOCAL] != ST_ECHO).all(), "ingress port down: no reply leaves"
    want = set(range(15)) - {ST_OVERFLOW, ST_OOB, ST_TOO_LONG, ST_SRC_NO_IF_MAC}
    assert want <= seen, sorted(want - seen)
    assert ST_SRC_NO_IF_MAC not in seen
    path = os.path.join(HERE, "icmp_ref.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes,", len(frames), "frames")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()

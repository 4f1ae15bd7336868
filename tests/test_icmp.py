"""CPU tests of the ICMP responder's host side (nfcs_icmp_respond_host, nfcs_fib_resolve_host): the host walk
against what the reference's own IcmpProcessor sent (tests/golden/icmp_ref.npz), every message's checksums
under the oracle, the resolve against the lookup, the setter / commit convention, the statuses the reference
does not have (OOB, TOO_LONG, OVERFLOW, SRC_NO_IF_MAC), the overflow rule, the argument errors, and the host
code as a stand-alone program under the sanitizers."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import netflow_amd as nf
import oracle
from icmp_common import (FAR, FILL, HOST, ME, assert_layout, fixture_fib, fixture_icmp, icmp_fixture, ipv4, messages_of,
                         pack_with_region, region_for, round_up, run_of, small_tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    z, frames = icmp_fixture()
    with fixture_fib(z) as fib, fixture_icmp(z) as icmp:
        yield z, frames, fib, icmp


def fold_be(b):
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b[:len(b) & ~1])) + (b[-1] if len(b) & 1 else 0)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("msg_align", [16, 128])
def test_host_walk_equals_the_reference(fx, r, msg_align):
    z, frames, fib, icmp = fx
    run = run_of(z, frames, r)
    arena, desc, msg_base = pack_with_region(run["frames"], 16, region_for(run["sent"], msg_align), msg_align)
    before = arena.copy()
    cap = len(run["sent"]) + 3
    out = icmp.respond_host(fib, run["ingress"], arena, msg_base, msg_align, desc, run["verdict"], cap, ip_id=run["ip_id"])
    assert messages_of(arena, out) == run["sent"]  # source packet, port and every byte, in the reference's order
    assert np.array_equal(out["status"], run["status"])
    t = out["totals"]
    assert int(t["messages"]) == int(t["messages_needed"]) == len(run["sent"])
    assert int(t["echo_replies"]) == int((run["status"] == nf.ICMP_ST_ECHO_REPLY).sum())
    assert int(t["errors"]) == int(t["messages"]) - int(t["echo_replies"])
    assert int(t["msg_bytes"]) == int(t["msg_bytes_needed"]) == region_for(run["sent"], msg_align)
    assert_layout(out, arena, msg_base, msg_align, cap, before)


def test_messages_checksum_under_the_oracle(fx):
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    arena, desc, msg_base = pack_with_region(run["frames"], 16, region_for(run["sent"], 16), 16)
    out = icmp.respond_host(fib, run["ingress"], arena, msg_base, 16, desc, run["verdict"], len(run["sent"]), ip_id=run["ip_id"])
    msgs = messages_of(arena, out)
    assert len(msgs) >= 150
    odd = 0
    for _, _, m in msgs:
        # the oracle's sum: big-endian words, an odd last byte as the LOW byte (packet.hpp:898-905)
        assert fold_be(m[14:34]) == 0xFFFF and fold_be(m[34:]) == 0xFFFF
        odd += len(m) & 1
        after, st = oracle.update_frame(m)  # update_checksums() again changes nothing
        assert after == m and st == nf.ST_V4_ICMP
    assert odd >= 20


def test_resolve_equals_lookup_without_local_and_ttl(fx):
    z, frames, fib, icmp = fx
    ips = set(int(x) for x in z["arp_ip"]) | set(int(x) for x in z["if_ips"]) | set(int(x) for x in z["extra_local"])
    for f in frames:
        if len(f) >= 38 and f[12:14] in (b"\x08\x00", b"\x81\x00"):
            l2 = 18 if f[12:14] == b"\x81\x00" else 14
            ips |= {struct.unpack_from("<I", f, l2 + 12)[0], struct.unpack_from("<I", f, l2 + 16)[0]}
    seen = set()
    routes = [tuple(int(v) for v in row) for row in z["routes"]]
    for ip in sorted(ips):
        v, nh, eif = fib.resolve_host(ip)
        lv, lnh, leif = fib.lookup_host(ip, 64)
        first = next((r for r in routes if ip & r[1] == r[0]), None)
        assert v in (nf.RT_FORWARD, nf.RT_NO_ROUTE, nf.RT_ARP_MISS, nf.RT_NO_IF_MAC)
        assert eif == (first[3] if first else nf.IF_NONE)  # the route's interface whatever the verdict
        if lv != nf.RT_LOCAL:
            assert (v, nh) == (lv, lnh), hex(ip)
            assert leif == (eif if v == nf.RT_FORWARD else nf.IF_NONE)
        else:
            assert fib.lookup_host(ip, 1)[0] == nf.RT_LOCAL and v != nf.RT_LOCAL
        seen.add(v)
    assert {nf.RT_FORWARD, nf.RT_NO_ROUTE, nf.RT_ARP_MISS} <= seen
    with nf.Fib() as f2:  # an interface without a MAC: only this library's tables can say so
        rt = np.zeros(1, nf.FIB_ROUTE_DTYPE)
        rt[0] = (0x0000000A, 0x000000FF, 0, 5)
        arp = np.zeros(1, nf.FIB_ARP_DTYPE)
        arp[0]["ip"] = 0x0100000A
        f2.set_routes(rt).set_arp(arp)
        with pytest.raises(nf.NfcsError):
            f2.resolve_host(0x0100000A)  # before commit
        assert f2.commit().resolve_host(0x0100000A) == (nf.RT_NO_IF_MAC, nf.NH_NONE, 5) == f2.lookup_host(0x0100000A, 9)[:2] + (5,)
        assert f2.resolve_host(0x0200000A) == (nf.RT_ARP_MISS, nf.NH_NONE, 5)
        assert f2.resolve_host(0x0100000B) == (nf.RT_NO_ROUTE, nf.NH_NONE, nf.IF_NONE)


def test_statuses_the_reference_does_not_have():
    echo = struct.pack(">BBHHH", 8, 0, 0, 1, 2)
    frames = [
        ipv4(HOST, FAR, 17, bytes(30), ttl=1, ihl=15)[:14 + 40],      # OOB: the header claims 60 bytes, 40 are there
        # TOO_LONG: IHL 1 puts "type 8 code 0" into the identification; payload 65535 - 4 - 8, and 28 + 65523 > 65535
        ipv4(HOST, ME, 1, bytes(65515), ihl=1, tl=65535, ident=0x0800),
        ipv4(HOST, ME, 1, echo + bytes(65507), ihl=5),                # the longest reply that fits: 65,549 bytes
        ipv4(HOST, FAR, 17, bytes(8), ttl=1),                         # TIME_EXCEEDED
    ]
    fib, icmp = small_tables()
    with fib, icmp:
        verdict = np.array([nf.RT_TTL_EXPIRED, nf.RT_LOCAL, nf.RT_LOCAL, nf.RT_TTL_EXPIRED], np.uint8)
        arena, desc, msg_base = pack_with_region(frames, 16, 70000, 16)
        out = icmp.respond_host(fib, 0, arena, msg_base, 16, desc, verdict, 4)
        assert out["status"].tolist() == [nf.ICMP_ST_OOB, nf.ICMP_ST_TOO_LONG, nf.ICMP_ST_ECHO_REPLY, nf.ICMP_ST_TIME_EXCEEDED]
        msgs = messages_of(arena, out)
        assert [(s, p, len(m)) for s, p, m in msgs] == [(2, 0, 65549), (3, 1, 42 + 28)]
        for _, _, m in msgs:
            assert oracle.update_frame(m)[0] == m
        assert msgs[0][2][16:18] == b"\xff\xff" and msgs[0][2][42:] == frames[2][42:]
        # OVERFLOW: cap cuts the second message, the region the first
        out = icmp.respond_host(fib, 0, arena, msg_base, 16, desc, verdict, 1)
        assert out["status"].tolist()[2:] == [nf.ICMP_ST_ECHO_REPLY, nf.ICMP_ST_OVERFLOW]
        assert (int(out["totals"]["messages"]), int(out["totals"]["messages_needed"])) == (1, 2)
        small = pack_with_region(frames, 16, 65536, 16)[0]
        out = icmp.respond_host(fib, 0, small, msg_base, 16, desc, verdict, 4)
        assert out["status"].tolist()[2:] == [nf.ICMP_ST_OVERFLOW, nf.ICMP_ST_OVERFLOW]  # a prefix condition
        assert int(out["totals"]["messages"]) == 0 and int(out["totals"]["msg_bytes_needed"]) == 65552 + 80
        assert (small[msg_base:] == FILL).all()
    fib, icmp = small_tables(if_mac=False)  # SRC_NO_IF_MAC: an interface with an address and no MAC
    with fib, icmp:
        arena, desc, msg_base = pack_with_region(frames[3:], 16, 256, 16)
        out = icmp.respond_host(fib, 0, arena, msg_base, 16, desc, np.array([nf.RT_NO_ROUTE], np.uint8), 1)
        assert out["status"].tolist() == [nf.ICMP_ST_SRC_NO_IF_MAC] and int(out["totals"]["messages_needed"]) == 0


def test_other_verdicts_dead_packets_and_untrusted_verdicts(fx):
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    i = run["sent"][0][0]
    f = run["frames"][i]
    arena, desc, msg_base = pack_with_region([f, f, f[:20], b"\x00" * 60, f], 16, 4096, 16)
    desc[1]["off16"] = msg_base // 16  # not live: it starts in the region
    verdict = np.array([nf.RT_FORWARD, nf.RT_LOCAL, nf.RT_LOCAL, nf.RT_TTL_EXPIRED, nf.RT_LOCAL], np.uint8)
    out = icmp.respond_host(fib, 0, arena, msg_base, 16, desc, verdict, 5)
    assert out["status"].tolist() == [0, 0, 0, 0, nf.ICMP_ST_ECHO_REPLY]
    assert out["msg_src"].tolist() == [4] + [nf.ITEM_NONE] * 4
    for v in (nf.RT_BAD_DESC, nf.RT_NOT_IPV4, nf.RT_ARP_MISS, nf.RT_NO_IF_MAC, 200):
        out = icmp.respond_host(fib, 0, arena, msg_base, 16, desc[:1], np.array([v], np.uint8), 1)
        assert out["status"].tolist() == [0] and int(out["totals"]["messages_needed"]) == 0


def test_every_cut_of_a_burst_on_the_host(fx):
    z, frames, fib, icmp = fx
    run = run_of(z, frames, 0)
    take = [i for i, _, m in run["sent"] if len(m) < 400][:40]
    sub = [run["frames"][i] for i in take]
    verdict, ip_id = run["verdict"][take], run["ip_id"][take]
    by_src = {i: (p, m) for i, p, m in run["sent"]}
    want = [(k,) + by_src[i] for k, i in enumerate(take)]
    slots = np.cumsum([round_up(len(m), 64) for _, _, m in want])
    for cut in range(41):
        for by_cap in (True, False):
            region = int(slots[-1]) if by_cap else (int(slots[cut - 1]) if cut else 0) + (48 if cut < 40 else 0)
            cap = cut if by_cap else 40
            arena, desc, msg_base = pack_with_region(sub, 16, region, 64)
            before = arena.copy()
            out = icmp.respond_host(fib, 0, arena, msg_base, 64, desc, verdict, cap, ip_id=ip_id)
            assert messages_of(arena, out) == want[:cut], (cut, by_cap)
            assert int(out["totals"]["messages_needed"]) == 40 and int(out["totals"]["msg_bytes_needed"]) == int(slots[-1])
            assert (out["status"][cut:] == nf.ICMP_ST_OVERFLOW).all() and (out["status"][:cut] != nf.ICMP_ST_OVERFLOW).all()
            assert_layout(out, arena, msg_base, 64, cap, before)


def test_setters_commit_and_argument_errors(fx):
    z, frames, fib, _ = fx
    run = run_of(z, frames, 0)
    arena, desc, msg_base = pack_with_region(run["frames"][:4], 16, 4096, 16)
    verdict = run["verdict"][:4]
    with fixture_icmp(z) as icmp:
        a = icmp.respond_host(fib, 0, arena, msg_base, 16, desc, verdict, 4)
        for setter in (lambda: icmp.set_local(np.zeros(0, nf.ICMP_LOCAL_DTYPE)), lambda: icmp.set_if_ips([]),
                       lambda: icmp.set_ports_up([], 8)):
            icmp.commit()
            setter()  # invalidates the commit
            with pytest.raises(nf.NfcsError):
                icmp.respond_host(fib, 0, arena, msg_base, 16, desc, verdict, 4)
        b = icmp.commit().respond_host(fib, 0, arena, msg_base, 16, desc, verdict, 4)
        assert int(a["totals"]["messages"]) == 4 and int(b["totals"]["messages"]) == 0  # no local entry any more
        assert (b["status"] == nf.ICMP_ST_NO_LOCAL_MAC).all()
        with pytest.raises(nf.NfcsError):
            icmp.set_ports_up([0], nf.L2_MAX_PORTS + 1)
    L = nf.lib()
    with fixture_icmp(z) as icmp:
        tot, p = np.zeros(1, nf.ICMP_TOTALS_DTYPE), np.zeros(64, np.uint64).ctypes.data
        A = arena.ctypes.data

        def call(m=icmp.ptr, f=fib.ptr, a=A, base=msg_base, align=16, d=desc.ctypes.data, n=4, v=verdict.ctypes.data, cap=4,
                 items=p, totals=tot.ctypes.data):
            return L.nfcs_icmp_respond_host(m, f, 0, a, arena.nbytes, base, align, d, n, v, None, cap, items, items, items,
                                            None, totals)

        assert call() == 0
        for align in (0, 8, 24, 48):
            assert call(align=align) == -1, align               # not a power of two >= 16
        assert call(base=msg_base + 16, align=32) == -1         # msg_base not a multiple of msg_align
        assert call(base=arena.nbytes + 16) == -1               # msg_base past the arena
        assert call(base=arena.nbytes) == 0                     # an empty region is legal
        assert call(m=None) == -1 and call(f=None) == -1 and call(a=None) == -1 and call(d=None) == -1
        assert call(v=None) == -1 and call(totals=None) == -1 and call(items=None) == -1
        assert call(cap=0, items=None) == 0
        assert call(n=0, d=None, v=None, items=None, totals=None, a=None) == 0  # n == 0: nothing is looked at
        with nf.Fib() as raw:                                   # a fib that was never committed
            assert call(f=raw.ptr) == -1
        assert L.nfcs_icmp_set_local(icmp.ptr, None, 1) == -1 and L.nfcs_icmp_set_if_ips(icmp.ptr, None, 1) == -1
        assert L.nfcs_icmp_set_ports_up(icmp.ptr, None, 1, 8) == -1 and L.nfcs_icmp_commit(None) == -1
        assert L.nfcs_icmp_upload(None, icmp.ptr) == -1 and L.nfcs_icmp_destroy(None) == -1


def test_first_duplicate_wins():
    fib, _ = small_tables()
    la = np.zeros(2, nf.ICMP_LOCAL_DTYPE)
    la["ip"] = ME
    la[0]["mac"], la[1]["mac"] = (2, 0, 0, 0, 0, 0x11), (2, 0, 0, 0, 0, 0x22)
    ia = np.array([(1, 0x0300000A), (1, 0x0400000A)], nf.ICMP_IF_IP_DTYPE)
    echo = ipv4(HOST, ME, 1, struct.pack(">BBHHH", 8, 0, 0, 1, 2) + b"abc")
    err = ipv4(HOST, FAR, 6, bytes(20), ttl=0)
    with fib, nf.Icmp().set_local(la).set_if_ips(ia).set_ports_up([0, 1, 5], 2).commit() as icmp:
        arena, desc, msg_base = pack_with_region([echo, err], 16, 256, 16)
        out = icmp.respond_host(fib, 0, arena, msg_base, 16, desc, np.array([nf.RT_LOCAL, nf.RT_TTL_EXPIRED], np.uint8), 2,
                                ip_id=np.array([0xBEEF, 0x1234], np.uint16))
        (s0, p0, m0), (s1, p1, m1) = messages_of(arena, out)
        assert m0[6:12] == bytes((2, 0, 0, 0, 0, 0x11)) and m0[18:20] == b"\0\0" and m0[42:] == b"abc" and p0 == 0
        assert m1[26:30] == struct.pack("<I", 0x0300000A) and m1[18:20] == b"\x12\x34" and p1 == 1
        assert m1[34:42] == bytes([11, 0]) + m1[36:38] + bytes(4) and m1[42:] == err[14:14 + 28]


def test_icmp_test_under_sanitizers(tmp_path):
    """The compile step, the plan and the host walk as a stand-alone host program (its own main, no HIP, nothing
    loaded into Python) under AddressSanitizer + UBSan, every array in a heap block of its exact size."""
    exe = str(tmp_path / "icmp_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "netflow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "icmp_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "icmp host walk OK" in r.stdout


def test_python_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "nfcs.h")).read()
    m = re.search(r"#define\s+NFCS_ICMP_TILE_PKTS\s+(\d+)u", hdr)
    assert m and int(m.group(1)) == nf.ICMP_TILE_PKTS
    for name in ("NONE", "ECHO_REPLY", "TIME_EXCEEDED", "UNREACHABLE", "TO_CPU", "IGNORED", "NO_LOCAL_MAC", "SRC_NO_ROUTE",
                 "SRC_NO_IF_IP", "SRC_ARP_MISS", "SRC_NO_IF_MAC", "PORT_DOWN", "OOB", "TOO_LONG", "OVERFLOW"):
        m = re.search(r"NFCS_ICMP_ST_" + name + r"\s*=\s*(\d+)", hdr)
        assert m and int(m.group(1)) == getattr(nf, "ICMP_ST_" + name), name
    assert nf.ICMP_TOTALS_DTYPE.names == ("messages", "messages_needed", "echo_replies", "errors", "msg_bytes",
                                          "msg_bytes_needed")

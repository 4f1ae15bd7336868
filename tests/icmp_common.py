"""Shared inputs for the ICMP responder's tests: the reference-made fixture tests/golden/icmp_ref.npz
(tests/golden/make_icmp_golden.py), a Fib and an Icmp built from the tables the reference's managers held, the
packed arena with its message region, and what the reference sent in the form the stage reports it."""
import os
import struct

import numpy as np

import netflow_amd as nf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = 0xEE


def round_up(x, a):
    return (int(x) + a - 1) // a * a


def icmp_fixture():
    z = np.load(os.path.join(GOLD, "icmp_ref.npz"))
    fs, fb = z["frame_start"], z["frame_bytes"]
    frames = [bytes(fb[int(fs[i]):int(fs[i + 1])]) for i in range(len(fs) - 1)]
    return z, frames


def run_of(z, frames, r):
    """Run r of the fixture: its frames, ingress port, verdicts, ip ids, statuses, and the messages the reference
    sent as [(source index, port, bytes)] in order."""
    sub = frames[::int(z["stride"][r])]
    ms, mb = z[f"msg_start_{r}"], z[f"msg_bytes_{r}"]
    sent = [(i, int(z[f"port_{r}"][i]), bytes(mb[int(ms[i]):int(ms[i + 1])])) for i in range(len(sub)) if ms[i + 1] > ms[i]]
    return {"frames": sub, "ingress": int(z["ingress"][r]), "verdict": z[f"verdict_{r}"], "ip_id": z[f"ip_id_{r}"],
            "status": z[f"status_{r}"], "sent": sent}


def fixture_fib(z) -> nf.Fib:
    """The Fib a caller builds from the reference's managers: get_routing_table() as it is, the ARP cache, every
    configured interface's MAC, and the addresses the lookup calls local (the interfaces' plus the extra one)."""
    routes = np.zeros(len(z["routes"]), nf.FIB_ROUTE_DTYPE)
    for i, (net, mask, nh, ifid) in enumerate(z["routes"]):
        routes[i] = (net, mask, nh, ifid)
    arp = np.zeros(len(z["arp_ip"]), nf.FIB_ARP_DTYPE)
    arp["ip"], arp["mac"] = z["arp_ip"], z["arp_mac"]
    ifm = np.zeros(len(z["if_id"]), nf.FIB_IF_MAC_DTYPE)
    ifm["egress_if"], ifm["mac"] = z["if_id"], z["if_mac"]
    local = np.concatenate([z["if_ips"], z["extra_local"]]).astype(np.uint32)
    return nf.Fib().set_routes(routes).set_arp(arp).set_if_macs(ifm).set_local_ips(local).commit()


def fixture_icmp(z) -> nf.Icmp:
    """get_mac_for_ip / get_interface_ip / is_port_link_up as tables, interfaces ascending as the reference scans."""
    local, if_ips = [], []
    for k, ifid in enumerate(z["if_id"]):
        for ip in z["if_ips"][int(z["if_ip_start"][k]):int(z["if_ip_start"][k + 1])]:
            local.append((int(ip), bytes(z["if_mac"][k])))
            if_ips.append((int(ifid), int(ip)))
    la = np.zeros(len(local), nf.ICMP_LOCAL_DTYPE)
    for i, (ip, m) in enumerate(local):
        la[i]["ip"], la[i]["mac"] = ip, np.frombuffer(m, np.uint8)
    ia = np.array(if_ips, dtype=nf.ICMP_IF_IP_DTYPE)
    up = z["if_id"][z["if_up"] != 0]
    return nf.Icmp().set_local(la).set_if_ips(ia).set_ports_up(up, int(z["num_ports"])).commit()


def pack_with_region(frames, align, region, msg_align=128, fill=FILL, lead=0):
    """Frames packed at `align`-byte starts from byte `lead`, then `region` bytes of message region:
    (arena, desc, msg_base). The region and the padding between frames hold `fill`."""
    desc = np.zeros(len(frames), nf.DESC_DTYPE)
    pos = lead
    for i, f in enumerate(frames):
        desc[i] = (pos // 16, len(f))
        pos += round_up(max(len(f), 1), align)
    msg_base = round_up(pos, msg_align)
    arena = np.full(msg_base + region, fill, np.uint8)
    for d, f in zip(desc, frames):
        o = int(d["off16"]) * 16
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    return arena, desc, msg_base


def region_for(sent, msg_align):
    return sum(round_up(len(m), msg_align) for _, _, m in sent)


def messages_of(arena, out):
    """[(source index, port, bytes)] of the emitted messages, read from the arena through their descriptors."""
    m = int(out["totals"]["messages"])
    res = []
    for k in range(m):
        o, ln = int(out["msg_desc"][k]["off16"]) * 16, int(out["msg_desc"][k]["len"])
        res.append((int(out["msg_src"][k]), int(out["msg_port"][k]), bytes(arena[o:o + ln])))
    return res


def assert_layout(out, arena, msg_base, msg_align, cap, before):
    """Slots in message order from msg_base, zero padding to the 16-byte chunk, inert entries past `messages`, and
    nothing else written: `before` is the arena before the call."""
    m = int(out["totals"]["messages"])
    pos = msg_base
    touched = np.zeros(len(arena), bool)
    for k in range(m):
        o, ln = int(out["msg_desc"][k]["off16"]) * 16, int(out["msg_desc"][k]["len"])
        assert o == pos, (k, o, pos)
        assert not arena[o + ln:o + round_up(ln, 16)].any(), f"message {k}: padding to the chunk is not zero"
        touched[o:o + round_up(ln, 16)] = True
        pos += round_up(ln, msg_align)
    assert pos - msg_base == int(out["totals"]["msg_bytes"])
    assert pos <= len(arena)
    assert np.array_equal(arena[~touched], before[~touched]), "bytes outside the emitted messages changed"
    assert (out["msg_desc"][m:cap]["off16"] == 0).all() and (out["msg_desc"][m:cap]["len"] == 0).all()
    assert (out["msg_port"][m:cap] == nf.IF_NONE).all() and (out["msg_src"][m:cap] == nf.ITEM_NONE).all()


def assert_same_respond(got, want, what=""):
    for k in ("messages", "messages_needed", "echo_replies", "errors", "msg_bytes", "msg_bytes_needed"):
        assert int(got["totals"][k]) == int(want["totals"][k]), f"{what}totals.{k}: {got['totals'][k]} != {want['totals'][k]}"
    for k in ("msg_desc", "msg_port", "msg_src", "status"):
        assert np.array_equal(got[k], want[k]), f"{what}{k} differs"


def device_respond(eng, icmp, fib, ingress, arena, msg_base, msg_align, desc, verdict, cap, ip_id=None, guard=8):
    """Engine.icmp_respond_device on uploaded copies: the dict Icmp.respond_host returns, plus the arena after.
    The message arrays carry `guard` extra entries behind cap, filled with 0xA5 and checked untouched."""
    n = len(desc)
    d_arena = eng.alloc(arena.nbytes).upload(arena)
    d_desc = eng.alloc(max(desc.nbytes, 16)).upload(desc)
    d_v = eng.alloc(max(n, 16)).upload(np.ascontiguousarray(verdict, np.uint8))
    d_id = None if ip_id is None else eng.alloc(max(2 * n, 16)).upload(np.ascontiguousarray(ip_id, np.uint16))
    pat8 = np.full((cap + guard) * 8, 0xA5, np.uint8)
    d_md = eng.alloc(len(pat8)).upload(pat8)
    d_mp = eng.alloc((cap + guard) * 4).upload(pat8[:(cap + guard) * 4])
    d_ms = eng.alloc((cap + guard) * 4).upload(pat8[:(cap + guard) * 4])
    d_st = eng.alloc(max(n, 16))
    d_tot = eng.alloc(32).upload(np.zeros(32, np.uint8))
    eng.icmp_respond_device(icmp, fib, ingress, d_arena, arena.nbytes, msg_base, msg_align, d_desc, n, d_v, cap, d_md, d_mp,
                            d_ms, d_tot, ip_id=d_id, status=d_st)
    eng.sync()
    md = d_md.download(np.uint8, len(pat8))
    mp = d_mp.download(np.uint8, (cap + guard) * 4)
    ms = d_ms.download(np.uint8, (cap + guard) * 4)
    assert (md[cap * 8:] == 0xA5).all() and (mp[cap * 4:] == 0xA5).all() and (ms[cap * 4:] == 0xA5).all(), \
        "entries past cap were written"
    out = {"msg_desc": md[:cap * 8].view(nf.DESC_DTYPE).copy(), "msg_port": mp[:cap * 4].view(np.uint32).copy(),
           "msg_src": ms[:cap * 4].view(np.uint32).copy(), "status": d_st.download(np.uint8, n),
           "totals": d_tot.download(nf.ICMP_TOTALS_DTYPE, 1)[0], "arena": d_arena.download(np.uint8, arena.nbytes)}
    for b in (d_arena, d_desc, d_v, d_md, d_mp, d_ms, d_st, d_tot) + ((d_id,) if d_id is not None else ()):
        b.free()
    return out


# ---- a two-port switch and hand-made frames for the cases the fixture cannot hold ----------------------

def ipv4(src, dst, proto, l4, ttl=64, ihl=5, tl=None, ident=7):
    h = struct.pack(">BBHHHBBH", 0x40 | ihl, 0, (ihl * 4 + len(l4)) if tl is None else tl, ident, 0, ttl, proto, 0)
    return bytes(6) + b"\x02\x00\x00\x00\x00\x09" + b"\x08\x00" + h + struct.pack("<II", src, dst) + bytes(max(ihl - 5, 0) * 4) + l4


def small_tables(if_mac=True):
    """Interface 1 = 10.0.0.1 / 02:..:01 on 10.0.0.0/24, host 10.0.0.2 in the ARP table, 2 ports, both up."""
    rt = np.zeros(1, nf.FIB_ROUTE_DTYPE)
    rt[0] = (0x0000000A, 0x00FFFFFF, 0, 1)
    arp = np.zeros(1, nf.FIB_ARP_DTYPE)
    arp[0]["ip"], arp[0]["mac"] = 0x0200000A, (2, 0, 0, 0, 0, 9)
    ifm = np.zeros(1 if if_mac else 0, nf.FIB_IF_MAC_DTYPE)
    if if_mac:
        ifm[0]["egress_if"], ifm[0]["mac"] = 1, (2, 0, 0, 0, 0, 1)
    fib = nf.Fib().set_routes(rt).set_arp(arp).set_if_macs(ifm).set_local_ips(np.array([0x0100000A], np.uint32)).commit()
    la = np.zeros(1, nf.ICMP_LOCAL_DTYPE)
    la[0]["ip"], la[0]["mac"] = 0x0100000A, (2, 0, 0, 0, 0, 1)
    icmp = nf.Icmp().set_local(la).set_if_ips(np.array([(1, 0x0100000A)], nf.ICMP_IF_IP_DTYPE)).set_ports_up([0, 1], 2).commit()
    return fib, icmp


HOST, ME, FAR = 0x0200000A, 0x0100000A, 0x08080808

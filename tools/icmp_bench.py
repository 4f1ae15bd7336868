#!/usr/bin/env python3
"""Times the ICMP responder (nfcs_icmp_respond_device) against yardsticks timed in the same run, all of them code
that existed before the stage: nfcs_flood_expand_device at fan-out 1 over the same frames (every packet flooded
to one port: the same reads, as many bytes written, the same four launches; the new stage adds the sums and the
dword shift), a device-to-device hipMemcpyAsync of as many bytes as the messages occupy, and the flow-key kernel
(hashes only: one header line per frame) for the case without a message. Prints one JSON line.

    python tools/icmp_bench.py [--steps 10] [--rounds 3] [--out profiles/icmp_bench.json]

Cases:
  echo_c1    C1-sized (1,500-byte) echo requests to a local address in 1,536-byte slots, all answered
  ttl10_c3   the C3 mix, 10% of the packets marked NFCS_RT_TTL_EXPIRED (one default route, so every source resolves)
  ttl100_c3  the C3 mix, every packet marked NFCS_RT_TTL_EXPIRED
  none_c1    C1 frames, every verdict NFCS_RT_FORWARD: classify + scan alone; the flood yardstick is its compaction
             alone (every packet a unicast item)
The timed calls rotate over two arenas, each with its own region, as bench.py's do. Variants are timed interleaved
in one process, `rounds` times; each figure is the median over the rounds of (HIP-event ms over `steps` calls) /
steps, with the minimum beside it; `spread` is (max - min) / median of the respond's rounds. After timing, the
messages whose source is among the first 4,096 packets are compared byte for byte with nfcs_icmp_respond_host.
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import netflow_amd as nf  # noqa: E402

SEED = 20250620
NROT = 2
NONE = 0xFFFFFFFF
PREFIX = 4096
ME, GW = 0x0100000A, 0x0200000A  # 10.0.0.1 (ours, on port 1), 10.0.0.2 (the gateway)


def event_ms(eng, step, steps: int) -> float:
    import torch
    st = torch.cuda.ExternalStream(eng.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        step()
    e1.record(st)
    e1.synchronize()
    return float(e0.elapsed_time(e1))


def med_min(xs):
    return {"ms": round(statistics.median(xs), 5), "ms_min": round(min(xs), 5),
            "spread": round((max(xs) - min(xs)) / statistics.median(xs), 4)}


def tables(eng):
    rt = np.zeros(1, nf.FIB_ROUTE_DTYPE)
    rt[0] = (0, 0, GW, 1)  # the default route
    arp = np.zeros(1, nf.FIB_ARP_DTYPE)
    arp[0]["ip"], arp[0]["mac"] = GW, (2, 0, 0, 0, 0, 2)
    ifm = np.zeros(1, nf.FIB_IF_MAC_DTYPE)
    ifm[0]["egress_if"], ifm[0]["mac"] = 1, (2, 0, 0, 0, 0, 1)
    fib = nf.Fib().set_routes(rt).set_arp(arp).set_if_macs(ifm).set_local_ips(np.array([ME], np.uint32)).commit().upload(eng)
    la = np.zeros(1, nf.ICMP_LOCAL_DTYPE)
    la[0]["ip"], la[0]["mac"] = ME, (2, 0, 0, 0, 0, 1)
    icmp = nf.Icmp().set_local(la).set_if_ips(np.array([(1, ME)], nf.ICMP_IF_IP_DTYPE)).set_ports_up([0, 1], 2).commit().upload(eng)
    fdb = nf.Fdb().set_port(0, native_vlan=1).set_port(1, native_vlan=1).commit().upload(eng)
    return fib, icmp, fdb


def echo_block(rng, count, length=1500, slot=1536):
    """`count` echo requests of `length` bytes to ME in `slot`-byte slots: random sources, ids and payloads."""
    b = np.zeros((count, slot), np.uint8)
    payload = length - 42
    b[:, 0:6], b[:, 6:12] = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 9)
    b[:, 12:14] = (8, 0)
    hdr = struct.pack(">BBHHHBBH", 0x45, 0, 28 + payload, 0, 0, 64, 1, 0)
    b[:, 14:26] = np.frombuffer(hdr, np.uint8)
    b[:, 26:30] = rng.integers(1, 255, (count, 4), dtype=np.uint8)
    b[:, 30:34] = np.frombuffer(struct.pack("<I", ME), np.uint8)
    b[:, 34] = 8
    b[:, 38:length] = rng.integers(0, 256, (count, length - 38), dtype=np.uint8)
    return b.reshape(-1)


def run_case(eng, hip, tabs, name, n, args):
    fib, icmp, fdb = tabs
    rng = np.random.default_rng(len(name))
    config = nf.CFG_C3 if name.endswith("c3") else nf.CFG_C1
    if name == "echo_c1":
        hdesc = np.zeros(n, nf.DESC_DTYPE)
        hdesc["off16"], hdesc["len"] = np.arange(n, dtype=np.uint64) * 96, 1500
        frames = n * 1536
        verdict = np.full(n, nf.RT_LOCAL, np.uint8)
    else:
        hdesc, _ = nf.layout_config(config, SEED, 0, n, 128)
        frames = (int(hdesc["off16"][-1]) * 16 + int(hdesc["len"][-1]) + 127) // 128 * 128
        share = {"ttl10_c3": 0.1, "ttl100_c3": 1.0, "none_c1": 0.0}[name]
        verdict = np.where(rng.random(n) < share, nf.RT_TTL_EXPIRED, nf.RT_FORWARD).astype(np.uint8)
    ip_id = rng.integers(0, 65536, n).astype(np.uint16)
    d_desc = eng.alloc(hdesc.nbytes).upload(hdesc)
    # size the region: an upper bound first (a reply is shorter than its request, an error at most 110 bytes)
    # and room for the flood yardstick's copies of whole frames
    bound = int(((hdesc["len"].astype(np.int64) + 127) // 128 * 128).sum()) + 128 * n
    arenas = [eng.alloc(frames + bound + 16) for _ in range(NROT)]
    block = echo_block(rng, min(1 << 15, n)) if name == "echo_c1" else None  # repeated every 32,768 packets
    for a in arenas:
        if name == "echo_c1":
            for lo in range(0, n, 1 << 15):
                a.upload(block[:min(1 << 15, n - lo) * 1536], lo * 1536)
        else:
            eng.gen_config_device(config, SEED, 0, n, a, frames, d_desc)
    d_v, d_id = eng.alloc(n).upload(verdict), eng.alloc(2 * n).upload(ip_id)
    d_md, d_mp, d_ms, d_st, d_tot = eng.alloc(8 * n + 16), eng.alloc(4 * n + 16), eng.alloc(4 * n + 16), eng.alloc(n), eng.alloc(32)
    d_ftot, d_hash = eng.alloc(32), eng.alloc(4 * n)
    # the flood yardstick: every packet of a message-making case floods to the one other port; none_c1: all unicast
    flood = name != "none_c1"
    l2 = np.full(n, NONE if flood else 1, np.uint32)
    if name == "ttl10_c3":
        l2 = np.where(verdict == nf.RT_TTL_EXPIRED, NONE, 1).astype(np.uint32)
    d_l2 = eng.alloc(4 * n).upload(l2)
    d_lv = eng.alloc(n).upload(np.where(l2 == NONE, nf.L2_FLOOD, nf.L2_FORWARD).astype(np.uint8))
    d_vl = eng.alloc(2 * n).upload(np.ones(n, np.uint16))
    arena_bytes = frames + bound
    eng.sync()
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return arenas[ctr[0] % NROT]

    def respond():
        eng.icmp_respond_device(icmp, fib, 0, nxt(), arena_bytes, frames, 128, d_desc, n, d_v, n, d_md, d_mp, d_ms, d_tot,
                                ip_id=d_id, status=d_st)

    def expand():
        eng.flood_expand_device(fdb, 0, 2, nxt(), arena_bytes, frames, 128, d_desc, n, n, d_md, d_mp, d_ms, d_ftot,
                                l2_port=d_l2, l2_verdict=d_lv, l2_vlan=d_vl)

    respond()
    eng.sync()
    tot = d_tot.download(nf.ICMP_TOTALS_DTYPE, 1)[0]
    mbytes = int(tot["msg_bytes"])
    assert int(tot["messages"]) == int(tot["messages_needed"]), "the region's bound was too small"
    d_src = eng.alloc(mbytes + 16) if mbytes else None

    def memcpy():
        rc = hip.hipMemcpyAsync(ctypes.c_void_p(nxt().ptr + frames), ctypes.c_void_p(d_src.ptr), ctypes.c_size_t(mbytes), 3,
                                ctypes.c_void_p(eng.stream))  # 3: hipMemcpyDeviceToDevice
        if rc:
            raise RuntimeError(f"hipMemcpyAsync: {rc}")

    variants = {"flood_fan1": expand, "respond": respond,
                "flowkey_hash": lambda: eng.flow_keys_device(nxt(), frames, d_desc, n, None, d_hash)}
    if mbytes:
        variants["memcpy_d2d"] = memcpy
    times = {k: [] for k in variants}
    for step in variants.values():
        for _ in range(args.warmup):
            step()
    eng.sync()
    for r in range(args.rounds):
        order = list(variants.items())
        for k, step in (order if r % 2 == 0 else order[::-1]):  # alternating order
            times[k].append(event_ms(eng, step, args.steps) / args.steps)
    # the check: one more respond on each arena (the yardsticks write the same region), then compare
    checked = 0
    for a in arenas:
        eng.icmp_respond_device(icmp, fib, 0, a, arena_bytes, frames, 128, d_desc, n, d_v, n, d_md, d_mp, d_ms, d_tot,
                                ip_id=d_id, status=d_st)
        eng.sync()
        k = min(PREFIX, n)
        end = int(hdesc["off16"][k - 1]) * 16 + (int(hdesc["len"][k - 1]) + 15) // 16 * 16
        base = (end + 127) // 128 * 128
        host = np.zeros(base + 128 * k + (1536 * k if name == "echo_c1" else 0), np.uint8)
        host[:end] = a.download(np.uint8, end)
        want = icmp.respond_host(fib, 0, host, base, 128, hdesc[:k], verdict[:k], k, ip_id=ip_id[:k])
        m = int(want["totals"]["messages"])
        md, ms = d_md.download(nf.DESC_DTYPE, max(m, 1)), d_ms.download(np.uint32, max(m, 1))
        assert np.array_equal(d_st.download(np.uint8, k), want["status"]), "status differs from the host walk"
        for j in range(m):
            ln = int(want["msg_desc"][j]["len"])
            assert int(ms[j]) == int(want["msg_src"][j]) and int(md[j]["len"]) == ln
            ho = int(want["msg_desc"][j]["off16"]) * 16
            got = a.download(np.uint8, (ln + 15) // 16 * 16, int(md[j]["off16"]) * 16)
            assert np.array_equal(got, host[ho:ho + len(got)]), f"message {j} differs from the host walk"
        checked += m
    res = {"packets": n, "messages": int(tot["messages"]), "echo_replies": int(tot["echo_replies"]), "msg_bytes": mbytes,
           "frame_bytes": frames, "checked_messages": checked}
    for k, xs in times.items():
        res[k] = med_min(xs)
    res["respond"]["x_flood_fan1"] = round(res["respond"]["ms"] / res["flood_fan1"]["ms"], 3)
    res["respond"]["x_flowkey"] = round(res["respond"]["ms"] / res["flowkey_hash"]["ms"], 3)
    if mbytes:
        res["respond"]["x_memcpy"] = round(res["respond"]["ms"] / res["memcpy_d2d"]["ms"], 3)
        res["respond"]["msg_gb_s"] = round(mbytes / (res["respond"]["ms"] * 1e-3) / 1e9, 1)
    for b in arenas + [d_desc, d_v, d_id, d_md, d_mp, d_ms, d_st, d_tot, d_ftot, d_hash, d_l2, d_lv, d_vl] + ([d_src] if d_src else []):
        b.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--cases", default="echo_c1,ttl10_c3,ttl100_c3,none_c1")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events are torch's, on the runtime the engine shares
    torch.cuda.init()
    try:  # the runtime the engine and torch already loaded
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpyAsync.restype = ctypes.c_int
    with nf.Engine(0) as eng:
        res = {"tool": "tools/icmp_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds, "
                         "variants interleaved in alternating order",
               "x_flood_fan1_is": "respond ms over the ms of nfcs_flood_expand_device at fan-out 1 over the same frames",
               "x_memcpy_is": "respond ms over the ms of a device-to-device hipMemcpyAsync of msg_bytes",
               "x_flowkey_is": "respond ms over flowkey_hash ms",
               "library": os.path.basename(os.path.dirname(os.path.abspath(nf.LIB_PATH))) + "/" + os.path.basename(nf.LIB_PATH)}
        fib, icmp, fdb = tables(eng)
        with fib, icmp, fdb:
            for name in args.cases.split(","):
                res[name] = run_case(eng, hip, (fib, icmp, fdb), name, args.packets, args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

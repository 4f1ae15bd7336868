#!/usr/bin/env python3
"""Times nfcs_route_lookup_device against the flow-key kernel (hashes only: the same read pattern, one
header line per frame) and the fused forward fed by the lookup. Prints one JSON line.

    python tools/route_bench.py [--steps 20] [--rounds 3] [--out profiles/route_lookup_bench.json]

Per workload (1M C1 frames, the 4M C3 mix; 128-byte frame starts as bench.py's default) the timed
calls rotate over separately generated batches (4 up to 1M packets, 2 above) as bench.py's do, so no
call finds its header lines in the memory-side cache. Variants are timed interleaved in one process,
`rounds` times; each figure is the median over the rounds of (HIP-event ms over `steps` calls) / steps,
with the minimum beside it.

Route tables:
  worst(N)   N - 1 host routes no frame matches, then a default route through a gateway: every frame
             scans all N entries (the linear scan's worst case). N = 16, 256, 4096.
  spread256  256 /8 routes by first octet, each through its own gateway: the generator's random
             destinations spread over 256 next hops and leave the scan after 128 entries on average.
The forward comparison (C1 only) times nfcs_l3_forward_device on the same batches with the next hops
and the 512-entry table of spread256 against bench.py's 8-entry table with next hop i % 9 (one frame
in nine not forwarded) and i % 8 (all forwarded).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import netflow_amd as nf  # noqa: E402

SEED = 20250620
HBM_PEAK_GBS = 8000.0
MAC = lambda k: [0x02, 0xBB, (k >> 24) & 255, (k >> 16) & 255, (k >> 8) & 255, k & 255]


def fib_worst(n_routes: int) -> nf.Fib:
    rng = np.random.default_rng(n_routes)
    r = np.zeros(n_routes, dtype=nf.FIB_ROUTE_DTYPE)
    r["network"][:-1] = rng.integers(0, 1 << 32, size=n_routes - 1, dtype=np.uint64).astype(np.uint32)
    r["mask"][:-1] = 0xFFFFFFFF
    r["egress_if"] = 1
    r["next_hop_ip"][-1] = nf.ip4("10.0.0.254")  # network 0, mask 0: the default route, last
    a = np.zeros(1, dtype=nf.FIB_ARP_DTYPE)
    a["ip"], a["mac"] = nf.ip4("10.0.0.254"), MAC(1)
    m = np.zeros(1, dtype=nf.FIB_IF_MAC_DTYPE)
    m["egress_if"], m["mac"] = 1, MAC(2)
    return nf.Fib().set_routes(r).set_arp(a).set_if_macs(m).set_local_ips(np.zeros(0, np.uint32)).commit()


def fib_spread256() -> nf.Fib:
    r = np.zeros(256, dtype=nf.FIB_ROUTE_DTYPE)
    r["network"] = np.arange(256, dtype=np.uint32)  # first octet = the low byte of the u32
    r["mask"] = 0xFF
    r["next_hop_ip"] = [nf.ip4(f"10.200.{i}.1") for i in range(256)]
    r["egress_if"] = np.arange(256) % 16
    a = np.zeros(256, dtype=nf.FIB_ARP_DTYPE)
    a["ip"] = r["next_hop_ip"]
    a["mac"] = [MAC(1000 + i) for i in range(256)]
    m = np.zeros(16, dtype=nf.FIB_IF_MAC_DTYPE)
    m["egress_if"] = np.arange(16)
    m["mac"] = [MAC(2000 + i) for i in range(16)]
    return nf.Fib().set_routes(r).set_arp(a).set_if_macs(m).set_local_ips(np.zeros(0, np.uint32)).commit()


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
    return {"ms": round(statistics.median(xs), 5), "ms_min": round(min(xs), 5)}


def run_workload(eng, config: int, n: int, steps: int, rounds: int, warmup: int, forward: bool):
    nrot = 4 if n <= (1 << 20) else 2
    batches = [eng.config_batch(config, SEED, 0, n, 128) for _ in range(nrot)]
    hdesc = batches[0][3]
    hdr = float(np.minimum(hdesc["len"].astype(np.float64), 128.0).sum())
    d_nh, d_if, d_v, d_hash = eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(n), eng.alloc(4 * n)
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return batches[ctr[0] % nrot][:3]

    fibs = {"worst16": fib_worst(16), "worst256": fib_worst(256), "worst4096": fib_worst(4096),
            "spread256": fib_spread256()}
    for f in fibs.values():
        f.upload(eng)
    variants = {"flowkey_hash": lambda: eng.flow_keys_device(*nxt(), n, None, d_hash)}
    for name, f in fibs.items():
        variants["lookup_" + name] = (lambda f=f: eng.route_lookup_device(f, *nxt(), n, d_nh, d_if, d_v))
    # the same lookup writing next hops only (egress interface and verdict left out)
    variants["lookup_worst16_nh_only"] = lambda: eng.route_lookup_device(fibs["worst16"], *nxt(), n, d_nh)
    times = {k: [] for k in variants}
    for k, step in variants.items():
        for _ in range(warmup):
            step()
    eng.sync()
    for _ in range(rounds):
        for k, step in variants.items():
            times[k].append(event_ms(eng, step, steps) / steps)
    out = {"packets": n, "batches_rotated": nrot, "frame_align": 128}
    for k, xs in times.items():
        bytes_moved = hdr + (12.0 if k in ("flowkey_hash", "lookup_worst16_nh_only") else 17.0) * n
        out[k] = med_min(xs)
        out[k]["frac"] = round(bytes_moved / (out[k]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        out[k]["gpkt_s"] = round(n / (out[k]["ms"] * 1e-3) / 1e9, 2)
    # what the spread table decides on this workload (the forward below runs on these next hops)
    eng.route_lookup_device(fibs["spread256"], *batches[0][:3], n, d_nh, d_if, d_v)
    eng.sync()
    v = d_v.download(np.uint8, n)
    out["spread256_forward_share"] = round(float((v == nf.RT_FORWARD).mean()), 4)
    if forward:
        fsteps = min(steps, 12)  # each forward decrements TTL (64 in the generator); batches are regenerated
        d_tab_fib, tab_n = fibs["spread256"].nexthops()
        rng = np.random.default_rng(8)
        d_tab8 = eng.alloc(96).upload(rng.integers(0, 256, size=96, dtype=np.uint8))
        d_nh9 = eng.alloc(4 * n).upload((np.arange(n) % 9).astype(np.uint32))
        d_nh8 = eng.alloc(4 * n).upload((np.arange(n) % 8).astype(np.uint32))
        fvars = {"forward_fib_table": (d_nh, d_tab_fib, tab_n), "forward_bench_table_mod9": (d_nh9, d_tab8, 8),
                 "forward_bench_table_mod8": (d_nh8, d_tab8, 8)}
        ftimes = {k: [] for k in fvars}
        for _ in range(rounds):
            for k, (nh, tab, tn) in fvars.items():
                for a, b, d, _ in batches:
                    eng.gen_config_device(config, SEED, 0, n, a, b, d)
                eng.sync()
                step = lambda: eng.l3_forward_device(*nxt(), nh, n, tab, tn)
                step()
                ftimes[k].append(event_ms(eng, step, fsteps) / fsteps)
        for k, xs in ftimes.items():
            out[k] = med_min(xs)
        out["forward_fib_table"]["table_entries"] = tab_n
    for f in fibs.values():
        f.close()
    for b in batches:
        b[0].free()
        b[2].free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c1-packets", type=int, default=1 << 20)
    ap.add_argument("--c3-packets", type=int, default=1 << 22)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events below are torch's, on the runtime the engine shares
    torch.cuda.init()
    with nf.Engine(0) as eng:
        res = {"tool": "tools/route_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "frac_is_on": "min(len, 128) header line + 8 descriptor + outputs (lookup 4 + 4 + 1, hash 4) per "
                             "packet, against 8000 GB/s",
               "c1": run_workload(eng, nf.CFG_C1, args.c1_packets, args.steps, args.rounds, args.warmup, True),
               "c3": run_workload(eng, nf.CFG_C3, args.c3_packets, args.steps, args.rounds, args.warmup, False)}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

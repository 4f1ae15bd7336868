#!/usr/bin/env python3
"""Times nfcs_l2_lookup_device against the flow-key kernel (hashes only: one header line per frame) in the
same run. Prints one JSON line.

    python tools/l2_bench.py [--steps 20] [--rounds 3] [--out profiles/l2_lookup_bench.json]

Per workload (1M C1 frames, the 4M C3 mix; 128-byte frame starts as bench.py's default) the timed calls
rotate over separately generated batches (4 up to 1M packets, 2 above) as bench.py's do, so no call finds
its frames in the memory-side cache. Variants are timed interleaved in one process, `rounds` times; each
figure is the median over the rounds of (HIP-event ms over `steps` calls) / steps, with the minimum beside it.

Sweep: an empty table (no probe at all: what the frame reads and the outputs cost), then a table of 1K, 128K
and 1M random entries on the ingress port's native VLAN (16-byte slots at load factor <= 0.5: 32 KiB,
4 MiB, 32 MiB), a hit rate of 100% and 50%, with and without d_learn. Before a
variant is timed the destination and source MACs of every frame of every batch are overwritten on the
device: with probability `hit` by the MAC of a uniformly drawn entry, else by a MAC no entry has (drawn
independently for the two). The frames keep everything else the generator gave them; tagged frames of the
mix look up their own VLAN and miss, so the measured share of hits (`dst_hit`) is reported next to the
target. Every port is a TRUNK that allows the VLAN, so a hit forwards.
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
TABLES = {"0": 0, "1k": 1 << 10, "128k": 1 << 17, "1m": 1 << 20}  # "0": no probe at all, everything floods
INGRESS, NATIVE = 0, 1


class TorchArena:
    """A device arena torch owns, so that the MAC bytes can be scattered into it on the device; .ptr is all
    the engine's calls need."""

    def __init__(self, nbytes: int):
        import torch
        self.t = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()


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


def make_table(entries_n: int):
    rng = np.random.default_rng(entries_n)
    macs = np.unique(rng.integers(0, 256, size=(entries_n + entries_n // 8 + 64, 6), dtype=np.uint8), axis=0)
    macs = macs[rng.permutation(len(macs))[:entries_n]]
    macs[:, 0] &= 0xFE  # unicast; the absent MACs below set this bit, so they are in no table
    macs = np.unique(macs, axis=0)
    e = np.zeros(len(macs), dtype=nf.FDB_ENTRY_DTYPE)
    e["mac"], e["vlan_id"], e["port"] = macs, NATIVE, rng.integers(1, 8, len(macs))
    fdb = nf.Fdb().set_entries(e)
    for p in range(8):
        fdb.set_port(p, type=nf.L2_TRUNK, native_vlan=NATIVE, allowed_vlans=[NATIVE])
    return fdb.commit(), macs


def write_macs(arena: TorchArena, off_dev, macs: np.ndarray, hit: float, rng):
    """Destination and source MAC of every frame: an entry's with probability `hit`, else an absent one."""
    import torch
    n = off_dev.shape[0]
    hdr = np.empty((n, 12), np.uint8)
    for k in (0, 6):
        m = macs[rng.integers(0, len(macs), n)] if len(macs) else np.zeros((n, 6), np.uint8)
        miss = rng.random(n) >= (hit if len(macs) else 0.0)
        m[miss] = rng.integers(0, 256, size=(int(miss.sum()), 6), dtype=np.uint8)
        m[miss, 0] |= 0x01
        hdr[:, k:k + 6] = m
    idx = off_dev[:, None] + torch.arange(12, device="cuda")[None, :]
    arena.t[idx] = torch.from_numpy(hdr).cuda()
    torch.cuda.synchronize()


def run_workload(eng, config: int, n: int, steps: int, rounds: int, warmup: int, tables):
    import torch
    nrot = 4 if n <= (1 << 20) else 2
    hdesc, nbytes = nf.layout_config(config, SEED, 0, n, 128)
    d_desc = eng.alloc(max(hdesc.nbytes, 16)).upload(hdesc)
    arenas = [TorchArena(nbytes) for _ in range(nrot)]
    for a in arenas:
        eng.gen_config_device(config, SEED, 0, n, a, nbytes, d_desc)
    eng.sync()
    off_dev = torch.from_numpy(hdesc["off16"].astype(np.int64) * 16).cuda()
    hdr_line = float(np.minimum(hdesc["len"].astype(np.float64), 128.0).sum())  # the yardstick's frame bytes
    hdr_l2 = float(np.minimum((hdesc["len"].astype(np.float64) + 15) // 16 * 16, 32.0).sum())  # one 32-byte sector
    d_port, d_v, d_vl, d_le, d_hash = eng.alloc(4 * n), eng.alloc(n), eng.alloc(2 * n), eng.alloc(n), eng.alloc(4 * n)
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return arenas[ctr[0] % nrot].ptr, nbytes, d_desc

    out = {"packets": n, "batches_rotated": nrot, "frame_align": 128}
    for tname, (fdb, macs) in tables.items():
        st = fdb.stats()
        for hit in (1.0, 0.5):
            rng = np.random.default_rng(int(hit * 100) + len(macs))
            for a in arenas:
                write_macs(a, off_dev, macs, hit, rng)
            fdb.upload(eng)
            variants = {
                "flowkey_hash": lambda: eng.flow_keys_device(*nxt(), n, None, d_hash),
                "l2_learn": lambda: eng.l2_lookup_device(fdb, INGRESS, *nxt(), n, d_port, verdict=d_v, vlan=d_vl,
                                                         learn=d_le),
                "l2_no_learn": lambda: eng.l2_lookup_device(fdb, INGRESS, *nxt(), n, d_port, verdict=d_v, vlan=d_vl),
            }
            times = {k: [] for k in variants}
            for step in variants.values():
                for _ in range(warmup):
                    step()
            eng.sync()
            for _ in range(rounds):
                for k, step in variants.items():
                    times[k].append(event_ms(eng, step, steps) / steps)
            res = {"entries": st["entries"], "slots": st["slots"], "table_bytes": 16 * st["slots"],
                   "max_probe": st["max_probe"], "hit_target": hit}
            # bytes per packet beside the frame: descriptor 8 + outputs (hash 4; port 4 + verdict 1 + VLAN 2 [+ learn 1])
            per_packet = {"flowkey_hash": (hdr_line, 12.0), "l2_learn": (hdr_l2, 16.0), "l2_no_learn": (hdr_l2, 15.0)}
            for k, xs in times.items():
                res[k] = med_min(xs)
                frame_bytes, pp = per_packet[k]
                res[k]["frac"] = round((frame_bytes + pp * n) / (res[k]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                # the same bytes as the yardstick's, so that the two times compare as one number
                res[k]["frac_at_yardstick_bytes"] = round((hdr_line + 12.0 * n) / (res[k]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                res[k]["gpkt_s"] = round(n / (res[k]["ms"] * 1e-3) / 1e9, 2)
            variants["l2_learn"]()
            eng.sync()
            verdict, learn = d_v.download(np.uint8, n), d_le.download(np.uint8, n)
            res["dst_hit"] = round(float((verdict == nf.L2_FORWARD).mean()), 4)
            res["src_hit"] = round(float((learn == nf.L2_LEARN_MOVED).mean()), 4)
            out[f"{tname}_hit{int(hit * 100)}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--c1-packets", type=int, default=1 << 20)
    ap.add_argument("--c3-packets", type=int, default=1 << 22)
    ap.add_argument("--tables", default="0,1k,128k,1m")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)  # the events and the arenas are torch's, on the runtime the engine shares
    torch.cuda.init()
    tables = {t: make_table(TABLES[t]) for t in args.tables.split(",")}
    with nf.Engine(0) as eng:
        res = {"tool": "tools/l2_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "frac_is_on": "flow keys: min(len, 128) header line + 8 descriptor + 4 hash per packet; L2: 32 frame "
                             "bytes (the sector holding bytes 0..15) + 8 descriptor + 4 port + 1 verdict + 2 VLAN "
                             "(+ 1 learn) per packet, table reads not counted; against 8000 GB/s. "
                             "frac_at_yardstick_bytes charges every variant the flow-key kernel's bytes",
               "c1": run_workload(eng, nf.CFG_C1, args.c1_packets, args.steps, args.rounds, args.warmup, tables),
               "c3": run_workload(eng, nf.CFG_C3, args.c3_packets, args.steps, args.rounds, args.warmup, tables)}
        for fdb, _ in tables.values():
            fdb.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

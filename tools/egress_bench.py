#!/usr/bin/env python3
"""Times the egress stage (nfcs_egress_plan_device, nfcs_egress_enqueue_device) against the flow-key kernel
(hashes only: one header line per frame) in the same run. Prints one JSON line.

    python tools/egress_bench.py [--steps 20] [--rounds 3] [--out profiles/egress_bench.json]

Per workload (1M C1 frames, the 4M C3 mix; 128-byte frame starts as bench.py's default) the timed calls
rotate over separately generated batches (4 up to 1M packets, 2 above) as bench.py's do, so no call finds
its frames in the memory-side cache. Variants are timed interleaved in one process, `rounds` times; each
figure is the median over the rounds of (HIP-event ms over `steps` calls) / steps, with the minimum beside it.

Port distributions (the egress port per packet, handed to the plan as d_l2_port; the queue per packet handed
to the enqueue is drawn uniformly over the port's queues, because the generated frames are untagged and
would all classify to the last queue):
  one_key    every packet on port 0, queue 0: the longest ranks
  48x4       48 ports x 4 queues, uniform
  1024x8     1,024 ports x 8 queues, uniform: the largest histogram and scan
each with queues that have room for everything ("room") and with max_queue_depth at half of the key's
packets, so that half are tail-dropped ("half"; the depths are copied back from a zeroed array on the stream
before every call, and that 32 KiB copy is inside the timed region).
Variants: flowkey_hash (the yardstick), plan (alone), enqueue (alone, on the ports the plan wrote), and
plan_enqueue (the two calls back to back). `x` is the variant's time over the yardstick's in the same run.
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
DISTS = {"one_key": (1, 1), "48x4": (48, 4), "1024x8": (1024, 8)}


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


def run_workload(eng, config: int, n: int, steps: int, rounds: int, warmup: int):
    import torch
    st = torch.cuda.ExternalStream(eng.stream)
    nrot = 4 if n <= (1 << 20) else 2
    hdesc, nbytes = nf.layout_config(config, SEED, 0, n, 128)
    d_desc = eng.alloc(max(hdesc.nbytes, 16)).upload(hdesc)
    arenas = [eng.alloc(nbytes) for _ in range(nrot)]
    for a in arenas:
        eng.gen_config_device(config, SEED, 0, n, a, nbytes, d_desc)
    eng.sync()
    d_hash, d_port, d_ops, d_queue_plan = eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(n)
    d_res, d_order = eng.alloc(n), eng.alloc(4 * n)
    ctr = [0]

    def nxt():
        ctr[0] += 1
        return arenas[ctr[0] % nrot], nbytes, d_desc

    out = {"packets": n, "batches_rotated": nrot, "frame_align": 128}
    rng = np.random.default_rng(n)
    for dname, (ports, queues) in DISTS.items():
        port = rng.integers(0, ports, n).astype(np.uint32)
        queue = rng.integers(0, queues, n).astype(np.uint8)
        d_in, d_queue = eng.alloc(4 * n).upload(port), eng.alloc(n).upload(queue)
        per_key = n // (ports * queues)
        for room in ("room", "half"):
            with nf.Egress() as eg:
                for p in range(ports):
                    eg.set_port(p, has_vlan_config=False, num_queues=queues,
                                max_queue_depth=0xFFFFFFFF if room == "room" else max(per_key // 2, 1))
                eg.commit().upload(eng)
                keys = eg.keys()[1]
                depth = torch.zeros(keys, dtype=torch.int32, device="cuda")
                zero = torch.zeros(keys, dtype=torch.int32, device="cuda")
                d_ks, d_drop = eng.alloc(4 * (keys + 1)), eng.alloc(4 * keys)
                torch.cuda.synchronize()

                def plan():
                    eng.egress_plan_device(eg, *nxt(), n, d_port, d_ops, d_queue_plan, l2_port=d_in)

                def enqueue():
                    if room == "half":
                        with torch.cuda.stream(st):
                            depth.copy_(zero, non_blocking=True)
                    eng.egress_enqueue_device(eg, d_port, d_queue, n, depth.data_ptr(), d_order, d_ks, result=d_res,
                                              key_dropped=d_drop)

                def both():
                    plan()
                    enqueue()

                variants = {"flowkey_hash": lambda: eng.flow_keys_device(*nxt(), n, None, d_hash), "plan": plan,
                            "enqueue": enqueue, "plan_enqueue": both}
                plan()
                eng.sync()
                times = {k: [] for k in variants}
                for step in variants.values():
                    for _ in range(warmup):
                        step()
                eng.sync()
                for _ in range(rounds):
                    for k, step in variants.items():
                        times[k].append(event_ms(eng, step, steps) / steps)
                res = {"ports": ports, "queues": queues, "keys": keys,
                       "tiles": (n + nf.EGRESS_TILE_PKTS - 1) // nf.EGRESS_TILE_PKTS}
                for k, xs in times.items():
                    res[k] = med_min(xs)
                    res[k]["gpkt_s"] = round(n / (res[k]["ms"] * 1e-3) / 1e9, 2)
                for k in ("plan", "enqueue", "plan_enqueue"):
                    res[k]["x"] = round(res[k]["ms"] / res["flowkey_hash"]["ms"], 3)
                enqueue()
                eng.sync()
                r = d_res.download(np.uint8, n)
                res["enqueued"] = round(float((r == nf.EQ_ENQUEUED).mean()), 4)
                res["dropped_full"] = round(float((r == nf.EQ_DROP_FULL).mean()), 4)
                out[f"{dname}_{room}"] = res
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
    torch.cuda.set_device(0)  # the events and the depth arrays are torch's, on the runtime the engine shares
    torch.cuda.init()
    with nf.Engine(0) as eng:
        res = {"tool": "tools/egress_bench.py", "steps": args.steps, "rounds": args.rounds,
               "timing": "HIP events on the engine's stream around the rotated calls; median (and min) over rounds",
               "x_is": "the variant's ms over flowkey_hash's ms in the same run",
               "c1": run_workload(eng, nf.CFG_C1, args.c1_packets, args.steps, args.rounds, args.warmup),
               "c3": run_workload(eng, nf.CFG_C3, args.c3_packets, args.steps, args.rounds, args.warmup)}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
